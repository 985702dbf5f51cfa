"""K1's pass 2 over the calls k_p2_probe lists (k_smem4.h) on the device, the product build: p2_probe_cases.py's cases — one genome of 240 kb with planted copies, a
few dozen to a few hundred reads each — against the oracle, against LH_F_P2_SCAN byte for byte and against the model of the lister's counts.  (Slots of four
intervals and the probe one window short are builds of the emulator suite.)"""
import pytest

import p2_probe_cases as cases
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_gpu_p2_probe(lib, oracle, case):
    cases.check_case(lib, oracle, case)


def test_gpu_p2_probe_empty_list(lib, oracle):
    cases.check_empty_list_keeps_n_intv(lib, oracle)


@pytest.mark.parametrize("case", cases.COUNT_CASES)
def test_gpu_p2_probe_read_counts(lib, oracle, case):
    cases.check_case(lib, oracle, case)


@pytest.mark.parametrize("case", cases.BASE_CASES)
@pytest.mark.parametrize("flags", [capi.LH_F_NO_SWEEP_FILTER, capi.LH_F_P2_TASKS], ids=["no_filter", "tasks"])
def test_gpu_p2_probe_flags(lib, oracle, case, flags):
    cases.check_case(lib, oracle, case, flags=flags)


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_gpu_p2_probe_two_lanes(lib, oracle, case):
    ctx, _ = cases.check_case(lib, oracle, case, ctx_kw={"lanes": 2}, counts=False)
    assert ctx.rounds(1)["n_rounds"] >= 1, "the batch was not split over the lanes"


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_gpu_p2_probe_rounds(lib, oracle, case):
    cases.check_rounds(lib, oracle, case)


def test_gpu_p2_probe_too_long(lib, oracle):
    cases.check_too_long(lib, oracle)
