"""K1's pass-2 probe and pass 3 in one lockstep kernel (k_p23_lock, k_p2_close: k_smem4.h) on the device, the product build: lock_tail_cases.py's cases — genomes of
at most 600 kb, a few dozen to a few hundred reads each — the default sequence against LH_F_P3_LAST byte for byte and both against the oracle.  (Slots of four
intervals and the builds that must fail are the emulator suite's.)"""
import pytest

import lock_tail_cases as cases
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.mark.parametrize("case", ["walks", "subs", "odd", "fin", "rep"])
def test_gpu_lock_tail(lib, oracle, case):
    cases.check_case(lib, oracle, case)


def test_gpu_lock_tail_too_long(lib, oracle):
    cases.check_too_long(lib, oracle)


def test_gpu_lock_tail_overflow(lib, oracle):
    """low-complexity reads: more than LH_MAX_INTV = 64 intervals, the 65th pass 2's in some reads and pass 3's in others"""
    cases.check_case(lib, oracle, "low")


def test_gpu_lock_tail_shares(lib, oracle):
    cases.check_shares(oracle)
    cases.check_case(lib, oracle, "family")


def test_gpu_lock_tail_other_paths(lib, oracle):
    cases.check_other_paths(lib, oracle)


def test_gpu_lock_tail_rounds(lib, oracle):
    cases.check_rounds(lib, oracle)


def test_gpu_lock_tail_two_lanes(lib, oracle):
    cases.check_two_lanes(lib, oracle)
