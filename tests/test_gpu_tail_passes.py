"""A read's K5 on the lane that finishes its extension, k_dedup_fast over the reads that finish elsewhere, K8's prologue beside K7 (tail_pass_cases.py), on
the device with the product library."""
import pytest

import tail_pass_cases as tp
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


def test_dedup_where_extension_finishes(lib, oracle):
    print(tp.check_part1(lib, oracle))


def test_dedup_ext_wave(lib, oracle):
    print(tp.check_part1(lib, oracle, flags=capi.LH_F_EXT_WAVE))


def test_rfa_prologue(lib, oracle):
    cov = tp.check_part3(lib, oracle, n_barcodes=300)
    print(cov)
    assert cov["barcodes"] >= 300


def test_rfa_prologue_two_lanes(lib, oracle):
    print(tp.check_part3(lib, oracle, n_barcodes=300, lanes=2))


def test_mixed_batches(lib, oracle):
    tp.check_mixed_batches(lib, oracle)
