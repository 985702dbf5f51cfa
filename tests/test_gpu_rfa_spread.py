"""K8's small-barcode instance with several lanes per sink and per molecule (k_rfa.h: dev_fast_score_spread, the molecule status) on the device, the product build:
the cases of rfa_spread_cases.py — a handful of barcodes of at most 100 pairs each —, against the oracle, against the regular instance byte for byte
(LH_F_RFA_SLAB) and against a second run."""
import pytest

import rfa_spread_cases as sc
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def cover(lib, oracle):
    return {}


@pytest.mark.parametrize("which", ["small_genome", "many_contigs"])
def test_gpu_rfa_spread_case(lib, oracle, cover, which):
    cov, cls = sc.check_case(lib, oracle, which)
    cover[which] = cov
    print(cov, cls)
    assert cls["small"] > 0 and cls["turned_away"] == 0, cls


def test_gpu_rfa_spread_cover(lib, oracle, cover):
    """the two cases together hold a small barcode of every group width, one on the one-lane form, and sources of one alignment, of a partial step, of two steps"""
    for which in ("small_genome", "many_contigs"):
        if which not in cover:
            cover[which] = sc.check_case(lib, oracle, which)[0]
    sc.assert_cover(sc.merge(cover["small_genome"], cover["many_contigs"]))
