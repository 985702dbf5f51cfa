"""K8's small-barcode instance (k_rfa.h: k_rfa<1>, hot tables in LDS) on the device, the product build: the shapes of rfa_small_cases.py — genomes of a few hundred
kilobases, a handful of barcodes of up to 100 pairs —, with and without LH_F_RFA_SLAB, against the oracle and against each other byte for byte."""
import importlib.util
import os

import pytest

import helpers
import rfa_small_cases as rc
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def test_gpu_rfa_small_usual(lib, oracle):
    out = rc.check_usual(lib, oracle, rc.DEFAULT_CAPS)
    assert out["within_caps"] == 6, out
    print(out)


def test_gpu_rfa_small_hundred_pairs(lib, oracle):
    """the headline's shape: barcodes of 100 pairs, a few candidates a read"""
    out = rc.check_usual(lib, oracle, rc.DEFAULT_CAPS, n_barcodes=3, pairs=100, seed=7)
    assert out["within_caps"] == 4, out


def test_gpu_rfa_small_molecule_overflow(lib, oracle):
    print(rc.check_molecules(lib, oracle, rc.DEFAULT_CAPS, 100))


def test_gpu_rfa_small_mixed_classes(lib, oracle):
    print(rc.check_mixed(lib, oracle, rc.DEFAULT_CAPS, 256, ["exact"] * 12 + ["copies3", "junk"], ["copies12"] * 100, ["copies12"] * 30))


def test_gpu_rfa_small_candidate_cap(lib, oracle):
    """candidates at cap - 1, cap, cap + 1 in 86 pairs (the read cap lies beyond 100 pairs: the emulator suite holds it)"""
    from tail_pass_cases import feature_genome
    names, contigs = feature_genome()
    per = rc.kind_counts(oracle)
    bcs = [rc.mix_for(nc, per, 100) for nc in (511, 512, 513)] + rc.PAD[:7]
    _, shapes, cls = rc.check(lib, oracle, names, contigs, rc.feature_reads(contigs[0], bcs), rc.DEFAULT_CAPS)
    assert [s[1] for s in shapes[:3]] == [511, 512, 513] and all(s[0] <= 200 for s in shapes), shapes
    assert cls == dict(big=0, rest=1, small=9, turned_away=0), cls


def test_gpu_rfa_small_heavy_pair(lib, oracle):
    print(rc.check_heavy_pair(lib, oracle, rc.DEFAULT_CAPS))


def test_gpu_rfa_small_fuzz_seed_95343(lib, oracle):
    spec = importlib.util.spec_from_file_location("fuzz_rfa_slab", os.path.join(helpers.ROOT, "tests", "checkers", "fuzz_rfa_slab.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    fz.run_case_both(lib, oracle, 95343)
