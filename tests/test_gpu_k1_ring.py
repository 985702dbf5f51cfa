"""K1's interval lists on chip (k_smem4.h: LIST_PUT / LIST_GET) on the device: the instance for short reads (small query staging, two ring
entries per list) and the full one (long reads, one entry) against the oracle, with and without the exact shortcuts, on reads whose lists fit
the ring, long noisy reads and low-complexity sequence whose forward lists overflow it."""
import numpy as np
import pytest

import helpers
from lariat_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


def _shortcut_inputs():
    names, contigs = helpers.small_genome()
    rs = helpers.small_reads(names, contigs, n_barcodes=2, pairs=25, junk=0.05, seed=41)
    rs.seq[np.arange(7, len(rs.seq), 211)] = 4
    return names, contigs, rs


def _long_noisy_inputs():
    names, contigs = helpers.small_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=40, seed=31, len1=240, len2=236, sub_lo=0.005, sub_hi=0.03, indel_rate=0.003, junk_frac=0.02)
    return names, contigs, rs


def _low_complexity_inputs():
    names, contigs = helpers.low_complexity_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=6, pairs_per_barcode=60, seed=3, sub_lo=0.002, sub_hi=0.03, indel_rate=0.002, mol_min=2, mol_max=3)
    return names, contigs, rs


INPUTS = {"shortcuts": _shortcut_inputs, "long_noisy": _long_noisy_inputs, "low_complexity": _low_complexity_inputs}


@pytest.mark.parametrize("inp", sorted(INPUTS))
def test_k1_ring_parity(lib, oracle, inp):
    names, contigs, rs = INPUTS[inp]()
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    ctx = lib.index_from_arrays(oidx.arrays()).context(rs.n_pairs)
    want = oidx.stage_dump(b)
    helpers.assert_same_dump(ctx.stage_dump(b), want, helpers.DUMP_FRONT)
    helpers.assert_same_result(ctx.align_barcodes(b), oidx.align_barcodes(b), inference=True)
    NOF = capi.LH_F_NO_SWEEP_FILTER
    helpers.assert_same_dump(ctx.stage_dump(b, lib.opts(flags=NOF)), want, helpers.DUMP_FRONT)
    got = ctx.align_barcodes(b, lib.opts(run_inference=0, flags=NOF)).counters["n_ext"]
    assert got == oidx.align_barcodes(b, oracle.opts(run_inference=0)).counters["n_ext"]
