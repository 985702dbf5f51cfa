"""Reads at contig ends, on short contigs and in indices of about a thousand contigs, through the kernel sources under the CPU emulator, against
the oracle (stage dumps DUMP_FRONT + DUMP_REGS and every result field).

The genome (helpers.fragmented_genome) is one long contig in front, one in the middle and ~1,100 short ones (12 bp to 6 kb; some shorter than
min_seed_len, a read, an insert; some overlapping the previous contig).  The reads (helpers.geometry_reads) cross junctions, hang off contig ends
and off both ends of the concatenation, cover contigs shorter than themselves, or have their mates on unrelated contigs.  What they reach:

  * mem_chain's skip of a seed that bridges two contigs or l_pac (k_chain.h, k_chain_cl.h, k_chain_lane.h);
  * mem_chain2aln's window clamped to [0, 2 l_pac), to one side of l_pac, to the seed's contig (k_extend.h; k_chain_lane.h dev_fetch_clamp);
  * mem_matesw's window clamped to the contig of its midpoint, no attempt when too short (k_rescue2.h, k_rescue3.h): pairs whose mates overlap
    across a contig end, one of them without a seed;
  * mem_reg2aln's rejection of a region across l_pac (k_aln.h);
  * K8's grouping by contig (k_rfa.h): with 1,000 contigs the contig tables fit LDS (n_contigs + 2 <= LH_RFA_NCONT_LDS = 1024) — one barcode over
    256 candidates takes the atomic form, the others the serial one; with 1,100 contigs both forms run from the slab.

The same reads go against both contig counts: the 1,000-contig genome is the 1,100-contig one without 100 short contigs away from the ends.
Every case asserts minimum counts of the edges it reached (helpers.geometry_coverage, read from the oracle's output)."""
import os
import subprocess

import numpy as np
import pytest

import helpers
from lariat_amd import capi

EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu")
BUILDS = {"default": "liblariat_emu.so", "small": "liblariat_emu_small.so"}
FLAGS = [0, capi.LH_F_CHAIN_WAVE, capi.LH_F_EXT_SERIAL, capi.LH_F_EXT_WAVE, capi.LH_F_RESCUE_FULL, capi.LH_F_P2_TASKS]
INDEX_ALT = [("arrays", False), ("device", True), ("arrays", True), ("device", False)]
GENOME_SEED, READS_SEED = 7, 3
PAIRS = [150, 30, 40]   # barcode 0: more than 256 filtered candidates; the others fewer


def geometry_case(n_contigs, seed=GENOME_SEED, reads_seed=READS_SEED, pairs=PAIRS):
    """(names, contigs, alt, reads): the reads are drawn on the 1,000-contig form whatever n_contigs is (1,000 or 1,100)"""
    names, contigs, alt = helpers.fragmented_genome(seed, 1100, short_max=6000, alt_frac=0.1)
    keep = np.ones(1100, dtype=bool)
    keep[100:200] = False            # short contigs only (the long ones are contigs 0 and 550)
    sub = [c for c, k in zip(contigs, keep) if k]
    rs = helpers.geometry_reads(sub, pairs, seed=reads_seed)
    if n_contigs == 1000:
        return [n for n, k in zip(names, keep) if k], sub, alt[keep], rs
    assert n_contigs == 1100
    return names, contigs, alt, rs


def build_index(lib, oidx, names, contigs, how):
    if how == "arrays":
        return lib.index_from_arrays(oidx.arrays())
    pac, l_pac, _, _ = lib.reference_pack(contigs)
    lens = [len(c) for c in contigs]
    offs = np.concatenate([[0], np.cumsum(lens)])
    return lib.index_build_device(pac, l_pac, [(names[i], lens[i], int(offs[i])) for i in range(len(names))])


def run_geometry(lib, oracle, n_contigs, runs, threads=8):
    """runs: [(flags, index form, alt on)]; each against the oracle's stage dump and result.  Returns the coverage counts per alt setting."""
    names, contigs, alt, rs = geometry_case(n_contigs)
    assert (len(contigs) + 2 <= 1024) == (n_contigs == 1000)
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    want, cov = {}, {}
    for a in (False, True):
        oidx.set_alt(alt if a else np.zeros_like(alt))
        od = oidx.stage_dump(b)
        ores = oidx.align_barcodes(b, threads=threads)
        want[a] = (od, ores)
        cov[a] = helpers.geometry_coverage([len(c) for c in contigs], od, ores, b)
    idxs = {}
    for flags, how, a in runs:
        if how not in idxs:
            idxs[how] = build_index(lib, oidx, names, contigs, how)
        idx = idxs[how]
        idx.set_alt(alt if a else np.zeros_like(alt))
        ctx = idx.context(rs.n_pairs)
        what = "%d contigs, flags %d, index %s, alt %s" % (n_contigs, flags, how, a)
        try:
            helpers.assert_same_dump(ctx.stage_dump(b, lib.opts(flags=flags)), want[a][0], helpers.DUMP_FRONT + helpers.DUMP_REGS)
            helpers.assert_same_result(ctx.align_barcodes(b, lib.opts(flags=flags)), want[a][1], inference=True)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))
        ctx.close()
    for a in (False, True):
        helpers.assert_geometry_coverage(cov[a], bridging_seeds=50, regions_on_contig_end=50, cand_pos0=20, cand_aend_at_contig_end=20,
                                         soft_clips_at_contig_end=20, cand_on_contig_shorter_than_read=20, n_rescue=20)
        assert cov[a]["max_filtered"] > 256, cov[a]
    (d0, _), (d1, _) = want[False], want[True]
    alt_changed = sum(not np.array_equal(d0.chain_kept[d0.chain_off[r]:d0.chain_off[r + 1]], d1.chain_kept[d1.chain_off[r]:d1.chain_off[r + 1]]) for r in range(2 * rs.n_pairs))
    assert alt_changed >= 1   # the ALT mask reaches mem_chain_flt: a junction read on an ALT contig that overlaps a primary one
    return cov


@pytest.fixture(scope="module")
def emu_libs():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "small"])
    return {k: capi.Library(os.path.join(helpers.ROOT, "tests", "_build", v)) for k, v in BUILDS.items()}


@pytest.mark.parametrize("n_contigs", [1000, 1100])
@pytest.mark.parametrize("build", ["default", "small"])
def test_emu_geometry(emu_libs, oracle, build, n_contigs):
    """every flag set in both builds; each flag set runs with ALT off at one contig count and on at the other, and the flag sets alternate between the index from
    arrays and the one the device builder makes from the .pac"""
    shift = 0 if n_contigs == 1000 else 2
    runs = [(f, *INDEX_ALT[(k + shift) % 4]) for k, f in enumerate(FLAGS)]
    cov = run_geometry(emu_libs[build], oracle, n_contigs, runs)
    print("%s, %d contigs: %s" % (build, n_contigs, cov))


def test_emu_geometry_rescue_at_contig_ends(emu_libs, oracle):
    """pairs whose one mate lies on a contig shorter than an insert or next to a contig end: mem_matesw's window is cut by the contig (or dropped when what is
    left is shorter than min_seed_len) — whole-window and certificate rescue, both builds, against the oracle"""
    names, contigs, alt = helpers.fragmented_genome(17, 300, long_lens=(60000,), short_max=2500, overlap_frac=0.3)
    rs = helpers.geometry_reads(contigs, [60, 60], seed=19, kinds=("junction", "overhang", "inside_short", "ends", "rescue_edge"), sub_hi=0.04)
    b = helpers.batch_of(rs)
    oidx = oracle.index_build_naive(names, contigs)
    od, want = oidx.stage_dump(b), oidx.align_barcodes(b, threads=8)
    cov = helpers.geometry_coverage([len(c) for c in contigs], od, want, b)
    helpers.assert_geometry_coverage(cov, n_rescue=20, barcodes_over_256=0)
    for lib in emu_libs.values():
        idx = lib.index_from_arrays(oidx.arrays())
        for flags in (0, capi.LH_F_RESCUE_FULL):
            helpers.assert_same_result(idx.context(rs.n_pairs).align_barcodes(b, lib.opts(flags=flags)), want, inference=True)
