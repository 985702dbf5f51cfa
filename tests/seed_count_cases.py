"""The inputs of test_emu_seed_counts.py and test_gpu_seed_counts.py and what each case asserts: K1's pass 3 counts a read's seeds and lists the reads whose
intervals k_smem_fin still has to sort in memory (more than 16 intervals, or one above max_occ), and K2 ranks the intervals of every other read inside its 16-lane
group (k_smem4.h: k_smem_p3_lock, k_smem_fin; k_seed.h: k_seed_grp).

Coverage conditions are computed from the oracle's stage dump alone."""
import numpy as np

import helpers
import seed_group_cases as cases
from lariat_amd import capi, synth

MAX_OCC = 500   # lh_opts_init's
CHUNK_EDGE_KEEP = (1, 8)   # the emulator's pairs of the chunk_edge set: reads of 11 (a duplicate, an interval above max_occ), 14, 16 and 17 intervals


def chunk_edge_reads(keep=None, barcode_each=False):
    """the reads of seed_group_cases.low_complexity_case(2, 12); keep: only these pairs, as one barcode (barcode_each: one barcode a pair, so that two lanes split them)"""
    _, _, rs, _ = cases.low_complexity_case(2, 12, keep=keep)()
    if keep is not None and barcode_each:
        rs.bc_pair_off = np.arange(len(keep) + 1, dtype=rs.bc_pair_off.dtype)
    return rs


def chunk_edge_case(keep=None):
    """low-complexity reads with min_seed_len = 10 (library and oracle alike): reads of 15, 16, 17 and 18 intervals — either side of K2's one chunk of 16 —, two
    intervals of equal `info` in a read, and reads of at most 16 intervals that hold one above max_occ"""
    def make():
        names, contigs = helpers.low_complexity_genome()
        return names, contigs, chunk_edge_reads(keep), {"min_seed_len": 10}
    return make


def unique_max_mem_intv_case(v):
    """seed_group_cases.unique_case with max_mem_intv = v.  0: no pass 3, so k_smem_fin runs over every read; 1: pass 3 runs without its walks by text (text_ok is
    false) and still has to count every read"""
    def make():
        names, contigs, rs, kw = cases.unique_case()
        return names, contigs, rs, dict(kw, max_mem_intv=v)
    return make


def _per_read(want):
    n = np.diff(want.intv_off)
    return n, [want.intv[want.intv_off[r]:want.intv_off[r + 1]] for r in range(len(n))]


def cover_chunk_edge(want):
    n, per = _per_read(want)
    assert (n == 16).any() and (n == 17).any(), np.bincount(n)
    assert any(len(np.unique(iv[:, 3])) < len(iv) for iv in per), "no read with two intervals of equal info"
    assert any(0 < len(iv) <= 16 and (iv[:, 2] > MAX_OCC).any() for iv in per), "no read of at most 16 intervals with one above max_occ"


def cover_out_of_order(want, min_seed_len=19):
    """K1 appends pass 3's intervals (min_seed_len + 1 bases) behind the others: in some read one of them starts before a longer interval does, so that the order K1
    leaves is not the sorted one and K2's rank has something to do"""
    _, per = _per_read(want)
    hit = 0
    for iv in per:
        qb = (iv[:, 3] >> np.uint64(32)).astype(np.int64)
        ln = (iv[:, 3] & np.uint64(0xffffffff)).astype(np.int64) - qb
        short = qb[ln == min_seed_len + 1]
        longer = qb[ln > min_seed_len + 1]
        hit += bool(len(short) and len(longer) and short.min() < longer.max())
    assert hit > 0, "no read whose pass-3 interval starts before a longer one"
    return hit


def cover_max_mem_intv(want):
    n, _ = _per_read(want)
    assert list(np.bincount(n)) == [4, 23, 50, 18, 5], np.bincount(n)


def oracle_dump(oracle, case):
    names, contigs, rs, kw = case()
    return oracle.index_build_naive(names, contigs).stage_dump(helpers.batch_of(rs), oracle.opts(**kw))


def check_p2_tasks(lib, oracle):
    """pass 2 as tasks (LH_F_P2_TASKS): its lanes append to a read's slots through an atomic counter, in any order"""
    names, contigs, rs, kw = cases.repeat_case()
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    want = oidx.stage_dump(b, oracle.opts(**kw))
    assert (np.diff(want.intv_off) > 1).any()
    ctx = lib.index_from_arrays(oidx.arrays()).context(rs.n_pairs)
    helpers.assert_same_dump(ctx.stage_dump(b, lib.opts(flags=capi.LH_F_P2_TASKS, **kw)), want, helpers.DUMP_FRONT)
    helpers.assert_same_result(ctx.align_barcodes(b, lib.opts(flags=capi.LH_F_P2_TASKS, **kw)), oidx.align_barcodes(b, oracle.opts(**kw)), inference=True)


def _both_genomes():
    names, contigs = helpers.small_genome()
    lnames, lcontigs = helpers.low_complexity_genome()
    return names + lnames, contigs + lcontigs


def check_three_batches(lib, oracle, keep=None):
    """chunk_edge, the unique reads, chunk_edge again on ONE context (over both genomes): no list length, seed count or l_rep of the batch before may survive —
    the first batch lists reads for k_smem_fin and has reads with l_rep > 0, the second has far fewer listed reads, the third has fewer reads than the second"""
    names, contigs = _both_genomes()
    oidx = oracle.index_build_naive(names, contigs)
    edge = chunk_edge_reads(keep)
    _, _, uniq, _ = cases.unique_case()
    seq = [(edge, {"min_seed_len": 10}), (uniq, {}), (edge, {"min_seed_len": 10})]
    listed = []
    for rs, kw in seq[:2]:
        n, per = _per_read(oidx.stage_dump(helpers.batch_of(rs), oracle.opts(**kw)))
        listed.append(sum(1 for k, iv in zip(n, per) if k > 16 or (iv[:, 2] > MAX_OCC).any()))
    assert listed[0] > 0 and listed[1] * 4 < len(uniq.seq_off) - 1, listed
    assert uniq.n_pairs > edge.n_pairs
    ctx = lib.index_from_arrays(oidx.arrays()).context(max(edge.n_pairs, uniq.n_pairs))
    for rs, kw in seq:
        b = helpers.batch_of(rs)
        helpers.assert_same_result(ctx.align_barcodes(b, lib.opts(**kw)), oidx.align_barcodes(b, oracle.opts(**kw)), inference=True)


def check_two_lanes(lib, oracle, keep=None):
    """chunk_edge through two lanes: the list and its counter are each pipeline's own"""
    names, contigs = helpers.low_complexity_genome()
    rs = chunk_edge_reads(keep, barcode_each=True)
    kw = {"min_seed_len": 10}
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    ctx = lib.index_from_arrays(oidx.arrays()).context(max(rs.n_pairs, 4), lanes=2)
    res = ctx.align_barcodes(b, lib.opts(**kw))
    assert ctx.rounds(1)["n_rounds"] >= 1, "the batch was not split over the lanes"
    helpers.assert_same_result(res, oidx.align_barcodes(b, oracle.opts(**kw)), inference=True)
