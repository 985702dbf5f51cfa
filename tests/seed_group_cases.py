"""The inputs of test_emu_seed_groups.py and test_gpu_seed_groups.py (K2 as a 16-lane group per read, k_seed.h: k_seed_grp) and what each case asserts.

Coverage conditions are computed from the oracle's stage dump alone."""
import numpy as np

import helpers
from lariat_amd import capi, synth


class _Reads:
    pass


def _with_reads(rs, reads):
    out = _Reads()
    out.seq = np.concatenate(reads).astype(np.uint8)
    out.seq_off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in reads], out=out.seq_off[1:])
    out.bc_pair_off, out.name_seed, out.n_pairs = rs.bc_pair_off, rs.name_seed, rs.n_pairs
    return out


def unique_case():
    """reads on unique sequence with junk pairs and some N bases; the first and the last read of the batch have no bases, one read is shorter than min_seed_len"""
    names, contigs = helpers.small_genome()
    rs = helpers.small_reads(names, contigs, n_barcodes=2, pairs=25, junk=0.05, seed=41)
    seq = rs.seq.copy()
    seq[np.arange(7, len(seq), 211)] = 4
    reads = [seq[rs.seq_off[i]:rs.seq_off[i + 1]] for i in range(len(rs.seq_off) - 1)]
    reads[0] = reads[0][:0]
    reads[-1] = reads[-1][:0]
    reads[5] = reads[5][:11]
    return names, contigs, _with_reads(rs, reads), {}


def repeat_case():
    names, contigs, rs = helpers.repeat_family_case(13, 2, pairs=6)
    return names, contigs, rs, {}


def repeat_max_occ3_case():
    """max_occ = 3: intervals with more occurrences are sampled with a step above one, capped at three seeds (the 64-bit divisions).  The library's suffix
    array keeps every eighth row, so that a seed's position is found by LF steps from row x0 + u * step (n_lf)"""
    names, contigs, rs = helpers.repeat_family_case(13, 2, pairs=6)
    return names, contigs, rs, {"max_occ": 3, "sa_intv": 8}


def low_complexity_case(n_barcodes, pairs, keep=None):
    """the low-complexity genome and the reads of test_gpu_k1_ring.py's _low_complexity_inputs.  With the default min_seed_len = 19 no read of theirs has more than
    14 intervals in the oracle's dump; with min_seed_len = 8 (library and oracle alike) reads have more than 16 and more than 64, which is what the case is for.
    keep: only these pairs of the read set, as one barcode (the emulator takes seconds per such read)"""
    def make():
        names, contigs = helpers.low_complexity_genome()
        rs = synth.make_reads(contigs, names, n_barcodes=n_barcodes, pairs_per_barcode=pairs, seed=3, sub_lo=0.002, sub_hi=0.03, indel_rate=0.002, mol_min=2, mol_max=3)
        if keep is not None:
            reads = [rs.seq[rs.seq_off[i]:rs.seq_off[i + 1]] for p in keep for i in (2 * p, 2 * p + 1)]
            sub = _with_reads(rs, reads)
            sub.bc_pair_off, sub.name_seed, sub.n_pairs = np.array([0, len(keep)], dtype=rs.bc_pair_off.dtype), rs.name_seed[list(keep)], len(keep)
            rs = sub
        return names, contigs, rs, {"min_seed_len": 8}
    return make


def coverage(name, want):
    """the property the case is there for, from the oracle's dump"""
    n_intv = np.diff(want.intv_off)
    n_seed = np.diff(want.seed_off)
    if name == "unique":
        assert n_seed[0] == 0 and n_seed[-1] == 0 and (n_seed == 0).sum() >= 3 and (n_seed > 0).sum() > 50
    if name == "low_complexity":
        assert (n_intv > 16).any() and (n_intv > 64).any()
    if name == "repeat_max_occ3":
        assert (want.intv[:, 2] > 3).any()
        assert n_seed.sum() < n_intv.sum() * 3 + 1


def check_case(lib, oracle, name, case):
    """the stage dump against the oracle's and, field by field, against the lane-per-seed path's (LH_F_SEED_LANE); the SA counters under both; the result"""
    names, contigs, rs, kw = case()
    kw = dict(kw)
    sa_intv = kw.pop("sa_intv", 0)
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    want = oidx.stage_dump(b, oracle.opts(**kw))
    coverage(name, want)
    idx = lib.index_from_arrays(oidx.arrays())
    if sa_intv:
        idx.resample_sa(sa_intv)
    ctx = idx.context(rs.n_pairs)
    got = ctx.stage_dump(b, lib.opts(**kw))
    helpers.assert_same_dump(got, want, helpers.DUMP_FRONT)
    lane = ctx.stage_dump(b, lib.opts(flags=capi.LH_F_SEED_LANE, **kw))
    helpers.assert_same_dump(got, lane, [n for n, _, _, _ in capi._DUMP_FIELDS])
    c_grp = ctx.align_barcodes(b, lib.opts(run_inference=0, **kw)).counters
    c_lane = ctx.align_barcodes(b, lib.opts(run_inference=0, flags=capi.LH_F_SEED_LANE, **kw)).counters
    assert c_grp["n_sa"] == c_lane["n_sa"] == int(want.seed_off[-1]) and c_grp["n_lf"] == c_lane["n_lf"]
    assert (c_grp["n_lf"] > 0) == bool(sa_intv)
    helpers.assert_same_result(ctx.align_barcodes(b, lib.opts(**kw)), oidx.align_barcodes(b, oracle.opts(**kw)), inference=True)
