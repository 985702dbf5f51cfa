"""The inputs of test_emu_tail_passes.py and test_gpu_tail_passes.py and what each case asserts: a read's K5 (k_dedup.h: dev_dedup_fast_read) runs on the lane
that finishes the read's extension (k_extend2.h: ext_control), k_dedup_fast only passes over the reads that finish elsewhere, and K8's prologue (k_rfa.h:
k_rfa_init, k_rfa_order) runs beside K7.  Every case is held to the oracle and, byte for byte, to the same batch under LH_F_TAIL_PASSES (the passes in their
old places).

Coverage conditions are computed from the oracle's stage dump and result alone."""
import numpy as np

import helpers
from lariat_amd import capi, synth

COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
W, MAX_CHAIN_GAP, PATCH_MAX_R_BW = 100, 10000, 0.05   # lh_opts_init's w and max_chain_gap; k_dedup.h's LH_PATCH_MAX_R_BW
UNIT = 400
AT2, AT3, AT12 = (10000, 40000), (15000, 45000, 70000), tuple(80000 + 1200 * i for i in range(12))


def feature_genome(seed=17):
    """one random contig with three planted units: two, three and twelve EXACT copies (the first two sets further apart than max_chain_gap).  A read inside a unit
    has as many full-length chains: nothing to extend, as many regions, none of them redundant"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=100000).astype(np.uint8)
    for at in (AT2, AT3, AT12):
        u = rng.integers(0, 4, size=UNIT).astype(np.uint8)
        for p in at:
            g[p:p + UNIT] = u
    return ["chrT"], [g]


def _rc(x):
    return COMP[x[::-1]]


def _read_set(reads, names, bc_pair_off):
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads).astype(np.uint8)
    rs.bc_pair_off = np.asarray(bc_pair_off, dtype=np.int32)
    rs.names = names
    rs.name_seed = synth._name_seeds(names)
    return rs


# what read 1 of a pair is (read 2: 150 exact bases of the reverse strand a few hundred bases on, unless said otherwise)
KINDS = ("exact", "junk", "copies2", "copies3", "copies12", "mismatch_end", "long_deletion", "equal_re", "patch_dp")


def feature_pair(g, kind, p, rng):
    """read 1 of `kind` at p, and its mate"""
    mate = _rc(g[p + 250:p + 400])
    if kind == "exact":              # one region, found in round 0 without a DP
        r1 = g[p:p + 150].copy()
    elif kind == "junk":             # no region: the read's candidate is its placeholder
        r1 = rng.integers(0, 4, size=150).astype(np.uint8)
    elif kind in ("copies2", "copies3", "copies12"):   # 2 / 3 regions in round 0 without a DP; 12 chains: more than a lane chains
        at = {"copies2": AT2, "copies3": AT3, "copies12": AT12}[kind][0]
        r1 = g[at + 20:at + 170].copy()
        mate = _rc(g[at + 200:at + 350])
    elif kind == "mismatch_end":     # three mismatches in the first 19 bases: the left side loses more than a gap costs, a DP in a later round
        r1 = g[p:p + 150].copy()
        r1[[6, 11, 16]] ^= 1
    elif kind == "long_deletion":    # 25 bases missing behind base 90 of 200: the longest seed's left side is long and not the diagonal (the wave extension kernel)
        r1 = np.concatenate([g[p:p + 90], g[p + 115:p + 225]])
    elif kind == "equal_re":         # bases [e - 100, e) and then [e - 50, e) again: two regions that end at e
        r1 = np.concatenate([g[p:p + 100], g[p + 50:p + 100]])
    elif kind == "patch_dp":         # 40 mismatches between two matching stretches on one diagonal: two regions mem_patch_reg re-aligns (and does not merge)
        r1 = np.concatenate([g[p:p + 70], g[p + 70:p + 110] ^ 2, g[p + 110:p + 180]])
    else:
        raise ValueError(kind)
    return r1, mate


def feature_reads(g, kinds_per_barcode, seed=23):
    """barcodes of the given kinds' pairs, on unique sequence between the planted units"""
    rng = np.random.default_rng(seed)
    reads, names, off, kinds = [], [], [0], []
    slot = 0
    for bc in kinds_per_barcode:
        for kind in bc:
            p = 20000 + 700 * (slot % 25) + 37 * (slot // 25)   # [20000, 38000): unique sequence
            slot += 1
            r1, r2 = feature_pair(g, kind, p, rng)
            reads += [r1, r2]
            names.append("%s:%d" % (kind, len(names)))
            kinds.append(kind)
        off.append(len(names))
    return _read_set(reads, names, off), kinds


def part1_case():
    def make():
        names, contigs = feature_genome()
        bcs = [list(KINDS), ["exact", "copies2", "equal_re", "patch_dp", "junk", "mismatch_end"], ["long_deletion", "copies3", "copies12", "exact"]]
        rs, kinds = feature_reads(contigs[0], bcs)
        return names, contigs, rs, {}, kinds
    return make


def _needs_dp(a, b, l_pac):
    """dev_patch_needs_dp (k_dedup.h) on two (rb, re, qb, qe) spans: mem_patch_reg up to its DP"""
    if a[0] < l_pac <= b[0]:
        return False
    if a[2] >= b[2] or a[3] >= b[3] or a[1] >= b[1]:
        return False
    w = abs((a[1] - b[0]) - (a[3] - b[2]))
    r = abs((a[1] - b[0]) / (b[1] - a[0]) - (a[3] - b[2]) / (b[3] - a[2]))
    if a[1] < b[0] or a[3] < b[2]:
        return not (w > W << 1 or r >= PATCH_MAX_R_BW)
    return not (w > W << 2 or r >= PATCH_MAX_R_BW * 2)


def cover_part1(want, kinds, l_pac):
    """from the oracle's regions after K5: reads 1 of every kind have the regions the kind is there for"""
    n = np.diff(want.reg_off)
    by = {k: [2 * i for i, x in enumerate(kinds) if x == k] for k in KINDS}
    assert all(by[k] for k in KINDS)
    assert all(n[r] == 0 for r in by["junk"]) and all(n[r] == 1 for r in by["exact"] + by["mismatch_end"]), n
    assert all(n[r] == 2 for r in by["copies2"]) and all(n[r] == 3 for r in by["copies3"]) and all(n[r] == 12 for r in by["copies12"]), n
    assert all(n[r] >= 1 for r in by["long_deletion"])
    spans = lambda r: [(int(want.reg_rb[i]), int(want.reg_re[i]), int(want.reg_qb[i]), int(want.reg_qe[i])) for i in range(want.reg_off[r], want.reg_off[r + 1])]
    eq = [r for r in by["equal_re"] if n[r] == 2 and spans(r)[0][1] == spans(r)[1][1]]
    assert eq, "no read with two regions that end at the same position"
    dp = []
    for r in by["patch_dp"]:
        if n[r] == 2:   # (not merged: the records are as K4 left them)
            a, b = sorted(spans(r), key=lambda s: s[1])
            dp += [r] * bool(a[0] < b[0] and _needs_dp(a, b, l_pac))
    assert dp, "no read whose two regions reach mem_patch_reg's DP"
    return dict(equal_re=len(eq), patch_dp=len(dp), regions=np.bincount(n).tolist())


def part3_case(n_barcodes=300, seed=29):
    """barcodes of one to a dozen pairs (k_rfa_order's size classes: a quarter of an octave of the candidate count), pairs with a read that has no region among
    them, one barcode without inference"""
    def make():
        names, contigs = feature_genome()
        rng = np.random.default_rng(seed)
        bcs = []
        for b in range(n_barcodes):
            k = 1 + int(rng.integers(0, 12)) if b % 7 else 1 + b % 3
            bcs.append([("junk" if rng.random() < 0.1 else "copies3" if rng.random() < 0.1 else "exact") for _ in range(k)])
        bcs[3][0] = "junk"
        rs, kinds = feature_reads(contigs[0], bcs, seed=seed + 1)
        do_rfa = np.ones(n_barcodes, dtype=np.uint8)
        do_rfa[5] = 0
        return names, contigs, rs, {}, kinds, do_rfa
    return make


def cover_part3(ores, rs, do_rfa):
    n_cand = np.diff(ores.cand_off)
    placeholders = int(((n_cand == 1) & (ores.rid[ores.cand_off[:-1]] < 0)).sum())
    assert placeholders > 0, "no read without a region"
    per_bc = np.array([ores.cand_off[2 * rs.bc_pair_off[b + 1]] - ores.cand_off[2 * rs.bc_pair_off[b]] for b in range(len(rs.bc_pair_off) - 1)])
    x = per_bc + 1
    lg = np.floor(np.log2(x)).astype(int)
    cls = 4 * lg + np.where(lg >= 2, (x >> np.maximum(lg - 2, 0)) & 3, 0)   # k_rfa_order's cls_of
    assert len(np.unique(cls)) >= 6 and (do_rfa == 0).sum() == 1 and len(per_bc) >= 16, np.unique(cls)
    return dict(placeholders=placeholders, classes=len(np.unique(cls)), barcodes=len(per_bc))


RESULT_COLUMNS = helpers.INT_FIELDS + helpers.INF_FIELDS + helpers.F64_FIELDS + ["mapq"]


def assert_same_bytes(got, old):
    """every result column of the two runs, float64 columns included, byte for byte"""
    for f in RESULT_COLUMNS:
        a, b = getattr(got, f), getattr(old, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "result column %s differs between the fused sequence and LH_F_TAIL_PASSES" % f
    assert got.counters == old.counters, (got.counters, old.counters)


def check(lib, oracle, names, contigs, rs, kw, do_rfa=None, flags=0, lanes=1, dump=True):
    """the batch against the oracle (regions after K5, then the result) and against itself under LH_F_TAIL_PASSES"""
    oidx = oracle.index_build_naive(names, contigs)
    b = capi.Batch.from_arrays(rs.seq, rs.seq_off, rs.bc_pair_off, rs.name_seed, bc_do_rfa=do_rfa)
    ctx = lib.index_from_arrays(oidx.arrays()).context(max(rs.n_pairs, 4), **({"lanes": lanes} if lanes > 1 else {}))
    want = oidx.stage_dump(b, oracle.opts(**kw))
    if dump:
        helpers.assert_same_dump(ctx.stage_dump(b, lib.opts(flags=flags, **kw)), want, helpers.DUMP_FRONT + helpers.DUMP_REGS)
    ores = oidx.align_barcodes(b, oracle.opts(**kw))
    got = ctx.align_barcodes(b, lib.opts(flags=flags, **kw))
    if lanes > 1:
        assert ctx.rounds(1)["n_rounds"] >= 1, "the batch was not split over the lanes"
    helpers.assert_same_result(got, ores, inference=True)
    for c in ("n_rescue", "rescue_cells"):
        assert got.counters[c] == ores.counters[c], (c, got.counters[c], ores.counters[c])
    old = ctx.align_barcodes(b, lib.opts(flags=flags | capi.LH_F_TAIL_PASSES, **kw))
    assert_same_bytes(got, old)
    return want, ores


def check_part1(lib, oracle, flags=0):
    names, contigs, rs, kw, kinds = part1_case()()
    want, _ = check(lib, oracle, names, contigs, rs, kw, flags=flags)
    return cover_part1(want, kinds, len(contigs[0]))


def check_part3(lib, oracle, n_barcodes=300, lanes=1):
    names, contigs, rs, kw, kinds, do_rfa = part3_case(n_barcodes)()
    _, ores = check(lib, oracle, names, contigs, rs, kw, do_rfa=do_rfa, lanes=lanes, dump=False)
    return cover_part3(ores, rs, do_rfa)


def check_mixed_batches(lib, oracle):
    """the feature reads, a batch of unique reads with junk, the feature reads again on ONE context: no mark or list length of the batch before may survive"""
    names, contigs, rs, kw, _ = part1_case()()
    oidx = oracle.index_build_naive(names, contigs)
    plain, _ = feature_reads(contigs[0], [["exact"] * 6 + ["junk"] * 2, ["mismatch_end"] * 3], seed=31)
    ctx = lib.index_from_arrays(oidx.arrays()).context(max(rs.n_pairs, plain.n_pairs))
    for x in (rs, plain, rs):
        b = helpers.batch_of(x)
        helpers.assert_same_result(ctx.align_barcodes(b, lib.opts(**kw)), oidx.align_barcodes(b, oracle.opts(**kw)), inference=True)
