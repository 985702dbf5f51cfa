"""The inputs of test_emu_rfa_small.py and test_gpu_rfa_small.py and what each case asserts.  K8's barcode program has two instances (k_rfa.h): the regular one
keeps every table in its HBM slab, the small one (barcodes of up to LH_RFA_SM_NC candidates and LH_RFA_SM_NR reads, k_rfa_order's third class) keeps the tables
the optimizer and the probability sums walk in LDS, and hands a barcode with more than LH_RFA_SM_M molecules to the regular one.  Every case is held to the oracle
and, byte for byte, to the same batch with every barcode in the regular instance (LH_F_RFA_SLAB).

Which class a barcode falls in is computed from the oracle's result alone (candidates and reads per barcode, molecules = the molecule ids it hands out)."""
import numpy as np

import helpers
import tail_pass_cases as tp
from lariat_amd import capi, synth

DEFAULT_CAPS = dict(nr=256, nc=512, m=128)   # LH_RFA_SM_NR, LH_RFA_SM_NC, LH_RFA_SM_M as shipped
TINY_CAPS = dict(nr=8, nc=12, m=4)           # the `tiny` test build
TINY_DEFINES = ["-DLH_RFA_SM_NR=8", "-DLH_RFA_SM_NC=12", "-DLH_RFA_SM_M=4"]


def assert_same_bytes(got, old):
    for f in tp.RESULT_COLUMNS:
        a, b = getattr(got, f), getattr(old, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "result column %s differs between the two instances (LH_F_RFA_SLAB)" % f
    assert got.counters == old.counters, (got.counters, old.counters)


def shape_of(ores, bc_pair_off):
    """per barcode: reads, candidates, molecules (the oracle's)"""
    out = []
    for b in range(len(bc_pair_off) - 1):
        r0, r1 = 2 * int(bc_pair_off[b]), 2 * int(bc_pair_off[b + 1])
        c0, c1 = int(ores.cand_off[r0]), int(ores.cand_off[r1])
        mid = ores.molecule_id[c0:c1]
        out.append((r1 - r0, c1 - c0, int(mid.max()) + 1 if len(mid) and mid.max() >= 0 else 0))
    return out


def expected_classes(shapes, caps, do_rfa=None):
    """what k_rfa_order and the small instance must report (Context.rfa_classes) for barcodes of these shapes in a context whose slabs hold the small instance's carve:
    small = the barcodes within the caps, listed only where at most an eighth of the batch is beyond them; turned away = those of them with more molecules than the cap"""
    fits = [s for s in shapes if s[0] <= caps["nr"] and s[1] <= caps["nc"]]
    split = 8 * (len(shapes) - len(fits)) <= len(shapes)
    return dict(small=len(fits) if split else 0, turned_away=sum(s[2] > caps["m"] for s in fits) if split else 0)


PAD = [["exact"]] * 14   # one-pair barcodes that keep a batch's barcodes beyond the caps (two in the cases below) at an eighth of it


def check(lib, oracle, names, contigs, rs, caps, do_rfa=None, ctx_kw=None, flags=0):
    """the batch against the oracle and against itself under LH_F_RFA_SLAB, on one context, and which instance took how many barcodes; returns the oracle's result and
    the barcodes' shapes"""
    oidx = oracle.index_build_naive(names, contigs)
    b = capi.Batch.from_arrays(rs.seq, rs.seq_off, rs.bc_pair_off, rs.name_seed, bc_do_rfa=do_rfa)
    ctx = lib.index_from_arrays(oidx.arrays()).context(max(rs.n_pairs, 4), **(ctx_kw or {}))
    ores = oidx.align_barcodes(b, oracle.opts(), threads=8)
    got = ctx.align_barcodes(b, lib.opts(flags=flags))
    cls = ctx.rfa_classes()
    helpers.assert_same_result(got, ores, inference=True)
    shapes = shape_of(ores, rs.bc_pair_off)
    want = expected_classes(shapes, caps)
    if do_rfa is not None:   # (a barcode without inference has no molecules: it is never turned away)
        want["turned_away"] = expected_classes([s for s, d in zip(shapes, do_rfa) if d], caps)["turned_away"] if want["small"] else 0
    assert cls["small"] == want["small"] and cls["turned_away"] == want["turned_away"] and cls["big"] + cls["rest"] + cls["small"] == len(shapes), (cls, want, shapes)
    slab = ctx.align_barcodes(b, lib.opts(flags=flags | capi.LH_F_RFA_SLAB))
    cls_slab = ctx.rfa_classes()
    assert cls_slab["small"] == 0 and cls_slab["turned_away"] == 0, cls_slab
    helpers.assert_same_result(slab, ores, inference=True)
    assert_same_bytes(got, slab)
    again = ctx.align_barcodes(b, lib.opts(flags=flags))   # (the lists and counters of the run before must not survive)
    assert ctx.rfa_classes() == cls
    assert_same_bytes(again, got)
    return ores, shapes, cls


# ---- candidates and reads at the caps.  Pairs on the planted units of tail_pass_cases.feature_genome: "exact" and "junk" give 2 candidates a pair, "copies2" 4,
# "copies3" 6; "odd3" (read 1 in the two-copy unit, its mate on unique sequence behind the first copy) an odd number
def _odd_pair(g):
    at = tp.AT2[0]
    return g[at + 250:at + 400].copy(), tp._rc(g[at + 500:at + 650])


def feature_reads(g, kinds_per_barcode, seed=23):
    rs, kinds = tp.feature_reads(g, [[k if k != "odd3" else "exact" for k in bc] for bc in kinds_per_barcode], seed=seed)
    reads = [rs.seq[rs.seq_off[i]:rs.seq_off[i + 1]].copy() for i in range(len(rs.seq_off) - 1)]
    p = 0
    for bc in kinds_per_barcode:
        for k in bc:
            if k == "odd3":
                reads[2 * p], reads[2 * p + 1] = _odd_pair(g)
            p += 1
    return tp._read_set(reads, rs.names, rs.bc_pair_off)


# (barcodes whose reads are at cap - 2, cap, cap + 2 — a barcode holds whole pairs — with few candidates, and barcodes of cap - 1, cap, cap + 1 candidates in fewer
# reads than the cap: the mix of kinds comes from the oracle's counts per kind, and cover_caps asserts what came out)
def kind_counts(oracle):
    """candidates per pair of each kind, measured on the oracle: one barcode per kind"""
    names, contigs = tp.feature_genome()
    kinds = ["exact", "junk", "copies2", "copies3", "odd3"]
    rs = feature_reads(contigs[0], [[k] for k in kinds])
    oidx = oracle.index_build_naive(names, contigs)
    ores = oidx.align_barcodes(helpers.batch_of(rs), oracle.opts())
    return {k: s[1] for k, s in zip(kinds, shape_of(ores, rs.bc_pair_off))}


def mix_for(target, per, max_pairs):
    """kinds of one barcode with `target` candidates in at most max_pairs pairs (most candidates per pair first; None: not reachable)"""
    order = sorted(per, key=lambda k: -per[k])
    best = None

    def rec(i, left, acc):
        nonlocal best
        if best is not None:
            return
        if left == 0:
            best = list(acc)
            return
        if i == len(order) or len(acc) >= max_pairs:
            return
        k = order[i]
        top = min(left // per[k], max_pairs - len(acc))
        for n in range(top, max(-1, top - 3), -1):   # (greedy with a little slack: the last few pairs fix the remainder)
            rec(i + 1, left - n * per[k], acc + [k] * n)
    rec(0, target, [])
    return best


def caps_barcodes(per, caps):
    bcs = []
    for pairs in (caps["nr"] // 2 - 1, caps["nr"] // 2, caps["nr"] // 2 + 1):   # reads at the cap, candidates below theirs
        bcs.append(["exact"] * pairs)
    for nc in (caps["nc"] - 1, caps["nc"], caps["nc"] + 1):
        mix = mix_for(nc, per, caps["nr"] // 2 - 1)
        assert mix is not None, ("no mix of pairs with %d candidates" % nc, per)
        bcs.append(mix)
    return bcs


def cover_caps(shapes, caps):
    nrs = {s[0] for s in shapes if s[1] <= caps["nc"]}
    ncs = {s[1] for s in shapes if s[0] <= caps["nr"]}
    assert {caps["nr"] - 2, caps["nr"], caps["nr"] + 2} <= nrs, (sorted(nrs), caps)
    assert {caps["nc"] - 1, caps["nc"], caps["nc"] + 1} <= ncs, (sorted(ncs), caps)
    return dict(reads=sorted(nrs), candidates=sorted(ncs))


def check_caps(lib, oracle, caps):
    names, contigs = tp.feature_genome()
    per = kind_counts(oracle)
    assert per["odd3"] % 2 == 1 and per["exact"] == 2, per
    rs = feature_reads(contigs[0], caps_barcodes(per, caps) + PAD)
    _, shapes, cls = check(lib, oracle, names, contigs, rs, caps)
    assert cls["small"] == len(shapes) - 2, (cls, shapes)   # (all but the barcode of cap + 2 reads and the one of cap + 1 candidates)
    return dict(cover_caps(shapes, caps), classes=cls)


# ---- small barcodes of the usual kind: a few molecules each, reads without a region, one barcode without inference, a barcode of one pair
def usual_case(n_barcodes=5, pairs=40, seed=5):
    names, contigs = helpers.small_genome()
    rs = helpers.small_reads(names, contigs, n_barcodes=n_barcodes, pairs=pairs, seed=seed, junk=0.05)
    one = synth.make_reads(contigs, names, n_barcodes=1, pairs_per_barcode=1, seed=seed + 1, junk_frac=0.0)
    rs = join_read_sets([rs, one])
    do_rfa = np.ones(len(rs.bc_pair_off) - 1, dtype=np.uint8)
    do_rfa[1] = 0
    return names, contigs, rs, do_rfa


def join_read_sets(sets):
    reads, names, off = [], [], [0]
    for rs in sets:
        reads += [rs.seq[rs.seq_off[i]:rs.seq_off[i + 1]] for i in range(len(rs.seq_off) - 1)]
        off += [len(names) + int(x) for x in rs.bc_pair_off[1:]]
        names += list(rs.names)
    out = tp._read_set(reads, names, off)
    out.name_seed = np.concatenate([rs.name_seed for rs in sets])
    return out


def check_usual(lib, oracle, caps, **kw):
    names, contigs, rs, do_rfa = usual_case(**kw)
    ores, shapes, cls = check(lib, oracle, names, contigs, rs, caps, do_rfa=do_rfa)
    n_cand = np.diff(ores.cand_off)
    placeholders = int(((n_cand == 1) & (ores.rid[ores.cand_off[:-1]] < 0)).sum())
    assert placeholders > 0, "no read without a region"
    assert shapes[-1][0] == 2, shapes
    small = [s for s in shapes if s[0] <= caps["nr"] and s[1] <= caps["nc"]]
    return dict(placeholders=placeholders, shapes=shapes, within_caps=len(small), classes=cls)


# ---- molecules beyond the on-chip tables: known only inside the program.  A molecule needs an active alignment and a read has one, so a barcode within the read cap
# exceeds the molecule cap only where mates lie apart: every pair here has its reads on two different short contigs, two molecules a pair (the 140-molecule barcode
# of test_emu_front.py is the model: a molecule per contig)
def chimeric_case(n_pairs, seed=8):
    rng = np.random.default_rng(seed)
    contigs = [rng.integers(0, 4, size=1000).astype(np.uint8) for _ in range(2 * n_pairs + 2)]
    names = ["u%03d" % i for i in range(len(contigs))]
    reads, rn = [], []
    for p in range(n_pairs):
        reads += [contigs[2 * p][100:250].copy(), tp._rc(contigs[2 * p + 1][300:450])]
        rn.append("chim:%d" % p)
    usual = [contigs[-1][50:200].copy(), tp._rc(contigs[-1][400:550]), contigs[-2][60:210].copy(), tp._rc(contigs[-2][380:530])]   # a barcode of two ordinary pairs in front
    return names, contigs, tp._read_set(usual + reads, ["u:0", "u:1"] + rn, [0, 2, 2 + n_pairs])


def check_molecules(lib, oracle, caps, n_pairs):
    names, contigs, rs = chimeric_case(n_pairs)
    _, shapes, cls = check(lib, oracle, names, contigs, rs, caps)
    assert shapes[1][0] <= caps["nr"] and shapes[1][1] <= caps["nc"] and shapes[1][2] > caps["m"], (shapes, caps)
    assert shapes[0][0] <= caps["nr"] and 0 < shapes[0][2] <= caps["m"], (shapes, caps)
    assert cls == dict(big=0, rest=0, small=2, turned_away=1), cls
    return dict(shapes=shapes, classes=cls)


# ---- the three classes in one batch, by candidates: with a slab of slab_kb the barcode `big` cannot fit (a lower bound of what k_rfa_order adds up exceeds it: routed
# to the tiers), `rest` is beyond the small caps and fits, the others are small
def check_mixed(lib, oracle, caps, slab_kb, small, big, rest):
    names, contigs = tp.feature_genome()
    rs = feature_reads(contigs[0], [small, big, rest, small[:max(1, len(small) // 2)], ["exact"]] + PAD)
    _, shapes, cls = check(lib, oracle, names, contigs, rs, caps, ctx_kw=dict(rfa_slab_kb=slab_kb, rfa_tier_kb=(8 * slab_kb, 64 * slab_kb)))
    assert cls == dict(big=1, rest=1, small=len(shapes) - 2, turned_away=0), (cls, shapes)
    slab = slab_kb << 10
    upper = lambda s: 120 * s[1] + 116 * s[0] + 31 * 1024 + s[0] * s[0]   # above rfa_carve_bytes + nR^2 for an index of one contig
    lower = lambda s: 96 * s[1] + 30 * 1024 + s[0] * s[0]   # below it: 96 bytes of tables a candidate, the sort stacks
    assert lower(shapes[1]) > slab, (shapes, "the large barcode fits the slab")
    assert (shapes[2][0] > caps["nr"] or shapes[2][1] > caps["nc"]) and upper(shapes[2]) < slab, shapes
    assert all(shapes[i][0] <= caps["nr"] and shapes[i][1] <= caps["nc"] and upper(shapes[i]) < slab for i in (0, 3, 4)), shapes
    return dict(shapes=shapes[:5], classes=cls)


# ---- a pair heavy enough for k_rfa_tag_w (more than LH_RFA_TAG_WAVE = 128 combinations): both reads inside the twelve-copy unit
def check_heavy_pair(lib, oracle, caps):
    names, contigs = tp.feature_genome()
    rs, _ = tp.feature_reads(contigs[0], [["copies12", "exact", "exact"], ["exact", "copies12"]])
    ores, shapes, cls = check(lib, oracle, names, contigs, rs, caps)
    n = np.diff(ores.cand_off)
    in_f = np.add.reduceat(ores.in_filtered.astype(np.int64), ores.cand_off[:-1]) if hasattr(ores, "in_filtered") else n
    comb = in_f[0::2] * in_f[1::2]
    assert comb.max() > 128, comb
    return dict(combinations=int(comb.max()), shapes=shapes)
