"""The inputs of test_emu_p2_probe.py and test_gpu_p2_probe.py and what each case asserts.  K1's pass 2 re-seeds inside every long, rare SMEM of pass 1 (one bwt_smem1
call from its middle, min_intv = occurrences + 1).  k_p2_probe (k_smem4.h) judges every such call first, one thread per read: a call whose 19 middle windows lie
inside the SMEM and hold no 19-mer that occurs twice in the text is dropped, the others are listed — with the probe's bits, or unprobed where the windows are not
inside — and pass 2 runs over the list; a read with more than LH_P2_SPLIT listed calls is listed as shares.  LH_F_P2_SCAN keeps the state machine over every read.

Every case is held to the oracle (stage dump and result), to the same batch under LH_F_P2_SCAN byte for byte (work counters included), and to a model of the lister's
counts (Context.p2_calls) that knows the oracle's stage dump and the genome alone:

* pass 1's SMEMs are the read's intervals that no other interval of the read contains (what passes 2 and 3 add lies inside one of them);
* a 19-mer "occurs again" if it is found twice among the 19-mers of the text, forward strand then reverse complement.

One genome serves all cases: a random contig with planted copies.  A call's middle base cannot be ambiguous (an SMEM holds bases only), so the cases for that
branch are reads with an N where an error-free read's call would start: the SMEMs on either side are judged on their own."""
import numpy as np

import helpers
import tail_pass_cases as tp
from lariat_amd import capi

K = 19             # LH_BLOOM_K
SPLIT_LEN = 28     # (int)(min_seed_len * split_factor + .499) of lh_opts_init: 19 * 1.5
SPLIT_WIDTH = 10   # lh_opts_init's
P2_SPLIT = 4       # LH_P2_SPLIT
RLEN = 150
GLEN = 240000
DEST0 = 150000     # planted copies live behind this position; reads are taken in front of it


# ------------------------------------------------------------------------------------------------ the genome and the reads
def _flip(read, at):
    read = read.copy()
    for a in at:
        read[a] ^= 1
    return read


class _Plan:
    """loci for reads in front of DEST0, places for planted copies behind it"""

    def __init__(self, g):
        self.g, self.next_locus, self.next_dest = g, 4000, DEST0

    def locus(self, t0_mod=None, span=RLEN, gap=600):
        """the next read locus; t0_mod: (p + RLEN // 2 - (K - 1)) & 63, the bit of rep_t the probe of an error-free read of RLEN bases starts at"""
        p = self.next_locus
        if t0_mod is not None:
            while (p + RLEN // 2 - (K - 1)) & 63 != t0_mod:
                p += 1
        self.next_locus = p + span + gap
        assert self.next_locus < DEST0 - 1000
        return p

    def plant(self, src, n):
        """a copy of g[src : src + n] behind DEST0"""
        d = self.next_dest
        self.g[d:d + n] = self.g[src:src + n]
        self.next_dest = d + n + 181
        assert self.next_dest < GLEN - 1000
        return d


_built = {}


def build():
    """names, contigs, {case: (reads, first pairs of the barcodes)}.  Reads are cut after every copy is planted"""
    if _built:
        return _built["v"]
    rng = np.random.default_rng(20261019)
    g = rng.integers(0, 4, size=GLEN).astype(np.uint8)
    plan = _Plan(g)
    todo = {}   # case -> list of (locus of read 1, function of g -> read 1)

    def add(case, p, make=None, mate=True):
        todo.setdefault(case, []).append((p, make or (lambda g, p=p: g[p:p + RLEN].copy()), mate))

    # dropped: error-free reads on unique sequence
    for _ in range(20):
        add("dropped", plan.locus())
    # probed: a 19-mer, a 25-mer of the middle windows planted a second time; the set bit at the first, the last and an inner window.  Window k of a read at p
    # starts at p + 57 + k
    for n in (19, 25):
        for k in (0, 18, 9, 3):
            p = plan.locus()
            plan.plant(p + RLEN // 2 - (K - 1) + k, n)
            add("probed", p)
    # word boundaries: the first window's text position at bit 0, 63 and 46 of a word of rep_t, a planted window at either end of the 19; and the reverse strand of the
    # genome's first bases, whose SMEM ends with the text
    for mod in (0, 63, 46):
        for k in (0, 18):
            p = plan.locus(t0_mod=mod)
            plan.plant(p + RLEN // 2 - (K - 1) + k, K)
            add("words", p)
    plan.plant(65, K)
    plan.plant(300, K)
    add("words", 0, lambda g: tp._rc(g[0:RLEN]))
    add("words", 240, lambda g: tp._rc(g[240:240 + RLEN]))
    # unprobed: SMEMs of 28 to 36 bases between mismatches
    for at in ((30, 63, 96, 129), (28, 57, 94, 131), (36, 73, 110), (33, 70)):
        for _ in range(3):
            p = plan.locus()
            add("unprobed", p, lambda g, p=p, at=at: _flip(g[p:p + RLEN], at))
    # rows: a 60-mer with 2, 10 and 11 copies (each with the base before and the base behind it, so that one read base differs from every copy's neighbour); the
    # read differs from the genome right outside the copy it lies on, so that the copy is an SMEM of that many rows
    for copies in (2, 10, 11):
        src = plan.locus()
        where = [src + 45] + [plan.plant(src + 44, 62) + 1 for _ in range(copies - 1)]
        for q in (where[0], where[-1]):
            add("rows", q - 45, lambda g, q=q: _flip(g[q - 45:q - 45 + RLEN], (44, 105)))
    # odd reads: an N in the middle of an error-free read, reads shorter than min_seed_len, empty reads, a read of LH_MAX_READ_LEN bases
    for _ in range(3):
        p = plan.locus()

        def with_n(g, p=p):
            r = g[p:p + RLEN].copy()
            r[RLEN // 2] = 4
            return r
        add("odd", p, with_n)
    p = plan.locus(); add("odd", p, lambda g, p=p: g[p:p + 11].copy())
    p = plan.locus(); add("odd", p, lambda g, p=p: g[p:p + 18].copy())
    p = plan.locus(); add("odd", p, lambda g, p=p: g[p:p].copy())
    p = plan.locus(span=250); add("odd", p, lambda g, p=p: g[p:p + 250].copy(), mate=False)
    # many calls: 2, 4, 5 and 8 listed calls in a read (mismatches 29 to 37 bases apart: unprobed calls); the last is a read of 250 bases
    for at, n in (((33, 66), RLEN), ((36, 73, 110, 147), RLEN), ((29, 59, 89, 119), RLEN), ((30, 61, 92, 123, 154, 185, 216), 250)):
        for _ in range(2):
            p = plan.locus(span=n)
            add("many", p, lambda g, p=p, at=at, n=n: _flip(g[p:p + n], at), mate=n == RLEN)
    # overflow: three SMEMs of about 50 bases, a planted 19-mer in the middle of each: three intervals of pass 1 and three of pass 2 in a read
    for _ in range(4):
        p = plan.locus()
        for mid in (24, 74, 124):
            plan.plant(p + mid - 9, K)
        add("overflow", p, lambda g, p=p: _flip(g[p:p + RLEN], (49, 99)))
    # read counts: the first n reads of a batch carry a listed call (one mismatch 33 bases in: an SMEM of 33 bases), the others none
    count_loci = [plan.locus(span=450, gap=10) for _ in range(130)]
    out = {}
    for case, items in todo.items():
        reads = []
        for p, make, mate in items:
            r1 = make(g)
            r2 = tp._rc(g[p + 200:p + 200 + RLEN]) if mate else g[p + 20:p + 20].copy()
            reads += [r1, r2]
        out[case] = reads
    for n in (1, 63, 64, 65, 257):
        reads = []
        for i in range((n + 2) // 2 if n > 1 else 1):
            p = count_loci[i]
            for m in (0, 1):
                r = g[p + 300 * m:p + 300 * m + RLEN]
                reads.append(_flip(r, (33,)) if 2 * i + m < n else r.copy())
        out["count%d" % n] = reads
    _built["v"] = (["chrP"], [g], out)
    return _built["v"]


def read_set(reads, n_barcodes=2):
    n_pairs = len(reads) // 2
    cut = sorted(set([0, n_pairs] + [n_pairs * b // n_barcodes for b in range(1, n_barcodes)]))
    return tp._read_set(reads, ["p2:%d" % i for i in range(n_pairs)], cut)


# ------------------------------------------------------------------------------------------------ the model
def _kmer_codes(t):
    """the 19-mers of t as numbers; those with a base beyond 3 get distinct negative codes"""
    n = len(t) - K + 1
    code = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for j in range(K):
        code |= (t[j:j + n].astype(np.int64) & 3) << (2 * j)
        bad |= t[j:j + n] > 3
    code[bad] = -1 - np.arange(n)[bad]
    return code


_rep = {}


def repeated_kmers(contigs):
    key = id(contigs[0])
    if key not in _rep:
        fwd = np.concatenate(contigs)
        codes, cnt = np.unique(_kmer_codes(np.concatenate([fwd, tp._rc(fwd)])), return_counts=True)
        _rep[key] = set(codes[cnt > 1].tolist())
    return _rep[key]


def expected_calls(want, rs, contigs, probe=True):
    """(dropped, probed, unprobed, shares) as k_p2_probe must count them, and per read the list of (start, end, occurrences, verdict, bits)"""
    rep = repeated_kmers(contigs)
    tot = dict(dropped=0, probed=0, unprobed=0, shares=0)
    per_read = []
    for r in range(len(rs.seq_off) - 1):
        read = rs.seq[rs.seq_off[r]:rs.seq_off[r + 1]]
        iv = want.intv[want.intv_off[r]:want.intv_off[r + 1]]
        s = (iv[:, 3] >> np.uint64(32)).astype(np.int64)
        e = (iv[:, 3] & np.uint64(0xffffffff)).astype(np.int64)
        smems = sorted({(int(s[i]), int(e[i]), int(iv[i, 2])) for i in range(len(iv))
                        if not ((s <= s[i]) & (e >= e[i]) & ((s < s[i]) | (e > e[i]))).any()})
        calls, cnt = [], dict(dropped=0, probed=0, unprobed=0)
        for a, b, occ in smems:
            if b - a < SPLIT_LEN or occ > SPLIT_WIDTH:
                continue
            xm = (a + b) >> 1
            assert read[xm] <= 3
            inside = probe and xm - (K - 1) >= a and xm + K <= b
            bits = 0
            if inside:
                codes = _kmer_codes(read[xm - (K - 1):xm + K])
                bits = sum(1 << k for k in range(K) if int(codes[k]) in rep)
            verdict = "unprobed" if not inside else "probed" if bits else "dropped"
            cnt[verdict] += 1
            calls.append((a, b, occ, verdict, bits))
        if cnt["probed"] + cnt["unprobed"] > P2_SPLIT:
            tot["shares"] += 1
            cnt["probed"] = cnt["unprobed"] = 0
        for k, v in cnt.items():
            tot[k] += v
        per_read.append(calls)
    return tot, per_read


def expected_tasks(per_read):
    """under LH_F_P2_TASKS: every read with a long, rare SMEM is listed as shares, nothing is judged"""
    return dict(dropped=0, probed=0, unprobed=0, shares=sum(1 for c in per_read if c))


# ------------------------------------------------------------------------------------------------ coverage, from the model alone
def cover(case, tot, per_read, want):
    calls = [c for cs in per_read for c in cs]
    listed = [sum(c[3] != "dropped" for c in cs) for cs in per_read]
    if case == "dropped":
        assert tot == dict(dropped=len(per_read), probed=0, unprobed=0, shares=0), tot
        assert (np.diff(want.intv_off) >= 1).all()
    if case == "probed":
        bits = [c[4] for c in calls if c[3] == "probed"]
        assert any(b & 1 for b in bits) and any(b >> (K - 1) & 1 for b in bits) and any(b & 0x3fe00 and not b & 1 and not b >> (K - 1) & 1 for b in bits), [hex(b) for b in bits]
        assert any(bin(b).count("1") >= 7 for b in bits) and any(bin(b).count("1") <= 2 for b in bits), [hex(b) for b in bits]
    if case == "words":
        assert tot["probed"] >= 8, tot
    if case == "unprobed":
        assert tot["unprobed"] >= 30 and all(SPLIT_LEN <= c[1] - c[0] <= 36 for c in calls if c[3] == "unprobed"), (tot, calls)
    if case == "rows":
        occ = sorted(c[2] for c in calls if c[3] == "probed" and c[2] > 1)
        assert occ == [2, 2, 10, 10], calls
        assert (want.intv[:, 2] == 11).any()   # the 11-copy segment is an SMEM of its reads, and no call
    if case == "odd":
        n = np.diff(want.intv_off)
        assert (n == 0).sum() >= 3 and tot["dropped"] >= 6, (n, tot)
    if case == "many":
        assert sorted(set(listed)) == [0, 2, 4, 5, 8] and tot["shares"] == 4 and tot["unprobed"] == 2 * 2 + 2 * 4, (listed, tot)
    if case == "overflow":
        assert sum(k == 3 for k in listed) >= 4, listed
    if case.startswith("count"):
        n = int(case[5:])
        assert tot["unprobed"] + tot["probed"] == n and listed[:n] == [1] * n and not any(listed[n:]), (tot, listed)


# ------------------------------------------------------------------------------------------------ the checks
WORK = ("n_ext", "n_ext_exec_p2", "n_ktree_p2")


def assert_same_bytes(got, old, what):
    for f in tp.RESULT_COLUMNS:
        a, b = getattr(got, f), getattr(old, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "result column %s differs between %s" % (f, what)
    assert got.counters == old.counters, (what, {k: (v, old.counters[k]) for k, v in got.counters.items() if v != old.counters[k]})


_oracle = {}


def oracle_side(oracle, case, kw=None):
    """the oracle's index (one for all cases), and per case its stage dump and result"""
    names, contigs, sets = build()
    if "idx" not in _oracle:
        _oracle["idx"] = oracle.index_build_naive(names, contigs)
    key = (case, tuple(sorted((kw or {}).items())))
    if key not in _oracle:
        rs = read_set(sets[case])
        b = helpers.batch_of(rs)
        _oracle[key] = (rs, b, _oracle["idx"].stage_dump(b, oracle.opts(**(kw or {}))), _oracle["idx"].align_barcodes(b, oracle.opts(**(kw or {}))))
    return (_oracle["idx"],) + _oracle[key]


_lib_idx = {}


def lib_index(lib, oracle):
    if lib.path not in _lib_idx:
        build()
        oracle_side(oracle, "dropped")
        _lib_idx[lib.path] = lib.index_from_arrays(_oracle["idx"].arrays())
    return _lib_idx[lib.path]


def check_case(lib, oracle, case, flags=0, ctx_kw=None, counts=True):
    """the stage dump and the result against the oracle; the default against LH_F_P2_SCAN byte for byte; the lister's counts against the model.  flags: set in every
    run (LH_F_NO_SWEEP_FILTER, LH_F_P2_TASKS).  counts = False: a batch in lanes or rounds, whose read-out covers one part"""
    _, contigs, _ = build()
    _, rs, b, want, ores = oracle_side(oracle, case)
    filt = not flags & capi.LH_F_NO_SWEEP_FILTER
    tot, per_read = expected_calls(want, rs, contigs, probe=filt)
    if filt:
        cover(case, tot, per_read, want)
    if flags & capi.LH_F_P2_TASKS:
        tot = expected_tasks(per_read)
    ctx = lib_index(lib, oracle).context(max(rs.n_pairs, 4), **(ctx_kw or {}))
    if not ctx_kw:
        got_dump = ctx.stage_dump(b, lib.opts(flags=flags))
        if counts:
            assert ctx.p2_calls() == tot, (ctx.p2_calls(), tot)
        helpers.assert_same_dump(got_dump, want, helpers.DUMP_FRONT)
        scan_dump = ctx.stage_dump(b, lib.opts(flags=flags | capi.LH_F_P2_SCAN))
        helpers.assert_same_dump(got_dump, scan_dump, [n for n, _, _, _ in capi._DUMP_FIELDS])
    got = ctx.align_barcodes(b, lib.opts(flags=flags))
    if counts:
        assert ctx.p2_calls() == tot, (ctx.p2_calls(), tot)
    helpers.assert_same_result(got, ores, inference=True)
    if not filt:
        assert got.counters["n_ext"] == ores.counters["n_ext"], (got.counters["n_ext"], ores.counters["n_ext"])   # without the filters every bwt_extend of the reference is counted
    scan = ctx.align_barcodes(b, lib.opts(flags=(flags & ~capi.LH_F_P2_TASKS) | capi.LH_F_P2_SCAN))
    none = ctx.p2_calls()
    assert none["dropped"] == none["probed"] == none["unprobed"] == 0, none
    assert_same_bytes(got, scan, "the listed calls and LH_F_P2_SCAN")
    for k in WORK:
        assert got.counters[k] == scan.counters[k], k
    again = ctx.align_barcodes(b, lib.opts(flags=flags))   # (the list and the counts of the run before must not survive)
    if counts:
        assert ctx.p2_calls() == tot, (ctx.p2_calls(), tot)
    assert_same_bytes(again, got, "two runs of one batch")
    return ctx, tot


def check_empty_list_keeps_n_intv(lib, oracle):
    """every call dropped: pass 2 runs over an empty list, and the intervals of pass 1 (and their number) reach the dump"""
    ctx, tot = check_case(lib, oracle, "dropped")
    assert tot["probed"] + tot["unprobed"] + tot["shares"] == 0


def check_too_long(lib, oracle):
    """a read beyond LH_MAX_READ_LEN is refused with LH_E_LIMIT whichever way pass 2 runs (pass 1 flags it; no lister may lose the flag)"""
    import pytest
    _, contigs, sets = build()
    reads = [r.copy() for r in sets["unprobed"][:6]]
    reads[2] = contigs[0][90000:90251].copy()
    rs = read_set(reads, 1)
    ctx = lib_index(lib, oracle).context(4)
    for flags in (0, capi.LH_F_P2_SCAN, capi.LH_F_P2_TASKS):
        with pytest.raises(capi.LhError) as e:
            ctx.align_barcodes(helpers.batch_of(rs), lib.opts(flags=flags))
        assert e.value.code == capi.LH_E_LIMIT, (flags, e.value.code)


def check_rounds(lib, oracle, case):
    """the batch in rounds of barcodes (seed_budget_kb): every part's pass 2 has its own list"""
    _, rs, b, want, ores = oracle_side(oracle, case)
    idx = lib_index(lib, oracle)
    whole = idx.context(max(rs.n_pairs, 4))
    ref = whole.align_barcodes(b)
    info = whole.rounds()
    budget = -(-int(max(info["need_bytes"] / 1.5, info["max_barcode_need_bytes"])) // 1024)
    ctx = idx.context(max(rs.n_pairs, 4), seed_budget_kb=budget)
    got = ctx.align_barcodes(b)
    assert ctx.rounds()["n_rounds"] >= 2, ctx.rounds()
    helpers.assert_same_result(got, ores, inference=True)
    scan = ctx.align_barcodes(b, lib.opts(flags=capi.LH_F_P2_SCAN))
    for f in tp.RESULT_COLUMNS:
        assert getattr(got, f).tobytes() == getattr(scan, f).tobytes() == getattr(ref, f).tobytes(), f
    for k in WORK:
        assert got.counters[k] == scan.counters[k], k


BASE_CASES = ["dropped", "probed", "words", "unprobed", "rows", "odd", "many", "overflow"]
COUNT_CASES = ["count1", "count63", "count64", "count65", "count257"]
