"""The inputs of test_emu_lock_tail.py and test_gpu_lock_tail.py and what each case asserts.  Behind K1's pass 1 one lockstep kernel (k_p23_lock, k_smem4.h) judges
pass 2's re-seeding calls AND makes pass 3's walks, from one scan of the read's pass-1 intervals; pass 2 then appends behind pass 3's intervals, every interval that
gets a slot adding its occurrences to the read's count word, and k_p2_close clamps, finishes the count and lists the reads k_smem_fin must sort (more than 16
intervals, or one above max_occ).  LH_F_P3_LAST keeps the sequence before it: k_p2_probe, pass 2, k_p2_clamp, k_smem_p3_lock.

Every case runs its whole batch under both sequences and compares byte for byte: the stage dump (sorted intervals, the seeds whose offsets are the reads' seed
counts, and on), every result column, every work counter (n_ext, n_ext_exec_p3 and n_ktree_p3 among them: the final walk is not pruned), and k_smem_fin's list as a
set; and both against the oracle.  What a batch is FOR is asserted from the oracle alone (coverage below), so that no case passes empty: the oracle's stage dump
with pass 2 switched off (split_factor beyond every read), with pass 3 switched off (max_mem_intv = 0) and with both off gives every read's number of intervals
per pass, and which intervals each pass emitted."""
import numpy as np

import helpers
import p2_probe_cases as p2c
import tail_pass_cases as tp
from lariat_amd import capi

K = 19           # LH_BLOOM_K and lh_opts_init's min_seed_len
LW = K + 1       # pass 3's shortest seed
RLEN = 150
GLEN = 200000
DEST0 = 130000   # planted copies live behind this position; reads are taken in front of it
FIN = 16         # K2 ranks a read of at most this many intervals itself
NO_P2 = dict(split_factor=100.0)
NO_P3 = dict(max_mem_intv=0)


# ------------------------------------------------------------------------------------------------ genomes and reads
def _flip(read, at):
    read = read.copy()
    for a in at:
        read[a] ^= 1
    return read


def _with_n(read, at):
    read = read.copy()
    for a in at:
        read[a] = 4
    return read


_built = {}


def _unique_sets():
    """one random contig with planted 19-mers: the cases on unique sequence"""
    rng = np.random.default_rng(20261020)
    g = rng.integers(0, 4, size=GLEN).astype(np.uint8)
    state = dict(locus=3000, dest=DEST0)
    todo = {}

    def locus(span=RLEN):
        p = state["locus"]
        state["locus"] = p + span + 250
        assert state["locus"] < DEST0 - 1000
        return p

    def plant(src, n=K):
        d = state["dest"]
        g[d:d + n] = g[src:src + n]
        state["dest"] = d + n + 131
        assert state["dest"] < GLEN - 1000

    def add(case, p, make, mate=True):
        todo.setdefault(case, []).append((p, make, mate))

    # walks: error-free reads of every length from 131 to 150 (143 and 150 among them).  Pass 3's walks start at 0, 20, 40 ...: the last one starts at
    # x = 20 * ((len - 1) // 20) and can emit iff x + 19 < len — at len 140 it starts exactly at len - min_seed_len - 1 and emits with the read's last base, at 139 it
    # starts a base later in the read's terms (x = 120 = len - 19) and cannot; one of the lengths has x + ktree_levels == len whatever the index's levels (<= 19)
    for n in range(131, RLEN + 1):
        p = locus()
        add("walks", p, lambda g, p=p, n=n: g[p:p + n].copy())
    # subs: 0, 1, 2 and 3 substitutions: one, two, three and four unique SMEMs of at least 36 bases (pass 3 keeps the two longest: the third and the fourth are walked
    # through the tables)
    for at in ((), (75,), (50, 101), (37, 74, 112), (36, 75, 112), (40, 78, 114)):
        for _ in range(3):
            p = locus()
            add("subs", p, lambda g, p=p, at=at: _flip(g[p:p + RLEN], at))
    # odd: an N at the first, at the last and at an inner base of what would be one unique SMEM; reads shorter than min_seed_len; empty reads
    for at in ((0,), (RLEN - 1,), (75,), (0, RLEN - 1), (19,), (RLEN - 20,)):
        p = locus()
        add("odd", p, lambda g, p=p, at=at: _with_n(g[p:p + RLEN], at))
    for n in (11, 18, 19, 20, 0):
        p = locus()
        add("odd", p, lambda g, p=p, n=n: g[p:p + n].copy(), mate=n > 0)
    # fin: reads of 250 bases with an N at 40, 81, 122 ...: the walk that meets an N ends there and the next starts behind it, so pass 3 emits 12 intervals whatever the
    # number of Ns (a substitution costs a whole walk), and pass 1 one interval per segment; a planted 19-mer in the middle of a segment is a listed call of pass 2
    # that emits one more.  0 to 5 Ns and 0 to 3 planted 19-mers: totals of 13 to 21, those of 16 and 17 made without pass 2, by pass 2 on top of fewer than 16, and
    # by pass 2 behind a pass 3 that reached 16
    for n_n in range(6):
        for n_plant in range(min(3, n_n + 1) + 1):
            for _ in range(3):
                p = locus(span=250)
                at = [40 + 41 * j for j in range(n_n)]
                edges = [-1] + at + [250]
                for j in range(n_plant):
                    plant(p + ((edges[j] + 1 + edges[j + 1]) >> 1) - 9)
                add("fin", p, lambda g, p=p, at=at: _with_n(g[p:p + 250], at), mate=False)
    # short: for slots of four intervals (the emulator's small build).  60 bases: one interval of pass 1 and three of pass 3 fill the slots, and a planted 19-mer's
    # interval of pass 2 finds none; 150 bases: pass 3 alone overflows
    for i in range(12):
        p = locus()
        if i % 2 == 0:
            plant(p + 30 - 9)
        add("short", p, lambda g, p=p, i=i: g[p:p + (60 if i < 8 else RLEN)].copy())
    sets = {}
    for case, items in todo.items():
        reads = []
        for p, make, mate in items:
            r1 = make(g)
            reads += [r1, tp._rc(g[p + 230:p + 230 + 143]) if mate else g[p:p].copy()]
        sets[case] = reads
    return ["chrU"], [g], sets


def _repeat_sets():
    """two contigs of exact copies of a unit, 15 and 25 of them: reads that begin in the unique spacer before a copy and end inside it, run with max_occ = 10.
    15 copies: pass 3's 20-mers inside the unit occur 15 times — fewer than max_mem_intv = 20, so they are emitted, and more than max_occ.  25 copies: pass 3's walks
    inside the unit never come below 20 occurrences, and pass 2's call from the middle of the read (one unique SMEM) returns the longest match there that occurs
    twice: the read's part of the unit, 25 occurrences, because the base before the reads' copies is given to no other copy.  The coverage says which reads have which"""
    _, c15, unit, spacer = helpers.exact_repeat_genome(copies=15, unit=300, spacer=400, seed=31)
    _, c25, _, _ = helpers.exact_repeat_genome(copies=25, unit=300, spacer=400, seed=32)
    g25 = c25[0]
    for copy in range(25):
        g25[copy * (unit + spacer) + spacer - 1] = {2: 1, 5: 2, 9: 3}.get(copy, 0)
    reads = []
    for g in (c15[0], g25):
        for copy in (2, 5, 9):
            for inside in (50, 60, 75, 90):
                base = copy * (unit + spacer) + spacer   # the copy's first base
                reads += [g[base - (RLEN - inside):base + inside].copy(), tp._rc(g[base + 100:base + 243])]
    tail = c15[0][-15000:]
    for i in range(6):   # and plain unique pairs
        reads += [tail[500 + 700 * i:650 + 700 * i].copy(), tp._rc(tail[800 + 700 * i:943 + 700 * i])]
    return ["chrR15", "chrR25"], [c15[0], g25], {"rep": reads}


def _low_sets():
    """low-complexity sequence with substitutions and indels, seeded from 8 bases on (seed_group_cases.low_complexity_case): dozens to hundreds of intervals per read"""
    from lariat_amd import synth
    names, contigs = helpers.low_complexity_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=24, seed=3, sub_lo=0.002, sub_hi=0.03, indel_rate=0.002, mol_min=2, mol_max=3)
    return names, contigs, {"low": rs}


def _family_sets():
    """repeat families (tens of chains per read), and on the same genome four reads with a substitution every 30 bases: five SMEMs of 29 or 30 bases, five calls the
    probe cannot judge — more than LH_P2_SPLIT: listed as shares"""
    names, contigs, rs = helpers.repeat_family_case(5, 2, pairs=40)
    reads = [rs.seq[rs.seq_off[i]:rs.seq_off[i + 1]].copy() for i in range(len(rs.seq_off) - 1)]
    g = contigs[0]
    for i in range(4):
        p = 300000 + 1000 * i
        reads += [_flip(g[p:p + RLEN], (29, 59, 89, 119)), tp._rc(g[p + 230:p + 373])]
    return names, contigs, {"family": reads}


GENOMES = {"unique": _unique_sets, "repeat": _repeat_sets, "low": _low_sets, "family": _family_sets}
CASE_GENOME = {"walks": "unique", "subs": "unique", "odd": "unique", "fin": "unique", "short": "unique", "rep": "repeat", "low": "low", "family": "family"}
CASE_OPTS = {"rep": dict(max_occ=10), "low": dict(min_seed_len=8)}


def genome(name):
    if name not in _built:
        _built[name] = GENOMES[name]()
    return _built[name]


def read_set(reads, n_barcodes=2):
    if not isinstance(reads, list):
        return reads
    n_pairs = len(reads) // 2
    cut = sorted(set([0, n_pairs] + [n_pairs * b // n_barcodes for b in range(1, n_barcodes)]))
    return tp._read_set(reads, ["lt:%d" % i for i in range(n_pairs)], cut)


# ------------------------------------------------------------------------------------------------ the oracle's side
_oracle = {}


def oracle_index(oracle, gname):
    if ("idx", gname) not in _oracle:
        names, contigs, _ = genome(gname)
        _oracle[("idx", gname)] = oracle.index_build_naive(names, contigs)
    return _oracle[("idx", gname)]


def _keys(d, r):
    """a read's intervals as a sorted list of (info, occurrences)"""
    iv = d.intv[d.intv_off[r]:d.intv_off[r + 1]]
    return sorted((int(iv[i, 3]), int(iv[i, 2])) for i in range(len(iv)))


def _minus(a, b):
    b = list(b)
    out = []
    for k in a:
        if k in b:
            b.remove(k)
        else:
            out.append(k)
    return out


def oracle_side(oracle, case):
    """read set, batch, the oracle's stage dump and result, and per read the intervals (info, occurrences) of pass 1, pass 2 and pass 3"""
    if case not in _oracle:
        gname = CASE_GENOME[case]
        idx = oracle_index(oracle, gname)
        rs = read_set(genome(gname)[2][case])
        b = helpers.batch_of(rs)
        kw = CASE_OPTS.get(case, {})
        want = idx.stage_dump(b, oracle.opts(**kw))
        no2 = idx.stage_dump(b, oracle.opts(**dict(kw, **NO_P2)))
        no3 = idx.stage_dump(b, oracle.opts(**dict(kw, **NO_P3)))
        only1 = idx.stage_dump(b, oracle.opts(**dict(kw, **NO_P2, **NO_P3)))
        per = []
        for r in range(len(rs.seq_off) - 1):
            p1 = _keys(only1, r)
            p2, p3 = _minus(_keys(no3, r), p1), _minus(_keys(no2, r), p1)
            assert sorted(p1 + p2 + p3) == _keys(want, r), "read %d: the passes' intervals do not add up" % r
            per.append((p1, p2, p3))
        _oracle[case] = (rs, b, want, idx.align_barcodes(b, oracle.opts(**kw)), per)
    return _oracle[case]


# ------------------------------------------------------------------------------------------------ coverage, from the oracle alone
def _len(info):
    return (info & 0xffffffff) - (info >> 32)


def cover(case, rs, per, max_intv, max_occ=500):
    n = [(len(a), len(b), len(c)) for a, b, c in per]
    tot = [sum(x) for x in n]
    lens = np.diff(rs.seq_off)
    if case == "walks":
        assert sorted(set(lens[0::2].tolist())) == list(range(131, RLEN + 1)) and (lens[1::2] == 143).all()
        for r in range(0, len(per), 2):   # one unique SMEM; a 20-mer every 20 bases while 20 bases are left
            assert n[r][0] == 1 and n[r][2] == lens[r] // LW, (r, n[r], lens[r])
    if case == "subs":
        uniq = [sum(1 for info, occ in a if occ == 1 and _len(info) > LW) for a, _, _ in per]
        assert set(uniq[0::2]) == {1, 2, 3, 4}, uniq
        third = [sorted((_len(info) for info, occ in a if occ == 1), reverse=True)[2] for a, _, _ in per if len(a) >= 3]
        assert third and min(third) > LW + 1, third
    if case == "odd":
        assert (lens == 0).sum() >= 2 and ((lens > 0) & (lens < K)).sum() >= 2 and (np.array(tot)[lens < K] == 0).all()
        first = [rs.seq[rs.seq_off[r]] == 4 for r in range(len(lens)) if lens[r]]
        last = [rs.seq[rs.seq_off[r + 1] - 1] == 4 for r in range(len(lens)) if lens[r]]
        assert any(first) and any(last)
    if case == "fin":
        kinds = set()
        for (n1, n2, n3), t in zip(n, tot):
            if t in (FIN, FIN + 1):
                kinds.add((t, "p3" if n2 == 0 else "p2" if n1 + n3 < FIN else "both"))
        # 16 and 17 intervals: without an interval of pass 2; with pass 2's intervals taking the count to and over the threshold (pass 1 + pass 3 stay below 16);
        # pass 3 reaching 16 and pass 2 adding the 17th
        want = {(FIN, "p3"), (FIN + 1, "p3"), (FIN, "p2"), (FIN + 1, "p2"), (FIN + 1, "both")}
        assert want <= kinds, (sorted(want - kinds), sorted(set(tot)))
    if case == "rep":
        p2_only = [r for r, (a, b, c) in enumerate(per) if any(o > max_occ for _, o in b) and not any(o > max_occ for _, o in a + c)]
        p3_only = [r for r, (a, b, c) in enumerate(per) if any(o > max_occ for _, o in c) and not any(o > max_occ for _, o in a + b)]
        assert p2_only and p3_only, (p2_only, p3_only)
    if case in ("short", "low"):
        by_p2 = [r for r, (n1, n2, n3) in enumerate(n) if n1 <= max_intv and n1 + n3 <= max_intv < n1 + n3 + n2]
        by_p3 = [r for r, (n1, n2, n3) in enumerate(n) if n1 <= max_intv and n1 + n2 <= max_intv < n1 + n3 + n2]
        assert by_p2 and by_p3, (by_p2, by_p3, n)
    return n, tot


def expected_fin(per, max_intv, max_occ):
    """the reads k_smem_fin is given: more than 16 intervals in the regular slots, or one above max_occ (reads beyond their slots may or may not be listed: they
    are sorted in the big slab) -> (must be listed, may be listed)"""
    must, may = set(), set()
    for r, (a, b, c) in enumerate(per):
        t = len(a) + len(b) + len(c)
        if t > max_intv:
            may.add(r)
        elif t > FIN or any(o > max_occ for _, o in a + b + c):
            must.add(r)
    return must, may


# ------------------------------------------------------------------------------------------------ the checks
_lib_idx = {}


def lib_index(lib, oracle, gname):
    if (lib.path, gname) not in _lib_idx:
        _lib_idx[(lib.path, gname)] = lib.index_from_arrays(oracle_index(oracle, gname).arrays())
    return _lib_idx[(lib.path, gname)]


ALL_DUMP = [n for n, _, _, _ in capi._DUMP_FIELDS]


def check_case(lib, oracle, case, max_intv=64, flags=0, kw=None, covered=True):
    """every read of the batch: the default sequence against LH_F_P3_LAST and both against the oracle.  flags / kw: set in every run"""
    rs, b, want, ores, per = oracle_side(oracle, case)
    okw = dict(CASE_OPTS.get(case, {}), **(kw or {}))
    assert not kw or not covered, "other options: the oracle's side is the case's own"
    max_occ = okw.get("max_occ", 500)
    if covered:
        cover(case, rs, per, max_intv, max_occ)
    ctx = lib_index(lib, oracle, CASE_GENOME[case]).context(max(rs.n_pairs, 4))
    new_dump = ctx.stage_dump(b, lib.opts(flags=flags, **okw))
    new_fin = set(ctx.fin_list().tolist())
    old_dump = ctx.stage_dump(b, lib.opts(flags=flags | capi.LH_F_P3_LAST, **okw))
    old_fin = set(ctx.fin_list().tolist())
    helpers.assert_same_dump(new_dump, old_dump, ALL_DUMP)
    if not kw:
        helpers.assert_same_dump(new_dump, want, helpers.DUMP_FRONT)
    must, may = expected_fin(per, max_intv, max_occ)
    if not kw and not flags & capi.LH_F_SEED_LANE:
        assert must <= new_fin <= must | may, (sorted(must - new_fin), sorted(new_fin - must - may))
    assert new_fin - may == old_fin - may, (sorted(new_fin ^ old_fin), sorted(may))
    new = ctx.align_barcodes(b, lib.opts(flags=flags, **okw))
    assert set(ctx.fin_list().tolist()) - may == new_fin - may
    old = ctx.align_barcodes(b, lib.opts(flags=flags | capi.LH_F_P3_LAST, **okw))
    p2c.assert_same_bytes(new, old, "the default sequence and LH_F_P3_LAST")   # (every counter too: n_ext, n_ext_exec_p3, n_ktree_p3)
    if not kw:
        helpers.assert_same_result(new, ores, inference=True)
    again = ctx.align_barcodes(b, lib.opts(flags=flags, **okw))   # (nothing of the run before may survive: the list, the count words)
    p2c.assert_same_bytes(again, new, "two runs of one batch")
    return ctx, new


def check_too_long(lib, oracle):
    """a read beyond LH_MAX_READ_LEN is refused with LH_E_LIMIT under both sequences"""
    import pytest
    _, contigs, sets = genome("unique")
    reads = [r.copy() for r in sets["subs"][:6]]
    reads[2] = contigs[0][90000:90251].copy()
    rs = read_set(reads, 1)
    ctx = lib_index(lib, oracle, "unique").context(4)
    for flags in (0, capi.LH_F_P3_LAST):
        with pytest.raises(capi.LhError) as e:
            ctx.align_barcodes(helpers.batch_of(rs), lib.opts(flags=flags))
        assert e.value.code == capi.LH_E_LIMIT, (flags, e.value.code)


def check_other_paths(lib, oracle, case="fin"):
    """split_width = 15, LH_F_P2_SCAN, LH_F_P2_TASKS, LH_F_SEED_LANE: the sequence before this kernel runs — no lister's counts, or no list for k_smem_fin — and the
    results are the default's"""
    rs, b, want, ores, per = oracle_side(oracle, case)
    ctx = lib_index(lib, oracle, CASE_GENOME[case]).context(max(rs.n_pairs, 4))
    ref = ctx.align_barcodes(b)
    calls, fin = ctx.p2_calls(), ctx.fin_list()
    assert calls["dropped"] > 0 and len(fin) > 0, (calls, fin)
    helpers.assert_same_result(ref, ores, inference=True)
    for what, flags, kw in (("split_width", 0, dict(split_width=15)), ("scan", capi.LH_F_P2_SCAN, {}), ("tasks", capi.LH_F_P2_TASKS, {}), ("seed_lane", capi.LH_F_SEED_LANE, {})):
        got = ctx.align_barcodes(b, lib.opts(flags=flags, **kw))
        c = ctx.p2_calls()
        if what == "seed_lane":
            assert len(ctx.fin_list()) == 0, what   # k_smem_fin sorts every read: pass 3 lists none
        else:
            assert c["dropped"] == c["probed"] == c["unprobed"] == 0, (what, c)
        old = ctx.align_barcodes(b, lib.opts(flags=flags | capi.LH_F_P3_LAST, **kw))
        p2c.assert_same_bytes(got, old, what + " and LH_F_P3_LAST")
        if what != "split_width":   # (more SMEMs count as rare at split_width 15: another result, held to the flag's sequence alone)
            for f in tp.RESULT_COLUMNS:
                assert getattr(got, f).tobytes() == getattr(ref, f).tobytes(), (what, f)


def check_rounds(lib, oracle, case="fin"):
    """the batch in rounds of barcodes (seed_budget_kb): every part's k_p23_lock, pass 2 and k_p2_close have their own lists and count words"""
    rs, b, want, ores, per = oracle_side(oracle, case)
    idx = lib_index(lib, oracle, CASE_GENOME[case])
    whole = idx.context(max(rs.n_pairs, 4))
    ref = whole.align_barcodes(b)
    info = whole.rounds()
    budget = -(-int(max(info["need_bytes"] / 1.5, info["max_barcode_need_bytes"])) // 1024)
    ctx = idx.context(max(rs.n_pairs, 4), seed_budget_kb=budget)
    got = ctx.align_barcodes(b)
    assert ctx.rounds()["n_rounds"] >= 2, ctx.rounds()
    helpers.assert_same_result(got, ores, inference=True)
    old = ctx.align_barcodes(b, lib.opts(flags=capi.LH_F_P3_LAST))
    for f in tp.RESULT_COLUMNS:
        assert getattr(got, f).tobytes() == getattr(old, f).tobytes() == getattr(ref, f).tobytes(), f
    for k in ("n_ext", "n_ext_exec_p3", "n_ktree_p3"):
        assert got.counters[k] == old.counters[k], k


def check_two_lanes(lib, oracle, case="fin"):
    rs, b, want, ores, per = oracle_side(oracle, case)
    ctx = lib_index(lib, oracle, CASE_GENOME[case]).context(max(rs.n_pairs, 4), lanes=2)
    got = ctx.align_barcodes(b)
    assert ctx.rounds(1)["n_rounds"] >= 1, "the batch was not split over the lanes"
    helpers.assert_same_result(got, ores, inference=True)
    old = ctx.align_barcodes(b, lib.opts(flags=capi.LH_F_P3_LAST))
    p2c.assert_same_bytes(got, old, "two lanes: the default sequence and LH_F_P3_LAST")


def check_shares(oracle, case="family"):
    """the batch has reads with more than LH_P2_SPLIT surviving calls (share entries), by the model of p2_probe_cases.py"""
    rs, b, want, ores, per = oracle_side(oracle, case)
    tot, _ = p2c.expected_calls(want, rs, genome(CASE_GENOME[case])[1])
    assert tot["shares"] > 0, tot
    return tot
