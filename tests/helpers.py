"""shared helpers for the test-suite"""
import gzip
import os

import numpy as np

from lariat_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PHIX = os.path.join(GOLDEN, "phix", "PhiX.fa")

# go/src/test/gobwa_test.go:18,23
PHIX_READ_A = "TCAAAAACTGACGCGTTGGATGAGGAGAAGTGGCTTAATATGCTTGGCACGTTCGTCAAGGACTGGTTTA"
PHIX_READ_B = "TATGACCAGTGTTTCCAGTCCGTTCAGTTGTTGCAGTGGAATAGTCAGGTTAAATTTAATGTGACCGCTT"


def read_fasta(path):
    names, seqs = [], []
    for line in open(path):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            seqs.append([])
        else:
            seqs[-1].append(line.strip())
    return names, ["".join(s) for s in seqs]


def read_fastq9(path, trim):
    """minimal 9-line reader (reader.go:91-174 semantics that matter here: trim the first `trim` bases of read 1)"""
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    lines = [l.rstrip(b"\n") for l in op(path, "rb").read().split(b"\n")]
    recs = []
    for i in range(0, len(lines) - 8, 9):
        name, r1, q1, r2, q2, bc = lines[i:i + 6]
        recs.append(dict(name=name[1:].decode(), r1=r1[trim:].decode(), r2=r2.decode(), bc=bc.decode()))
    return recs


def small_genome(seed=1):
    names = ["chrA", "chrB", "chrC"]
    contigs = synth.make_genome([300000, 200000, 100000], seed=seed, n_dup=6, dup_len=5000, dup_identity=0.99, n_rep_family=2, rep_copies=20)
    return names, contigs


def small_reads(names, contigs, n_barcodes=8, pairs=40, seed=5, junk=0.02):
    return synth.make_reads(contigs, names, n_barcodes=n_barcodes, pairs_per_barcode=pairs, seed=seed, junk_frac=junk)


def batch_of(rs):
    return capi.Batch.from_arrays(rs.seq, rs.seq_off, rs.bc_pair_off, rs.name_seed)


DUMP_FRONT = ["intv_off", "intv", "seed_off", "seed_rbeg", "seed_qbeg", "seed_len", "seed_rid", "chain_off", "chain_nseeds", "chain_rid", "chain_w",
              "chain_kept", "chain_pos"]
DUMP_REGS = ["reg_off", "reg_rb", "reg_re", "reg_qb", "reg_qe", "reg_rid", "reg_score", "reg_truesc", "reg_w", "reg_seedcov", "reg_seedlen0", "reg_csub",
             "reg_secondary"]


def assert_same_dump(d, od, fields):
    for f in fields:
        a, b = getattr(d, f), getattr(od, f)
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if not (a == b).all():
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError("stage dump field %s differs at %s (got %s want %s)" % (f, bad[:5], a[bad[:3]], b[bad[:3]]))


INT_FIELDS = ["cand_off", "rid", "pos", "aend", "rb", "re", "reversed", "score", "qb", "qe", "nm", "matches", "mismatches", "indels", "soft_clipped",
              "soft_clipped_length", "in_filtered", "cigar_off", "cigar", "mm_off", "mm_ref_loc", "mm_read_loc"]
INF_FIELDS = ["active", "is_proper", "bwa_pick", "active_molecule", "duplicate", "molecule_id", "mate_idx", "active_idx", "second_best_idx", "split_idx",
              "split_mapq"]
F64_FIELDS = ["log_alignment_probability", "molecule_difference", "molecule_confidence", "sum_move_probability_change", "second_best_score", "as_score",
              "split_second_best", "split_score"]


MAPQ_ULP = 2.0 ** -52
MAPQ_ETA = 69 * MAPQ_ULP   # 1.53e-14, see mapq_reference
MAPQ_P_ONE = 1e-7           # 1 - p in (-MAPQ_P_ONE, 0) is p = 1, see mapq_reference


def _mapq_raw_decimal(score, total, sum_move, centromere, ctx):
    """min(60, -10 log10(1 - 10^score / total), -10 log10(1 - 1 / sum_move)) of three Decimals; None for NaN (a logarithm of a negative number)"""
    import decimal
    D = decimal.Decimal
    if centromere:
        return D(0)
    out = D(60)
    for one_minus in (1 - ctx.divide(ctx.power(D(10), score), total), 1 - ctx.divide(D(1), sum_move)):
        if -D(MAPQ_P_ONE) < one_minus < 0:
            one_minus = D(0)
        if one_minus < 0:
            return None
        if one_minus > 0:           # (0: -log10(0) = +Inf, the other term or the cap binds)
            out = min(out, -10 * ctx.log10(one_minus))
    return out


def _trunc_mapq(x):
    """Go's int(float64) as the product applies it: towards zero, NaN -> INT_MIN"""
    return -2 ** 31 if x is None else int(x)


def mapq_reference(terms, eta=MAPQ_ETA, screen=True):
    """What the MAPQ of every candidate must be, from the terms the oracle held when it wrote it (oracle_py.MAPQ_TERMS: pair score, total_probability,
    sum_move_probability_change, centromere), evaluated again in 50-digit decimal arithmetic:

        raw = min(60, -10 log10(1 - 10^score / total), -10 log10(1 - 1 / sum_move)),   0 inside a centromere,   mapq = int(raw)   (NaN -> INT_MIN)

    A correct double-precision implementation holds score, total and sum_move only to rounding noise, so for every candidate the closed interval of raw
    values is computed that is reachable when each of the three moves by a relative eta (raw is monotone in each: rising in score, falling in total and
    in sum_move; the ends are widened by a relative eta once more for the last logarithm).  A candidate is DECIDABLE when both ends truncate to the same
    integer (both >= 60, both in (-1, 1) and both NaN included): there the product's MAPQ must equal it.  Elsewhere it must lie between the truncations
    of the two ends.

    eta is not the contract's 1e-9 for the float scores: it is the noise of evaluating the same double-precision expressions in another order with another
    libm, counted in ulp (2^-52) with a rounded +, -, *, / at 0.5 ulp and, as no error table of the ROCm device library is at hand, the OpenCL
    double-precision bounds for the functions, which are looser: log10 3 ulp, pow 16 ulp.
      * the pair score (scoreAlignment, lariat.go:599-624): up to 8 additions of terms of one sign (4 ulp), one of them the log molecule penalty,
        log10(dnaLength / genome_length * 0.05): a division, a multiplication (1 ulp, and less after the logarithm) and the log10 (3 ulp)          8    ulp
      * total_probability: 14 additions of positive terms                                                                                    7    ulp
      * the expression itself: one pow (16), one division (0.5), one log10 (3)                                                               19.5 ulp
    34.5 ulp, times a safety factor of 2: eta = 69 ulp = 1.53e-14.  (The terms of sum_move_probability_change are pow's of sums of the same kind, summed
    in the molecules' order: the same bound.)  What this buys: Lariat's penalties are whole or half log10 units, so raw values cluster 4.3e-6 below an
    integer (-10 log10(1.000001e-6) = 59.9999957); there 1 - p ~ 1e-6 turns a relative eta' of p into 4.3e6 eta' of raw, and eta' = (|score| ln 10 + 2) eta
    is 5e-13 at a pair score of -15: the cluster stays decidable by a factor of about 8 (tests/test_mapq.py prints the smallest factor of its workload; DESIGN.md
    section 2 has the figure).  With the contract's 1e-9 in eta's place the same candidates are undecidable.

    p = 1: an alignment whose own 10^score is one of the terms of total_probability has p <= 1 in every correct implementation (the terms are positive, a
    rounded sum is not below its largest term), and p = 1 exactly when the other terms vanish beside it — every uniquely placed read.  The terms reported
    here do not say whether the own term is in the sum, and 10^score evaluated afresh may exceed the reported total by a rounding error; so 1 - p in
    (-1e-7, 0) counts as 0 (-log10(0) = +Inf: the cap or the molecule term binds).  A true NaN has 10^score above the total by a factor, not by 1e-7: the scores
    lie on a lattice of half log10 units, and eta moves p by (|score| ln 10 + 2) eta < 1e-11.

    `screen`: candidates whose interval, evaluated in double with 4096 eta in eta's place (which covers the double evaluation's own error: that is what eta
    bounds), truncates to one integer at both ends are decided there and then; only the others (those within ~1e-7 of an integer) go through decimal.
    screen=False sends all through decimal.

    Returns a dict of arrays over all candidates: `set` (the candidate went through estimateMapQualities), `lo`, `hi` (the truncated ends), `decidable`,
    `raw` (the decimal value as a float, NaN where screened or NaN), `margin` (distance of the decimal value to the next integer boundary over the
    interval's half width; Inf where screened)."""
    import decimal
    ctx = decimal.Context(prec=50)
    D = decimal.Decimal
    t = np.asarray(terms, dtype=np.float64)
    n = len(t)
    isset = t[:, 0] != 0
    lo, hi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    raw, margin = np.full(n, np.nan), np.full(n, np.inf)
    todo = isset.copy()
    if screen and n:
        w = 4096 * eta
        sc, tot, sm, cen = t[:, 1], t[:, 2], t[:, 4], t[:, 5] != 0

        def f(sc_, tot_, sm_):
            with np.errstate(all="ignore"):
                om = 1.0 - 10.0 ** sc_ / tot_
                a = -10.0 * np.log10(np.where((om < 0) & (om > -MAPQ_P_ONE), 0.0, om))
                om = 1.0 - 1.0 / sm_
                b = -10.0 * np.log10(np.where((om < 0) & (om > -MAPQ_P_ONE), 0.0, om))
                v = np.where(np.isnan(a) | np.isnan(b), np.nan, np.minimum(60.0, np.minimum(a, b)))
            return np.where(cen, 0.0, v)

        a_lo = f(sc * (1 + w), tot * (1 + w), sm * (1 + w))   # (score < 0: score (1 + w) is the lower one)
        a_hi = f(sc * (1 - w), tot * (1 - w), sm * (1 - w))
        with np.errstate(all="ignore"):
            a_lo, a_hi = a_lo - np.abs(a_lo) * w, a_hi + np.abs(a_hi) * w
            fine = isset & np.isfinite(a_lo) & np.isfinite(a_hi) & (sc <= 0) & (np.trunc(a_lo) == np.trunc(a_hi)) & (a_lo <= a_hi)
        lo[fine] = hi[fine] = np.trunc(a_lo[fine]).astype(np.int64)
        todo &= ~fine
    for i in np.nonzero(todo)[0]:
        sc, tot, sm, cen = D(float(t[i, 1])), D(float(t[i, 2])), D(float(t[i, 4])), t[i, 5] != 0
        e = D(eta)
        s_lo, s_hi = (sc * (1 + e), sc * (1 - e)) if sc < 0 else (sc * (1 - e), sc * (1 + e))
        mid = _mapq_raw_decimal(sc, tot, sm, cen, ctx)
        r_lo = _mapq_raw_decimal(s_lo, tot * (1 + e), sm * (1 + e), cen, ctx)
        r_hi = _mapq_raw_decimal(s_hi, tot * (1 - e), sm * (1 - e), cen, ctx)
        if r_lo is not None and r_lo < 60:
            r_lo -= abs(r_lo) * e
        if r_hi is not None and r_hi < 60:
            r_hi += abs(r_hi) * e
        ends = sorted([_trunc_mapq(r_lo), _trunc_mapq(r_hi), _trunc_mapq(mid)])   # (a NaN end: INT_MIN, below every value)
        lo[i], hi[i] = ends[0], ends[-1]
        if mid is not None:
            raw[i] = float(mid)
            if r_lo is not None and r_hi is not None and r_hi > r_lo and 0 < mid < 60:
                margin[i] = float(min(mid - int(mid), int(mid) + 1 - mid) / ((r_hi - r_lo) / 2))
    return dict(set=isset, lo=lo, hi=hi, decidable=isset & (lo == hi), raw=raw, margin=margin)


def assert_mapq(mapq, ref, eta=MAPQ_ETA, screen=True):
    """the product's MAPQ against the oracle result `ref` and its terms (mapq_reference): EQUAL to the reference integer wherever that is decidable, between
    the truncated ends of the interval elsewhere; the oracle's own integer is held the same way.  Returns counts: candidates compared, those whose raw value
    lies in [0.5, 60), the undecidable ones, and those of them where the product differs from the oracle."""
    m = mapq_reference(ref.mapq_terms, eta=eta, screen=screen)
    s = m["set"].copy()
    s[ref.split_idx[ref.split_idx >= 0]] = False   # a read's split alignment: CheckSplitReads wrote its MAPQ afterwards, a difference of integer scores (split.go:103-135): exact, below
    got, want = np.asarray(mapq).astype(np.int64), ref.mapq.astype(np.int64)
    assert got.shape == want.shape, ("mapq", got.shape, want.shape)
    for name, v in (("the oracle's", want), ("mapq", got)):
        bad = np.nonzero(s & ((v < m["lo"]) | (v > m["hi"])))[0]
        if len(bad):
            raise AssertionError("%s differs from the high-precision reference at %s (got %s, reference %s..%s, oracle %s, terms %s)"
                                 % (name, bad[:5], v[bad[:5]], m["lo"][bad[:5]], m["hi"][bad[:5]], want[bad[:5]], ref.mapq_terms[bad[:3]]))
    rest = np.nonzero(~s & (got != want))[0]   # (candidates that estimateMapQualities never saw keep their initial 0)
    assert not len(rest), ("mapq of a candidate outside the filtered lists", rest[:5], got[rest[:5]], want[rest[:5]])
    t = ref.mapq_terms
    mid = s & (t[:, 6] >= 0.5) & (t[:, 6] < 60)
    und = s & ~m["decidable"]
    m["margin"][~s] = np.inf
    return dict(compared=int(s.sum()), in_range=int(mid.sum()), undecidable=int(und.sum()), undecidable_in_range=int((und & mid).sum()),
                differ_undecidable=int((und & (got != want)).sum()), min_margin=float(m["margin"].min()) if s.any() else float("inf"))


def assert_same_result(r, ref, inference=True, mapq_tol=1, rel=1e-9):
    """bit-exact for integer/index fields; float scores within 1e-9 relative (BASELINE.json north_star); MAPQ: against an oracle result (one that carries
    the terms of its MAPQs, oracle_py) EXACT wherever the integer is decidable at double-precision rounding noise and inside the interval's truncated ends
    elsewhere (assert_mapq) — and within mapq_tol of the reference's in any case; a reference without terms (a second run of the product): within mapq_tol"""
    for f in INT_FIELDS + (INF_FIELDS if inference else []):
        a, b = getattr(r, f), getattr(ref, f)
        assert a.shape == b.shape, (f, a.shape, b.shape)
        if not (a == b).all():
            bad = np.nonzero(a != b)[0]
            raise AssertionError("result field %s differs at %s (got %s want %s)" % (f, bad[:5], a[bad[:5]], b[bad[:5]]))
    fl = ["log_alignment_probability"] + (F64_FIELDS[1:] if inference else [])
    for f in fl:
        a, b = getattr(r, f), getattr(ref, f)
        assert a.shape == b.shape, f
        ok = np.isclose(a, b, rtol=rel, atol=1e-12, equal_nan=True)
        assert ok.all(), (f, np.nonzero(~ok)[0][:5], a[~ok][:5], b[~ok][:5])
    if inference:
        d = np.abs(r.mapq.astype(np.int64) - ref.mapq.astype(np.int64))
        assert (d <= mapq_tol).all(), ("mapq", np.nonzero(d > mapq_tol)[0][:5])
        if getattr(ref, "mapq_terms", None) is not None:
            return assert_mapq(r.mapq, ref)


def mapq_workload(seed=31):
    """a batch whose MAPQs live between 0 and 60: reads with two to twenty near-equal placements.  Returns (names, contigs, batch, kinds) — kinds: one word per barcode.

    The genome: two random contigs with (a) six TANDEM families of 2, 3, 5, 8, 14 and 20 copies of a 900-base unit, 300 random bases between them: a family's
    copies lie within 50 kb, so a barcode's reads on them share ONE molecule and the molecule prior cancels — what is left are the copies' differences: each copy
    is 0.1 - 1.2 % off the unit (substitutions, a few one-base indels), a read sees 0 ... 3 of them per mate, and the pair scores differ by 0 ... 6 and more log10
    units; the family of 14 is nearly exact (a read on it has 14 alignments and 15 scores with the pseudo-count's); the family of 20 is nineteen exact copies and a first one with three substitutions
    290 bases apart, where most of its reads come from: a pair that covers one of them has one placement without mismatch and nineteen equal ones two log10
    units below (9.1 with the 15 largest scores summed, 8.8 with 16), more scores than are summed, and the sixteenth would move the integer;
    (b) three DISPERSED families of 4 copies of 3 kb, 70 kb and more apart at 0.2 - 0.8 %: a barcode's reads on one copy form a molecule, the other copies
    candidate molecules that the optimizer may move reads to — sum_move_probability_change is finite and the molecule term binds.
    The barcodes: `tandem` (12 pairs in one tandem family, some hanging over a unit's end into the spacer: clipped on every copy but their own, half-unit score
    differences), `dispersed` (9 pairs on one copy of a dispersed family and 3 on another), `thin` (2 pairs on a tandem family and 2 on a dispersed one: no
    molecule of more than four reads, none active), and of each a few that fail worthRunningRFA (`*_norfa`).  A fifth of the pairs carry three substitutions in
    read 2: where read 1 has two equal placements, the inactive one's score without a mate (improper, -4) beats every pair score (-6): 10^score > total, NaN.
    The centromere table covers the first tandem family (and nothing else)."""
    rng = np.random.default_rng(seed)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    contigs = [rng.choice(4, size=n, p=[0.295, 0.205, 0.205, 0.295]).astype(np.uint8) for n in (420000, 300000)]

    def mutated(unit, rate, indels):
        c = unit.copy()
        m = rng.random(len(c)) < rate
        c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        for _ in range(indels):
            at = int(rng.integers(100, len(c) - 100))
            c = np.concatenate([c[:at], c[at + 1:], rng.integers(0, 4, size=1).astype(np.uint8)]) if rng.random() < 0.5 else np.concatenate([c[:at], rng.integers(0, 4, size=1).astype(np.uint8), c[at:-1]])
        return c

    tandem, at = [], 20000   # per family: [(contig, position of copy)]
    for n_copies in (2, 3, 5, 8, 14, 20):
        unit = rng.integers(0, 4, size=900).astype(np.uint8)
        copies = []
        for k in range(n_copies):
            rate = rng.uniform(0.0, 0.0015) if n_copies == 14 else rng.uniform(0.001, 0.012)
            contigs[0][at:at + 900] = mutated(unit, rate, int(rng.random() < 0.25) if n_copies < 14 else 0)
            if n_copies == 20:
                contigs[0][at:at + 900] = unit
                if k == 0:
                    own = np.array([100, 390, 680])
                    contigs[0][at + own] = (unit[own] + 1) & 3
            copies.append((0, at))
            at += 1200
        tandem.append(copies)
        at += 60000
    cen_start, cen_end = np.array([tandem[0][0][1] - 500, -1], dtype=np.int64), np.array([tandem[0][-1][1] + 1400, -1], dtype=np.int64)
    dispersed = []
    for f in range(3):
        unit = rng.integers(0, 4, size=3000).astype(np.uint8)
        copies = []
        for k in range(4):
            pos = 10000 + 72000 * k + 4000 * f
            contigs[1][pos:pos + 3000] = mutated(unit, rng.uniform(0.002, 0.008), int(rng.random() < 0.5))
            copies.append((1, pos))
        dispersed.append(copies)

    reads, names, bc_off, kinds, do_rfa = [], [], [0], [], []

    def pair(ctg, lo, hi, tag, overhang=False):
        """an FR pair inside contigs[ctg][lo:hi) (or with read 1 starting up to 14 bases before lo)"""
        ins = int(rng.integers(300, 520))
        s = lo - int(rng.integers(3, 15)) if overhang else int(rng.integers(lo, hi - ins))
        g = contigs[ctg]
        r1, r2 = g[s:s + 143].copy(), comp[g[s + ins - 150:s + ins][::-1]]
        for r in (r1, r2):
            for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2]))):
                k = int(rng.integers(8, len(r) - 8)); r[k] = (r[k] + int(rng.integers(1, 4))) & 3
        if rng.random() < 0.2:
            for k in rng.choice(np.arange(20, 130), size=3, replace=False):
                r2[k] = (r2[k] + 1) & 3
        if rng.random() < 0.5:
            r1, r2 = r2, r1
        reads.extend([r1, r2])
        names.append("mq:%d:%s:%d" % (seed, tag, len(names)))

    def barcode(kind, rfa=1):
        bc_off.append(len(names)); kinds.append(kind if rfa else kind + "_norfa"); do_rfa.append(rfa)

    for rep in range(3):
        for f, copies in enumerate(tandem):
            for i in range(12):
                c, pos = copies[0 if len(copies) == 20 and i % 3 else int(rng.integers(len(copies)))]
                pair(c, pos, pos + 900, "t%d" % f, overhang=i % 4 == 3)
            barcode("tandem", rfa=0 if rep == 2 and f % 2 else 1)
    for rep in range(4):
        for f, copies in enumerate(dispersed):
            a, b = rng.choice(4, size=2, replace=False)
            for i in range(12):
                c, pos = copies[int(a if i < 9 else b)]
                pair(c, pos, pos + 3000, "d%d" % f)
            barcode("dispersed", rfa=0 if rep == 3 and f == 0 else 1)
    for rep in range(8):
        for i in range(2):
            copies = tandem[int(rng.integers(len(tandem)))]
            c, pos = copies[int(rng.integers(len(copies)))]
            pair(c, pos, pos + 900, "lt")
        for i in range(2):
            copies = dispersed[int(rng.integers(3))]
            c, pos = copies[int(rng.integers(4))]
            pair(c, pos, pos + 3000, "ld")
        barcode("thin", rfa=0 if rep == 7 else 1)
    from lariat_amd import synth
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    batch = capi.Batch.from_arrays(np.concatenate(reads), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.array(bc_off, dtype=np.int32), synth._name_seeds(names),
                                   bc_do_rfa=np.array(do_rfa, dtype=np.uint8), cen_start=cen_start, cen_end=cen_end)
    return ["chrT", "chrD"], contigs, batch, kinds


def mapq_coverage(ref, eta=MAPQ_ETA):
    """which edges of the MAPQ computation a batch reaches, counted on the ORACLE's terms alone (mapq_reference of ref.mapq_terms): decidable candidates per
    bin of the raw value, with a fractional part of a half and more, within 1e-5 below an integer, with the molecule term / the pair term the smaller one,
    of reads with fewer than 15, exactly 15 and more than 15 scores, NaN, zeroed by a centromere"""
    t = ref.mapq_terms
    m = mapq_reference(t, eta=eta)
    d = m["decidable"]
    raw, sc, tot, sm, cen, ns = t[:, 6], t[:, 1], t[:, 2], t[:, 4], t[:, 5] != 0, t[:, 7]
    with np.errstate(all="ignore"):
        pair_term, mol_term = -10.0 * np.log10(1.0 - 10.0 ** sc / tot), -10.0 * np.log10(1.0 - 1.0 / sm)
    live = d & ~cen & (raw >= 0.5) & (raw < 60)
    cov = {"bin_0.5_1": int((live & (raw < 1)).sum()), "bin_1_10": int((live & (raw >= 1) & (raw < 10)).sum())}
    for lo in range(10, 60, 10):
        cov["bin_%d_%d" % (lo, lo + 10)] = int((live & (raw >= lo) & (raw < lo + 10)).sum())
    frac = raw - np.floor(raw)
    cov.update(frac_ge_half=int((live & (frac >= 0.5)).sum()), just_below_integer=int((live & (frac > 1 - 1e-5)).sum()),
               molecule_term_smaller=int((live & (mol_term < pair_term)).sum()), pair_term_smaller=int((live & (pair_term < mol_term)).sum()),
               scores_under_15=int((live & (ns < 15)).sum()), scores_15=int((live & (ns == 15)).sum()), scores_over_15=int((live & (ns > 15)).sum()),
               nan=int((m["set"] & np.isnan(raw)).sum()), centromere_zero=int((m["set"] & cen).sum()), in_range=int((m["set"] & (raw >= 0.5) & (raw < 60)).sum()),
               undecidable_in_range=int((m["set"] & ~d & (raw >= 0.5) & (raw < 60)).sum()), compared=int(m["set"].sum()))
    return cov


def exact_repeat_genome(copies=20, unit=900, spacer=400, seed=3):
    """one contig holding `copies` EXACT copies of a unit between random spacers + a unique tail: reads from a unit have
    `copies` equally good candidates on both mates (tagBestAlignments then draws copies^2 jitter values per pair)"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 4, size=unit).astype(np.uint8)
    parts = []
    for _ in range(copies):
        parts += [rng.integers(0, 4, size=spacer).astype(np.uint8), u]
    parts.append(rng.integers(0, 4, size=20000).astype(np.uint8))
    return ["chrR"], [np.concatenate(parts)], unit, spacer


def repeat_unit_reads(contigs, unit, spacer, n_pairs, seed=4, copy=3, len1=120, len2=120):
    """FR pairs that lie inside copy `copy` of exact_repeat_genome's unit; one barcode"""
    rng = np.random.default_rng(seed)
    g = contigs[0]
    base = copy * (unit + spacer) + spacer
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    reads, names = [], []
    for i in range(n_pairs):
        ins = int(rng.integers(300, 500))
        s = base + int(rng.integers(0, unit - ins))
        r1 = g[s:s + len1].copy()
        r2 = comp[g[s + ins - len2:s + ins][::-1]]
        if rng.random() < 0.5:
            r1[int(rng.integers(len1))] ^= 1
        reads += [r1, r2]
        names.append("rep:%d" % i)
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads)
    rs.bc_pair_off = np.array([0, n_pairs], dtype=np.int32)
    rs.names = names
    rs.name_seed = synth._name_seeds(names)
    return rs


def chance_match_genome_and_reads(n_pairs=24, seed=8, plant=21, rlen=150):
    """a random contig in which the MIDDLE `plant` bases of every read 1 (and of some reads 2) also occur at an unrelated place:
    re-seeding (bwt_smem1 from the middle of a long SMEM with min_intv 2) then yields a second, one-seed chain per read that
    mem_chain_flt keeps as the first shadowed chain and mem_chain2aln extends with the full band over long query sides — at
    human-genome scale chance matches do that to every third read"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, size=260000).astype(np.uint8)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    loci = []
    for i in range(n_pairs):
        p = 5000 + i * 4000 + int(rng.integers(0, 1000))
        ins = int(rng.integers(320, 480))
        loci.append((p, ins))
        mid = p + rlen // 2 - plant // 2
        g[150000 + i * 300: 150000 + i * 300 + plant] = g[mid: mid + plant]
        if i % 3 == 0:   # read 2's middle as well (reverse strand)
            mid2 = p + ins - rlen // 2 - plant // 2
            g[200000 + i * 300: 200000 + i * 300 + plant] = g[mid2: mid2 + plant]
    reads, names = [], []
    for i, (p, ins) in enumerate(loci):
        r1 = g[p:p + rlen].copy()
        r2 = comp[g[p + ins - rlen:p + ins][::-1]]
        if i % 2:
            r1[int(rng.integers(5, 40))] ^= 2      # a mismatch off the middle: the planted match still covers the re-seeding point
        if i % 4 == 0:
            r2[int(rng.integers(100, 140))] ^= 1
        reads += [r1, r2]
        names.append("chance:%d" % i)
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads)
    rs.bc_pair_off = np.array([0, n_pairs // 2, n_pairs], dtype=np.int32)
    rs.names = names
    rs.name_seed = synth._name_seeds(names)
    return ["chrC"], [g], rs


def alt_genome_and_reads(seed=12, n_pairs=60):
    """two primary contigs + one ALT contig (configs[4]: "hg38 + ALT/decoy"): the ALT is a copy of 30 kb of chrP1 in which novel 90-base
    insertions alternate with 60 kept bases over a few kb (plus point mutations elsewhere), and chrP2 holds an exact copy of the same
    30 kb.  Reads from the ALT's inserted stretch have a heavy chain on the ALT and two light ones on the primaries (the kept 60 bases):
    with is_alt the light primary chains are not compared with the ALT chain in mem_chain_flt."""
    rng = np.random.default_rng(seed)
    p1 = rng.integers(0, 4, size=120000).astype(np.uint8)
    p2 = rng.integers(0, 4, size=90000).astype(np.uint8)
    src = p1[40000:70000].copy()
    p2[20000:50000] = src
    parts, pos = [], 0
    while pos < len(src):
        if 8000 <= pos < 16000:
            parts += [src[pos:pos + 60], rng.integers(0, 4, size=90).astype(np.uint8)]
            pos += 60
        else:
            seg = src[pos:pos + 500].copy()
            m = rng.random(len(seg)) < 0.004
            seg[m] = (seg[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
            parts.append(seg)
            pos += 500
    alt = np.concatenate(parts)
    names = ["chrP1", "chrP2", "chrP1_alt1"]
    contigs = [p1, p2, alt]
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    lo = 8000 * 150 // 60   # the inserted stretch in ALT coordinates
    reads, rnames = [], []
    for i in range(n_pairs):
        ins = int(rng.integers(300, 480))
        s = lo + int(rng.integers(0, 8000 * 150 // 60 - ins)) if i % 4 else int(rng.integers(0, len(alt) - ins))
        r1 = alt[s:s + 143].copy()
        r2 = comp[alt[s + ins - 150:s + ins][::-1]]
        if i % 3 == 0:
            r1[int(rng.integers(143))] ^= 1
        reads += [r1, r2]
        rnames.append("alt:%d" % i)
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads)
    rs.bc_pair_off = np.array([0, n_pairs // 2, n_pairs], dtype=np.int32)
    rs.names = rnames
    rs.name_seed = synth._name_seeds(rnames)
    return names, contigs, rs


def low_complexity_genome(seed=9):
    """poly-A tracts, di- and penta-nucleotide microsatellites and a 200-copy tandem repeat of a 37-base unit between random flanks: reads from
    them have intervals with thousands of occurrences, hundreds of chains per read and long runs of equal candidates"""
    rng = np.random.default_rng(seed)

    def rnd(n):
        return rng.integers(0, 4, size=n).astype(np.uint8)

    def tandem(unit, n):
        return np.tile(np.asarray(unit, dtype=np.uint8), n)

    parts = [rnd(20000), tandem([0], 5000), rnd(3000), tandem([1, 0], 1500), rnd(3000), tandem(rnd(37), 200), rnd(3000), tandem(rnd(5), 800), rnd(3000),
             tandem(rnd(2), 400), rnd(500), tandem([3], 600), rnd(20000)]
    return ["chrL"], [np.concatenate(parts)]


def k7_shift_case(g, ins_first):
    """a read pair whose read 1 has four mismatches on the diagonal of its alignment and NONE on a path with one insertion and one deletion of g
    bases: a stretch of A's with two interruptions, shifted by g inside its own span (K7's shifted-diagonal check, k_aln.h).  Returns
    (names, contigs, batch, position of the stretch)."""
    from lariat_amd import capi
    rng = np.random.default_rng(23)
    rnd = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)
    seg = np.array([0] * 6 + [2] + [0] * 6 + [3] + [0] * 6, dtype=np.uint8)                 # AAAAAA G AAAAAA T AAAAAA
    left, right = rnd(4000), rnd(4000)
    left[-1] = 1; right[0] = 1                                                                # (no A next to the stretch: the indels cannot slide out of it)
    contig = np.concatenate([left, seg, right])
    p = len(left)
    body = np.concatenate([[0] * g, seg[:-g]]) if ins_first else np.concatenate([seg[g:], [0] * g])   # the stretch shifted by g inside its own span
    r1 = np.concatenate([contig[p - 66:p], body, contig[p + len(seg):p + len(seg) + 150 - 66 - len(seg)]]).astype(np.uint8)
    assert len(r1) == 150 and int((r1 != contig[p - 66:p + 84]).sum()) == 4
    mate = contig[p + 250:p + 400]
    r2 = (3 - mate[::-1]).astype(np.uint8)
    return ["chrK"], [contig], capi.Batch([r1, r2], [0, 1]), p


def k7_band_case(g, ins_first):
    """a read pair whose read 1 runs g columns off its main diagonal for 60 bases: g inserted bases after base 40 and g deleted reference bases
    60 bases later (or the other way round) — equal spans, a path of two gaps.  K7's four-per-wave kernel (k_aln_grp, k_aln.h) runs a band
    of 7 and proves it sufficient; from g = 8 on the path lies outside that band and the proof must fail.  Returns (names, contigs, batch, p)."""
    from lariat_amd import capi
    rng = np.random.default_rng(1000 + 2 * g + int(ins_first))
    contig = rng.integers(0, 4, size=8400).astype(np.uint8)
    p = 4000
    R = contig[p:p + 150]
    X = rng.integers(0, 4, size=g).astype(np.uint8)
    if ins_first:
        X[0] = (R[40] + 1) & 3; X[-1] = (R[39] + 2) & 3
        r1 = np.concatenate([R[:40], X, R[40:100], R[100 + g:]])
    else:
        r1 = np.concatenate([R[:40], R[40 + g:110], X, R[110:]])
    r1 = r1.astype(np.uint8)
    assert len(r1) == 150
    mate = contig[p + 250:p + 400]
    r2 = (3 - mate[::-1]).astype(np.uint8)
    return ["chrB"], [contig], capi.Batch([r1, r2], [0, 1]), p


def _k7_low_complexity(rng, n):
    kind = int(rng.integers(0, 4))
    if kind == 0:      # a homopolymer with interruptions
        s = np.full(n, int(rng.integers(0, 4)), dtype=np.uint8)
    elif kind == 1:    # a short tandem repeat
        s = np.tile(rng.integers(0, 4, size=int(rng.integers(2, 8))).astype(np.uint8), n)[:n]
    elif kind == 2:    # two homopolymers
        s = np.concatenate([np.full(n // 2, int(rng.integers(0, 4))), np.full(n - n // 2, int(rng.integers(0, 4)))]).astype(np.uint8)
    else:              # a repeat of a longer unit with a homopolymer inside
        u = rng.integers(0, 4, size=int(rng.integers(8, 14))).astype(np.uint8); u[2:6] = u[2]
        s = np.tile(u, n)[:n]
    for _ in range(int(rng.integers(0, 5))):
        k = int(rng.integers(0, n)); s[k] = (s[k] + int(rng.integers(1, 4))) & 3
    return s


def _k7_deep_case(rng):
    """one locus and a read 1 on it whose middle is an excursion of two or three gap runs through low-complexity sequence (equal spans), plus substitutions"""
    lc = _k7_low_complexity(rng, int(rng.integers(24, 70)))
    left, right = rng.integers(0, 4, size=400).astype(np.uint8), rng.integers(0, 4, size=700).astype(np.uint8)
    locus = np.concatenate([left, lc, right])
    p = len(left)
    ref = locus[p - 50:p + 100].copy()
    a = 50 + int(rng.integers(0, max(1, len(lc) // 3)))
    runs = int(rng.choice([2, 2, 3, 3, 4]))
    total = int(rng.integers(1, 6)) if runs == 2 else int(rng.integers(2, 5))
    read = list(ref)
    # deletions of reference bases first or insertions first; the later runs give the bases back
    first_del = bool(rng.integers(0, 2))
    cuts = sorted(int(x) for x in rng.choice(np.arange(a, min(a + len(lc), 140)), size=runs, replace=False))
    if runs == 2:
        sizes_a, sizes_b = [total], [total]
        pos_a, pos_b = cuts[:1], cuts[1:]
    elif runs == 3:
        k = int(rng.integers(1, total))
        if rng.integers(0, 2): sizes_a, sizes_b, pos_a, pos_b = [k, total - k], [total], cuts[:2], cuts[2:]
        else: sizes_a, sizes_b, pos_a, pos_b = [total], [k, total - k], cuts[:1], cuts[1:]
    else:
        k, k2 = int(rng.integers(1, total)), int(rng.integers(1, total))
        sizes_a, sizes_b, pos_a, pos_b = [k, total - k], [k2, total - k2], cuts[:2], cuts[2:]
    ops = [(q, "d" if first_del else "i", n) for q, n in zip(pos_a, sizes_a)] + [(q, "i" if first_del else "d", n) for q, n in zip(pos_b, sizes_b)]
    out, at = [], 0
    for q, kind, n in sorted(ops):
        out += list(ref[at:q]); at = q
        if kind == "d": at = min(len(ref), q + n)
        else: out += [int(ref[max(0, q - 1 - j)]) if rng.random() < 0.7 else int(rng.integers(0, 4)) for j in range(n)]
    out += list(ref[at:])
    read = np.array(out[:150], dtype=np.uint8)
    if len(read) < 150:
        read = np.concatenate([read, locus[p + 100:p + 100 + 150 - len(read)]])
    for _ in range(int(rng.integers(0, 4))):
        k = int(rng.integers(5, 145)); read[k] = (read[k] + int(rng.integers(1, 4))) & 3
    mate = locus[p + 300:p + 450]
    return locus, read, (3 - mate[::-1]).astype(np.uint8), int((read != ref).sum())


def k7_deep_batch(seed, n):
    """n read pairs for K7's second look (k_aln.h, aln_deep_check): read 1 of each has five to seven mismatches on its diagonal and an excursion of two to four gap runs
    through low-complexity sequence beside it; which of the two wins is the DP's to say — or the proof's.  Returns (names, contigs, reads)."""
    rng = np.random.default_rng(seed)
    loci, reads, at = [], [], 0
    while len(loci) < n:
        locus, r1, r2, mm = _k7_deep_case(rng)
        if not 5 <= mm <= 7:
            continue
        loci.append(locus); reads += [r1, r2]
    contig = np.concatenate(loci)
    return ["chrD"], [contig], reads


def repeat_family_case(seed, n_barcodes, pairs=30):
    """a 600-kb genome with a family of 12 copies x 3 kb (0.2-1.2 % off the consensus, indels), one of 30 copies x 300 bp (2-8 %) and five tandem copies
    of 1.2 kb; every read pair drawn on and around the copies: tens of chains, regions and rescue attempts per read — the regime of BASELINE
    configs[4] in miniature.  Returns (names, contigs, read set)."""
    from lariat_amd import synth, workload
    rng = np.random.default_rng(seed)
    g = rng.choice(4, size=600000, p=[0.295, 0.205, 0.205, 0.295]).astype(np.uint8)
    q = g.reshape(-1, 4)
    pac = np.concatenate([(q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8), np.zeros(1, dtype=np.uint8)])
    ctg = [("c0", 400000, 0), ("c1", 200000, 400000)]
    fam = workload.plant_family(pac, ctg, rng, 3000, 12, 0.002, 0.012, indel_per_base=1 / 1500.0)
    fam2 = workload.plant_family(pac, ctg, rng, 300, 30, 0.02, 0.08, indel_per_base=1 / 300.0)
    tand = workload._unpack(pac, 100000, 1200)
    for k in range(1, 5):   # tandem copies: rescue windows that hold two alignments of the mate, regions next to each other
        seg = tand.copy(); m = rng.random(1200) < 0.01; seg[m] = (seg[m] + 1) & 3
        workload._repack(pac, 100000 + 1200 * k, seg)
    names = [c[0] for c in ctg]
    contigs = [workload._unpack(pac, off, ln) for _, ln, off in ctg]
    win = workload.windows_on(ctg, fam, 1000) + workload.windows_on(ctg, fam2, 850) + [("t", 9000, 98000)] * 6
    wnames = ["w%d" % i for i in range(len(win))]
    wcontigs = [workload._unpack(pac, off // 4 * 4, (ln + off % 4 + 3) // 4 * 4)[off % 4: off % 4 + ln] for _, ln, off in win]
    rs = synth.make_reads(wcontigs, wnames, n_barcodes=n_barcodes, pairs_per_barcode=pairs, seed=seed + 9, mol_min=2, mol_max=4, ins_mean=470, ins_sd=120, ins_max=900,
                          junk_frac=0.02)
    return names, contigs, rs


def fragmented_genome(seed, n_contigs, long_lens=(150000,), short_max=8000, short_min=20, overlap_frac=0.15, alt_frac=0.0):
    """a reference shaped like an analysis set's tail: `long_lens` long contigs plus n_contigs - len(long_lens) short ones whose lengths are
    log-uniform in [short_min, short_max].  The short ones always include contigs shorter than min_seed_len (19), shorter than a read and
    shorter than an insert; a fraction `overlap_frac` of the contigs start with a copy of the previous contig's last 30-400 bases (overlapping
    scaffolds: a read across that junction has candidates on both sides).  Returns (names, contigs, alt) — alt a per-contig 0/1 mask when
    alt_frac > 0 (never on the long contigs), else None."""
    rng = np.random.default_rng(seed)
    p = np.array([0.295, 0.205, 0.205, 0.295])
    n_short = n_contigs - len(long_lens)
    assert n_short >= 12
    lens = np.exp(rng.uniform(np.log(short_min), np.log(short_max), size=n_short)).astype(np.int64)
    lens[:12] = [12, 18, 19, 25, 40, 60, 90, 120, 140, 200, 300, 450]   # below min_seed_len, below a read, below an insert
    rng.shuffle(lens)
    lens = list(long_lens[:1]) + [int(x) for x in lens[:n_short // 2]] + list(long_lens[1:]) + [int(x) for x in lens[n_short // 2:]]
    is_long = np.zeros(n_contigs, dtype=bool)
    is_long[0] = True
    is_long[1 + n_short // 2:1 + n_short // 2 + len(long_lens) - 1] = True
    contigs = [rng.choice(4, size=int(n), p=p).astype(np.uint8) for n in lens]
    for k in range(1, n_contigs):
        if rng.random() < overlap_frac:
            ov = min(int(rng.integers(30, 401)), len(contigs[k - 1]), len(contigs[k]))
            contigs[k][:ov] = contigs[k - 1][len(contigs[k - 1]) - ov:]
    names = ["frag%d" % k if not is_long[k] else "chr%d" % k for k in range(n_contigs)]
    alt = None
    if alt_frac > 0:
        alt = ((rng.random(n_contigs) < alt_frac) & ~is_long).astype(np.uint8)
    return names, contigs, alt


GEOMETRY_KINDS = ("junction", "overhang", "inside_short", "split_mates", "ends", "plain", "rescue_edge")


def geometry_reads(contigs, pairs_per_barcode, seed, len1=143, len2=150, ins_lo=250, ins_hi=600, sub_hi=0.02, indel_frac=0.05, n_frac=0.05,
                   kinds=GEOMETRY_KINDS, weights=None):
    """FR pairs drawn from the CONCATENATED reference without regard to contig boundaries, one barcode per entry of `pairs_per_barcode`.  Each
    pair is one of `kinds`: across a junction between two contigs; hanging off a contig end (random bases beyond position 0 / l_pac, or past a
    junction); around a contig shorter than the read; mates on two unrelated contigs; inside the first or last 600 bases of the concatenation;
    anywhere; or mates that overlap almost entirely across a contig's start or end, one of them with a substitution every 10-16 bases (no seed:
    only mem_matesw finds it, in a window that the contig end cuts).  Substitutions, some indels and some N's; names (hence name seeds) per pair.  Returns a synth.ReadSet whose `kind` lists the kinds."""
    rng = np.random.default_rng(seed)
    g = np.concatenate(contigs)
    lpac = len(g)
    clen = np.array([len(c) for c in contigs], dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(clen)])
    shorter = np.nonzero(clen < min(len1, len2))[0]
    w = np.ones(len(kinds)) if weights is None else np.asarray(weights, dtype=float)
    w = w / w.sum()

    def seg(a, b):   # g[a:b] with random bases where it runs off either end of the concatenation
        lo, hi = max(a, 0), min(b, lpac)
        return np.concatenate([rng.integers(0, 4, size=max(0, lo - a)), g[lo:max(lo, hi)], rng.integers(0, 4, size=max(0, b - max(hi, lo)))]).astype(np.uint8)

    n_pairs = int(np.sum(pairs_per_barcode))
    reads, names, kind_of = [], [], []
    for i in range(n_pairs):
        kind = kinds[int(rng.choice(len(kinds), p=w))]
        ins = int(rng.integers(max(ins_lo, len1, len2), ins_hi + 1))
        if kind == "junction":     # the fragment or one of its reads across a junction
            j = int(coff[int(rng.integers(1, len(contigs)))])
            s = j - int(rng.integers(10, ins - 10))
        elif kind == "overhang":   # a read past a contig end: off position 0, off l_pac, or across a junction by a few bases
            r = rng.random()
            if r < 0.3:
                s = -int(rng.integers(5, len1 // 2))
            elif r < 0.6:
                s = lpac - ins + int(rng.integers(5, len2 // 2))
            else:
                j = int(coff[int(rng.integers(1, len(contigs)))])
                s = j - len1 + int(rng.integers(3, 30)) if rng.random() < 0.5 else j + int(rng.integers(3, 30)) - ins
        elif kind == "inside_short" and len(shorter):
            k = int(rng.choice(shorter))
            s = int(coff[k]) - int(rng.integers(0, len1 - clen[k] + 1)) if rng.random() < 0.5 else int(coff[k + 1]) - ins + int(rng.integers(0, len2 - clen[k] + 1))
        elif kind == "rescue_edge":
            k = int(rng.integers(1, len(contigs)))
            ins = int(rng.integers(max(len1, len2), max(len1, len2) + 30))
            d = int(rng.integers(5, 40))
            s = int(coff[k]) - d if rng.random() < 0.5 else int(coff[k + 1]) + d - ins
        elif kind == "ends":
            s = int(rng.integers(0, 600 - 200)) if rng.random() < 0.5 else lpac - int(rng.integers(200, 600))
            ins = min(ins, 600)
        else:
            s = int(rng.integers(0, lpac - ins))
        frag = seg(s, s + ins)
        r1, r2 = frag[:len1].copy(), _GEO_COMP[frag[ins - len2:][::-1]]
        if kind == "split_mates":   # read 2 from another place entirely, either strand
            t = int(rng.integers(0, lpac - len2))
            r2 = g[t:t + len2].copy() if rng.random() < 0.5 else _GEO_COMP[g[t:t + len2][::-1]]
        if kind == "rescue_edge":
            r2 = r2.copy()
            at = int(rng.integers(0, 10))
            while at < len(r2):
                r2[at] = (r2[at] + int(rng.integers(1, 4))) & 3
                at += int(rng.integers(10, 17))
        if rng.random() < 0.5:
            r1, r2 = r2, r1
        out = []
        for r in (r1, r2):
            m = rng.random(len(r)) < rng.uniform(0.0, sub_hi)
            r[m] = (r[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
            if rng.random() < indel_frac:
                at, ln = int(rng.integers(20, len(r) - 20)), int(rng.integers(1, 5))
                r = np.concatenate([r[:at], r[at + ln:]]) if rng.random() < 0.5 else np.concatenate([r[:at], rng.integers(0, 4, size=ln).astype(np.uint8), r[at:]])
            if rng.random() < n_frac:
                r[rng.integers(0, len(r), size=int(rng.integers(1, 4)))] = 4
            out.append(r.astype(np.uint8))
        reads += out
        names.append("geo:%d:%s:%d:%d" % (seed, kind, s, i))
        kind_of.append(kind)
    rs = synth.ReadSet()
    lens = np.array([len(x) for x in reads], dtype=np.int64)
    rs.seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rs.seq = np.concatenate(reads)
    rs.bc_pair_off = np.concatenate([[0], np.cumsum(pairs_per_barcode)]).astype(np.int32)
    rs.names = names
    rs.name_seed = synth._name_seeds(names)
    rs.kind = kind_of
    return rs


_GEO_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def geometry_coverage(contig_lens, od, ores, batch):
    """how many of each contig-geometry edge a batch reached, read from the ORACLE's stage dump `od` and result `ores` (fwd||rev coordinates:
    position x >= l_pac is forward position 2 l_pac - 1 - x)"""
    clen = np.asarray(contig_lens, dtype=np.int64)
    coff = np.concatenate([[0], np.cumsum(clen)])
    lpac = int(coff[-1])

    def fwd(b, e):   # [b, e) in fwd||rev -> forward [fb, fe)
        rev = b >= lpac
        return np.where(rev, 2 * lpac - e, b), np.where(rev, 2 * lpac - b, e)

    sb, se = fwd(od.seed_rbeg, od.seed_rbeg + od.seed_len)
    cross = (np.searchsorted(coff, sb, side="right") != np.searchsorted(coff, se - 1, side="right")) | ((od.seed_rbeg < lpac) & (od.seed_rbeg + od.seed_len > lpac))
    rb, re = fwd(od.reg_rb, od.reg_re)
    on_end = np.isin(rb, coff) | np.isin(re, coff)
    c = ores.rid >= 0
    rid = np.where(c, ores.rid, 0)
    at_end = c & ((ores.pos == 0) | (ores.aend == clen[rid]))
    rlen = np.diff(batch.seq_off)
    read_of = np.repeat(np.arange(len(rlen)), np.diff(ores.cand_off))
    ncand = np.diff(ores.cand_off[2 * batch.bc_pair_off.astype(np.int64)])
    nfilt = np.add.reduceat(ores.in_filtered.astype(np.int64), ores.cand_off[2 * batch.bc_pair_off[:-1].astype(np.int64)]) if ores.n_cand else np.zeros(0)
    return dict(bridging_seeds=int(cross.sum()), regions_on_contig_end=int(on_end.sum()), cand_pos0=int((c & (ores.pos == 0)).sum()),
                cand_aend_at_contig_end=int((c & (ores.aend == clen[rid])).sum()), soft_clips_at_contig_end=int((at_end & (ores.soft_clipped > 0)).sum()),
                cand_on_contig_shorter_than_read=int((c & (clen[rid] < rlen[read_of])).sum()), n_rescue=int(ores.counters["n_rescue"]),
                barcodes_over_256=int((ncand > 256).sum()), barcodes_under_256=int((ncand <= 256).sum()), max_filtered=int(nfilt.max()) if len(nfilt) else 0)


def assert_geometry_coverage(cov, **at_least):
    """every count of geometry_coverage at least 1 (or the given minimum)"""
    for k, v in cov.items():
        if k == "max_filtered":
            continue
        need = at_least.get(k, 1)
        assert v >= need, ("geometry coverage", k, v, need, cov)
