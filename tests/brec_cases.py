"""Cases shared by test_emu_brec.py (the kernel sources under the CPU emulator) and test_gpu_brec.py (the library on the device): BAM records derived and encoded
on the device (lariat_amd/csrc/k_brec.h, lh_brec.inc; lh_bam_set_device_records).  The judge is the host record path (records.cpp, bamfile.cpp::encode) with the
same device compressor: the files must be equal byte for byte, because the blocks are cut at the same places and k_bgzf's bytes are a function of its input alone."""
import contextlib
import copy
import gzip
import math
import os
import struct

import numpy as np

import bam_reader
from lariat_amd import capi, synth

RG = "s:lib:1:fc:1"
WRITER = dict(read_groups=RG + ",bad", position_chunk_size=150000, first_chunk=True, command_line="lariat_amd test", threads=3)


def fastq9(rs, trim_prefix=7, seed=7):
    """synth.to_fastq9 with what it leaves uniform varied, so that every optional tag is present on some records and absent on others: qualities that differ
    along the read (a reversed record must reverse them), a read group on two pairs of three, a sample index of one base (no BC / QT) on every fifth pair, and
    barcode 1 without its '-1' (not whitelisted: no BX, no DM)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(len(rs.bc_pair_off) - 1):
        for p in range(rs.bc_pair_off[b], rs.bc_pair_off[b + 1]):
            r1 = "".join("ACGTN"[v] for v in rs.read(2 * p))
            r2 = "".join("ACGTN"[v] for v in rs.read(2 * p + 1))
            pre = "".join("ACGT"[v] for v in rng.integers(0, 4, size=trim_prefix))
            q1 = "".join(chr(35 + (3 * i + p) % 38) for i in range(len(r1) + trim_prefix))
            q2 = "".join(chr(36 + (5 * i + p) % 37) for i in range(len(r2)))
            bc = rs.barcodes[b] if b != 1 else rs.barcodes[b].split("-")[0]
            si, siq = ("ACGTACGT", "FFFFGGGG") if p % 5 else ("A", "F")
            out += ["@" + rs.names[p] + (" " + RG if p % 3 else ""), pre + r1, q1, r2, q2, bc, "I" * 16, si, siq]
    return "\n".join(out) + "\n"


def make_batches(lib, align, names, contigs, tmp, n_barcodes, max_pairs, seed=67):
    """[(result, ingest batch)]: synthetic linked reads through the 9-line reader, aligned by `align` (the oracle under the emulator, the product on the GPU)"""
    rs = synth.make_reads(contigs, names, n_barcodes=n_barcodes, pairs_per_barcode=60, seed=seed, sub_hi=0.03, indel_rate=0.002, junk_frac=0.06)
    rng = np.random.default_rng(seed)
    rd = lambda r: slice(int(rs.seq_off[r]), int(rs.seq_off[r + 1]))   # noqa: E731
    for p in range(3, rs.n_pairs, 9):   # chimeric reads (read 0 or read 1 of the pair): the second half comes from another read's locus -> split records
        a, d = 2 * p + (p & 1), 2 * ((p * 7 + 11) % rs.n_pairs) + (p & 1)
        la, ld = rd(a).stop - rd(a).start, rd(d).stop - rd(d).start
        h = min(la, ld) // 2
        rs.seq[rd(a).stop - h:rd(a).stop] = rs.seq[rd(d).stop - h:rd(d).stop]
    for p in range(5, rs.n_pairs, 17):   # 33 bases of the locus, then noise, and a mate of noise: an improper alignment below AppendBam's score rule
        a = rd(2 * p)
        rs.seq[a.start + 33:a.stop] = rng.integers(0, 4, size=a.stop - a.start - 33)
        b = rd(2 * p + 1)
        rs.seq[b] = rng.integers(0, 4, size=b.stop - b.start)
    for p in range(7, rs.n_pairs - 1, 13):   # the next pair of the barcode is a copy: a duplicate
        if (p + 1) % 60 and all(rd(2 * p + m).stop - rd(2 * p + m).start == rd(2 * p + 2 + m).stop - rd(2 * p + 2 + m).start for m in (0, 1)):
            for m in (0, 1):
                rs.seq[rd(2 * p + 2 + m)] = rs.seq[rd(2 * p + m)]
    path = tmp / "r.fastq"
    path.write_text(fastq9(rs, trim_prefix=7))
    return [(align(b), b) for b in lib.ingest(str(path), trim=7, max_pairs=max_pairs)]


@contextlib.contextmanager
def open_writer(lib, outdir, names, lens, **kw):
    """a BamWriter that is closed when the block ends, however it ends: a writer left to the garbage collector would flush through a compressor that may have been
    freed before it"""
    w = lib.bam_writer(str(outdir), names, lens, **kw)
    try:
        yield w
        w.close()
    except BaseException:
        try:
            w.close()   # (a no-op after a close that failed: the handle is dropped first)
        except capi.LhError:
            pass
        raise


def write_files(lib, outdir, names, lens, batches, path_of, writer=WRITER, z=None, debug_tags=False):
    """one file set.  path_of(k), before append k (and, for k = len(batches), before the close): "zlib" = host records, host compression; "host" = host records,
    device compressor; "dev" = records on the device.  An entry of `batches` may be (result, batch, expected error code): that append must fail with it"""
    outdir.mkdir(parents=True)
    timings = []
    with open_writer(lib, outdir, names, lens, **writer) as w:
        if debug_tags:
            w.set_debug_tags(True)
        for k in range(len(batches) + 1):
            how = path_of(k)
            w.set_device(None if how == "zlib" else z)
            if how != "zlib":
                w.set_device_records(how == "dev")
            if k == len(batches):
                break
            if len(batches[k]) == 3:
                try:
                    w.append(batches[k][0], batches[k][1])
                    raise AssertionError("append %d did not fail" % k)
                except capi.LhError as e:
                    assert e.code == batches[k][2], (k, e.code, str(e))
            else:
                w.append(batches[k][0], batches[k][1])
                timings.append(w.timings())
    files = {f: open(outdir / f, "rb").read() for f in sorted(os.listdir(outdir))}
    files["_timings"] = timings
    return files


def same_files(lib, z, tmp, names, lens, batches, writer=WRITER, orders=("dev", "switch"), readable=True):
    """the file set written with host records + device compressor against the ones with device records (every append, or every other one): equal raw bytes; and
    against a writer without a compressor: equal after inflating"""
    want = write_files(lib, tmp / "host", names, lens, batches, lambda k: "host", writer, z)
    want.pop("_timings")
    sets = {"dev": lambda k: "dev", "switch": lambda k: "host" if k % 2 else "dev", "switch2": lambda k: "dev" if k % 2 else "host"}
    for name in orders:
        got = write_files(lib, tmp / name, names, lens, batches, sets[name], writer, z)
        t = got.pop("_timings")
        assert sorted(got) == sorted(want), name
        for f in want:
            assert got[f] == want[f], (name, f, len(got[f]), len(want[f]), _first_difference(got[f], want[f]))
            if readable:
                bam_reader.read_bam(str(tmp / name / f))
        if name == "dev":
            for x in t:
                assert x["join_s"] == 0 and 0 <= x["records_s"] <= x["gather_s"] + x["upload_s"] + x["plan_s"] + x["encode_s"] + 1e-9 and x["write_s"] >= 0, x
    zl = write_files(lib, tmp / "zlib", names, lens, batches, lambda k: "zlib", writer, None)
    zl.pop("_timings")
    assert sorted(zl) == sorted(want)
    for f in want:
        assert gzip.decompress(zl[f]) == gzip.decompress(want[f]), f
    return want


def _first_difference(a, b):
    """where the inflated streams first differ, with the bytes around it (for the assertion's message)"""
    try:
        x, y = gzip.decompress(a), gzip.decompress(b)
    except Exception as e:   # noqa: BLE001
        return "not inflatable: %r" % (e,)
    n = next((i for i in range(min(len(x), len(y))) if x[i] != y[i]), min(len(x), len(y)))
    return n, len(x), len(y), x[max(0, n - 40):n + 24], y[max(0, n - 40):n + 24]


# ---------------------------------------------------------------------------------------------------------------- case 2: what the batches hold
def feature_counts(lib, names, batches):
    """counts over the host path's text records (lh_records_text) of the features the device path has a rule of its own for"""
    n = dict.fromkeys(("reversed_primary", "split_of_forward", "split_of_reversed", "hard_clip", "unmapped_by_rule", "mate_unmapped", "no_second_best", "xc", "duplicate",
                       "no_bx", "no_bc", "no_rg", "dm", "odd_l_seq", "placeholder", "tlen_neg", "tlen_pos", "sa_on_primary", "sa_on_split"), 0)
    for res, b in batches:
        lines = lib.records_text(res, b, names).splitlines()
        k = 0
        for read in range(res.n_reads):
            a = int(res.active_idx[read])
            recs = [(a, lines[k])]
            k += 1
            if res.split_idx[read] >= 0:
                recs.append((int(res.split_idx[read]), lines[k]))
                k += 1
            for ci, line in recs:
                f = line.split("\t")
                flag, tags = int(f[1]), {t[:2]: t[5:] for t in f[11:]}
                split = bool(flag & 256)
                n["reversed_primary"] += (not split) and bool(flag & 16)
                if split:
                    n["split_of_reversed" if res.reversed[a] else "split_of_forward"] += 1
                    n["hard_clip"] += "H" in f[5]
                    n["sa_on_split"] += "SA" in tags
                else:
                    n["sa_on_primary"] += "SA" in tags
                n["unmapped_by_rule"] += bool(flag & 4) and res.pos[ci] >= 0
                n["placeholder"] += res.rid[ci] < 0
                n["mate_unmapped"] += bool(flag & 8)
                n["no_second_best"] += (not split) and tags["XC"] == "" and tags["XM"] == "0" and res.second_best_idx[read] < 0
                n["xc"] += tags["XC"] != ""
                n["duplicate"] += bool(flag & 0x400)
                n["no_bx"] += "BX" not in tags
                n["no_bc"] += "BC" not in tags and "QT" not in tags
                n["no_rg"] += "RG" not in tags
                n["dm"] += "DM" in tags
                n["odd_l_seq"] += f[9] != "*" and len(f[9]) % 2 == 1
                n["tlen_neg"] += int(f[8]) < 0
                n["tlen_pos"] += int(f[8]) > 0
        assert k == len(lines)
    return n


# ---------------------------------------------------------------------------------------------------------------- case 3: crafted pairs
def _proper_pair(res):
    """a pair whose two active alignments are each other's mates, proper, mapped on one contig, without splits"""
    for p in range(res.n_reads // 2):
        a0, a1 = int(res.active_idx[2 * p]), int(res.active_idx[2 * p + 1])
        if (res.mate_idx[a0] == a1 and res.mate_idx[a1] == a0 and res.is_proper[a0] and res.is_proper[a1] and res.rid[a0] == res.rid[a1] >= 0
                and res.split_idx[2 * p] < 0 and res.split_idx[2 * p + 1] < 0 and res.pos[a0] >= 0 and res.pos[a1] >= 0):
            return p, a0, a1
    raise AssertionError("no proper pair in the batch")


def _split_pair(res, a_reversed=None):
    for read in range(res.n_reads):
        a, s = int(res.active_idx[read]), int(res.split_idx[read])
        if s >= 0 and res.pos[a] >= 0 and res.pos[s] >= 0:
            return read, a, s
    raise AssertionError("no split read in the batch")


def crafted(res, which):
    """a copy of `res` with one pair edited for the order of AppendBam's edits (records.cpp: the edit of one record is read by the pair's later records)"""
    r = copy.deepcopy(res)
    if which == "a":     # read 1's active improper with score < 36, read 0's proper: read 0's record sees the mate's unedited pos, but takes the score[pm] - 17 < 19 branch only
        p, a0, a1 = _proper_pair(r)   # ... if its own alignment is improper: both forms follow
        r.is_proper[a1] = 0
        r.score[a1] = 30
    elif which == "a2":  # the same with read 0 improper but scored high: 0x8 from the mate's score, the mate's pos still unedited when read 0's record is made
        p, a0, a1 = _proper_pair(r)
        r.is_proper[a0] = 0
        r.is_proper[a1] = 0
        r.score[a0] = 90
        r.score[a1] = 30
    elif which == "b":   # both improper and low
        p, a0, a1 = _proper_pair(r)
        r.is_proper[a0] = 0
        r.is_proper[a1] = 0
        r.score[a0] = 20
        r.score[a1] = 35
    elif which == "c":   # a split whose primary the rule unmaps: the split's SA is suppressed, the primary's stays
        read, a, s = _split_pair(r)
        r.is_proper[a] = 0
        r.score[a] = 30
    elif which == "c2":  # ... and the other side: the split is unmapped when its own record is made, after the primary's SA has named it
        read, a, s = _split_pair(r)
        r.is_proper[s] = 0
        r.score[s] = 30
    elif which == "d":   # the mate on another contig
        p, a0, a1 = _proper_pair(r)
        r.rid[a1] = (int(r.rid[a0]) + 1) % 3
        r.is_proper[a0] = 0
        r.is_proper[a1] = 0
    else:
        raise KeyError(which)
    return r


CRAFTED = ("a", "a2", "b", "c", "c2", "d")


def crafted_extras(res):
    """rows the synthetic reads do not produce, edited into a copy: XS / AS values x86 converts to INT64_MIN (NaN, out of range), a negative one, a mismatch locus of
    several digits and a negative one, a molecule_difference on an exact rounding tie, a mapq above 255"""
    r = copy.deepcopy(res)
    r.second_best_score[0] = float("nan")
    r.as_score[0] = 1e30
    r.second_best_score[1] = -7.9
    r.as_score[1] = -3e9
    r.as_score[2] = 5e9       # in int64's range: the low 32 bits
    r.second_best_score[2] = -float("inf")
    a = int(r.active_idx[3])
    r.mapq[a] = 300
    for read in range(r.n_reads):
        a = int(r.active_idx[read])
        if r.mm_off[a + 1] > r.mm_off[a]:
            r.mm_ref_loc[r.mm_off[a]] = 123456789
            r.mm_read_loc[r.mm_off[a]] = -12
            break
    n = 0
    for a in range(r.n_cand):
        if r.active_molecule[a] and r.active[a]:
            r.molecule_difference[a] = (2.0 ** -7, 3 * 2.0 ** -7, 9.9999995, 0.0, 249.9999999)[n % 5]
            n += 1
    return r, n   # n: alignments whose DM tag now holds one of the crafted values


# ---------------------------------------------------------------------------------------------------------------- case 6: %.6f
def f6_values(n_random):
    """the kinds of values of the issue: dyadic fractions (the exact ties), quotients m / n (the shape of molecule_difference), the neighbours of every kind of
    rounding boundary, denormals, zeros, the largest value below 2^31, negatives"""
    rng = np.random.default_rng(20261019)
    v = [0.0, -0.0, 2.0 ** -7, 3 * 2.0 ** -7, 5e-324, 2.2250738585072014e-308, -5e-324, math.nextafter(2.0 ** 31, 0), -math.nextafter(2.0 ** 31, 0), 0.5e-6, 1.5e-6, 2.5e-6,
         0.9999995, 0.99999949999999, 9.9999995, 999999.9999995, 2147483647.9999995, 1e-7, 4.9999999e-7, 5.0000001e-7, 1.0, 123456.789, 2.0 ** 30 + 0.5 ** 22]
    for j in range(0, 25):
        ks = rng.integers(0, 250 << j, size=max(2, n_random // 100), dtype=np.int64)
        v += [int(k) / 2.0 ** j for k in ks]
        v += [(2 * int(k) + 1) / 2.0 ** j for k in ks[:4]]
    for _ in range(n_random // 3):
        n = int(rng.integers(1, 301))
        v.append(int(rng.integers(0, 250 * n + 1)) / n)
    for _ in range(n_random // 6):   # one ulp either side of d * 1e-6 + 5e-7
        d = int(rng.integers(0, 250000000))
        x = d * 1e-6 + 5e-7
        v += [x, math.nextafter(x, 0), math.nextafter(x, math.inf)]
    v += [-x for x in v[20:20 + n_random // 10]]
    return np.array(v, dtype=np.float64)


def check_f6(lib, n_random):
    v = f6_values(n_random)
    got = lib.diag_format_f6(v)
    bad = [(float(x), g, "%.6f" % x) for x, g in zip(v, got) if g != "%.6f" % x]
    assert not bad, (len(bad), bad[:8])
    assert "0.007812" in got and "0.023438" in got and "-0.000000" in got   # the ties to even, the sign of zero
    for x in (2.0 ** 31, -2.0 ** 31, float("inf"), -float("inf"), float("nan"), 1e300):
        try:
            lib.diag_format_f6([1.5, x])
            raise AssertionError("%r was not refused" % x)
        except capi.LhError as e:
            assert e.code == capi.LH_E_LIMIT, (x, e.code)
    assert lib.diag_format_f6([]) == []
    return len(v)


# ---------------------------------------------------------------------------------------------------------------- case 4: layouts
def empty_batch_like(lib, tmp):
    """an ingest batch without pairs: what lh_ingest_next hands out at the end of its input"""
    path = tmp / "one.fastq"
    path.write_text("@r0\nACGTACGTAC\nIIIIIIIIII\nACGTACGTAC\nIIIIIIIIII\nAAAACCCCGGGGTTTT-1\nIIIIIIIIIIIIIIII\nACGTACGT\nIIIIIIII\n")
    ing = lib.ingest(str(path), trim=0, max_pairs=10)
    first = ing.next()
    assert first.n_pairs == 1
    last = ing.next()
    assert last.n_pairs == 0
    return last, ing


def empty_result():
    r = capi.Result.__new__(capi.Result)
    r.n_reads, r.n_cand = 0, 0
    for name, _ in capi.LhResult._fields_:
        if name in ("abi_version", "n_reads", "n_cand", "arena_") or name in capi._COUNTERS:
            continue
        setattr(r, name, np.zeros(1, dtype=np.int64))
    r.counters = {}
    return r
