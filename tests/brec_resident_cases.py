"""Cases shared by test_emu_brec_resident.py (the kernel sources under the CPU emulator) and test_gpu_brec_resident.py (the library on the device):
lh_bam_append_resident, BAM records gathered on the device from the context's resident result (k_brec.h: k_brec_gather_count, k_brec_gather_fill; lh_brec.inc).
The judge is the project's own specification, lh_result_download + lh_bam_append with host records and the same compressor
(brec_cases.write_files(..., lambda k: "host", z=z)): the files must be equal byte for byte.

Every writer loop here does, per ingest batch: upload, align_resident, append_resident, and only afterwards the download whose result the judge (and
brec_cases.feature_counts) reads."""
import numpy as np

import brec_cases
import helpers
from lariat_amd import capi, synth


class Env:
    """a library with its compressor, and the small genome's index"""

    def __init__(self, lib, oracle, z):
        self.lib, self.oracle, self.z = lib, oracle, z
        self.names, self.contigs = helpers.small_genome()
        self.lens = [len(c) for c in self.contigs]
        self.idx = self.index(self.names, self.contigs)

    def index(self, names, contigs):
        return self.lib.index_from_arrays(self.oracle.index_build_naive(names, contigs).arrays())


def ingest_batches(lib, rs, tmp, max_pairs):
    """the read set through the 9-line reader (brec_cases.fastq9: every optional tag present on some records and absent on others)"""
    tmp.mkdir(parents=True, exist_ok=True)
    path = tmp / "r.fastq"
    path.write_text(brec_cases.fastq9(rs, trim_prefix=7))
    return list(lib.ingest(str(path), trim=7, max_pairs=max_pairs))


def feature_batches(env, tmp, n_barcodes, max_pairs):
    """brec_cases.make_batches' reads (chimeric, improper, duplicate, junk) as ingest batches: the pipeline aligns them in the writer loop, not the oracle here"""
    return [b for _, b in brec_cases.make_batches(env.lib, lambda b: None, env.names, env.contigs, tmp, n_barcodes=n_barcodes, max_pairs=max_pairs)]


def written(outdir):
    return {f.name: f.read_bytes() for f in sorted(outdir.iterdir())}


def resident_files(env, ctx, outdir, batches, path_of=lambda k: "res", names=None, lens=None, opts=None, download_first=False):
    """one file set.  path_of(k), before append k: "res" = lh_bam_append_resident; "dev" / "host" = download, then lh_bam_append with device / host records.
    Returns (files, [(result, batch)], [timings of the resident appends]); an ingest batch without pairs is not aligned: it has no resident counterpart"""
    lib = env.lib
    outdir.mkdir(parents=True)
    results, timings = [], []
    with brec_cases.open_writer(lib, outdir, names or env.names, lens or env.lens, **brec_cases.WRITER) as w:
        w.set_device(env.z)
        for k, b in enumerate(batches):
            how = path_of(k)
            w.set_device_records(how != "host")
            if b.n_pairs == 0:
                res = brec_cases.empty_result()
                if how == "res":
                    w.append_resident(ctx, b)
                else:
                    w.append(res, b)
                results.append((res, b))
                continue
            ctx.upload(b)
            ctx.align_resident(opts or lib.opts())
            if how == "res":
                first = ctx.download() if download_first else None
                w.append_resident(ctx, b)
                timings.append(w.timings())
                res = first or ctx.download()   # only afterwards: for the judge
            else:
                res = ctx.download()
                w.append(res, b)
            results.append((res, b))
    return written(outdir), results, timings


def judge(env, outdir, results, names=None, lens=None):
    want = brec_cases.write_files(env.lib, outdir, names or env.names, lens or env.lens, results, lambda k: "host", z=env.z)
    want.pop("_timings")
    return want


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want), what
    for f in want:
        assert got[f] == want[f], (what, f, len(got[f]), len(want[f]), brec_cases._first_difference(got[f], want[f]))


# ---------------------------------------------------------------------------------------------------------------- case 1
def case_entry_point(lib):
    getattr(lib.L, "lh_bam_append_resident")
    assert "lh_bam_append_resident" in capi.EXPORTED_SYMBOLS
    assert hasattr(capi.BamWriter, "append_resident")


# ---------------------------------------------------------------------------------------------------------------- case 2
def case_files_equal(env, tmp, batches, cap, all_features):
    """the resident path on every append against the judge; returns the feature counts of what was written"""
    assert len(batches) >= 3
    got, results, timings = resident_files(env, env.idx.context(cap), tmp / "res", batches)
    counts = brec_cases.feature_counts(env.lib, env.names, results)
    print(counts)
    assert_same(got, judge(env, tmp / "host", results), "resident")
    assert len(got) == 7
    for f in got:
        brec_cases.bam_reader.read_bam(str(tmp / "res" / f))
    for x in timings:   # out[0] the gather kernels' time from events, out[1] the text's upload
        assert x["gather_s"] > 0 and x["upload_s"] >= 0 and x["join_s"] == 0 and x["write_s"] >= 0, x
        assert 0 <= x["records_s"] <= x["gather_s"] + x["upload_s"] + x["plan_s"] + x["encode_s"] + 1e-9, x
    present = {k for k, v in counts.items() if v >= 1}
    if all_features:
        assert present == set(counts), counts
    return counts


# ---------------------------------------------------------------------------------------------------------------- case 3
def case_alternation(env, tmp, batches, cap):
    """resident, device and host records between the appends of one writer, in two phases: `pending` is all the paths share"""
    assert len(batches) >= 3
    orders = {"phase0": ("res", "dev", "host"), "phase1": ("host", "res", "dev"), "phase2": ("dev", "host", "res")}
    want = None
    for name, order in orders.items():
        got, results, _ = resident_files(env, env.idx.context(cap), tmp / name, batches, path_of=lambda k: order[k % 3])
        if want is None:
            want = judge(env, tmp / "host", results)
        assert_same(got, want, name)


# ---------------------------------------------------------------------------------------------------------------- case 4
UNEVEN = [7, 43, 11, 39, 20]   # pairs per barcode: the lanes' cuts fall at different reads for two and for three lanes


def uneven_batch(env, tmp):
    rs = synth.make_reads(env.contigs, env.names, n_barcodes=len(UNEVEN), pairs_per_barcode=sum(UNEVEN) // len(UNEVEN), seed=23, sub_hi=0.03, indel_rate=0.002, junk_frac=0.05)
    assert rs.n_pairs == sum(UNEVEN)
    rs.bc_pair_off = np.concatenate([[0], np.cumsum(UNEVEN)]).astype(rs.bc_pair_off.dtype)
    bs = ingest_batches(env.lib, rs, tmp / "in", max_pairs=sum(UNEVEN))
    assert len(bs) == 1 and bs[0].n_pairs == sum(UNEVEN) and list(np.diff(bs[0].bc_pair_off)) == UNEVEN, [list(b.bc_pair_off) for b in bs]
    return bs


def case_lanes(env, tmp):
    bs = uneven_batch(env, tmp)
    one, results, _ = resident_files(env, env.idx.context(sum(UNEVEN)), tmp / "lanes1", bs)
    assert_same(one, judge(env, tmp / "host", results), "lanes=1")
    firsts = []
    for lanes in (2, 3):
        ctx = env.idx.context(sum(UNEVEN), lanes=lanes)
        got, _, _ = resident_files(env, ctx, tmp / ("lanes%d" % lanes), bs)
        assert_same(got, one, "lanes=%d" % lanes)
        info = [ctx.rounds(lane) for lane in range(lanes)]
        assert all(i["n_rounds"] == 1 for i in info), info   # every lane took its part
        firsts.append([int(i["first_barcode"][0]) for i in info])
    assert firsts[0][1:] != firsts[1][1:2], firsts   # the cuts differ
    return firsts


# ---------------------------------------------------------------------------------------------------------------- case 5
def case_many_candidates(env, tmp, n_barcodes, pairs):
    """the repeat-family miniature (helpers.repeat_family_case): a read's active alignment, second best and mate lie far behind cand_off[read]"""
    names, contigs, rs = helpers.repeat_family_case(13, n_barcodes, pairs=pairs)
    lens = [len(c) for c in contigs]
    bs = ingest_batches(env.lib, rs, tmp / "in", max_pairs=rs.n_pairs)
    ctx = env.index(names, contigs).context(rs.n_pairs)
    got, results, _ = resident_files(env, ctx, tmp / "res", bs, names=names, lens=lens)
    res = results[0][0]
    per_read = res.n_cand / res.n_reads
    far = np.asarray(res.active_idx) - np.asarray(res.cand_off[:-1])
    sb = np.asarray(res.second_best_idx)
    print("%.1f candidates per read, active up to %d behind cand_off, %d reads with a second best" % (per_read, far.max(), (sb >= 0).sum()))
    assert per_read > 4 and far.max() >= 4 and (sb >= 0).sum() > 10   # (the input's own shape: indices well behind the read's first candidate)
    assert_same(got, judge(env, tmp / "host", results, names, lens), "repeat families")
    return per_read


def case_pool_continuation(env, tmp):
    """a 235-base read with 80 bases N between clean ends: its alignment has more mismatch loci than the 64 slots per candidate, the rest continue in the batch's
    pool (DCand::mm_xoff); its record's AC tag lists them all"""
    rs = synth.make_reads(env.contigs, env.names, n_barcodes=2, pairs_per_barcode=12, seed=5, len1=235, len2=150, sub_lo=0.0, sub_hi=0.0, indel_rate=0.0)
    long_reads = [r for r in range(0, 2 * rs.n_pairs, 2) if rs.seq_off[r + 1] - rs.seq_off[r] == 235]
    for r in long_reads[:6]:
        at = int(rs.seq_off[r])
        rs.seq[at + 21:at + 181:2] = 4
    bs = ingest_batches(env.lib, rs, tmp / "in", max_pairs=rs.n_pairs)
    got, results, _ = resident_files(env, env.idx.context(rs.n_pairs), tmp / "res", bs)
    res = results[0][0]
    n_mm = np.diff(np.asarray(res.mm_off))[np.asarray(res.active_idx)]
    print("mismatch loci of the active alignments, the largest:", sorted(n_mm)[-6:])
    assert n_mm.max() >= 70, sorted(n_mm)[-6:]
    assert_same(got, judge(env, tmp / "host", results), "pool")
    return int(n_mm.max())


# ---------------------------------------------------------------------------------------------------------------- case 6
def case_context_untouched(env, tmp, batch):
    """a download after append_resident returns what a twin context that only downloaded returns; download first, then append: the same files"""
    a, b = env.idx.context(batch.n_pairs), env.idx.context(batch.n_pairs)
    got, results, _ = resident_files(env, a, tmp / "a", [batch])
    ra = results[0][0]
    b.upload(batch)
    b.align_resident(env.lib.opts())
    rb = b.download()
    assert (ra.n_reads, ra.n_cand) == (rb.n_reads, rb.n_cand)
    n = 0
    for name, _ in capi.LhResult._fields_:
        if name in ("abi_version", "n_reads", "n_cand", "arena_") or name in capi._COUNTERS:
            continue
        x, y = np.asarray(getattr(ra, name)), np.asarray(getattr(rb, name))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
        n += 1
    assert n == 42 and ra.counters == rb.counters and len(ra.counters) == 19
    got2, _, _ = resident_files(env, env.idx.context(batch.n_pairs), tmp / "b", [batch], download_first=True)
    assert_same(got2, got, "download first")
    assert_same(got, judge(env, tmp / "host", results), "twin")


# ---------------------------------------------------------------------------------------------------------------- case 7
def sized_batches(env, tmp, barcodes, batches, seed=31):
    """ingest batches of `batches` pairs each, over barcodes of `barcodes` pairs (the reader hands out whole barcodes)"""
    n = len(barcodes)
    assert sum(barcodes) % n == 0 and sum(barcodes) == sum(batches)
    rs = synth.make_reads(env.contigs, env.names, n_barcodes=n, pairs_per_barcode=sum(barcodes) // n, seed=seed, sub_hi=0.03, indel_rate=0.002, junk_frac=0.05)
    rs.bc_pair_off = np.concatenate([[0], np.cumsum(barcodes)]).astype(rs.bc_pair_off.dtype)
    (tmp / "in").mkdir(parents=True)
    path = tmp / "in" / "r.fastq"
    path.write_text(brec_cases.fastq9(rs, trim_prefix=7))
    ing = env.lib.ingest(str(path), trim=7, max_pairs=max(batches))
    bs = [ing.next(max_pairs=k) for k in batches]
    assert [b.n_pairs for b in bs] == list(batches), [b.n_pairs for b in bs]
    return bs, ing


def case_reuse(env, tmp, sizes):
    """one context and one encoder (a compressor of its own: its buffers start empty): a larger batch, a smaller one, one larger than both"""
    assert sizes[1] < sizes[0] < sizes[2]
    bs, ing = sized_batches(env, tmp, sizes, sizes)
    z0, env.z = env.z, env.lib.bgzf(max_blocks=4)
    try:
        got, results, _ = resident_files(env, env.idx.context(max(sizes)), tmp / "res", bs)
        assert_same(got, judge(env, tmp / "host", results), "reuse")
    finally:
        env.z.close()
        env.z = z0
    ing.close()


# ---------------------------------------------------------------------------------------------------------------- case 8
def case_empty(env, tmp, batches):
    empty, ing = brec_cases.empty_batch_like(env.lib, tmp)
    seq = [batches[0], empty, batches[1]]
    got, results, _ = resident_files(env, env.idx.context(max(b.n_pairs for b in batches[:2])), tmp / "mid", seq)
    assert_same(got, judge(env, tmp / "mid_host", results), "empty between")
    got, results, _ = resident_files(env, env.idx.context(8), tmp / "only", [empty])   # (a context that has aligned nothing: nothing of it is read)
    assert_same(got, judge(env, tmp / "only_host", results), "empty alone")
    ing.close()


# ---------------------------------------------------------------------------------------------------------------- case 9
def kib_up(nbytes):
    return -(-int(nbytes) // 1024)


def case_errors(env, tmp):
    """every refusal one device can reach: LH_E_ARG each, its cause named, and the writer's files afterwards are those written without that append.  (Not
    reachable here: compressor and context on different devices, which needs two; the device-side "no active alignment" word, since a run with inference gives
    every read an active alignment, a placeholder for a read without candidates.  A result that fails the checks shared with lh_result_download: case_shared_check.)"""
    lib, z = env.lib, env.z
    (b0, b1), ing = sized_batches(env, tmp, (20, 20, 20, 28), (60, 28), seed=37)   # three barcodes: rounds are reachable
    cap = 60

    def refused(w, ctx, b, *words):
        try:
            w.append_resident(ctx, b)
        except capi.LhError as e:
            assert e.code == capi.LH_E_ARG, (e.code, str(e))
            for word in words:
                assert word in str(e), (word, str(e))
            return
        raise AssertionError("append_resident was not refused (%s)" % (words,))

    ctx = env.idx.context(cap)
    fresh = env.idx.context(cap)
    whole = env.idx.context(cap)   # for the rounds: what the batch needs when it runs whole
    whole.upload(b0)
    whole.align_resident(lib.opts())
    info = whole.rounds()
    assert info["n_rounds"] == 1
    in_rounds = env.idx.context(cap, seed_budget_kb=kib_up(max(info["need_bytes"] / 3.5, info["max_barcode_need_bytes"])))
    outdir = tmp / "got"
    outdir.mkdir(parents=True)
    results = []
    with brec_cases.open_writer(lib, outdir, env.names, env.lens, **brec_cases.WRITER) as w:
        refused(w, ctx, b0, "compressor")                       # no compressor
        w.set_device(z)
        refused(w, ctx, b0, "device records")                   # a compressor, no device records
        w.set_device_records(True)
        refused(w, None, b0, "null")
        refused(w, ctx, None, "null")
        refused(w, fresh, b0, "lh_align_resident first")        # nothing aligned yet
        fresh.upload(b0)
        refused(w, fresh, b0, "lh_align_resident first")        # ... uploaded, not aligned
        ctx.upload(b0)
        ctx.align_resident(lib.opts(run_inference=0))
        refused(w, ctx, b0, "without inference")
        ctx.align_resident(lib.opts())
        w.set_debug_tags(True)
        refused(w, ctx, b0, "LH_REC_DEBUG_TAGS")
        w.set_debug_tags(False)
        refused(w, ctx, b1, "28 pairs", "aligned 60")           # not the batch the context aligned
        w.append_resident(ctx, b0)                              # the same context and writer go on
        results.append((ctx.download(), b0))
        in_rounds.upload(b0)
        in_rounds.align_resident(lib.opts())
        assert in_rounds.rounds()["n_rounds"] > 1
        refused(w, in_rounds, b0, "rounds", "lh_result_download + lh_bam_append cost nothing extra")
        ctx.upload(b1)
        refused(w, ctx, b1, "lh_align_resident first")          # the upload made the previous result stale
        ctx.align_resident(lib.opts())
        refused(w, ctx, b0, "60 pairs", "aligned 28")
        w.append_resident(ctx, b1)
        results.append((ctx.download(), b1))
    assert_same(written(outdir), judge(env, tmp / "host", results), "after the refusals")
    ing.close()


def case_shared_check(env, tmp):
    """a result that lh_result_download refuses is refused by lh_bam_append_resident with the same code and message, nothing is appended and the writer goes on.
    The refusal: 28,000 reads of 247 bases with 94 N each; every alignment has 94 mismatch loci, 30 more than a candidate's slots, and takes 183 entries of the
    batch's pool of 2^22, which runs out after some 22,900 of them: LH_ST_MM_OVERFLOW, LH_E_LIMIT.  (A batch of this size is the smallest that fills the pool:
    the device aligns it in well under a second, the emulator would take minutes, so this case runs on the device alone.)"""
    lib = env.lib
    pac, l_pac, _, _ = lib.reference_pack(env.contigs)
    offs = np.concatenate([[0], np.cumsum(env.lens)])
    ctg = [(env.names[k], env.lens[k], int(offs[k])) for k in range(len(env.names))]
    r = lib.synth_reads(pac, l_pac, ctg, seed=41, n_barcodes=2, pairs_per_barcode=7000, len1=247, len2=247, sub_lo=0.0, sub_hi=0.0, indel_rate=0.0)
    so = np.asarray(r["seq_off"][:-1])
    assert (np.diff(r["seq_off"]) == 247).all()
    r["seq"][(so[:, None] + np.arange(31, 219, 2)[None, :]).ravel()] = 4
    (tmp / "in").mkdir(parents=True)
    lib.write_fastq9(str(tmp / "in" / "big.fastq"), r, gz_level=0)
    ing = lib.ingest(str(tmp / "in" / "big.fastq"), trim=7, max_pairs=r["n_pairs"])
    big = ing.next()
    assert big.n_pairs == r["n_pairs"]
    (good,), ing2 = sized_batches(env, tmp / "good", (12, 12), (24,), seed=43)
    ctx = env.idx.context(big.n_pairs)
    outdir = tmp / "got"
    outdir.mkdir(parents=True)
    results = []
    with brec_cases.open_writer(lib, outdir, env.names, env.lens, **brec_cases.WRITER) as w:
        w.set_device(env.z)
        w.set_device_records(True)
        ctx.upload(big)
        ctx.align_resident(lib.opts())
        errs = []
        for call in (lambda: w.append_resident(ctx, big), ctx.download):
            try:
                call()
                raise AssertionError("a result over the mismatch pool was not refused")
            except capi.LhError as e:
                errs.append((e.code, str(e)))
        print(errs)
        assert errs[0][0] == errs[1][0] == capi.LH_E_LIMIT, errs
        named = errs[1][1][errs[1][1].index("read "):]   # "read N (pair M) exceeds a per-read limit (status bits ...); K such reads in the batch"
        assert "exceeds a per-read limit" in named and named in errs[0][1] and "nothing was appended" in errs[0][1], errs
        ctx.upload(good)
        ctx.align_resident(lib.opts())
        w.append_resident(ctx, good)   # the same context, compressor and writer go on
        results.append((ctx.download(), good))
    assert_same(written(outdir), judge(env, tmp / "host", results), "after the refused result")
    ing.close()
    ing2.close()
