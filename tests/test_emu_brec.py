"""BAM records derived and encoded on the device (lariat_amd/csrc/k_brec.h, lh_brec.inc; lh_bam_set_device_records) with the kernel sources under the CPU
emulator.  The judge is the host record path with the same compressor (brec_cases.same_files): equal files, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import brec_cases
import helpers
from lariat_amd import capi

EMU = os.environ.get("LH_EMU_LIB") or os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "hipemu")])
    return capi.Library(EMU)


@pytest.fixture(scope="module")
def z(emu):
    z = emu.bgzf(max_blocks=4)   # an append spans several chunks and both buffer sets
    yield z
    z.close()


@pytest.fixture(scope="module")
def genome():
    names, contigs = helpers.small_genome()
    return names, contigs, [len(c) for c in contigs]


@pytest.fixture(scope="module")
def batches(emu, oracle, genome, tmp_path_factory):
    """4 barcodes x 60 pairs aligned by the oracle, three appends or more"""
    names, contigs, _ = genome
    oidx = oracle.index_build_naive(names, contigs)
    got = brec_cases.make_batches(emu, lambda b: oidx.align_barcodes(b, threads=4), names, contigs, tmp_path_factory.mktemp("brec"), n_barcodes=4, max_pairs=100)
    assert len(got) >= 3
    return got


def test_entry_points(emu):
    for sym in ("lh_bam_set_device_records", "lh_bam_records_timings", "lh_diag_format_f6"):
        getattr(emu.L, sym)
        assert sym in capi.EXPORTED_SYMBOLS


def test_files_equal(emu, z, genome, batches, tmp_path):
    """cases 1 and 2: the comparison is over batches that hold every feature the device path has a rule for, and the files are equal byte for byte"""
    names, _, lens = genome
    counts = brec_cases.feature_counts(emu, names, batches)
    print(counts)
    assert all(v >= 1 for v in counts.values()), counts
    files = brec_cases.same_files(emu, z, tmp_path, names, lens, batches, orders=("dev", "switch", "switch2"))
    assert len(files) == 7


def test_crafted_values(emu, z, genome, batches, tmp_path):
    """what the synthetic reads do not produce: NaN / out-of-range XS and AS (x86's conversion), long and negative loci, DM values on rounding ties, a mapq over 255"""
    names, _, lens = genome
    made = [brec_cases.crafted_extras(res) for res, _ in batches[:2]]
    assert sum(n for _, n in made) >= 5
    edited = [(r, b) for (r, _), (_, b) in zip(made, batches)]
    brec_cases.same_files(emu, z, tmp_path, names, lens, edited, orders=("dev",))


@pytest.mark.parametrize("which", brec_cases.CRAFTED)
def test_crafted_pairs(emu, z, genome, batches, tmp_path, which):
    """case 3: the order of AppendBam's edits inside a pair"""
    names, _, lens = genome
    src = next((res, b) for res, b in batches if which not in ("c", "c2") or (np.asarray(res.split_idx) >= 0).any())
    brec_cases.same_files(emu, z, tmp_path, names, lens, [(brec_cases.crafted(src[0], which), src[1])], orders=("dev",))


def test_layout_many_contigs(emu, z, genome, batches, tmp_path):
    """case 4: 2,000 short contigs behind the real ones: the header exceeds one block before the first record, the short contigs' packing yields many files"""
    names, _, lens = genome
    names2 = names + ["short%04d" % k for k in range(2000)]
    lens2 = lens + [20000 + 7 * k for k in range(2000)]
    wide = dict(brec_cases.WRITER, position_chunk_size=2000000)   # (the emulator compresses some 40 blocks a second: every file's header is two)
    files = brec_cases.same_files(emu, z, tmp_path, names2, lens2, batches[:2], writer=wide, orders=("dev",), readable=False)
    assert len(files) > 25 and all(len(brec_cases.gzip.decompress(f)) > 0xff00 for f in files.values())


def test_layout_one_bucket_and_small_chunks(emu, z, genome, batches, tmp_path):
    """case 4: every record in one bucket (the other files' segments are empty); a contig of more than 30 buckets with positions past the last chunk's start"""
    names, _, lens = genome
    one = dict(brec_cases.WRITER, position_chunk_size=1000000)
    res, b = batches[0]
    mapped = brec_cases.copy.deepcopy(res)   # every alignment on chrA, mapped: nothing goes to the unmapped file either
    mapped.rid[:] = 0
    mapped.pos[:] = np.abs(mapped.pos) % 200000
    mapped.aend[:] = mapped.pos + 100
    mapped.is_proper[:] = 1
    files = brec_cases.same_files(emu, z, tmp_path / "one", names, lens, [(mapped, b)], writer=one, orders=("dev",))
    assert len(files) == 3
    tmp2 = tmp_path / "small"
    small = dict(brec_cases.WRITER, position_chunk_size=9000)
    far = brec_cases.copy.deepcopy(res)
    a = int(far.active_idx[0])
    far.pos[a] = 299990; far.aend[a] = 300100   # in the last chunk
    a = int(far.active_idx[2])
    far.pos[a] = 400000; far.aend[a] = 400100   # past the contig's end: the last chunk
    files = brec_cases.same_files(emu, z, tmp2, names, lens, [(far, b)] + batches[1:2], writer=small, orders=("dev",), readable=False)
    assert len(files) > 60


def test_layout_empty_batch(emu, z, genome, batches, tmp_path):
    names, _, lens = genome
    empty, ing = brec_cases.empty_batch_like(emu, tmp_path)
    seq = [batches[0], (brec_cases.empty_result(), empty), batches[1]]
    brec_cases.same_files(emu, z, tmp_path / "w", names, lens, seq, orders=("dev",))
    brec_cases.same_files(emu, z, tmp_path / "only", names, lens, [(brec_cases.empty_result(), empty)], orders=("dev",))
    ing.close()


def test_limits_and_errors(emu, z, oracle, genome, tmp_path):
    names, contigs, lens = genome
    oidx = oracle.index_build_naive(names, contigs)

    def batches_with_name(n, d):
        rs = brec_cases.synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=12, seed=5)
        rs.names[7] = "n" * n
        d.mkdir()
        p = d / "r.fastq"
        p.write_text(brec_cases.fastq9(rs))
        return [(oidx.align_barcodes(b, threads=2), b) for b in emu.ingest(str(p), trim=7, max_pairs=100)]

    ok = batches_with_name(254, tmp_path / "n254")
    bad = batches_with_name(255, tmp_path / "n255")
    brec_cases.same_files(emu, z, tmp_path / "ok", names, lens, ok, orders=("dev",))
    # a 255-byte name: LH_E_LIMIT, and the files written afterwards equal those of a writer that never saw that batch
    want = brec_cases.write_files(emu, tmp_path / "want", names, lens, ok, lambda k: "host", z=z)
    got = brec_cases.write_files(emu, tmp_path / "got", names, lens, [(bad[0][0], bad[0][1], capi.LH_E_LIMIT)] + ok, lambda k: "dev", z=z)
    want.pop("_timings"); got.pop("_timings")
    assert got == want
    # no compressor: LH_E_ARG; debug tags with device records: LH_E_ARG, nothing appended
    with brec_cases.open_writer(emu, tmp_path, names, lens) as w:
        with pytest.raises(capi.LhError) as e:
            w.set_device_records(True)
        assert e.value.code == capi.LH_E_ARG
        w.set_device(z)
        w.set_device_records(True)
        w.set_device(None)   # ... which also switches the device records off: the append below is the host's
        w.append(*ok[0])
    got = brec_cases.write_files(emu, tmp_path / "dbg", names, lens, [(ok[0][0], ok[0][1], capi.LH_E_ARG)], lambda k: "dev", z=z, debug_tags=True)
    none = brec_cases.write_files(emu, tmp_path / "none", names, lens, [], lambda k: "host", z=z)
    got.pop("_timings"); none.pop("_timings")
    assert got == none


def test_allocation_failures(emu, genome, batches, tmp_path):
    """every device allocation of the encoder's first append made to fail in turn: an error each time, and every device buffer is given back"""
    names, _, lens = genome
    L = emu.L
    L.emu_alloc_live.restype = C.c_longlong
    L.emu_alloc_calls.restype = C.c_longlong
    L.emu_alloc_fail_at.argtypes = [C.c_longlong]
    live0 = L.emu_alloc_live()

    def run(k, fail_at):
        z2 = emu.bgzf(max_blocks=2)
        try:
            calls0 = L.emu_alloc_calls()
            d = tmp_path / ("f%d" % k)
            d.mkdir()
            failed = None
            try:
                with brec_cases.open_writer(emu, d, names, lens, **brec_cases.WRITER) as w:   # (closed before its compressor is)
                    w.set_device(z2)
                    w.set_device_records(True)
                    L.emu_alloc_fail_at(fail_at)
                    try:
                        w.append(*batches[0])
                    finally:
                        L.emu_alloc_fail_at(0)
                    n = L.emu_alloc_calls() - calls0
            except capi.LhError as e:   # the append's error, or the close's of a writer that has failed
                failed = e
                n = L.emu_alloc_calls() - calls0
            return n, failed
        finally:
            z2.close()

    n_allocs, failed = run(0, 0)
    assert failed is None and n_allocs >= 6 and L.emu_alloc_live() == live0
    for k in range(1, n_allocs + 1):
        _, failed = run(k, k)
        assert failed is not None and failed.code == capi.LH_E_IO, k
        assert L.emu_alloc_live() == live0, k


def test_format_f6(emu):
    """case 6: the device's %.6f against Python's (correctly rounded, as glibc's is)"""
    assert brec_cases.check_f6(emu, 1500) > 1500
