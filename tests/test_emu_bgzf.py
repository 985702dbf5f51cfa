"""The device compressor of BGZF blocks (lariat_amd/csrc/k_bgzf.h, lh_bgzf.inc) with its kernel source under the CPU emulator.  The judge is Python's gzip / zlib
(bgzf_cases.check): every member must inflate to its input with the right CRC-32 and ISIZE, and tests/bam_reader.py must accept the framing."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_reader
import bgzf_cases
import helpers
from lariat_amd import capi, synth

EMU = os.environ.get("LH_EMU_LIB") or os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "hipemu")])
    return capi.Library(EMU)


@pytest.fixture(scope="module")
def z(emu):
    z = emu.bgzf(max_blocks=4)
    yield z
    z.close()


@pytest.mark.parametrize("case", sorted(bgzf_cases.CASES))
def test_case(z, case):
    """cases 1 - 7: lengths on three contents, the distance boundary, every length and distance code, the 15-bit limit, degenerate codes, the literal-only
    coding, matches"""
    bgzf_cases.CASES[case](z)


def test_determinism_and_chunking(emu):
    bgzf_cases.case_chunking(emu)


@pytest.fixture(scope="module")
def bam_batches(emu, oracle, tmp_path_factory):
    """the batch of test_records.py::test_bam_files_round_trip, aligned by the oracle"""
    tmp = tmp_path_factory.mktemp("bgzf_bam")
    names, contigs = helpers.small_genome()
    oidx = oracle.index_build_naive(names, contigs)
    rs = synth.make_reads(contigs, names, n_barcodes=4, pairs_per_barcode=60, seed=67, sub_hi=0.03, indel_rate=0.002, junk_frac=0.06)
    path = tmp / "r.fastq"
    path.write_text(synth.to_fastq9(rs, trim_prefix=7))
    batches = [(oidx.align_barcodes(b, threads=4), b) for b in emu.ingest(str(path), trim=7, max_pairs=100)]
    assert len(batches) >= 3
    return names, [len(c) for c in contigs], batches


def write_files(lib, outdir, bam_batches, device_of):
    """one file set; device_of(k): the compressor (or None) set before append k and, for k = number of batches, before close"""
    names, lens, batches = bam_batches
    outdir.mkdir()
    w = lib.bam_writer(str(outdir), names, lens, read_groups="s:lib:1:fc:1,bad", position_chunk_size=150000, first_chunk=True, command_line="lariat_amd test", threads=3)
    for k, (res, b) in enumerate(batches):
        w.set_device(device_of(k))
        w.append(res, b)
    w.set_device(device_of(len(batches)))
    w.close()
    return {f: open(outdir / f, "rb").read() for f in sorted(os.listdir(outdir))}


def test_writer_on_the_device(emu, z, bam_batches, tmp_path):
    host = write_files(emu, tmp_path / "host", bam_batches, lambda k: None)
    dev = write_files(emu, tmp_path / "dev", bam_batches, lambda k: z)
    mixed = write_files(emu, tmp_path / "mixed", bam_batches, lambda k: None if k % 2 else z)   # device, host, device, ...
    assert len(host) == 7 and sorted(dev) == sorted(host) == sorted(mixed)
    for f in host:
        want = gzip.decompress(host[f])
        for name, got in (("dev", dev), ("mixed", mixed)):
            assert gzip.decompress(got[f]) == want, (name, f)
            assert got[f].endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
            bam_reader.read_bam(str(tmp_path / name / f))   # framing, end-of-file block, records
    assert dev["bc_sorted_bam.bam"] != host["bc_sorted_bam.bam"]   # (another compressor wrote it)
    # a writer with no compressor set writes what the host path always wrote: zlib's bytes
    raw = host["bc_sorted_bam.bam"]
    size, isize = bam_reader.bgzf_blocks(raw)[0]
    data = gzip.decompress(raw)[:isize]
    c = __import__("zlib").compressobj(-1, 8, -15, 8, 0)
    assert raw[18:size - 8] == c.compress(data) + c.flush()


def test_errors(emu, z):
    L = emu.L
    data = np.frombuffer(bgzf_cases.content("counter", 1000), dtype=np.uint8)
    need = z.bound(data.size)
    assert need == 1000 + 31 and z.bound(0) == 0 and z.bound(bgzf_cases.BLOCK + 1) == bgzf_cases.BLOCK + 1 + 62
    out = np.full(need, 0xAB, dtype=np.uint8)
    n_out = C.c_int64(-7)
    assert L.lh_bgzf_compress(z.h, data.ctypes.data, data.size, out.ctypes.data, need - 1, C.byref(n_out)) == capi.LH_E_ARG
    assert (out == 0xAB).all() and n_out.value == -7   # nothing written
    with pytest.raises(capi.LhError):
        emu.bgzf(max_blocks=-1)
    # a device allocation that fails: an error, and every device buffer is given back.  The compressor allocates everything in lh_bgzf_create (a compress
    # allocates nothing on the device, so the loop's compress is only reached when the creation did not fail); the emulator counts hipMalloc alone, so the
    # failure paths of the page-locked staging (hipHostMalloc) are not reached by this test
    L.emu_alloc_live.restype = C.c_longlong
    L.emu_alloc_calls.restype = C.c_longlong
    L.emu_alloc_fail_at.argtypes = [C.c_longlong]
    live0 = L.emu_alloc_live()
    calls0 = L.emu_alloc_calls()
    z2 = emu.bgzf(max_blocks=2)
    assert z2.compress(data.tobytes()) == z.compress(data.tobytes())
    z2.close()
    n_allocs = L.emu_alloc_calls() - calls0
    assert n_allocs >= 5 and L.emu_alloc_live() == live0
    for k in range(1, n_allocs + 1):
        L.emu_alloc_fail_at(k)
        try:
            with pytest.raises(capi.LhError) as e:
                z3 = emu.bgzf(max_blocks=2)
                z3.compress(data.tobytes())
            assert e.value.code == capi.LH_E_HIP
        finally:
            L.emu_alloc_fail_at(0)
        assert L.emu_alloc_live() == live0, k
