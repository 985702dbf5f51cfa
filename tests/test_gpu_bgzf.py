"""The device compressor of BGZF blocks on the GPU: the cases of test_emu_bgzf.py through the product library, the BAM writer on the product's own result,
and one input large enough to span several launches.  The judge is Python's gzip / zlib (bgzf_cases.check)."""
import gzip
import os

import pytest

import bam_reader
import bgzf_cases
import helpers
from lariat_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


@pytest.fixture(scope="module")
def z(lib):
    z = lib.bgzf(max_blocks=64)
    yield z
    z.close()


@pytest.mark.parametrize("case", sorted(bgzf_cases.CASES))
def test_case(z, case):
    bgzf_cases.CASES[case](z)


def test_determinism_and_chunking(lib):
    bgzf_cases.case_chunking(lib)


def test_writer_on_the_device(lib, z, oracle, tmp_path):
    """the product's result of a small batch written by the host writer, the device writer and one that switches between them: the same files, inflated"""
    names, contigs = helpers.small_genome()
    lens = [len(c) for c in contigs]
    idx = lib.index_from_arrays(oracle.index_build_naive(names, contigs).arrays())
    rs = synth.make_reads(contigs, names, n_barcodes=6, pairs_per_barcode=60, seed=71, sub_hi=0.03, indel_rate=0.002, junk_frac=0.05)
    p = tmp_path / "reads.fastq"
    p.write_text(synth.to_fastq9(rs, trim_prefix=7))
    ctx = idx.context(rs.n_pairs)
    batches = [(ctx.align_barcodes(b), b) for b in lib.ingest(str(p), trim=7, max_pairs=130)]
    assert len(batches) >= 3

    def write(name, device_of):
        d = tmp_path / name
        d.mkdir()
        w = lib.bam_writer(str(d), names, lens, position_chunk_size=1000000, threads=4)   # the three contigs share one position bucket
        for k, (res, b) in enumerate(batches):
            w.set_device(device_of(k))
            w.append(res, b)
        w.set_device(device_of(len(batches)))
        w.close()
        return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}

    host = write("host", lambda k: None)
    dev = write("dev", lambda k: z)
    mixed = write("mixed", lambda k: None if k % 2 else z)
    assert sorted(host) == sorted(dev) == sorted(mixed) and len(host) == 3
    for f in host:
        want = gzip.decompress(host[f])
        for name, got in (("dev", dev), ("mixed", mixed)):
            assert gzip.decompress(got[f]) == want, (name, f)
            bam_reader.read_bam(str(tmp_path / name / f))
    for f in ("bc_sorted_bam.bam", "000000-chrA_0000000000_pos_bucketed.bam"):
        assert len(bam_reader.bgzf_blocks(dev[f])) > 2, f   # more than one member and the end-of-file block


def test_many_blocks(lib):
    """4,000 blocks of mixed content through a compressor of 1,024 blocks per launch: four launches whose transfers overlap"""
    data = bgzf_cases.many_blocks(4000)
    z = lib.bgzf(max_blocks=1024)
    raw = z.compress(data)
    t = z.timings()
    z.close()
    assert t["kernel_s"] > 0 and t["upload_s"] > 0 and t["download_s"] > 0
    assert len(raw) < 0.6 * len(data)   # a quarter of the blocks is noise, the others compress well
    assert gzip.decompress(raw) == data
