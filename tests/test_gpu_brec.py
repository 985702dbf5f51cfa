"""BAM records derived and encoded on the GPU (lariat_amd/csrc/k_brec.h, lh_brec.inc; lh_bam_set_device_records): the cases of test_emu_brec.py through the product
library, on the product's own result.  The judge is the host record path with the same compressor (brec_cases.same_files): equal files, byte for byte."""
import copy

import numpy as np
import pytest

import brec_cases
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
    z = lib.bgzf(max_blocks=4)   # an append spans several chunks and both buffer sets
    yield z
    z.close()


@pytest.fixture(scope="module")
def genome():
    names, contigs = helpers.small_genome()
    return names, contigs, [len(c) for c in contigs]


@pytest.fixture(scope="module")
def aligner(lib, oracle, genome):
    names, contigs, _ = genome
    idx = lib.index_from_arrays(oracle.index_build_naive(names, contigs).arrays())
    ctx = idx.context(400)
    return ctx.align_barcodes


@pytest.fixture(scope="module")
def batches(lib, aligner, genome, tmp_path_factory):
    """the product's own result of 6 barcodes x 60 pairs, three appends"""
    names, contigs, _ = genome
    got = brec_cases.make_batches(lib, aligner, names, contigs, tmp_path_factory.mktemp("brec"), n_barcodes=6, max_pairs=130)
    assert len(got) >= 3
    return got


def test_files_equal(lib, z, genome, batches, tmp_path):
    """cases 1 and 2"""
    names, _, lens = genome
    counts = brec_cases.feature_counts(lib, names, batches)
    print(counts)
    assert all(v >= 1 for v in counts.values()), counts
    files = brec_cases.same_files(lib, z, tmp_path, names, lens, batches, orders=("dev", "switch", "switch2"))
    assert len(files) == 7


def test_crafted_values(lib, z, genome, batches, tmp_path):
    names, _, lens = genome
    made = [brec_cases.crafted_extras(res) for res, _ in batches[:2]]
    assert sum(n for _, n in made) >= 5
    brec_cases.same_files(lib, z, tmp_path, names, lens, [(r, b) for (r, _), (_, b) in zip(made, batches)], orders=("dev",))


@pytest.mark.parametrize("which", brec_cases.CRAFTED)
def test_crafted_pairs(lib, z, genome, batches, tmp_path, which):
    """case 3: the order of AppendBam's edits inside a pair"""
    names, _, lens = genome
    src = next((res, b) for res, b in batches if which not in ("c", "c2") or (np.asarray(res.split_idx) >= 0).any())
    brec_cases.same_files(lib, z, tmp_path, names, lens, [(brec_cases.crafted(src[0], which), src[1])], orders=("dev",))


def test_layout_many_contigs(lib, z, genome, batches, tmp_path):
    """case 4: 2,000 short contigs: a header of more than one block in front of the first record, and several hundred files"""
    names, _, lens = genome
    names2 = names + ["short%04d" % k for k in range(2000)]
    lens2 = lens + [20000 + 7 * k for k in range(2000)]
    files = brec_cases.same_files(lib, z, tmp_path, names2, lens2, batches[:2], orders=("dev", "switch"), readable=False)
    assert len(files) > 200


def test_layout_one_bucket_and_small_chunks(lib, z, genome, batches, tmp_path):
    names, _, lens = genome
    res, b = batches[0]
    mapped = copy.deepcopy(res)   # every alignment on chrA, mapped: nothing goes to the unmapped file either
    mapped.rid[:] = 0
    mapped.pos[:] = np.abs(mapped.pos) % 200000
    mapped.aend[:] = mapped.pos + 100
    mapped.is_proper[:] = 1
    files = brec_cases.same_files(lib, z, tmp_path / "one", names, lens, [(mapped, b)], writer=dict(brec_cases.WRITER, position_chunk_size=1000000), orders=("dev",))
    assert len(files) == 3
    far = copy.deepcopy(res)
    a = int(far.active_idx[0])
    far.pos[a] = 299990; far.aend[a] = 300100   # in the last chunk
    a = int(far.active_idx[2])
    far.pos[a] = 400000; far.aend[a] = 400100   # past the contig's end: the last chunk
    files = brec_cases.same_files(lib, z, tmp_path / "small", names, lens, [(far, b)] + batches[1:2], writer=dict(brec_cases.WRITER, position_chunk_size=9000), orders=("dev",),
                                  readable=False)
    assert len(files) > 60


def test_layout_empty_batch(lib, z, genome, batches, tmp_path):
    names, _, lens = genome
    empty, ing = brec_cases.empty_batch_like(lib, tmp_path)
    brec_cases.same_files(lib, z, tmp_path / "w", names, lens, [batches[0], (brec_cases.empty_result(), empty), batches[1]], orders=("dev",))
    brec_cases.same_files(lib, z, tmp_path / "only", names, lens, [(brec_cases.empty_result(), empty)], orders=("dev",))
    ing.close()


def test_limits_and_errors(lib, z, aligner, genome, tmp_path):
    names, contigs, lens = genome

    def batches_with_name(n, d):
        rs = synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=12, seed=5)
        rs.names[7] = "n" * n
        d.mkdir()
        p = d / "r.fastq"
        p.write_text(brec_cases.fastq9(rs))
        return [(aligner(b), b) for b in lib.ingest(str(p), trim=7, max_pairs=100)]

    ok = batches_with_name(254, tmp_path / "n254")
    bad = batches_with_name(255, tmp_path / "n255")
    brec_cases.same_files(lib, z, tmp_path / "ok", names, lens, ok, orders=("dev",))
    want = brec_cases.write_files(lib, tmp_path / "want", names, lens, ok, lambda k: "host", z=z)
    got = brec_cases.write_files(lib, tmp_path / "got", names, lens, [(bad[0][0], bad[0][1], capi.LH_E_LIMIT)] + ok, lambda k: "dev", z=z)
    want.pop("_timings"); got.pop("_timings")
    assert got == want
    with brec_cases.open_writer(lib, tmp_path, names, lens) as w:
        with pytest.raises(capi.LhError) as e:
            w.set_device_records(True)
        assert e.value.code == capi.LH_E_ARG
    got = brec_cases.write_files(lib, tmp_path / "dbg", names, lens, [(ok[0][0], ok[0][1], capi.LH_E_ARG)], lambda k: "dev", z=z, debug_tags=True)
    none = brec_cases.write_files(lib, tmp_path / "none", names, lens, [], lambda k: "host", z=z)
    got.pop("_timings"); none.pop("_timings")
    assert got == none


def test_format_f6(lib):
    """case 6: 20,000 values against Python's '%.6f' (correctly rounded, as glibc's is)"""
    assert brec_cases.check_f6(lib, 18000) >= 20000
