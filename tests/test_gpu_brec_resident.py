"""lh_bam_append_resident on the GPU: BAM records gathered by k_brec_gather_count / k_brec_gather_fill (k_brec.h) from the context's resident result, without
lh_result_download.  The cases of test_emu_brec_resident.py through the product library; the judge is lh_result_download + lh_bam_append with host records and the same
compressor (brec_resident_cases): equal files, byte for byte."""
import pytest

import brec_resident_cases as cases
from lariat_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


@pytest.fixture(scope="module")
def env(lib, oracle):
    z = lib.bgzf(max_blocks=4)   # an append spans several chunks and both buffer sets
    yield cases.Env(lib, oracle, z)
    z.close()


@pytest.fixture(scope="module")
def batches(env, tmp_path_factory):
    """brec_cases.make_batches' reads, 6 barcodes x 60 pairs, three appends"""
    got = cases.feature_batches(env, tmp_path_factory.mktemp("brec_res"), n_barcodes=6, max_pairs=130)
    assert len(got) >= 3
    return got


def test_entry_point(lib):
    """case 1"""
    cases.case_entry_point(lib)


def test_files_equal(env, batches, tmp_path):
    """case 2: every append by the resident path, over batches that hold every feature the device path has a rule for"""
    cases.case_files_equal(env, tmp_path, batches, cap=130, all_features=True)


def test_alternation(env, batches, tmp_path):
    """case 3"""
    cases.case_alternation(env, tmp_path, batches, cap=130)


def test_lanes(env, tmp_path):
    """case 4: two and three lanes, cut at different reads"""
    print(cases.case_lanes(env, tmp_path))


def test_many_candidates(env, tmp_path):
    """case 5: the repeat-family miniature"""
    cases.case_many_candidates(env, tmp_path, n_barcodes=4, pairs=30)


def test_pool_continuation(env, tmp_path):
    """case 5: more mismatch loci than a candidate's 64 slots, continued in the batch's pool"""
    cases.case_pool_continuation(env, tmp_path)


def test_context_untouched(env, batches, tmp_path):
    """case 6"""
    cases.case_context_untouched(env, tmp_path, batches[0])


def test_reuse(env, tmp_path):
    """case 7"""
    cases.case_reuse(env, tmp_path, (60, 24, 96))


def test_empty_batch(env, batches, tmp_path):
    """case 8"""
    cases.case_empty(env, tmp_path, batches)


def test_errors(env, tmp_path):
    """case 9: every refusal one device can reach (two devices: not here)"""
    cases.case_errors(env, tmp_path)


def test_shared_result_check(env, tmp_path):
    """case 9: the checks shared with lh_result_download, through a batch that fills the mismatch pool"""
    cases.case_shared_check(env, tmp_path)
