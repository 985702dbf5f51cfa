"""lh_bam_append_resident (BAM records gathered on the device from the context's resident result: k_brec.h's k_brec_gather_count / k_brec_gather_fill, lh_brec.inc)
with the kernel sources under the CPU emulator: the emulator's own pipeline aligns, the judge is lh_result_download + lh_bam_append with host records and the same
compressor (brec_resident_cases): equal files, byte for byte.  tests/test_gpu_brec_resident.py runs the same cases on the device."""
import os
import subprocess

import pytest

import brec_resident_cases as cases
import helpers
from lariat_amd import capi

EMU = os.environ.get("LH_EMU_LIB") or os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "hipemu")])
    return capi.Library(EMU)


@pytest.fixture(scope="module")
def env(emu, oracle):
    z = emu.bgzf(max_blocks=4)   # an append spans several chunks and both buffer sets
    yield cases.Env(emu, oracle, z)
    z.close()


@pytest.fixture(scope="module")
def batches(env, tmp_path_factory):
    """brec_cases.make_batches' reads, 3 barcodes (the helper makes them of 60 pairs), an append per barcode"""
    got = cases.feature_batches(env, tmp_path_factory.mktemp("brec_res"), n_barcodes=3, max_pairs=70)
    assert [b.n_pairs for b in got] == [60, 60, 60]
    return got


def test_entry_point(emu):
    """case 1"""
    cases.case_entry_point(emu)


def test_files_equal(env, batches, tmp_path):
    """case 2: every append by the resident path; this input holds every feature the device path has a rule for (the counts are printed)"""
    cases.case_files_equal(env, tmp_path, batches, cap=70, all_features=True)


def test_alternation(env, batches, tmp_path):
    """case 3"""
    cases.case_alternation(env, tmp_path, batches, cap=70)


def test_lanes(env, tmp_path):
    """case 4: two and three lanes, cut at different reads"""
    print(cases.case_lanes(env, tmp_path))


def test_many_candidates(env, tmp_path):
    """case 5: the repeat-family miniature"""
    cases.case_many_candidates(env, tmp_path, n_barcodes=2, pairs=20)


def test_pool_continuation(env, tmp_path):
    """case 5: more mismatch loci than a candidate's 64 slots"""
    cases.case_pool_continuation(env, tmp_path)


def test_context_untouched(env, batches, tmp_path):
    """case 6"""
    cases.case_context_untouched(env, tmp_path, batches[0])


def test_reuse(env, tmp_path):
    """case 7"""
    cases.case_reuse(env, tmp_path, (30, 12, 48))


def test_empty_batch(env, batches, tmp_path):
    """case 8"""
    cases.case_empty(env, tmp_path, batches)


def test_errors(env, tmp_path):
    """case 9"""
    cases.case_errors(env, tmp_path)
