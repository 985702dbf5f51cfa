"""K8's small-barcode instance (k_rfa.h: k_rfa<1>, hot tables in LDS) under the CPU emulator, on the cases of rfa_small_cases.py.  Two builds: the default one
(256 reads, 512 candidates, 128 molecules) and `tiny` (8 reads, 12 candidates, 4 molecules: the class boundaries fall inside barcodes of a few pairs).  Every case
against the oracle and, byte for byte, against the same build with every barcode in the regular instance (LH_F_RFA_SLAB).

Variants tried while the tests were written, each of which these cases fail: no turn-away at the molecule cap (the molecule-overflow case: wrong confidences);
the on-chip molecule flags never written (caps and usual cases: active_molecule); the on-chip tables placed over fastScore's staging (default build: the usual case
crashes).  Which instance took how many barcodes is asserted too (Context.rfa_classes): k_rfa_order listing nothing, or everything, as small changes no result
— the instance itself turns away what is beyond its caps — and fails on the counts."""
import importlib.util
import os
import subprocess

import pytest

import helpers
import rfa_small_cases as rc
from lariat_amd import capi
from test_emu_k1_ring import CXXFLAGS, CS, HIPEMU, OUT

CAPS = {"default": rc.DEFAULT_CAPS, "tiny": rc.TINY_CAPS}


def _build_tiny():
    so = os.path.join(OUT, "liblariat_emu_rfa_tiny.so")
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + rc.TINY_DEFINES + ["-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
              [os.path.join(CS, f) for f in ("index_build.cpp", "ingest.cpp", "records.cpp", "bamfile.cpp", "synth.cpp")] + ["-lz"]
        subprocess.check_call(cmd, cwd=HIPEMU)
        os.replace(so + ".tmp", so)
    return so


@pytest.fixture(scope="module")
def libs():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    return {"default": capi.Library(os.path.join(OUT, "liblariat_emu.so")), "tiny": capi.Library(_build_tiny())}


@pytest.mark.parametrize("build", ["default", "tiny"])
def test_emu_rfa_small_caps(libs, oracle, build):
    """reads at cap - 2, cap, cap + 2 and candidates at cap - 1, cap, cap + 1"""
    print(rc.check_caps(libs[build], oracle, CAPS[build]))


@pytest.mark.parametrize("build", ["default", "tiny"])
def test_emu_rfa_small_usual(libs, oracle, build):
    """40-pair barcodes, reads without a region, a barcode with bc_do_rfa = 0, a barcode of one pair"""
    out = rc.check_usual(libs[build], oracle, CAPS[build])
    assert out["within_caps"] >= (6 if build == "default" else 1), out
    print(out)


@pytest.mark.parametrize("build,pairs", [("default", 100), ("tiny", 3)])
def test_emu_rfa_small_molecule_overflow(libs, oracle, build, pairs):
    """more molecules than the on-chip tables hold, known only after scrapMolecules: the barcode leaves the small instance for the regular one"""
    print(rc.check_molecules(libs[build], oracle, CAPS[build], pairs))


@pytest.mark.parametrize("build,slab_kb,small,big,rest", [
    ("default", 256, ["exact"] * 12 + ["copies3", "junk"], ["copies12"] * 100, ["copies12"] * 30),
    ("tiny", 64, ["exact", "odd3", "junk"], ["copies12"] * 30, ["exact"] * 20)])
def test_emu_rfa_small_mixed_classes(libs, oracle, build, slab_kb, small, big, rest):
    print(rc.check_mixed(libs[build], oracle, CAPS[build], slab_kb, small, big, rest))


@pytest.mark.parametrize("build", ["default", "tiny"])
def test_emu_rfa_small_heavy_pair(libs, oracle, build):
    """a pair with more combinations than a lane tags: k_rfa_tag_w before the barcode program, in a barcode of either instance"""
    print(rc.check_heavy_pair(libs[build], oracle, CAPS[build]))


@pytest.mark.parametrize("build", ["default", "tiny"])
def test_emu_rfa_small_fuzz_seed_95343(libs, oracle, build):
    spec = importlib.util.spec_from_file_location("fuzz_rfa_slab", os.path.join(helpers.ROOT, "tests", "checkers", "fuzz_rfa_slab.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    fz.run_case_both(libs[build], oracle, 95343)
