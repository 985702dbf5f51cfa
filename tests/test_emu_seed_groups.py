"""K2 as a 16-lane group per read (k_seed.h: k_seed_grp) under the CPU emulator: the seeds of unique reads (among them reads without bases and without
seeds), of repeat families (with max_occ = 3: sampled occurrences, the cap, the 64-bit divisions) and of low-complexity reads with more than 16 and more
than 64 intervals, against the oracle and against the lane-per-seed path (LH_F_SEED_LANE).  Two builds: the default one keeps LH_MAX_INTV = 64 intervals in a
read's regular slots (one to four chunks of 16), the other 4, so that most reads take the big slab."""
import os
import subprocess

import pytest

import helpers
import seed_group_cases as cases
from lariat_amd import capi

HIPEMU = os.path.join(helpers.ROOT, "tests", "hipemu")
CS = os.path.join(helpers.ROOT, "lariat_amd", "csrc")
OUT = os.path.join(helpers.ROOT, "tests", "_build")
# the flags of tests/hipemu/Makefile
CXXFLAGS = ["-O1", "-std=c++17", "-fPIC", "-Wall", "-Wno-sign-compare", "-Wno-unused-variable", "-Wno-unused-function", "-Wno-unknown-pragmas",
            "-ffp-contract=off", "-pthread", "-I.", "-DLH_EMU=1"]

CASES = {"unique": cases.unique_case, "repeat": cases.repeat_case, "repeat_max_occ3": cases.repeat_max_occ3_case,
         "low_complexity": cases.low_complexity_case(2, 12, keep=(3, 10))}


def _build_intv4():
    so = os.path.join(OUT, "liblariat_emu_intv4.so")
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)] + \
           [os.path.join(helpers.ROOT, "include", "lariat_hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-DLH_MAX_INTV=4", "-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
              [os.path.join(CS, f) for f in ("index_build.cpp", "ingest.cpp", "records.cpp", "bamfile.cpp", "synth.cpp")] + ["-lz"]
        subprocess.check_call(cmd, cwd=HIPEMU)
        os.replace(so + ".tmp", so)
    return so


@pytest.fixture(scope="module")
def libs():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    return {"intv64": capi.Library(os.path.join(OUT, "liblariat_emu.so")), "intv4": capi.Library(_build_intv4())}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("build", ["intv64", "intv4"])
def test_emu_seed_groups(libs, oracle, build, case):
    cases.check_case(libs[build], oracle, case, CASES[case])
