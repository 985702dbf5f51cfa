"""K1's pass 2 over the calls k_p2_probe lists (k_smem4.h), under the CPU emulator: p2_probe_cases.py's cases against the oracle, against LH_F_P2_SCAN byte for byte and
against the model of the lister's counts.  Three builds: the default one; `small` (tests/hipemu/Makefile: LH_MAX_INTV = 4, so that pass 2's calls overflow a read's
slots, the clamp and the second chance run); and one whose probe overlooks its last window (LH_P2_PROBE_WEAK), which must lose the planted 19-mer there."""
import os
import subprocess

import pytest

import helpers
import p2_probe_cases as cases
from lariat_amd import capi

HIPEMU = os.path.join(helpers.ROOT, "tests", "hipemu")
CS = os.path.join(helpers.ROOT, "lariat_amd", "csrc")
OUT = os.path.join(helpers.ROOT, "tests", "_build")
# the flags of tests/hipemu/Makefile
CXXFLAGS = ["-O1", "-std=c++17", "-fPIC", "-Wall", "-Wno-sign-compare", "-Wno-unused-variable", "-Wno-unused-function", "-Wno-unknown-pragmas",
            "-ffp-contract=off", "-pthread", "-I.", "-DLH_EMU=1"]


def _build_weak():
    so = os.path.join(OUT, "liblariat_emu_p2weak.so")
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)] + \
           [os.path.join(helpers.ROOT, "include", "lariat_hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-DLH_P2_PROBE_WEAK=1", "-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
              [os.path.join(CS, f) for f in ("index_build.cpp", "ingest.cpp", "records.cpp", "bamfile.cpp", "synth.cpp")] + ["-lz"]
        subprocess.check_call(cmd, cwd=HIPEMU)
        os.replace(so + ".tmp", so)
    return so


@pytest.fixture(scope="module")
def emu():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    return capi.Library(os.path.join(OUT, "liblariat_emu.so"))


@pytest.fixture(scope="module")
def small():
    subprocess.check_call(["make", "-s", "-C", HIPEMU, "small"])
    return capi.Library(os.path.join(OUT, "liblariat_emu_small.so"))


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_emu_p2_probe(emu, oracle, case):
    cases.check_case(emu, oracle, case)


def test_emu_p2_probe_empty_list(emu, oracle):
    cases.check_empty_list_keeps_n_intv(emu, oracle)


@pytest.mark.parametrize("case", cases.COUNT_CASES)
def test_emu_p2_probe_read_counts(emu, oracle, case):
    cases.check_case(emu, oracle, case)


@pytest.mark.parametrize("case", cases.BASE_CASES)
@pytest.mark.parametrize("flags", [capi.LH_F_NO_SWEEP_FILTER, capi.LH_F_P2_TASKS], ids=["no_filter", "tasks"])
def test_emu_p2_probe_flags(emu, oracle, case, flags):
    cases.check_case(emu, oracle, case, flags=flags)


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_emu_p2_probe_two_lanes(emu, oracle, case):
    ctx, _ = cases.check_case(emu, oracle, case, ctx_kw={"lanes": 2}, counts=False)
    assert ctx.rounds(1)["n_rounds"] >= 1, "the batch was not split over the lanes"


@pytest.mark.parametrize("case", cases.BASE_CASES)
def test_emu_p2_probe_rounds(emu, oracle, case):
    cases.check_rounds(emu, oracle, case)


@pytest.mark.parametrize("case", ["overflow", "many", "probed"])
def test_emu_p2_probe_overflow(small, oracle, case):
    """LH_MAX_INTV = 4: the calls of a read of three SMEMs ask for more slots than it has.  (`many`: reads whose pass 1 already overflows; the lister sees the four
    intervals that were kept, which the model does not know: no counts there)"""
    cases.check_case(small, oracle, case, counts=case != "many")
    if case == "overflow":
        _, rs, b, want, _ = cases.oracle_side(oracle, case)
        assert (cases.np.diff(want.intv_off)[0::2] > 4).all()


def test_emu_p2_probe_too_long(emu, oracle):
    cases.check_too_long(emu, oracle)


def test_emu_p2_probe_bite(emu, oracle):
    """a probe one window short drops the call whose only repeated 19-mer is the last window's: the stage dump loses that call's interval"""
    weak = capi.Library(_build_weak())
    _, rs, b, want, _ = cases.oracle_side(oracle, "probed")
    helpers.assert_same_dump(cases.lib_index(emu, oracle).context(rs.n_pairs).stage_dump(b), want, helpers.DUMP_FRONT)
    got = cases.lib_index(weak, oracle).context(rs.n_pairs).stage_dump(b)
    with pytest.raises(AssertionError):
        helpers.assert_same_dump(got, want, helpers.DUMP_FRONT)
    assert len(got.intv) < len(want.intv)
