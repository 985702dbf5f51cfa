"""K1's pass-2 probe and pass 3 in one lockstep kernel (k_p23_lock, k_p2_close: k_smem4.h), under the CPU emulator: lock_tail_cases.py's cases, the default sequence
against LH_F_P3_LAST byte for byte and both against the oracle.  Builds: the default one; `small` (tests/hipemu/Makefile: LH_MAX_INTV = 4, so that pass 2 and pass 3
each overflow a read's slots); one whose pass 2 leaves out its count add (LH_P23_NO_P2_COUNT) and one whose k_p2_close lists no read (LH_P23_NO_FIN_LIST), which
must fail."""
import os
import subprocess

import pytest

import helpers
import lock_tail_cases as cases
from lariat_amd import capi
from test_emu_p2_probe import CS, CXXFLAGS, HIPEMU, OUT, emu, small   # noqa: F401  (the fixtures)


def _build_variant(tag, define):
    so = os.path.join(OUT, "liblariat_emu_%s.so" % tag)
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)] + \
           [os.path.join(helpers.ROOT, "include", "lariat_hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-D%s=1" % define, "-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
              [os.path.join(CS, f) for f in ("index_build.cpp", "ingest.cpp", "records.cpp", "bamfile.cpp", "synth.cpp")] + ["-lz"]
        subprocess.check_call(cmd, cwd=HIPEMU)
        os.replace(so + ".tmp", so)
    return capi.Library(so)


@pytest.mark.parametrize("case", ["walks", "subs", "odd", "fin", "rep"])
def test_emu_lock_tail(emu, oracle, case):
    cases.check_case(emu, oracle, case)


def test_emu_lock_tail_too_long(emu, oracle):
    cases.check_too_long(emu, oracle)


def test_emu_lock_tail_overflow(small, oracle):
    """LH_MAX_INTV = 4: reads whose fifth interval is pass 2's, and reads whose fifth is pass 3's; the same reads reach the big slab under both sequences"""
    cases.check_case(small, oracle, "short", max_intv=4)


@pytest.mark.parametrize("case", ["subs", "fin"])
def test_emu_lock_tail_small_slots(small, oracle, case):
    cases.check_case(small, oracle, case, max_intv=4, covered=False)


def test_emu_lock_tail_shares(emu, oracle):
    cases.check_shares(oracle)
    cases.check_case(emu, oracle, "family")


def test_emu_lock_tail_other_paths(emu, oracle):
    cases.check_other_paths(emu, oracle)


def test_emu_lock_tail_rounds(emu, oracle):
    cases.check_rounds(emu, oracle)


def test_emu_lock_tail_two_lanes(emu, oracle):
    cases.check_two_lanes(emu, oracle)


@pytest.mark.parametrize("case", ["fin", "rep"])
def test_emu_lock_tail_bite_count(emu, oracle, case):
    """pass 2's count add left out: a read of at most 16 intervals with one of pass 2's has too few seed slots (fin); a read whose only interval above max_occ is
    pass 2's is not listed (rep)"""
    weak = _build_variant("p23nocount", "LH_P23_NO_P2_COUNT")
    with pytest.raises((AssertionError, capi.LhError)):
        cases.check_case(weak, oracle, case)


def test_emu_lock_tail_bite_list(emu, oracle):
    """k_p2_close lists no read: the reads of 17 intervals reach K2 unsorted"""
    weak = _build_variant("p23nolist", "LH_P23_NO_FIN_LIST")
    with pytest.raises((AssertionError, capi.LhError)):
        cases.check_case(weak, oracle, "fin")
