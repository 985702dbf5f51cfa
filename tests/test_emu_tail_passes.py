"""A read's K5 on the lane that finishes its extension, k_dedup_fast over the reads that finish elsewhere, K8's prologue beside K7 (tail_pass_cases.py), under
the CPU emulator.  Two builds: the default one, and `small` (tests/hipemu/Makefile: two extension rounds, so that reads are left to the wave extension kernel
after the last round, and K4's long queue for every wave-chained read)."""
import os
import subprocess

import pytest

import tail_pass_cases as tp
from lariat_amd import capi
from test_emu_seed_groups import HIPEMU, OUT

BUILDS = ["default", "small"]


@pytest.fixture(scope="module")
def libs():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    default, small = os.path.join(OUT, "liblariat_emu.so"), os.path.join(OUT, "liblariat_emu_small.so")
    if not os.path.exists(small) or os.path.getmtime(small) < os.path.getmtime(default):   # (the target has no prerequisites: it is the default library's sources)
        subprocess.check_call(["make", "-s", "-C", HIPEMU, "small"])
    return {"default": capi.Library(os.path.join(OUT, "liblariat_emu.so")), "small": capi.Library(os.path.join(OUT, "liblariat_emu_small.so"))}


@pytest.mark.parametrize("build", BUILDS)
def test_emu_dedup_where_extension_finishes(libs, oracle, build):
    print(tp.check_part1(libs[build], oracle))


def test_emu_dedup_ext_wave(libs, oracle):
    print(tp.check_part1(libs["default"], oracle, flags=capi.LH_F_EXT_WAVE))


@pytest.mark.parametrize("build", BUILDS)
def test_emu_rfa_prologue(libs, oracle, build):
    print(tp.check_part3(libs[build], oracle, n_barcodes=40))


def test_emu_rfa_prologue_two_lanes(libs, oracle):
    print(tp.check_part3(libs["default"], oracle, n_barcodes=40, lanes=2))


def test_emu_mixed_batches(libs, oracle):
    tp.check_mixed_batches(libs["default"], oracle)
