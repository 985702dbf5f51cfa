"""K1's interval lists on chip (k_smem4.h: LIST_PUT / LIST_GET): the first entries of each lane's lists live in an LDS ring beside the query, the
rest in the slab.  The kernel sources are built under the CPU emulator with the ring at 0 and 1 entries, as they ship, and with a small query
staging (the instance for short reads holds 152 bases; longer reads take the full one); every variant must give the oracle's intervals, seeds,
chains and results on reads whose lists fit the ring, on long noisy reads and on low-complexity sequence whose forward lists overflow any ring."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers
from lariat_amd import capi, synth

HIPEMU = os.path.join(helpers.ROOT, "tests", "hipemu")
CS = os.path.join(helpers.ROOT, "lariat_amd", "csrc")
OUT = os.path.join(helpers.ROOT, "tests", "_build")
# the flags of tests/hipemu/Makefile, plus the variant's own
CXXFLAGS = ["-O1", "-std=c++17", "-fPIC", "-Wall", "-Wno-sign-compare", "-Wno-unused-variable", "-Wno-unused-function", "-Wno-unknown-pragmas",
            "-ffp-contract=off", "-pthread", "-I.", "-DLH_EMU=1"]
VARIANTS = {"ring0": ["-DLH_K1_RING=0"], "ring1": ["-DLH_K1_RING=1"], "qw19": ["-DLH_K1_QW_SMALL=19"]}


def _build(name):
    so = os.path.join(OUT, "liblariat_emu_k1_%s.so" % name)
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + VARIANTS[name] + ["-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
              [os.path.join(CS, f) for f in ("index_build.cpp", "ingest.cpp", "records.cpp", "bamfile.cpp", "synth.cpp")] + ["-lz"]
        subprocess.check_call(cmd, cwd=HIPEMU)
        os.replace(so + ".tmp", so)
    return so


@pytest.fixture(scope="module")
def libs():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    with ThreadPoolExecutor(len(VARIANTS)) as ex:
        built = dict(zip(VARIANTS, ex.map(_build, VARIANTS)))
    out = {"default": capi.Library(os.path.join(OUT, "liblariat_emu.so"))}
    out.update({k: capi.Library(v) for k, v in built.items()})
    return out


def _shortcut_inputs():   # the inputs of test_emu_front.py::test_emu_k1_sweep_filter_and_text_shortcuts
    names, contigs = helpers.small_genome()
    rs = helpers.small_reads(names, contigs, n_barcodes=2, pairs=25, junk=0.05, seed=41)
    rs.seq[np.arange(7, len(rs.seq), 211)] = 4
    return names, contigs, rs


def _long_noisy_inputs():
    names, contigs = helpers.small_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=20, seed=31, len1=240, len2=236, sub_lo=0.005, sub_hi=0.03, indel_rate=0.003, junk_frac=0.02)
    return names, contigs, rs


def _low_complexity_inputs():
    names, contigs = helpers.low_complexity_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=2, pairs_per_barcode=12, seed=3, sub_lo=0.002, sub_hi=0.03, indel_rate=0.002, mol_min=2, mol_max=3)
    return names, contigs, rs


INPUTS = {"shortcuts": _shortcut_inputs, "long_noisy": _long_noisy_inputs, "low_complexity": _low_complexity_inputs}


@pytest.mark.parametrize("inp", sorted(INPUTS))
@pytest.mark.parametrize("variant", ["ring0", "ring1", "default", "qw19"])
def test_emu_k1_ring_variants(libs, oracle, variant, inp):
    names, contigs, rs = INPUTS[inp]()
    oidx = oracle.index_build_naive(names, contigs)
    b = helpers.batch_of(rs)
    lib = libs[variant]
    ctx = lib.index_from_arrays(oidx.arrays()).context(rs.n_pairs)
    helpers.assert_same_dump(ctx.stage_dump(b), oidx.stage_dump(b), helpers.DUMP_FRONT)
    helpers.assert_same_result(ctx.align_barcodes(b), oidx.align_barcodes(b), inference=True)
    if inp == "shortcuts":   # the reference's every bwt_extend without the exact shortcuts
        NOF = capi.LH_F_NO_SWEEP_FILTER
        helpers.assert_same_dump(ctx.stage_dump(b, lib.opts(flags=NOF)), oidx.stage_dump(b), helpers.DUMP_FRONT)
        got = ctx.align_barcodes(b, lib.opts(run_inference=0, flags=NOF)).counters["n_ext"]
        assert got == oidx.align_barcodes(b, oracle.opts(run_inference=0)).counters["n_ext"]
