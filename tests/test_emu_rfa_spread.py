"""K8's small-barcode instance with several lanes per sink and per molecule (k_rfa.h: dev_fast_score_spread, the molecule status) under the CPU emulator, on the
cases of rfa_spread_cases.py: against the oracle, against the regular instance byte for byte (LH_F_RFA_SLAB) and against a second run.  Three builds: the default
one; `tiny` (8 reads, 12 candidates, 4 molecules: every barcode of a few pairs is small, the widest groups at work); and one that leaves out the last partial step
of a source's alignments (LH_RFA_SPREAD_WEAK, never shipped), which the cases must catch."""
import os
import subprocess

import pytest

import helpers
import rfa_small_cases as rc
import rfa_spread_cases as sc
from lariat_amd import capi, synth
from test_emu_k1_ring import CXXFLAGS, CS, HIPEMU, OUT
from test_emu_rfa_small import _build_tiny


def _build_weak():
    so = os.path.join(OUT, "liblariat_emu_rfa_spread_weak.so")
    srcs = [os.path.join(HIPEMU, f) for f in ("emu_lib.cpp", "hip_emu.cpp", "hip_emu.h")] + [os.path.join(CS, f) for f in os.listdir(CS)] + \
           [os.path.join(helpers.ROOT, "include", "lariat_hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-DLH_RFA_SPREAD_WEAK=1", "-shared", "-o", so + ".tmp", "emu_lib.cpp", "hip_emu.cpp"] + \
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
def cover(emu, oracle):
    return {which: sc.check_case(emu, oracle, which) for which in ("small_genome", "many_contigs")}


@pytest.mark.parametrize("which", ["small_genome", "many_contigs"])
def test_emu_rfa_spread_case(cover, which):
    cov, cls = cover[which]
    print(cov, cls)
    assert cls["small"] > 0 and cls["turned_away"] == 0, cls


def test_emu_rfa_spread_cover(cover):
    """the two cases together hold a small barcode of every group width, one on the one-lane form, and sources of one alignment, of a partial step, of two steps"""
    sc.assert_cover(sc.merge(cover["small_genome"][0], cover["many_contigs"][0]))


def test_emu_rfa_spread_tiny(oracle):
    """barcodes of four pairs in the build whose caps are 8 reads, 12 candidates, 4 molecules: one to four molecules, 32 or 16 lanes a sink"""
    os.makedirs(OUT, exist_ok=True)
    tiny = capi.Library(_build_tiny())
    names, contigs = helpers.small_genome()
    rs = synth.make_reads(contigs, names, n_barcodes=16, pairs_per_barcode=4, seed=9, mol_min=4, mol_max=4, junk_frac=0.0)
    ores, _, cls = rc.check(tiny, oracle, names, contigs, rs, rc.TINY_CAPS)
    cov = sc.covered(sc.spread_shapes(ores, rs.bc_pair_off), [1] * 16, rc.TINY_CAPS)
    print(cov, cls)
    assert cov["classes"] >= {(1, 1), (2, 2), (3, 4)} and cls["small"] > 0, (cov, cls)


def test_emu_rfa_spread_bite(emu, oracle):
    """a build that leaves out a source's last partial step loses those alignments' terms: scores, moves and probability sums change"""
    weak = capi.Library(_build_weak())
    for which in ("small_genome", "many_contigs"):
        names, contigs, rs, do_rfa = sc.case(which)
        with pytest.raises(AssertionError):
            rc.check(weak, oracle, names, contigs, rs, rc.DEFAULT_CAPS, do_rfa=do_rfa)
