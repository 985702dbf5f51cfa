"""K1's pass 3 counts a read's seeds and lists the reads k_smem_fin still sorts in memory; K2 ranks every other read's intervals inside its 16-lane group
(seed_count_cases.py), under the CPU emulator.  Two builds, as in test_emu_seed_groups.py: LH_MAX_INTV = 64 regular slots per read, and 4, where most reads take
the big slab and no regular read is ever listed."""
import os
import subprocess

import pytest

import helpers
import seed_count_cases as sc
import seed_group_cases as cases
from lariat_amd import capi
from test_emu_seed_groups import _build_intv4, HIPEMU, OUT

BUILDS = ["intv64", "intv4"]
COVER = {"chunk_edge": (sc.chunk_edge_case(sc.CHUNK_EDGE_KEEP), sc.cover_chunk_edge), "unique": (cases.unique_case, sc.cover_out_of_order),
         "max_mem_intv_0": (sc.unique_max_mem_intv_case(0), sc.cover_max_mem_intv), "max_mem_intv_1": (sc.unique_max_mem_intv_case(1), sc.cover_max_mem_intv)}


@pytest.fixture(scope="module")
def libs():
    os.makedirs(OUT, exist_ok=True)
    subprocess.check_call(["make", "-s", "-C", HIPEMU])
    return {"intv64": capi.Library(os.path.join(OUT, "liblariat_emu.so")), "intv4": capi.Library(_build_intv4())}


@pytest.mark.parametrize("case", sorted(COVER))
def test_coverage(oracle, case):
    make, cover = COVER[case]
    print(cover(sc.oracle_dump(oracle, make)))


def test_coverage_chunk_edge_whole_set(oracle):
    want = sc.oracle_dump(oracle, sc.chunk_edge_case())
    sc.cover_chunk_edge(want)


@pytest.mark.parametrize("case", ["chunk_edge", "max_mem_intv_0", "max_mem_intv_1"])
@pytest.mark.parametrize("build", BUILDS)
def test_emu_seed_counts(libs, oracle, build, case):
    cases.check_case(libs[build], oracle, case, COVER[case][0])


@pytest.mark.parametrize("build", BUILDS)
def test_emu_p2_tasks(libs, oracle, build):
    sc.check_p2_tasks(libs[build], oracle)


@pytest.mark.parametrize("build", BUILDS)
def test_emu_three_batches(libs, oracle, build):
    sc.check_three_batches(libs[build], oracle, keep=sc.CHUNK_EDGE_KEEP)


@pytest.mark.parametrize("build", BUILDS)
def test_emu_two_lanes(libs, oracle, build):
    sc.check_two_lanes(libs[build], oracle, keep=sc.CHUNK_EDGE_KEEP)
