"""K1's pass 3 counts a read's seeds and lists the reads k_smem_fin still sorts in memory; K2 ranks every other read's intervals inside its 16-lane group
(seed_count_cases.py), on the device with the product library: the whole chunk_edge set (reads of 15 to 24 intervals)."""
import pytest

import seed_count_cases as sc
import seed_group_cases as cases
from lariat_amd import capi

pytestmark = pytest.mark.gpu

CASES = {"chunk_edge": (sc.chunk_edge_case(), sc.cover_chunk_edge), "unique": (cases.unique_case, sc.cover_out_of_order),
         "max_mem_intv_0": (sc.unique_max_mem_intv_case(0), sc.cover_max_mem_intv), "max_mem_intv_1": (sc.unique_max_mem_intv_case(1), sc.cover_max_mem_intv)}


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


@pytest.mark.parametrize("case", sorted(CASES))
def test_seed_counts(lib, oracle, case):
    make, cover = CASES[case]
    cover(sc.oracle_dump(oracle, make))
    cases.check_case(lib, oracle, case, make)


def test_p2_tasks(lib, oracle):
    sc.check_p2_tasks(lib, oracle)


def test_three_batches(lib, oracle):
    sc.check_three_batches(lib, oracle)


def test_two_lanes(lib, oracle):
    sc.check_two_lanes(lib, oracle)
