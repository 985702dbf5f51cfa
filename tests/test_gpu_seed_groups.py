"""K2 as a 16-lane group per read (k_seed.h: k_seed_grp) on the device: the cases of test_emu_seed_groups.py with the product library, whose regular slots
hold LH_MAX_INTV = 64 intervals (one to four chunks of 16 per read; the low-complexity reads with more take the big slab)."""
import pytest

import seed_group_cases as cases
from lariat_amd import capi

pytestmark = pytest.mark.gpu

CASES = {"unique": cases.unique_case, "repeat": cases.repeat_case, "repeat_max_occ3": cases.repeat_max_occ3_case,
         "low_complexity": cases.low_complexity_case(2, 12)}


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


@pytest.mark.parametrize("case", sorted(CASES))
def test_seed_groups(lib, oracle, case):
    cases.check_case(lib, oracle, case, CASES[case])
