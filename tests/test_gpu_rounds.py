"""A batch whose seed workspace exceeds the seed budget, aligned in rounds of whole barcodes inside one lh_align_resident, on the device: the cases of
test_emu_rounds.py (k_round_cost, k_round_plan, k_batch_view and the unchanged kernel sequence per part), and the A/B flags once each in rounds."""
import pytest

from lariat_amd import capi
import test_emu_rounds as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = capi.load_library()
    assert L.device_count() >= 1
    return L


def test_rounds_uneven_barcodes(lib, oracle):
    print(cases.case_uneven_barcodes(lib, oracle))


def test_rounds_budget_is_largest_barcode(lib, oracle):
    print(cases.case_budget_is_largest_barcode(lib, oracle))


def test_rounds_budget_below_largest_barcode(lib, oracle):
    cases.case_budget_below_largest_barcode(lib, oracle)


def test_rounds_low_complexity_middle(lib, oracle):
    print(cases.case_low_complexity_middle(lib, oracle))


def test_rounds_lanes(lib, oracle):
    print(cases.case_lanes(lib, oracle))


def test_rounds_split_download(lib, oracle):
    cases.case_split_download(lib, oracle)


def test_rounds_second_slot_centromeres(lib, oracle):
    print(cases.case_second_slot_centromeres(lib, oracle))


@pytest.mark.parametrize("flags", [capi.LH_F_CHAIN_WAVE, capi.LH_F_EXT_WAVE, capi.LH_F_RESCUE_FULL])
def test_rounds_flags(lib, oracle, flags):
    cases.case_uneven_barcodes(lib, oracle, flags=flags)
