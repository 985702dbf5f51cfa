"""The differential fuzzer's geometry leg (tests/checkers/fuzz_gpu.py run_case_geometry, small genomes) through the kernel sources under the CPU emulator:
fragmented references of 13 to 400 contigs, reads across junctions, off contig ends and l_pac, around contigs shorter than the read, random options, flags and
context options — stage dumps and every result field against the oracle.  Sized by time, not by a count: consecutive seeds from 1 for about a minute."""
import importlib.util
import os
import subprocess
import time

import helpers
from lariat_amd import capi

BUDGET_S = 50.0


def test_emu_differential_fuzz_geometry_slice(oracle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "hipemu")])
    emu = capi.Library(os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu.so"))
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(helpers.ROOT, "tests", "checkers", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    t_end = time.time() + BUDGET_S
    seed, total = 1, {}
    while seed <= 3 or time.time() < t_end:
        fz.add_coverage(total, fz.run_case_geometry(emu, oracle, seed, small=True))
        seed += 1
    print("%d geometry cases: %s" % (seed - 1, total))
    helpers.assert_geometry_coverage(total, barcodes_over_256=0)
