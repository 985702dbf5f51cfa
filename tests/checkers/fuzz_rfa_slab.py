"""fuzz_gpu.py's cases with K8's barcode program in its regular instance for every barcode (LH_F_RFA_SLAB, the A/B leg of k_rfa.h) and without, beside whatever
flags a case draws:   python tests/checkers/fuzz_rfa_slab.py [seconds] [first seed]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_gpu
from lariat_amd import capi
import oracle_py


class RfaSlabLib:
    """the library with LH_F_RFA_SLAB set in every lh_opts it hands out"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def opts(self, **kw):
        kw["flags"] = int(kw.get("flags", 0)) | capi.LH_F_RFA_SLAB
        return self._lib.opts(**kw)


def run_case_both(lib, oracle, seed):
    """one case of fuzz_gpu.py with the flag unset, then set"""
    fuzz_gpu.run_case(lib, oracle, seed)
    fuzz_gpu.run_case(RfaSlabLib(lib), oracle, seed)


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    lib = capi.load_library()
    oracle = oracle_py.load()
    t_end = time.time() + budget
    it = 0
    while time.time() < t_end:
        try:
            run_case_both(lib, oracle, seed0 + it)
        except AssertionError as e:
            print("DIFF at " + str(e), flush=True)
            sys.exit(1)
        it += 1
    print("fuzz ok (LH_F_RFA_SLAB unset and set): %d cases from seed %d in %.0f s" % (it, seed0, budget))
