"""MAPQ held to the oracle EXACTLY wherever its integer is decidable (helpers.mapq_reference: the formula evaluated again in 50-digit decimal arithmetic
from the terms the oracle held, with the interval that double-precision rounding noise eta can reach), on inputs whose MAPQs live between 0 and 60
(helpers.mapq_workload, and two of helpers.repeat_family_case for the values just below an integer that the molecule term yields), through the kernel
sources under the CPU emulator: the standard build (the lane form of estimateMapQualities for most reads), the `small` build (the wave form, k_rfa_mq_w,
for nearly all) and two host lanes.  The same kernel sources with the MAPQ made wrong by less than a unit in four ways (LH_MAPQ_WEAK, k_rfa.h) must FAIL.
The device runs the same inputs in tests/test_gpu_inference.py."""
import os
import subprocess

import numpy as np
import pytest

import helpers
from lariat_amd import capi

EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu")
WEAK = {1: "rounds to nearest", 2: "the two terms in float", 3: "sums 16 scores", 4: "ignores the molecule term"}

# Minimum counts over the three inputs together, of the ORACLE's terms alone (helpers.mapq_coverage); about two thirds of what the committed seeds yield
# (0.5-1: 140, 1-10: 224, 10-20: 148, 20-30: 110, 30-40: 240, 40-50: 58, 50-60: 160; fractional part >= 0.5: 632; within 1e-5 below an integer: 8, seven of
# them from the repeat_family_case inputs; molecule term the smaller: 23, pair term: 1057; reads with < 15 / 15 / > 15 scores: 830 / 163 / 87; NaN 227;
# centromere zeros 138)
COVERAGE_MIN = {"bin_0.5_1": 90, "bin_1_10": 150, "bin_10_20": 100, "bin_20_30": 70, "bin_30_40": 160, "bin_40_50": 38, "bin_50_60": 105, "frac_ge_half": 420,
                "just_below_integer": 5, "molecule_term_smaller": 15, "pair_term_smaller": 700, "scores_under_15": 550, "scores_15": 105, "scores_over_15": 58,
                "nan": 150, "centromere_zero": 90}
UNDECIDABLE_CAP = 0.01   # of the candidates whose raw value lies in [0.5, 60), on every input


def mapq_inputs():
    """[(what, names, contigs, batch)]"""
    names, contigs, batch, _ = helpers.mapq_workload(31)
    out = [("mapq_workload(31)", names, contigs, batch)]
    for seed, n_bc in ((5, 4), (7, 6)):
        names, contigs, rs = helpers.repeat_family_case(seed, n_bc)
        out.append(("repeat_family_case(%d, %d)" % (seed, n_bc), names, contigs, helpers.batch_of(rs)))
    return out


def check_inputs(cases, run):
    """run(index of the case, oracle index, batch) -> the product's result, held to the oracle's by helpers.assert_same_result; returns the counts summed"""
    tot = {}
    for k, (what, oidx, batch, ref) in enumerate(cases):
        c = helpers.assert_same_result(run(k, oidx, batch), ref, inference=True)
        print("%s: %s" % (what, c))
        assert c["undecidable_in_range"] <= UNDECIDABLE_CAP * c["in_range"], (what, c)
        for key, v in c.items():
            tot[key] = min(tot.get(key, v), v) if key == "min_margin" else tot.get(key, 0) + v
    return tot


@pytest.fixture(scope="module")
def cases(oracle):
    out = []
    for what, names, contigs, batch in mapq_inputs():
        oidx = oracle.index_build_naive(names, contigs)
        out.append((what, oidx, batch, oidx.align_barcodes(batch, threads=8)))
    return out


def _lib(target):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR] + ([target] if target else []))
    return capi.Library(os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu%s.so" % ("_" + target if target else "")))


def test_workload_reaches_the_edges(cases):
    """the inputs' coverage, from the oracle's terms: every bin of [0.5, 60), fractional parts of a half and more (where rounding differs from truncation), the
    cluster just below an integer (where a relative 1e-7 flips the integer), both terms binding, reads with fewer than, exactly and more than 15 scores, NaN,
    centromere zeros; and at most 1 % undecidable candidates per input"""
    tot = {}
    for what, oidx, batch, ref in cases:
        cov = helpers.mapq_coverage(ref)
        print("%s: %s" % (what, cov))
        assert cov["undecidable_in_range"] <= UNDECIDABLE_CAP * cov["in_range"], (what, cov)
        for k, v in cov.items():
            tot[k] = tot.get(k, 0) + v
    print("together: %s" % tot)
    for k, need in COVERAGE_MIN.items():
        assert tot[k] >= need, ("mapq coverage", k, tot[k], need)
    kinds = helpers.mapq_workload(31)[3]
    assert {"tandem", "tandem_norfa", "dispersed", "dispersed_norfa", "thin", "thin_norfa"} <= set(kinds)


def test_oracle_mapq_against_decimal(cases):
    """the oracle's own double `mapq` against the 50-digit evaluation of its own terms, every candidate through decimal: its integer inside the eta-interval's
    truncated ends (equal where decidable), and its double within the interval's reach of the decimal value"""
    for what, oidx, batch, ref in cases:
        c = helpers.assert_mapq(ref.mapq, ref, screen=False)
        t = ref.mapq_terms
        m = helpers.mapq_reference(t, screen=False)
        s = m["set"] & np.isfinite(m["raw"]) & (m["raw"] < 60)
        # raw = -10 log10(1 - p): an eta' = (|score| ln 10 + 2) eta of p moves it by 10 / ln 10 * eta' / (1 - p), and 1 - p = 10^(-raw / 10)
        reach = 10.0 / np.log(10.0) * (np.abs(t[:, 1]) * np.log(10.0) + 2) * helpers.MAPQ_ETA * 10.0 ** (m["raw"] / 10.0) + 60 * helpers.MAPQ_ETA
        d = np.abs(t[:, 6] - m["raw"])
        print("%s: %s; largest |double - decimal| %.3g, largest share of its reach %.3g" % (what, c, d[s].max(), (d[s] / reach[s]).max()))
        assert (d[s] <= reach[s]).all(), (what, np.nonzero(s & (d > reach))[0][:5])
        assert (np.isnan(t[:, 6]) == (ref.mapq == -2 ** 31))[m["set"]].all()
        # what screening decides, decimal decides the same way
        ms = helpers.mapq_reference(t, screen=True)
        assert (ms["lo"] == m["lo"]).all() and (ms["hi"] == m["hi"]).all()


@pytest.mark.parametrize("build", ["default", "small", "lanes2"])
def test_emu_mapq_exact_where_decidable(cases, build):
    lib = _lib("small" if build == "small" else None)
    idxs = [lib.index_from_arrays(c[1].arrays()) for c in cases]

    def run(k, oidx, batch):
        ctx = idxs[k].context(batch.n_pairs, **({"lanes": 2} if build == "lanes2" else {}))
        return ctx.align_barcodes(batch)

    tot = check_inputs(cases, run)
    print("%s: %s" % (build, tot))
    assert tot["compared"] > 7000 and tot["in_range"] > 1000


def test_subtly_wrong_mapq_fails(cases):
    """dev_mapq made wrong in four ways: each must raise under the new comparison; the old rule (|mapq - oracle's| <= 1 alone) would have passed the first two"""
    subprocess.check_call(["make", "-s", "-j4", "-C", EMU_DIR] + ["mapqweak%d" % w for w in WEAK])
    old_rule_passes = {}
    for w, what in WEAK.items():
        lib = capi.Library(os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu_mapqweak%d.so" % w))
        raised, old_ok = 0, True
        for name, oidx, batch, ref in cases:
            res = lib.index_from_arrays(oidx.arrays()).context(batch.n_pairs).align_barcodes(batch)
            d = np.abs(res.mapq.astype(np.int64) - ref.mapq.astype(np.int64))
            old_ok = old_ok and bool((d <= 1).all())
            print("LH_MAPQ_WEAK=%d (%s), %s: %d of %d MAPQs differ from the oracle's, %d by more than one" % (w, what, name, int((d > 0).sum()), len(d), int((d > 1).sum())))
            no_mapq = capi.Result.__new__(capi.Result)
            no_mapq.__dict__.update(res.__dict__)
            no_mapq.mapq = ref.mapq
            helpers.assert_same_result(no_mapq, ref, inference=True)   # everything but the MAPQ is as it was
            try:
                helpers.assert_same_result(res, ref, inference=True)
            except AssertionError as e:
                assert "mapq" in str(e)
                raised += 1
        assert raised >= 1, "LH_MAPQ_WEAK=%d (%s) passes the comparison" % (w, what)
        old_rule_passes[w] = old_ok
    print("the +-1 rule alone would have passed: %s" % old_rule_passes)
    assert old_rule_passes[1] and old_rule_passes[2]
