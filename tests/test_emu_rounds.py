"""A batch whose seed workspace exceeds the seed budget is aligned in rounds of whole barcodes inside one lh_align_resident (k_rounds.h; lh_host.inc:
align_rounds), through the kernel sources under the CPU emulator, against the oracle and against the same batch aligned whole.

lh_context_opts.seed_budget_kb makes the path reachable on a few hundred pairs: context A (default budget) runs the batch whole and reports, through
lh_last_rounds, the workspace of the whole batch and of its largest barcode; context B gets a budget derived from those two figures.  The budget is a
whole number of KiB, so "the largest barcode's need" as a budget is that need rounded UP to a KiB (a part may then hold a seed or two more than that
barcode alone; every part's need is still asserted against budget_bytes), and "one KiB below" is the last KiB count that lies below the need.

The case functions take the library, so that tests/test_gpu_rounds.py runs the same cases on the device."""
import os
import subprocess

import numpy as np
import pytest

import helpers
from lariat_amd import capi, synth

EMU_DIR = os.path.join(helpers.ROOT, "tests", "hipemu")
BUILDS = {"default": "liblariat_emu.so", "small": "liblariat_emu_small.so"}
FIELDS = helpers.INT_FIELDS + helpers.INF_FIELDS + helpers.F64_FIELDS + ["mapq"]
# uneven barcodes over helpers.repeat_family_case's 300 pairs: an empty one, two under five pairs (worthRunningRFA is false for those, lariat.go:1088)
SIZES = [3, 60, 0, 25, 90, 4, 38, 45, 20, 15]
NO_RFA = [0, 2, 5]
SEED = 13
CAP = 320   # pairs: every context of the uneven case has this capacity (the need counts the rescue slots of the capacity's reads), enough for helpers.small_reads too


def kib_up(nbytes):
    return -(-int(nbytes) // 1024)


def recut(rs, sizes, no_rfa):
    """the reads of `rs` cut into barcodes of `sizes` pairs (only bc_pair_off and bc_do_rfa change)"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert off[-1] == rs.n_pairs
    rfa = np.ones(len(sizes), dtype=np.uint8)
    rfa[no_rfa] = 0
    return capi.Batch.from_arrays(rs.seq, rs.seq_off, off, rs.name_seed, bc_do_rfa=rfa)


def barcode_seeds(od, b):
    """seeds per barcode, from the oracle's stage dump"""
    return np.diff(od.seed_off[2 * b.bc_pair_off.astype(np.int64)])


def assert_same_bytes(r, want):
    assert (r.n_reads, r.n_cand) == (want.n_reads, want.n_cand)
    for f in FIELDS:
        a, b = getattr(r, f), getattr(want, f)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f


def assert_plan(info, n_barcodes, first=0, at_least=1):
    """a lane's report: cuts strictly increasing from `first` to n_barcodes, every part within the budget"""
    assert info["n_rounds"] >= at_least, info
    fb = info["first_barcode"]
    assert len(fb) == info["n_rounds"] + 1 and fb[0] == first and fb[-1] == n_barcodes and (np.diff(fb) > 0).all(), fb
    assert len(info["round_need_bytes"]) == info["n_rounds"] and (info["round_need_bytes"] <= info["budget_bytes"]).all(), info
    assert info["max_barcode_need_bytes"] <= info["budget_bytes"]
    assert first <= info["max_barcode"] < n_barcodes


_uneven = {}


def uneven(lib, oracle):
    """the shared case, made once per library: the batch, the oracle's result, the batch aligned whole (R) and context A's report"""
    if lib.path not in _uneven:
        names, contigs, rs = helpers.repeat_family_case(SEED, n_barcodes=10, pairs=30)
        assert np.median(np.diff(rs.seq_off)[0::2]) == 143 and np.median(np.diff(rs.seq_off)[1::2]) == 150   # pairs of 293 bases and a few indels
        b = recut(rs, SIZES, NO_RFA)
        assert (b.seq_off[2 * b.bc_pair_off.astype(np.int64)] % 2 == 1).any()
        oidx = oracle.index_build_naive(names, contigs)
        seeds = barcode_seeds(oidx.stage_dump(b), b)
        assert seeds.max() * 3 < seeds.sum(), seeds   # three rounds are reachable: no barcode holds a third of the seeds
        ref = oidx.align_barcodes(b, threads=8)
        idx = lib.index_from_arrays(oidx.arrays())
        a = idx.context(CAP)
        R = a.align_barcodes(b)
        info = a.rounds()
        assert info["n_rounds"] == 1 and list(info["first_barcode"]) == [0, b.n_barcodes] and list(info["round_seeds"]) == [seeds.sum()]
        assert info["max_barcode"] == int(np.argmax(seeds)) and info["need_bytes"] > info["max_barcode_need_bytes"] > 0
        assert info["need_bytes"] <= info["budget_bytes"]
        helpers.assert_same_result(R, ref, inference=True)
        _uneven[lib.path] = dict(oidx=oidx, idx=idx, b=b, ref=ref, R=R, info=info, seeds=seeds, genome=(names, contigs))
    return _uneven[lib.path]


def budget_kb(info):
    return kib_up(max(info["need_bytes"] / 3.5, info["max_barcode_need_bytes"]))


def case_uneven_barcodes(lib, oracle, flags=0):
    """case 1 (and, with flags, case 7): three rounds and more, the oracle's result, R byte for byte, no counter of the discarded K1 pass in the result"""
    u = uneven(lib, oracle)
    b = u["b"]
    ctx = u["idx"].context(CAP, seed_budget_kb=budget_kb(u["info"]))
    res = ctx.align_barcodes(b, lib.opts(flags=flags))
    info = ctx.rounds()
    assert_plan(info, b.n_barcodes, at_least=3)
    assert (b.seq_off[2 * b.bc_pair_off[info["first_barcode"][1:-1]].astype(np.int64)] % 8 != 0).any()   # parts begin off the 8-byte words k_pack_reads reads
    assert info["budget_bytes"] == budget_kb(u["info"]) * 1024 and info["need_bytes"] == u["info"]["need_bytes"] and info["round_seeds"].sum() == u["seeds"].sum()
    assert info["max_barcode"] == u["info"]["max_barcode"] and info["max_barcode_need_bytes"] == u["info"]["max_barcode_need_bytes"]
    assert [int(u["seeds"][info["first_barcode"][r]:info["first_barcode"][r + 1]].sum()) for r in range(info["n_rounds"])] == list(info["round_seeds"])
    helpers.assert_same_result(res, u["ref"], inference=True)
    assert_same_bytes(res, u["R"])
    for k in ("n_rescue", "rescue_cells"):
        assert res.counters[k] == u["ref"].counters[k], k
    if not flags:
        # K1's first pass does the same work for a read wherever it runs (later passes and K4 choose a path by the previous part: their counters may differ):
        # counted once per read — the K1 pass over the whole batch that found the overflow is not in the result
        print({k: (res.counters[k], v) for k, v in u["R"].counters.items() if res.counters[k] != v})
        for k in ("n_ext_exec_p1", "n_ktree_p1", "n_calls_by_text", "n_sa", "glob_cells"):
            assert res.counters[k] == u["R"].counters[k] > 0, k
        names = [n for n, _ in ctx.timings()]
        assert "k_round_plan" in names and "k1_discarded" in names and names.count("k_rfa") == 1, names
    with pytest.raises(capi.LhError):   # the merged result is handed out once
        ctx.download()
    return info


def case_budget_is_largest_barcode(lib, oracle):
    """case 2: the budget is the largest barcode's need (rounded up to a KiB): still aligned, every part within budget, R"""
    u = uneven(lib, oracle)
    b = u["b"]
    ctx = u["idx"].context(CAP, seed_budget_kb=kib_up(u["info"]["max_barcode_need_bytes"]))
    res = ctx.align_barcodes(b)
    info = ctx.rounds()
    assert_plan(info, b.n_barcodes, at_least=3)
    assert info["budget_bytes"] - u["info"]["max_barcode_need_bytes"] in range(1024)
    assert_same_bytes(res, u["R"])
    return info


def case_budget_below_largest_barcode(lib, oracle):
    """case 3: one KiB less: LH_E_CAPACITY naming the barcode; the context then aligns another batch to the oracle"""
    u = uneven(lib, oracle)
    b = u["b"]
    ctx = u["idx"].context(CAP, seed_budget_kb=kib_up(u["info"]["max_barcode_need_bytes"]) - 1)
    with pytest.raises(capi.LhError) as e:
        ctx.align_barcodes(b)
    assert e.value.code == capi.LH_E_CAPACITY and ("barcode %d " % u["info"]["max_barcode"]) in str(e.value), str(e.value)
    with pytest.raises(capi.LhError):   # the stage dump of such a batch: one pass over the whole batch or none
        ctx.stage_dump(b)
    names, contigs = u["genome"]
    rs = helpers.small_reads(names, contigs)
    assert rs.n_pairs == CAP
    b2 = helpers.batch_of(rs)
    helpers.assert_same_result(ctx.align_barcodes(b2), u["oidx"].align_barcodes(b2, threads=8), inference=True)


def case_low_complexity_middle(lib, oracle):
    """case 4: a barcode of 40 pairs on poly-A tracts, microsatellites and a tandem repeat (thousands of seeds per read) between ordinary barcodes, in a context
    whose big slab (reads with more SMEM intervals than the regular slots) has two slots: the slab's growth loop runs before the plan, in the discarded pass and in
    the rounds"""
    names, contigs = helpers.small_genome()
    lnames, lcontigs = helpers.low_complexity_genome()
    plain = helpers.small_reads(names, contigs, n_barcodes=4, pairs=20)
    low = synth.make_reads(lcontigs, lnames, n_barcodes=1, pairs_per_barcode=40, seed=3, sub_lo=0.002, sub_hi=0.03, indel_rate=0.002, mol_min=2, mol_max=3)
    order = [(plain, p) for p in range(40)] + [(low, p) for p in range(40)] + [(plain, p) for p in range(40, 80)]
    reads = [rs.read(2 * p + m) for rs, p in order for m in (0, 1)]
    seeds = np.array([rs.name_seed[p] for rs, p in order], dtype=np.uint64)
    b = capi.Batch(reads, [0, 20, 40, 80, 100, 120], name_seed=seeds)
    oidx = oracle.index_build_naive(names + lnames, contigs + lcontigs)
    per_bc = barcode_seeds(oidx.stage_dump(b), b)
    assert int(np.argmax(per_bc)) == 2 and per_bc[2] > 10 * np.delete(per_bc, 2).sum(), per_bc
    ref = oidx.align_barcodes(b, threads=8)
    idx = lib.index_from_arrays(oidx.arrays())
    a = idx.context(b.n_pairs, big_slots=2)
    helpers.assert_same_result(a.align_barcodes(b), ref, inference=True)
    whole = a.rounds()
    assert whole["n_rounds"] == 1 and whole["max_barcode"] == 2
    ctx = idx.context(b.n_pairs, big_slots=2, seed_budget_kb=kib_up(whole["max_barcode_need_bytes"]))
    res = ctx.align_barcodes(b)
    info = ctx.rounds()
    assert_plan(info, b.n_barcodes, at_least=3)   # the barcodes before it, the low-complexity one, the ones behind it
    assert 2 in list(info["first_barcode"]) and 3 in list(info["first_barcode"])
    helpers.assert_same_result(res, ref, inference=True)
    return info


def case_lanes(lib, oracle):
    """case 5: two lanes, each planning its own part against the budget: R, and lane 1's report continues lane 0's"""
    u = uneven(lib, oracle)
    b = u["b"]
    ctx = u["idx"].context(CAP, lanes=2, seed_budget_kb=budget_kb(u["info"]))
    res = ctx.align_barcodes(b)
    l0, l1 = ctx.rounds(0), ctx.rounds(1)
    assert l1["n_rounds"] >= 1, "the batch was not split over the lanes"
    assert_plan(l0, int(l1["first_barcode"][0]))
    assert_plan(l1, b.n_barcodes, first=int(l0["first_barcode"][-1]))
    assert max(l0["n_rounds"], l1["n_rounds"]) > 1
    assert l0["round_seeds"].sum() + l1["round_seeds"].sum() == u["seeds"].sum()
    for info in (l0, l1):
        fb = info["first_barcode"]
        assert [int(u["seeds"][fb[r]:fb[r + 1]].sum()) for r in range(info["n_rounds"])] == list(info["round_seeds"])
    assert_same_bytes(res, u["R"])
    with pytest.raises(capi.LhError):
        ctx.rounds(2)
    return l0, l1


def case_split_download(lib, oracle):
    """case 6: lh_result_download_begin / _end after an align in rounds; the next batch (whole) may be aligned in between"""
    u = uneven(lib, oracle)
    b = u["b"]
    ctx = u["idx"].context(CAP, seed_budget_kb=budget_kb(u["info"]))
    ctx.upload(b)
    ctx.align_resident(lib.opts())
    assert ctx.rounds()["n_rounds"] >= 3
    ctx.download_begin()
    assert_same_bytes(ctx.download_end(), u["R"])
    # a download begun for a batch that ran whole stays the host's while the next batch runs in rounds
    names, contigs = u["genome"]
    one = helpers.batch_of(helpers.small_reads(names, contigs, n_barcodes=2, pairs=10))
    ctx.upload(one)
    ctx.align_resident(lib.opts())
    assert ctx.rounds()["n_rounds"] == 1
    ctx.download_begin()
    ctx.upload(b)
    ctx.align_resident(lib.opts())
    assert ctx.rounds()["n_rounds"] >= 3
    helpers.assert_same_result(ctx.download_end(), u["oidx"].align_barcodes(one, threads=8), inference=True)
    assert_same_bytes(ctx.download(), u["R"])


def case_second_slot_centromeres(lib, oracle):
    """case 8: rounds on a batch that is not in slot 0 and that carries centromeres, between runs of another batch in slot 0: a part is the selected batch's (its
    centromere arrays included), the selection is the whole batch's again afterwards, and the other slot is untouched.  Context A (default budget) runs both batches
    whole, context B the same sequence within the budget of case 1"""
    u = uneven(lib, oracle)
    b = u["b"]
    names, contigs = u["genome"]
    cen_start, cen_end = np.array([0, -1], dtype=np.int64), np.array([len(contigs[0]), -1], dtype=np.int64)   # all of c0; c1 has none
    b2 = capi.Batch.from_arrays(b.seq, b.seq_off, b.bc_pair_off, b.name_seed, bc_do_rfa=b.bc_do_rfa, cen_start=cen_start, cen_end=cen_end)
    b0 = helpers.batch_of(helpers.small_reads(names, contigs, n_barcodes=4, pairs=40))   # half the capacity, on unique sequence: within context B's budget as a whole

    def sequence(ctx):
        ctx.upload_slot(0, b0)
        ctx.upload_slot(1, b2)
        out = []
        for slot in (1, 0):
            ctx.select(slot)
            ctx.align_resident(lib.opts())
            out += [ctx.download(), ctx.rounds()]
        return out

    Rc, whole1, R0, whole0 = sequence(u["idx"].context(CAP))
    assert whole1["n_rounds"] == 1 and whole0["n_rounds"] == 1
    assert Rc.n_cand == u["R"].n_cand and ((Rc.mapq == 0) & (u["R"].mapq != 0)).any() and (Rc.mapq != 0).any()   # a best hit inside the centromere; one outside
    ctx = u["idx"].context(CAP, seed_budget_kb=budget_kb(u["info"]))
    res1, info1, res0, info0 = sequence(ctx)
    assert_plan(info1, b2.n_barcodes, at_least=3)
    assert_same_bytes(res1, Rc)
    helpers.assert_same_result(res1, u["oidx"].align_barcodes(b2, threads=8), inference=True)
    print("slot 0:", {k: info0[k] for k in ("n_rounds", "need_bytes", "budget_bytes")})
    assert info0["n_rounds"] == 1 and info0["need_bytes"] <= info0["budget_bytes"], info0
    assert_same_bytes(res0, R0)
    # the selection after a run in rounds is the whole batch's, not the last part's: the stage dump is one pass over every read of it (or, over budget, none)
    ctx.select(1)
    ctx.align_resident(lib.opts())
    assert ctx.rounds()["n_rounds"] >= 3
    with pytest.raises(capi.LhError) as e:
        ctx.stage_dump()
    assert e.value.code == capi.LH_E_CAPACITY and ("the batch has %d seeds" % u["seeds"].sum()) in str(e.value), str(e.value)
    ctx.select(0)
    assert ctx.stage_dump().n_reads == 2 * b0.n_pairs
    return info1, info0


@pytest.fixture(scope="module")
def emu_libs():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "small"])
    return {k: capi.Library(os.path.join(helpers.ROOT, "tests", "_build", v)) for k, v in BUILDS.items()}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_uneven_barcodes(emu_libs, oracle, build):
    print(build, case_uneven_barcodes(emu_libs[build], oracle))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_budget_is_largest_barcode(emu_libs, oracle, build):
    print(build, case_budget_is_largest_barcode(emu_libs[build], oracle))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_budget_below_largest_barcode(emu_libs, oracle, build):
    case_budget_below_largest_barcode(emu_libs[build], oracle)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_low_complexity_middle(emu_libs, oracle, build):
    print(build, case_low_complexity_middle(emu_libs[build], oracle))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_lanes(emu_libs, oracle, build):
    print(build, case_lanes(emu_libs[build], oracle))


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_split_download(emu_libs, oracle, build):
    case_split_download(emu_libs[build], oracle)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_emu_rounds_second_slot_centromeres(emu_libs, oracle, build):
    print(build, case_second_slot_centromeres(emu_libs[build], oracle))
