"""The N>1 path: two torch.distributed ranks (gloo here; bench.py uses RCCL on a multi-GPU node) take contiguous barcode ranges
of ONE barcode-sorted input (lariat_amd.shard), align them through the PRODUCT's C-ABI — liblariat_hip.so on a device when one
is present (two ranks may share it), otherwise the same host pipeline and kernel sources built against the CPU emulator —
exchange nothing on the data path, and the rank-ordered concatenation of what they return equals the single-process result
(checked against the oracle on rank 0).  Only the check itself gathers; the product path uses a barrier and a MAX reduce."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import helpers

EMU = os.environ.get("LH_EMU_LIB") or os.path.join(helpers.ROOT, "tests", "_build", "liblariat_emu.so")   # (LH_EMU_LIB: e.g. an AddressSanitizer build, tests/hipemu/Makefile asan)
FIELDS = ["rid", "pos", "aend", "reversed", "score", "nm", "active", "is_proper", "mapq", "molecule_id", "duplicate"]


def _library(prefer_gpu):
    from lariat_amd import capi
    if prefer_gpu:
        lib = capi.load_library()
        if lib.device_count() >= 1:
            return lib, "hip"
    return capi.Library(EMU), "emu"


def _worker(rank, world, port, out, prefer_gpu):
    sys.path.insert(0, helpers.ROOT)
    sys.path.insert(0, os.path.join(helpers.ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lariat_amd import shard
    lib, kind = _library(prefer_gpu)
    # every rank builds the same index in its own memory (replicated, as on a node) and sees the same sorted input
    l_pac = 600000
    ctg = [("cA", 360000, 0), ("cB", 240000, 360000)]
    pac = lib.synth_genome(l_pac, seed=11, threads=2)
    idx = lib.index_build_device(pac, l_pac, ctg)
    r = lib.synth_reads(pac, l_pac, ctg, seed=3, n_barcodes=9, pairs_per_barcode=24, junk_frac=0.03, threads=2)
    (b0, b1), results = shard.align_rank_shard(lib, idx, r["seq"], r["seq_off"], r["bc_pair_off"], r["name_seed"], rank, world, max_pairs_per_batch=60)
    mine = {"range": (b0, b1), "n_batches": len(results), "kind": kind}
    for f in FIELDS:
        mine[f] = np.concatenate([getattr(x, f) for x in results]).tolist() if results else []
    gathered = [None] * world
    dist.all_gather_object(gathered, mine)   # for the check only
    tmax = shard.reduce_max(dist, 1.0 + rank)
    if rank == 0:
        import oracle_py
        from lariat_amd import capi
        o = oracle_py.load()
        oidx = o.index_from_arrays(idx.export(), pac)
        full = oidx.align_barcodes(capi.Batch.from_arrays(r["seq"], r["seq_off"], r["bc_pair_off"], r["name_seed"]), threads=4)
        ok = all(sum((g[f] for g in gathered), []) == getattr(full, f).tolist() for f in FIELDS if f != "mapq")
        try:   # the shards' MAPQs against the oracle's terms: exact wherever the integer is decidable (helpers.assert_mapq)
            helpers.assert_mapq(np.array(sum((g["mapq"] for g in gathered), []), dtype=np.int64), full)
        except AssertionError:
            ok = False
        with open(out, "w") as fh:
            fh.write("%d|%s|%s|%s|%s\n" % (int(ok), tmax, [g["range"] for g in gathered], [g["n_batches"] for g in gathered], gathered[0]["kind"]))
    dist.barrier()
    dist.destroy_process_group()


def _run(tmp_path, prefer_gpu):
    subprocess.check_call(["make", "-s", "-C", os.path.join(helpers.ROOT, "tests", "hipemu")])
    out = str(tmp_path / "r.txt")
    port = 29500 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, out, prefer_gpu), nprocs=2, join=True)
    ok, tmax, ranges, nb, kind = open(out).read().strip().split("|")
    assert ok == "1"
    assert float(tmax) == 2.0
    assert ranges.startswith("[(0, ") and ranges.endswith(", 9)]")
    assert all(int(x) >= 2 for x in nb.strip("[]").split(","))   # each rank streamed its range as several batches
    return kind


def test_two_rank_barcode_sharding_through_the_product(tmp_path):
    assert _run(tmp_path, prefer_gpu=False) == "emu"


@pytest.mark.gpu
def test_two_rank_barcode_sharding_on_the_device(tmp_path):
    """the same, the two ranks sharing the one GPU of the test box"""
    assert _run(tmp_path, prefer_gpu=True) == "hip"


def test_barcode_ranges_balanced():
    from lariat_amd import shard
    off = np.concatenate([[0], np.cumsum([100] * 10 + [5] * 40 + [300] * 3)])
    for w in (1, 2, 4, 8):
        rg = shard.barcode_ranges(off, w)
        assert rg[0][0] == 0 and rg[-1][1] == len(off) - 1
        assert all(rg[i][1] == rg[i + 1][0] for i in range(w - 1))
        loads = [off[b1] - off[b0] for b0, b1 in rg]
        assert max(loads) <= off[-1] / w + 300


def test_barcode_ranges_balance_the_cost_of_a_mixed_input():
    """a pair on a repeat family costs ~160 x a pair on unique sequence (bench.py: 3.0 us against 20 ns).  In a barcode-sorted input whose barcodes hold 5 of
    100 pairs on repeats each (Poisson), contiguous ranges of equal PAIR count are also ranges of equal cost to within 5 % at 8 ranks — the draws average out
    over 2,500 barcodes per rank; when the repeat-rich barcodes cluster (a block of the input from one repeat-rich sample), pair counts no longer say what a
    range costs, and the weighted split (weights = each barcode's cost, e.g. the cells an earlier pass counted) restores the balance."""
    from lariat_amd import shard
    rng = np.random.default_rng(7)
    nb, world = 20000, 8
    off = np.arange(0, 100 * (nb + 1), 100, dtype=np.int64)

    def spread(weights, ranges):
        c = np.array([weights[b0:b1].sum() for b0, b1 in ranges])
        return float(c.max() / c.mean())

    rep = rng.poisson(5.0, size=nb).clip(0, 100)
    cost = (100 - rep) * 1.0 + rep * 164.0
    rg = shard.barcode_ranges(off, world)
    assert rg[0][0] == 0 and rg[-1][1] == nb and all(rg[i][1] == rg[i + 1][0] for i in range(world - 1))
    assert spread(cost, rg) < 1.05
    # clustered: the first eighth of the input is repeat-rich (40 of 100 pairs)
    rep2 = rep.copy()
    rep2[: nb // 8] = rng.poisson(40.0, size=nb // 8).clip(0, 100)
    cost2 = (100 - rep2) * 1.0 + rep2 * 164.0
    assert spread(cost2, shard.barcode_ranges(off, world)) > 2.0            # equal pair counts: one rank has most of the work
    rgw = shard.barcode_ranges(off, world, weights=cost2)
    assert rgw[0][0] == 0 and rgw[-1][1] == nb and all(rgw[i][1] == rgw[i + 1][0] for i in range(world - 1))
    assert spread(cost2, rgw) < 1.05
