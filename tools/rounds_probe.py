"""One lh_align_resident in rounds against the quarter batches bench.py's mixed_20pct leg aligns today (run on a GPU box).

The input has that leg's shape at its full size — 20,000 barcodes x 100 pairs, 20 % of every barcode's pairs drawn on the repeat copies of
workload.config4_genome, the others on unique sequence — built with workload.py's generators, on the hg38-scale index the leg uses.

  --mode quarters   the batch cut into four at barcode boundaries, each quarter aligned by its own lh_align_resident in a context of a quarter's capacity
                    (what a host has to do without rounds); prints the four times and their sum
  --mode rounds     the whole batch resident in a context of its capacity, one lh_align_resident; prints its time, lh_last_rounds and lh_last_timings
  --mode both       quarters, then rounds, on the same index and reads

--tree DIR measures another checkout of this project (its lariat_amd package and built library) — the parent commit's quarters, for one.
Every mode aligns once to warm up (the pools grow to the workload) and times the second run.  One JSON line per mode on stdout."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["quarters", "rounds", "both"], default="both")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--genome-mb", type=float, default=3100.0)
    ap.add_argument("--barcodes", type=int, default=20000)
    ap.add_argument("--pairs-per-barcode", type=int, default=100)
    ap.add_argument("--frac", type=float, default=0.20)
    ap.add_argument("--seed-budget-kb", type=int, default=0, help="rounds: lh_context_opts.seed_budget_kb (0: free HBM)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    from lariat_amd import capi, workload

    lib = capi.load_library()
    t0 = time.time()
    g = workload.config4_genome(lib, a.genome_mb * 1e6 * 0.987)
    idx = lib.index_build_device(g["pac"], g["l_pac"], g["contigs"])
    idx.set_alt(g["alt_flags"])
    n_bc, ppb = a.barcodes, a.pairs_per_barcode
    n_rep = int(round(ppb * a.frac))
    seed = workload.READS_SEED + 700
    unique = workload.outside_windows(g["contigs"], g["alt_flags"], g["windows"])
    ra = lib.synth_reads(g["pac"], g["l_pac"], g["windows"], seed=seed, n_barcodes=n_bc, pairs_per_barcode=n_rep)
    rb = lib.synth_reads(g["pac"], g["l_pac"], unique, seed=seed + 100000, n_barcodes=n_bc, pairs_per_barcode=ppb - n_rep)
    r = workload.interleave_reads(ra, rb)
    seq, seq_off, bc_off, name_seed = np.asarray(r["seq"]), np.asarray(r["seq_off"]), np.asarray(r["bc_pair_off"]), np.asarray(r["name_seed"])
    n_pairs = int(bc_off[-1])
    print("[probe] %s: genome, index and %d pairs in %.0f s" % (a.tree, n_pairs, time.time() - t0), file=sys.stderr, flush=True)
    opts = lib.opts()
    common = {"tree": os.path.abspath(a.tree), "abi": capi.LH_ABI_VERSION, "pairs": n_pairs, "barcodes": n_bc, "repeat_pair_frac": a.frac}

    def k1_ms(timings):
        return round(sum(ms for name, ms in timings if name.startswith("k_smem")), 2)

    if a.mode in ("quarters", "both"):
        cuts = [n_bc * q // 4 for q in range(5)]
        parts = []
        for q in range(4):
            p0, p1 = int(bc_off[cuts[q]]), int(bc_off[cuts[q + 1]])
            s0, s1 = int(seq_off[2 * p0]), int(seq_off[2 * p1])
            parts.append(capi.Batch.from_arrays(seq[s0:s1], seq_off[2 * p0:2 * p1 + 1] - s0, bc_off[cuts[q]:cuts[q + 1] + 1] - p0, name_seed[p0:p1]))
        ctx = idx.context(max(p.n_pairs for p in parts))
        for q, p in enumerate(parts):
            ctx.upload_slot(q, p)
        ms, k1 = [], []
        for timed in (False, True):
            for q in range(4):
                ctx.select(q)
                t = time.perf_counter()
                ctx.align_resident(opts)
                if timed:
                    ms.append(round((time.perf_counter() - t) * 1e3, 2))
                    k1.append(k1_ms(ctx.timings()))
        n_cand = ctx.download_raw()[1]
        ctx.close()
        print(json.dumps(dict(common, mode="quarters", ms=ms, ms_sum=round(sum(ms), 2), k1_ms_sum=round(sum(k1), 2), last_quarter_n_cand=n_cand)), flush=True)
    if a.mode in ("rounds", "both"):
        ctx = idx.context(n_pairs, seed_budget_kb=a.seed_budget_kb)
        ctx.upload(capi.Batch.from_arrays(seq, seq_off, bc_off, name_seed))
        ctx.align_resident(opts)
        t = time.perf_counter()
        ctx.align_resident(opts)
        ms = round((time.perf_counter() - t) * 1e3, 2)
        info = ctx.rounds()
        timings = ctx.timings()
        t = time.perf_counter()
        n_reads, n_cand = ctx.download_raw()
        dl_ms = round((time.perf_counter() - t) * 1e3, 2)
        ctx.close()
        print(json.dumps(dict(common, mode="rounds", ms=ms, n_rounds=info["n_rounds"], first_barcode=[int(x) for x in info["first_barcode"]],
                              round_seeds=[int(x) for x in info["round_seeds"]], need_gb=round(info["need_bytes"] / 1e9, 2), budget_gb=round(info["budget_bytes"] / 1e9, 2),
                              k1_ms_sum=k1_ms(timings), timings={n: round(v, 2) for n, v in timings}, download_after_ms=dl_ms, n_reads=n_reads, n_cand=n_cand)), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
