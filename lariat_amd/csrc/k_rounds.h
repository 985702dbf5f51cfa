// k_rounds.h — a resident batch whose seed, chain and region pools do not fit their budget is aligned in ROUNDS of whole barcodes (lh_host.inc: align_rounds).
//
// The reference never turns a work unit away: BWA's vectors grow, and DoRFAForOneBarcode runs for every barcode the reader hands it (lariat.go:461-547).  Barcodes
// are independent, and after k_scan_seeds the seeds of every read are known on the device before anything is written to the pools: the exclusive scan seed_off over
// the reads, taken at the barcode boundaries, is all a plan needs.
//   k_round_cost   the prefix seed count at every barcode boundary;
//   k_round_plan   one wave: the barcode with the most seeds, then greedy cuts from barcode 0 such that every part's need stays within the budget (and, with the
//                  fewest rounds the budget allows, near an equal share of the seeds);
//   k_batch_view   part k as a batch of its own: offsets rebased to 0, bases copied to an 8-aligned buffer (k_pack_reads reads the batch buffer in 8-byte words,
//                  and a part starts wherever its first read does).
// The plan goes to page-locked host memory the device can write (as HostPeek does: not a copy-engine transfer).
#pragma once
#include "lh_dev.h"

// The workspace of `seeds` seeds in bytes — the ONE statement of the arithmetic (run_front, the plan, lh_last_rounds): the pools are allocated a quarter above the
// seed total; fixed_slots = the rescue slots of every read of the context's capacity (the region pools hold them on top); per_seed = LH_SEED_POOL_BYTES
__host__ __device__ static inline i64 lh_seed_need(i64 seeds, i64 fixed_slots, i64 per_seed) { return (seeds + seeds / 4 + fixed_slots) * per_seed; }

#define LH_WD_ROUND_PLAN 20   // watchdog slot of k_round_plan's loop over cuts

// what k_round_plan writes (mapped host memory): the header, then per cut r = 0 .. n_rounds its first barcode, first pair and first base, then per part its seeds
struct RoundPlanHdr {
    i64 n_rounds;            // 0: the barcode max_barcode alone exceeds the budget
    i64 max_barcode;         // the barcode with the most seeds (the first of equals)
    i64 max_barcode_seeds;
    i64 total_seeds;
};

__global__ void __launch_bounds__(256) k_round_cost(int n_bc, const int32_t* __restrict__ bc_pair_off, const i64* __restrict__ seed_off, i64* __restrict__ prefix) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b <= n_bc) prefix[b] = seed_off[2 * (i64)bc_pair_off[b]];
}

// One wave.  Every lane holds the same cut state (the searches are scalar and wave-uniform); lane 0 stores.  max_rounds: the room of the arrays (>= 1).
__global__ void __launch_bounds__(64) k_round_plan(int n_bc, const i64* __restrict__ prefix, const int32_t* __restrict__ bc_pair_off, const i64* __restrict__ seq_off,
                                                   i64 budget, i64 fixed_slots, i64 per_seed, int max_rounds, RoundPlanHdr* __restrict__ hdr, i64* __restrict__ cut_bc,
                                                   i64* __restrict__ cut_pair, i64* __restrict__ cut_base, i64* __restrict__ part_seeds, int32_t* __restrict__ wd) {
    const int lane = LANE();
    // the largest barcode: lanes stride over the barcodes, then a butterfly (more seeds wins, the lower index among equals)
    i64 best = -1; int best_b = 0;
    for (int b = lane; b < n_bc; b += 64) {
        const i64 s = prefix[b + 1] - prefix[b];
        if (s > best) { best = s; best_b = b; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const i64 s2 = (i64)shfl_u64((u64)best, lane ^ m);
        const int b2 = __shfl(best_b, lane ^ m);
        if (s2 > best || (s2 == best && b2 < best_b)) { best = s2; best_b = b2; }
    }
    if (best < 0) best = 0;
    int n_rounds = 0;
    if (lh_seed_need(best, fixed_slots, per_seed) <= budget) {
        // the most seeds a part may hold: need is monotone in the seeds, so a search over the seed count once, then one search over the prefix array per cut
        i64 lo = best, hi = prefix[n_bc];
        while (lo < hi) { const i64 m = lo + (hi - lo + 1) / 2; if (lh_seed_need(m, fixed_slots, per_seed) <= budget) lo = m; else hi = m - 1; }
        // ... and no part fuller than it has to be: with the fewest rounds that room allows, the parts aim at equal shares of the seeds (the pools of every round then
        // stay below the budget by what the last round would have left unused: the buffers that grow later in a round — candidates, rescue jobs, K8's tiers — find room)
        const i64 total = prefix[n_bc], fewest = lo > 0 ? (total + lo - 1) / lo : 1, share = fewest > 0 ? (total + fewest - 1) / fewest : 0;
        const i64 room = share > best ? share : best;
        int start = 0, wd_cuts = n_bc + 1;
        while (start < n_bc) {
            LH_WATCH(wd, wd_cuts, LH_WD_ROUND_PLAN, break)
            if (n_rounds >= max_rounds) { n_rounds = -1; break; }
            // the last boundary e > start with prefix[e] - prefix[start] <= room (start + 1 qualifies: no barcode holds more than `best`); equal neighbours —
            // empty barcodes — stay with the part to their left
            int a = start + 1, z = n_bc;
            const i64 top = prefix[start] + room;
            while (a < z) { const int m = a + (z - a + 1) / 2; if (prefix[m] <= top) a = m; else z = m - 1; }
            if (lane == 0) {
                cut_bc[n_rounds] = start; cut_pair[n_rounds] = bc_pair_off[start]; cut_base[n_rounds] = seq_off[2 * (i64)bc_pair_off[start]];
                part_seeds[n_rounds] = prefix[a] - prefix[start];
            }
            ++n_rounds;
            start = a;
        }
        if (n_rounds > 0 && start < n_bc) n_rounds = -1;   // (the watchdog ended the loop)
        if (lane == 0 && n_rounds > 0) { cut_bc[n_rounds] = n_bc; cut_pair[n_rounds] = bc_pair_off[n_bc]; cut_base[n_rounds] = seq_off[2 * (i64)bc_pair_off[n_bc]]; }
    }
    if (lane == 0) { hdr->max_barcode = best_b; hdr->max_barcode_seeds = best; hdr->total_seeds = prefix[n_bc]; hdr->n_rounds = n_rounds; }
}

// Part [b0, b0 + n_bc) of a batch — pairs from p0, bases from s0 — as a batch of its own: seq_off and bc_pair_off rebased to 0, the bases copied to the 8-aligned
// view (eight per thread and store; the tail word is padded with 4 = no base)
__global__ void __launch_bounds__(256) k_batch_view(int n_bc, int n_reads, i64 n_bases, int b0, int p0, i64 s0, const int32_t* __restrict__ bc_pair_off,
                                                    const i64* __restrict__ seq_off, const uint8_t* __restrict__ seq, int32_t* __restrict__ v_bc_pair_off,
                                                    i64* __restrict__ v_seq_off, u64* __restrict__ v_seq) {
    const i64 step = (i64)gridDim.x * blockDim.x, t0 = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (i64 b = t0; b <= n_bc; b += step) v_bc_pair_off[b] = bc_pair_off[b0 + b] - p0;
    for (i64 r = t0; r <= n_reads; r += step) v_seq_off[r] = seq_off[2 * (i64)p0 + r] - s0;
    const i64 nw = (n_bases + 7) / 8;
    for (i64 w = t0; w < nw; w += step) {
        u64 v = 0;
        for (int k = 0; k < 8; ++k) {
            const i64 i = w * 8 + k;
            v |= (u64)(i < n_bases ? seq[s0 + i] : 4) << (8 * k);
        }
        v_seq[w] = v;
    }
}
