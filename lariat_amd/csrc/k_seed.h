// k_seed.h — K2: SA lookups (bwt_sa) for every sampled occurrence of every SMEM interval, one 16-lane group per read
// (k_seed_grp; LH_F_SEED_LANE: one LANE per seed, k_seed_owner + k_seed), plus the exclusive scan that sizes the seed pool.  Replaces the `bwt_sa` / `bns_intv2rid` part of BWA's mem_chain
// (reached through mem_align1_core, go/src/gobwa/gobwa.go:244,253).
// Each lane chases ~sa_intv/2 dependent LF steps, every step one random 64-B occurrence block: pure HBM latency,
// hidden by running one independent chain per lane.
#pragma once
#include "lh_dev.h"

struct DSeed { i64 rbeg; int32_t qbeg, len; };

// exclusive scan out[i] = sum_{j<i} max(in[j] + add, at_least), out[n] = total, in three launches:
// (out2, if given: out2[i] = out[i] + i * add2, the scan of in[j] + add + add2 where at_least does not bind — the region slots from the seed counts)
//   k_scan_partial (per 2048-element tile: tile sums) -> k_scan_tiles (one workgroup scans the tile sums) -> k_scan_final.
#define LH_SCAN_TILE 2048
__device__ __forceinline__ i64 scan_val(const int32_t* in, int i, int n, int add, int at_least) {
    if (i >= n) return 0;
    i64 v = (i64)in[i] + add;
    return v < at_least ? at_least : v;
}
__global__ void __launch_bounds__(256) k_scan_partial(int n, const int32_t* __restrict__ in, int add, int at_least, i64* __restrict__ tile_sum) {
    __shared__ i64 part[256];
    int t = threadIdx.x, base = blockIdx.x * LH_SCAN_TILE + t * 8;
    i64 s = 0;
    for (int u = 0; u < 8; ++u) s += scan_val(in, base + u, n, add, at_least);
    part[t] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) part[t] += part[t + d];
        __syncthreads();
    }
    if (t == 0) tile_sum[blockIdx.x] = part[0];
}
__global__ void __launch_bounds__(256) k_scan_tiles(int n_tiles, i64* __restrict__ tile_sum) {   // in place: exclusive scan, total at [n_tiles]
    __shared__ i64 part[256];
    __shared__ i64 carry_s;
    int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n_tiles; base += 256) {
        int i = base + t;
        i64 v = i < n_tiles ? tile_sum[i] : 0;
        part[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            i64 o = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += o;
            __syncthreads();
        }
        i64 excl = part[t] - v + carry_s;
        __syncthreads();
        if (i < n_tiles) tile_sum[i] = excl;
        if (t == 255) carry_s += part[255];
        __syncthreads();
    }
    if (t == 0) tile_sum[n_tiles] = carry_s;
}
__global__ void __launch_bounds__(256) k_scan_final(int n, const int32_t* __restrict__ in, int add, int at_least, const i64* __restrict__ tile_sum, int n_tiles,
                                                    i64* __restrict__ out, i64* __restrict__ out2, int add2) {
    __shared__ i64 part[256];
    int t = threadIdx.x, base = blockIdx.x * LH_SCAN_TILE + t * 8;
    i64 loc[8], s = 0;
    for (int u = 0; u < 8; ++u) { loc[u] = s; s += scan_val(in, base + u, n, add, at_least); }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        i64 o = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    i64 excl = part[t] - s + tile_sum[blockIdx.x];
    for (int u = 0; u < 8; ++u) if (base + u < n) out[base + u] = excl + loc[u];
    if (blockIdx.x == 0 && t == 0) out[n] = tile_sum[n_tiles];
    if (out2) {
        for (int u = 0; u < 8; ++u) if (base + u < n) out2[base + u] = excl + loc[u] + (i64)(base + u) * add2;
        if (blockIdx.x == 0 && t == 0) out2[n] = tile_sum[n_tiles] + (i64)n * add2;
    }
}

// (LH_F_SEED_LANE) owner[g] = the read seed slot g belongs to (one lane per read writes its few slots): spares k_seed a 21-step binary search per seed
__global__ void __launch_bounds__(256) k_seed_owner(int n_reads, const i64* __restrict__ seed_off, i64 pool_cap, int32_t* __restrict__ owner) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) {
        i64 e = seed_off[r + 1] < pool_cap ? seed_off[r + 1] : pool_cap;
        for (i64 g = seed_off[r]; g < e; ++g) owner[g] = r;
    }
}

// K2 under LH_F_SEED_LANE.  one lane per seed; grid-stride over the pool.
__global__ void __launch_bounds__(256) k_seed(DIndex ix, DOpts o, int n_reads, const i64* __restrict__ seed_off, i64 pool_cap,
                                              const DIntv* __restrict__ intv, const int32_t* __restrict__ n_intv, DSeed* __restrict__ seeds,
                                              int32_t* __restrict__ s_rid, DCounters* __restrict__ ctr, const int32_t* __restrict__ owner,
                                              const int32_t* __restrict__ big_slot, const DIntv* __restrict__ big_slab) {
    i64 total = seed_off[n_reads];
    if (total > pool_cap) total = pool_cap;
    i64 stride = (i64)gridDim.x * blockDim.x;
    i64 nrounds = (total + stride - 1) / stride;
    for (i64 rd = 0; rd < nrounds; ++rd) {
        i64 g = rd * stride + (i64)blockIdx.x * blockDim.x + threadIdx.x;
        int nlf = 0, nsa = 0;
        if (g < total) {
            int r = owner[g];
            i64 u = g - seed_off[r];
            const int bs = big_slot ? big_slot[r] : -1;   // (a read with more than LH_MAX_INTV intervals: the sorted half of its big-slab slot, k_smem4.h)
            const DIntv* iv = bs < 0 ? intv + (size_t)r * LH_MAX_INTV : big_slab + ((size_t)bs * 2 + 1) * LH_BIG_INTV;
            int n = n_intv[r];
            u64 x0 = 0, step = 1, info = 0;
            for (int t = 0; t < n; ++t) {
                u64 s = iv[t].x2;
                u64 st = 1, c = s;   // (the usual interval has at most max_occ occurrences: every one is a seed; the 64-bit divisions are for the others)
                if (s > (u64)o.max_occ) {
                    st = s / (u64)o.max_occ;
                    c = (s + st - 1) / st;
                    if (c > (u64)o.max_occ) c = (u64)o.max_occ;
                }
                if ((u64)u < c) { x0 = iv[t].x0; step = st; info = iv[t].info; break; }
                u -= (i64)c;
            }
            i64 rbeg;
            if (x0 >> 62 & 1) rbeg = (i64)(x0 & ~(1ull << 62));   // K1 stored the interval's one occurrence by its text position (LH_POSF, k_smem4.h)
            else rbeg = (i64)dev_sa(ix, x0 + (u64)u * step, &nlf);
            nsa = 1;   // (n_sa counts the reference's bwt_sa calls: one per seed)
            int qbeg = (int)(info >> 32), slen = (int)(uint32_t)info - qbeg;
            DSeed sd;
            sd.rbeg = rbeg; sd.qbeg = qbeg; sd.len = slen;
            seeds[g] = sd;
            s_rid[g] = dev_intv2rid(ix, rbeg, rbeg + slen);
        }
        if (ctr) {
            int tl = wave_sum_i32(nlf), ts = wave_sum_i32(nsa);
            if (LANE() == 0 && ts) { atomicAdd(&LH_CTR(ctr)->n_lf, (u64)tl); atomicAdd(&LH_CTR(ctr)->n_sa, (u64)ts); }
        }
    }
}

// the seeds an interval of s occurrences yields (mem_chain: every step-th occurrence, at most max_occ) and the step between them
__device__ __forceinline__ u64 dev_seed_step(const DOpts& o, u64 s, u64* step) {
    *step = 1;
    if (s <= (u64)o.max_occ) return s;   // (the usual interval has at most max_occ occurrences: every one is a seed; the 64-bit divisions are for the others)
    const u64 st = s / (u64)o.max_occ, c = (s + st - 1) / st;
    *step = st;
    return c < (u64)o.max_occ ? c : (u64)o.max_occ;
}

// K2.  One 16-lane group per read, four reads per wave, the waves grid-stride over the batch.  The group takes the read's sorted intervals 16 at a time, lane `sub`
// entry sub + 16t of chunk t (k_smem_fin's layout): each lane counts its entry's seeds, a prefix over the row places them, and the chunk — position, query span,
// step, prefix: 28 B an entry, 1,792 B of LDS a wave — is staged in LDS.  The 16 lanes then stride over the chunk's seed slots: a slot finds its interval by four
// look-ups in the staged prefix and reads its entry there, so an interval is read from memory once, a repeat interval's up-to-max_occ occurrences and a unique read's
// ten intervals of one both keep their lanes busy, and sixteen consecutive slots are one write.  Seeds, their order (intervals in `info` order, occurrences
// u = 0 .. c-1 within each), the clamp at pool_cap and the counters are k_seed's.  Every cross-lane step is reached by the whole wave: trip counts are the wave's maxima.
struct K2Intv { u64 x0, x2, info; };   // what K2 reads of an interval
__device__ __forceinline__ K2Intv k2_load(const DIntv* __restrict__ iv, int e, int n) {
    K2Intv m;
    m.x0 = m.x2 = m.info = 0;
    if (e < n) { m.x0 = iv[e].x0; m.x2 = iv[e].x2; m.info = iv[e].info; }
    return m;
}
// the number of keys of the lane's 16-lane row that are below its own (the keys of a row differ: the rank of each is its place in their order)
__device__ __forceinline__ int row_rank_u32(uint32_t key) {
    int rank = 0;
#ifdef LH_EMU
    const int lane = LANE();
    for (int d = 1; d < 16; ++d) rank += __shfl(key, (lane & ~15) | ((lane + d) & 15)) < key;
#else
#define LH_ROW_ROR(d) rank += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x120 + (d), 0xF, 0xF, true) < key;   // row_ror:d
    LH_ROW_ROR(1) LH_ROW_ROR(2) LH_ROW_ROR(3) LH_ROW_ROR(4) LH_ROW_ROR(5) LH_ROW_ROR(6) LH_ROW_ROR(7) LH_ROW_ROR(8)
    LH_ROW_ROR(9) LH_ROW_ROR(10) LH_ROW_ROR(11) LH_ROW_ROR(12) LH_ROW_ROR(13) LH_ROW_ROR(14) LH_ROW_ROR(15)
#undef LH_ROW_ROR
#endif
    return rank;
}
#define LH_K2_GRID 16384   // waves of k_seed_grp: about twice what the device holds at eight waves per SIMD, so that the last ones to finish are short of work for less time
__global__ void __launch_bounds__(64) k_seed_grp(DIndex ix, DOpts o, int n_reads, const i64* __restrict__ seed_off, i64 pool_cap, const DIntv* __restrict__ intv,
                                                 const int32_t* __restrict__ n_intv, DSeed* __restrict__ seeds, int32_t* __restrict__ s_rid, DCounters* __restrict__ ctr,
                                                 const int32_t* __restrict__ big_slot, const DIntv* __restrict__ big_slab) {
    __shared__ u64 sh_x0[64], sh_info[64], sh_step[64];
    __shared__ int sh_incl[64];
    const int lane = LANE(), sub = lane & 15, row = lane & ~15;
    const int n_items = (n_reads + 3) >> 2;
    int nlf = 0, nsa = 0;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int r = item * 4 + (lane >> 4);
        const bool live = r < n_reads;
        int n = 0, S = 0;   // S: the read's seed slots below pool_cap
        i64 base = 0;
        const DIntv* iv = intv;
        if (live) {
            n = n_intv[r];
            base = seed_off[r];
            const i64 end = seed_off[r + 1] < pool_cap ? seed_off[r + 1] : pool_cap;
            S = end > base ? (int)(end - base) : 0;
            const int bs = big_slot ? big_slot[r] : -1;   // (a read with more than LH_MAX_INTV intervals: the sorted half of its big-slab slot, k_smem4.h)
            iv = bs < 0 ? intv + (size_t)r * LH_MAX_INTV : big_slab + ((size_t)bs * 2 + 1) * LH_BIG_INTV;
        }
        const int n_chunks = wave_max_i32((n + 15) >> 4);
        int run = 0;   // seeds of the chunks before this one
        for (int ch = 0; ch < n_chunks; ++ch) {
            const bool have = ch * 16 + sub < n;
            const K2Intv m = k2_load(iv, ch * 16 + sub, n);
            u64 m_step = 1;
            const int cnt = have ? (int)dev_seed_step(o, m.x2, &m_step) : 0;
            // a read of at most 16 intervals arrives as K1 emitted it (pass 3 has counted it: no k_smem_fin): its one chunk is ranked here by (info, slot) — query
            // span and slot are one 32-bit key, LH_MAXLEN < 256 — and staged at its rank, lanes without an entry last.  Rows of more intervals were sorted in
            // memory and keep their places, as sorted input would anyway
            int pos = lane;
            if (ch == 0) {
                const uint32_t key = n > 16 ? (uint32_t)sub : !have ? 0xfffffff0u | (uint32_t)sub : (uint32_t)(m.info >> 32) << 12 | ((uint32_t)m.info & 0xffu) << 4 | (uint32_t)sub;
                pos = row | row_rank_u32(key);
            }
            EMU_SYNC();   // (the slots of the chunk before have read theirs)
            sh_x0[pos] = m.x0; sh_info[pos] = m.info; sh_step[pos] = m_step; sh_incl[pos] = cnt;
            EMU_SYNC();
            const int incl = row_scan_add_i32(sh_incl[lane]);   // (a lane's own word: nobody else reads it before the next rendezvous)
            sh_incl[lane] = incl;
            EMU_SYNC();
            const int tot = sh_incl[row | 15];
            const int n_iter = wave_max_i32((tot + 15) >> 4);
            for (int it = 0; it < n_iter; ++it) {
                const int k = it * 16 + sub;   // the slot inside the chunk
                int j = 0;                     // its interval: the entries of the row whose prefix is <= k
#pragma unroll
                for (int w = 8; w >= 1; w >>= 1) j += sh_incl[row | (j + w - 1)] <= k ? w : 0;
                const int src = row | j;
                if (k < tot && run + k < S) {
                    const int u = k - (j ? sh_incl[src - 1] : 0);   // the occurrence inside the interval
                    const u64 x0 = sh_x0[src], st = sh_step[src], info = sh_info[src];
                    i64 rbeg;
                    if (x0 >> 62 & 1) rbeg = (i64)(x0 & ~(1ull << 62));   // K1 stored the interval's one occurrence by its text position (LH_POSF, k_smem4.h)
                    else { int lf = 0; rbeg = (i64)dev_sa(ix, x0 + (u64)u * st, &lf); nlf += lf; }
                    ++nsa;   // (n_sa counts the reference's bwt_sa calls: one per seed)
                    const int qbeg = (int)(info >> 32), slen = (int)(uint32_t)info - qbeg;
                    DSeed sd;
                    sd.rbeg = rbeg; sd.qbeg = qbeg; sd.len = slen;
                    const i64 g = base + run + k;
                    seeds[g] = sd;
                    s_rid[g] = dev_intv2rid(ix, rbeg, rbeg + slen);
                }
            }
            run += tot;
        }
    }
    if (ctr) {
        const int tl = wave_sum_i32(nlf), ts = wave_sum_i32(nsa);
        if (lane == 0 && ts) { atomicAdd(&LH_CTR(ctr)->n_lf, (u64)tl); atomicAdd(&LH_CTR(ctr)->n_sa, (u64)ts); }
    }
}
