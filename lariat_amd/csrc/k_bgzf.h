// k_bgzf.h — BGZF members on the device: one wave deflates one block of at most 0xff00 bytes (RFC 1951 / RFC 1952, the BC extra field of the SAM
// specification) into a complete gzip member, laid out as bgzf_block (bamfile.cpp) writes it.  Blocks are independent: nothing carries over.
//
// A wave (one single-wave workgroup, as everywhere here) takes blocks blockIdx.x, blockIdx.x + gridDim.x, ... and for each one
//   1. matches: 64 consecutive positions look up their hash's head (the latest earlier position of the same three bytes, LDS) and the
//      position before them (runs) and the last match's distance (a repeat that goes on), measure the matches, and the greedy choice — which lanes' matches survive — is made in lane order from
//      one ballot.  A head becomes the largest position of its hash in the step, whichever lane's store lands first, so the tokens are
//      a function of the block's bytes alone.  Tokens go to this wave's scratch in memory; two histograms build up in LDS: literal/length
//      and distance symbols of the tokens, and the bytes alone;
//   2. takes the CRC-32 of the block: a slice per lane through the table in LDS, the 64 values combined by multiplying each with
//      x^(8 * bytes behind its slice) mod P (the powers x^(8 * 2^k) come precomputed);
//   3. builds length-limited Huffman codes (15 bits; 7 for the code-length code) for both histograms: ranks by frequency with the wave, the
//      tree and zlib's overflow repair on lane 0, and from the lengths the exact size of three codings: stored, dynamic Huffman over the
//      bytes alone, dynamic Huffman over the tokens;
//   4. emits the smallest: every lane composes its token's bits, a prefix sum of the bit lengths places them, they are merged in an LDS
//      staging row (atomicOr into zeroed words) and leave as whole words.  The header's code lengths are sent without run-length codes.
// A member starts LH_BGZF_PAD bytes into its output slot, so that its deflate stream (18 bytes in) begins on a word.
#pragma once
#include "lh_dev.h"

#define LH_BGZF_DATA 0xff00        // uncompressed bytes per block at most
#define LH_BGZF_SLOT 0x10010       // bytes per output slot: the padding, a member of at most 0x10000 bytes, rounded up to 16
#define LH_BGZF_PAD 2
#define LH_BGZF_HASH_BITS 13       // 8,192 heads of 16 bits: the LDS words of BZ_WORDS
#define LH_BGZF_CONST_WORDS 272    // the CRC table (256 words), then x^(8 * 2^k) mod P, k = 0 .. 15
#define LH_BGZF_POLY 0xedb88320u
// watchdog words of the compressor (its own LH_WD_SLOTS words)
#define LH_BGZF_WD_GREEDY 1
#define LH_BGZF_WD_REPAIR 2
#define LH_BGZF_WD_SIZE 3     // a stream came out at another size than its histograms gave

// sections of the 4,096 words of LDS that hold the hash heads while a block is matched (in words)
#define BZ_CRCT 0      // [256] CRC table
#define BZ_WT 256      // [576] node weights, then depths
#define BZ_PAR 832     // [576] parents
#define BZ_ORD 1408    // [288] the used symbols by rising frequency
#define BZ_TABL 1696   // [288] literal/length code: bit-reversed code << 4 | length
#define BZ_TABD 1984   // [32] distance code
#define BZ_TABC 2016   // [32] code-length code
#define BZ_STAGE 2048  // [128] the bit writer's row
#define BZ_CLF 2176    // [32] how often each code length occurs in a header
#define BZ_BLC 2208    // [32] symbols per length; next code per length
#define BZ_WORDS 4096

__device__ const uint8_t lh_bgzf_member_head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};   // gzip header with one extra field, BC, of two bytes
__device__ const uint8_t lh_bgzf_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// a * b mod P, both in the reflected representation (bit 31 = x^0)
__host__ __device__ __forceinline__ uint32_t bgzf_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? LH_BGZF_POLY : 0u);
    }
    return p;
}
__device__ __forceinline__ int bgzf_len_code(int len, int* extra_bits, int* extra) {   // match length 3 .. 258 -> symbol - 257
    const int l = len - 3;
    if (len == 258) { *extra_bits = 0; *extra = 0; return 28; }
    if (l < 8) { *extra_bits = 0; *extra = 0; return l; }
    const int e = 29 - __clz((unsigned)l);   // bits above the code's two: 8..15 -> 1, .. 128..254 -> 5
    *extra_bits = e; *extra = l & ((1 << e) - 1);
    return 4 * e + 4 + ((l >> e) & 3);
}
__device__ __forceinline__ int bgzf_dist_code(int dist, int* extra_bits, int* extra) {   // distance 1 .. 32768 -> symbol
    const int d = dist - 1;
    if (d < 4) { *extra_bits = 0; *extra = 0; return d; }
    const int hb = 31 - __clz((unsigned)d), e = hb - 1;
    *extra_bits = e; *extra = d & ((1 << e) - 1);
    return 2 * hb + ((d >> e) & 1);
}
__device__ __forceinline__ int bgzf_len_extra(int sym) { const int c = sym - 257; return (c < 8 || c == 28) ? 0 : (c >> 2) - 1; }   // extra bits of a literal/length symbol
__device__ __forceinline__ int bgzf_dist_extra(int d) { return d < 4 ? 0 : (d >> 1) - 1; }
__device__ __forceinline__ int bgzf_wave_sum(int v) { for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m); return v; }
__device__ __forceinline__ int bgzf_wave_max(int v) { for (int m = 32; m; m >>= 1) { const int t = __shfl_xor(v, m); v = t > v ? t : v; } return v; }

// Huffman code lengths of at most maxb bits for the nsym frequencies f (LDS), into lens.  Fewer than two used symbols: symbol 0 and / or 1 join them at
// frequency 1 (as zlib does: a distance code of one 1-bit code, never an empty one); f itself is not changed.  Called by the whole wave; u: the LDS sections.
__device__ inline void bgzf_build_lens(const uint32_t* f, int nsym, int maxb, uint8_t* lens, uint32_t* u, int lane, int32_t* wd) {
    uint32_t *wt = u + BZ_WT, *par = u + BZ_PAR, *ord = u + BZ_ORD, *blc = u + BZ_BLC;
    int used = 0;
    for (int s0 = 0; s0 < nsym; s0 += 64) {
        const int s = s0 + lane;
        if (s < nsym) lens[s] = 0;
        used += __popcll(__ballot(s < nsym && f[s] > 0));
    }
    int pad0 = -1, pad1 = -1;
    if (used < 2) { pad0 = f[0] == 0 ? 0 : 1; if (used == 0) pad1 = 1; }
    const int n = used < 2 ? 2 : used;
    auto fq = [&](int s) -> uint32_t { return (s == pad0 || s == pad1) ? 1u : f[s]; };
    for (int s = lane; s < nsym; s += 64) {   // rank by (frequency, symbol): the order of equal frequencies is fixed
        const uint32_t fs = fq(s);
        if (!fs) continue;
        int r = 0;
        for (int j = 0; j < nsym; ++j) { const uint32_t fj = fq(j); r += (fj > 0 && (fj < fs || (fj == fs && j < s))) ? 1 : 0; }
        ord[r] = (uint32_t)s; wt[r] = fs;
    }
    WAVE_SYNC();
    if (lane == 0) {
        int i = 0, j = n;
        for (int k = n; LH_UNI(k < 2 * n - 1); ++k) {   // two queues: the leaves and the inner nodes, both by rising weight; a leaf first among equals
            int a, b;
            if (LH_UNI(i < n && (j >= k || wt[i] <= wt[j]))) a = i++; else a = j++;
            if (LH_UNI(i < n && (j >= k || wt[i] <= wt[j]))) b = i++; else b = j++;
            wt[k] = wt[a] + wt[b]; par[a] = (uint32_t)k; par[b] = (uint32_t)k;
        }
        wt[2 * n - 2] = 0;   // from here on: depths
        for (int k = 2 * n - 3; LH_UNI(k >= 0); --k) wt[k] = wt[par[k]] + 1;
        for (int b = 0; b <= 15; ++b) blc[b] = 0;
        int excess = -(1 << maxb);   // Kraft's sum over the clamped lengths, in units of 2^-maxb, less one
        for (int k = 0; LH_UNI(k < n); ++k) { int d = (int)wt[k]; if (d > maxb) d = maxb; blc[d]++; excess += 1 << (maxb - d); }
        int budget = 2 * nsym + 64;
        bool flat = false;
        while (LH_UNI(excess > 0)) {   // zlib's gen_bitlen: a leaf one level down, a leaf of the last level beside it: the sum falls by one unit
            LH_WATCH(wd, budget, LH_BGZF_WD_REPAIR, break)
            int bits = maxb - 1;
            while (LH_UNI(bits > 0 && blc[bits] == 0)) --bits;
            if (LH_UNI(bits == 0 || (bits < maxb - 1 && blc[maxb] == 0))) { flat = true; break; }
            blc[bits]--; blc[bits + 1] += 2; blc[maxb]--; --excess;
        }
        if (LH_UNI(flat)) {   // (not reached by a Huffman tree's depths) any complete code: 2^m - n symbols of m - 1 bits, the others of m
            int m = 1;
            while (LH_UNI((1 << m) < n)) ++m;
            for (int b = 0; b <= 15; ++b) blc[b] = 0;
            blc[m - 1] = (uint32_t)((1 << m) - n); blc[m] = (uint32_t)(2 * n - (1 << m));
        }
        int idx = 0;
        for (int bits = maxb; LH_UNI(bits >= 1); --bits)
            for (int c = (int)blc[bits]; LH_UNI(c > 0 && idx < n); --c) lens[ord[idx++]] = (uint8_t)bits;
    }
    WAVE_SYNC();
}

// canonical codes of lens, bit-reversed for the stream: tab[s] = code << 4 | length (0: unused).  Lane 0 works; the wave calls.
__device__ inline void bgzf_make_codes(const uint8_t* lens, int nsym, uint32_t* tab, uint32_t* u, int lane) {
    uint32_t* blc = u + BZ_BLC;
    if (lane == 0) {
        for (int b = 0; b < 32; ++b) blc[b] = 0;
        for (int s = 0; LH_UNI(s < nsym); ++s) blc[lens[s]]++;
        uint32_t code = 0;
        blc[0] = 0;
        for (int b = 1; b <= 15; ++b) { code = (code + blc[b - 1]) << 1; blc[16 + b] = code; }
        for (int s = 0; LH_UNI(s < nsym); ++s) {
            const int l = lens[s];
            tab[s] = l ? ((__brev(blc[16 + l]++) >> (32 - l)) << 4 | (uint32_t)l) : 0u;
        }
    }
    WAVE_SYNC();
}

// what a dynamic block with these code lengths costs, in bits, for the frequencies fl / fd (fd null: no distance is coded); the header's numbers come back too
struct BgzfHdr { int hlit, hdist, hclen; };
__device__ inline int bgzf_dyn_bits(const uint32_t* fl, const uint32_t* fd, const uint8_t* ll, const uint8_t* dl, uint8_t* cl, uint32_t* u, int lane, int32_t* wd, BgzfHdr* h) {
    uint32_t* clf = u + BZ_CLF;
    int last_l = 256, last_d = 0, body = 0;
    for (int s = lane; s < 286; s += 64) { if (ll[s]) last_l = s > last_l ? s : last_l; body += (int)fl[s] * (ll[s] + (s > 256 ? bgzf_len_extra(s) : 0)); }
    if (lane < 30) { if (dl[lane]) last_d = lane; if (fd) body += (int)fd[lane] * (dl[lane] + bgzf_dist_extra(lane)); }
    h->hlit = bgzf_wave_max(last_l) + 1; h->hdist = bgzf_wave_max(last_d) + 1;
    body = bgzf_wave_sum(body);
    if (lane < 32) clf[lane] = 0;
    WAVE_SYNC();
    for (int i = lane; i < h->hlit + h->hdist; i += 64) atomicAdd(&clf[i < h->hlit ? ll[i] : dl[i - h->hlit]], 1u);
    WAVE_SYNC();
    bgzf_build_lens(clf, 19, 7, cl, u, lane, wd);
    int last_c = 0, hb = 0;
    if (lane < 19) { if (cl[lh_bgzf_cl_order[lane]]) last_c = lane; hb = (int)clf[lane] * cl[lane]; }
    last_c = bgzf_wave_max(last_c) + 1;
    h->hclen = last_c < 4 ? 4 : last_c;
    return 17 + 3 * h->hclen + bgzf_wave_sum(hb) + body;
}

// the bit writer: every lane hands in nb (0 .. 48) bits, lane order is stream order.  stage: zeroed LDS row whose word 0 holds the bits of the stream's
// last, incomplete word; ow: the stream's words in memory
__device__ inline void bgzf_put(uint32_t* stage, uint32_t* ow, int& bitpos, u64 v, int nb, int lane) {
    int inc = nb;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, (unsigned)d); if (lane >= d) inc += t; }
    const int total = __shfl(inc, 63);
    const int wbase = bitpos >> 5, rel = bitpos & 31;
    if (nb) {
        const int off = rel + inc - nb, w = off >> 5, sh = off & 31;
        const u64 lo = v << sh;
        atomicOr(&stage[w], (uint32_t)lo);
        if ((uint32_t)(lo >> 32)) atomicOr(&stage[w + 1], (uint32_t)(lo >> 32));
        if (sh) { const uint32_t hi = (uint32_t)(v >> (64 - sh)); if (hi) atomicOr(&stage[w + 2], hi); }
    }
    WAVE_SYNC();
    const int full = (rel + total) >> 5;
    for (int i = lane; i < full; i += 64) ow[wbase + i] = stage[i];
    const uint32_t carry = stage[full];
    WAVE_SYNC();
    for (int i = lane; i <= full + 2; i += 64) stage[i] = 0;
    if (lane == 0) stage[0] = carry;
    bitpos += total;
    WAVE_SYNC();
}

__global__ void __launch_bounds__(64) k_bgzf(const uint8_t* __restrict__ in, const i64* __restrict__ blk_off, const int32_t* __restrict__ blk_len, int n_blocks,
                                             uint8_t* __restrict__ out, int32_t* __restrict__ out_size, uint32_t* __restrict__ tok_all, const uint32_t* __restrict__ consts, int32_t* wd) {
    // one region of LDS, two lives: 8,192 16-bit hash heads while a block is matched, then the words of the BZ_* sections.  A union, so that the compiler knows
    // both views name the same memory; a barrier separates the two lives
    __shared__ union { uint32_t w[BZ_WORDS]; uint16_t heads[2 * BZ_WORDS]; } s_mem;
    uint32_t* const s_u = s_mem.w;
    __shared__ uint32_t s_hc[320];   // the tokens' histogram: literal/length symbols at 0, distance symbols at 288
    __shared__ uint32_t s_hb[288];   // the bytes' histogram (and end-of-block)
    __shared__ uint8_t s_lc[320], s_lb[320];   // code lengths for the two, laid out like s_hc (s_lb's distance part: the one code a block without matches declares)
    __shared__ uint8_t s_cl[2][32];  // their code-length codes' lengths
    const int lane = LANE();
    uint32_t* tok = tok_all + (size_t)blockIdx.x * LH_BGZF_DATA;
    for (int blk = (int)blockIdx.x; blk < n_blocks; blk += (int)gridDim.x) {
        const uint8_t* d = in + blk_off[blk];
        int n = blk_len[blk];
        if (n < 0) n = 0;
        if (n > LH_BGZF_DATA) n = LH_BGZF_DATA;   // (the host cuts blocks; a longer one would not fit a member)
        uint8_t* m = out + (size_t)blk * LH_BGZF_SLOT + LH_BGZF_PAD;
        for (int i = lane; i < BZ_WORDS; i += 64) s_u[i] = 0;
        for (int i = lane; i < 320; i += 64) { s_hc[i] = 0; if (i < 288) s_hb[i] = 0; }
        WAVE_SYNC();
        // ---- 1. tokens
        int covered = 0, ntok = 0, last_dist = 0;   // the first position no token covers yet; tokens so far; the last match's distance
        uint16_t* const head = s_mem.heads;
        for (int base = 0; base < n; base += 64) {
            const int p = base + lane;
            const int c0 = p < n ? d[p] : 0;
            if (p < n) atomicAdd(&s_hb[c0], 1u);
            const bool canh = p + 2 < n;
            uint32_t h = 0, cand = 0;
            if (canh) {
                h = ((uint32_t)c0 | (uint32_t)d[p + 1] << 8 | (uint32_t)d[p + 2] << 16) * 0x9e3779b1u >> (32 - LH_BGZF_HASH_BITS);
                cand = head[h];   // position + 1 of the latest earlier step's occurrence
            }
            EMU_SYNC();
            // the head becomes the largest position of its hash in this step.  Lanes of one hash store together and one of them lands: the others see a smaller
            // value and store again, so the last word is the maximum whichever lane lands first (at most 64 rounds; one, unless hashes meet inside the step)
            for (int round = 0; round < 64; ++round) {
                if (canh && head[h] < (uint16_t)(p + 1)) head[h] = (uint16_t)(p + 1);
                WAVE_SYNC();   // (a barrier, so that what is read back is what landed, not what this lane stored)
                if (!__any(canh && head[h] < (uint16_t)(p + 1))) break;
            }
            int mlen = 0, mdist = 0;
            if (canh && p >= covered) {
                const int maxl = n - p < 258 ? n - p : 258;
                if (p >= 1 && d[p - 1] == c0) {   // a run: the byte before, the cheapest distance
                    int l = 1;
                    while (l < maxl && d[p + l] == c0) ++l;
                    if (l >= 3) { mlen = l; mdist = 1; }
                }
                if (cand && mlen < maxl && p - (int)(cand - 1) <= 32768) {
                    const uint8_t* q = d + (cand - 1);
                    int l = 0;
                    while (l < maxl && q[l] == d[p + l]) ++l;
                    const int dist = p - (int)(cand - 1);
                    if (l > mlen && l >= 3 && !(l == 3 && dist > 4096)) { mlen = l; mdist = dist; }
                }
                if (last_dist > 1 && last_dist <= p && last_dist != mdist && mlen < maxl) {   // the distance of the match before: a long repeat goes on
                    const uint8_t* q = d + (p - last_dist);
                    int l = 0;
                    while (l < maxl && q[l] == d[p + l]) ++l;
                    if (l > mlen && l >= 3 && !(l == 3 && last_dist > 4096)) { mlen = l; mdist = last_dist; }
                }
            }
            const unsigned long long mm = __ballot(mlen >= 3);
            const int end = base + 64 < n ? base + 64 : n;
            int cur = covered > base ? covered : base;
            int budget = 66;
            while (cur < end) {   // lane order: literals up to the next match that starts uncovered, then that match
                LH_WATCH(wd, budget, LH_BGZF_WD_GREEDY, break)
                const unsigned long long m2 = (mm >> (cur - base)) << (cur - base);
                const int f = m2 ? __ffsll(m2) - 1 : 64;
                const int fpos = base + f < end ? base + f : end;
                if (p >= cur && p < fpos) { tok[ntok + (p - cur)] = (uint32_t)c0; atomicAdd(&s_hc[c0], 1u); }
                ntok += fpos - cur; cur = fpos;
                if (f < 64 && cur < end) {
                    const int L = __shfl(mlen, f), D = __shfl(mdist, f);
                    if (lane == f) {
                        int eb, ev;
                        tok[ntok] = 0x80000000u | (uint32_t)(D - 1) << 8 | (uint32_t)(L - 3);
                        atomicAdd(&s_hc[257 + bgzf_len_code(L, &eb, &ev)], 1u);
                        atomicAdd(&s_hc[288 + bgzf_dist_code(D, &eb, &ev)], 1u);
                    }
                    ++ntok; cur += L; last_dist = D;
                }
            }
            if (cur > covered) covered = cur;
            EMU_SYNC();
        }
        WAVE_SYNC();
        if (lane == 0) { s_hc[256] = 1; s_hb[256] = 1; }
        // ---- 2. CRC-32 (the hash heads are dead: their words hold the tables from here on)
        for (int i = lane; i < 256; i += 64) s_u[BZ_CRCT + i] = consts[i];
        for (int i = lane; i < 128; i += 64) s_u[BZ_STAGE + i] = 0;
        WAVE_SYNC();
        uint32_t crc;
        {
            const int S = (n + 63) / 64;
            const int beg = lane * S < n ? lane * S : n, fin = beg + S < n ? beg + S : n;
            uint32_t c = 0xffffffffu;
            for (int i = beg; i < fin; ++i) c = s_u[BZ_CRCT + ((c ^ d[i]) & 0xff)] ^ (c >> 8);
            c ^= 0xffffffffu;
            const int after = n - fin;
            for (int k = 0; k < 16; ++k) if (after >> k & 1) c = bgzf_mulmod(consts[256 + k], c);
            for (int mk = 32; mk; mk >>= 1) c ^= __shfl_xor(c, mk);
            crc = c;
        }
        // ---- 3. the codes and what each coding costs
        bgzf_build_lens(s_hc, 286, 15, s_lc, s_u, lane, wd);
        bgzf_build_lens(s_hc + 288, 30, 15, s_lc + 288, s_u, lane, wd);
        bgzf_build_lens(s_hb, 286, 15, s_lb, s_u, lane, wd);
        if (lane < 32) s_lb[288 + lane] = lane < 2 ? 1 : 0;
        WAVE_SYNC();
        BgzfHdr hc, hb;
        const int bits_c = bgzf_dyn_bits(s_hc, s_hc + 288, s_lc, s_lc + 288, s_cl[0], s_u, lane, wd, &hc);
        const int bits_b = bgzf_dyn_bits(s_hb, nullptr, s_lb, s_lb + 288, s_cl[1], s_u, lane, wd, &hb);
        const int bytes_a = 5 + n, bytes_b = (bits_b + 7) >> 3, bytes_c = (bits_c + 7) >> 3;
        const int coding = (n == 0 || (bytes_a <= bytes_b && bytes_a <= bytes_c)) ? 0 : bytes_b <= bytes_c ? 1 : 2;
        const int zbytes = coding == 0 ? bytes_a : coding == 1 ? bytes_b : bytes_c;
        // ---- 4. the member
        if (lane < 16) m[lane] = lh_bgzf_member_head[lane];
        if (lane == 16) { m[16] = (uint8_t)(zbytes + 25); m[17] = (uint8_t)((zbytes + 25) >> 8); }   // BSIZE: the member's size less one
        uint8_t* z = m + 18;
        if (coding == 0) {
            if (lane == 0) { z[0] = 1; z[1] = (uint8_t)n; z[2] = (uint8_t)(n >> 8); z[3] = (uint8_t)~n; z[4] = (uint8_t)(~n >> 8); }
            for (int i = lane; i < n; i += 64) z[5 + i] = d[i];
        } else {
            const uint8_t *ll = coding == 1 ? s_lb : s_lc, *dl = ll + 288, *cl = s_cl[coding == 1 ? 1 : 0];
            const BgzfHdr hh = coding == 1 ? hb : hc;
            uint32_t *tabl = s_u + BZ_TABL, *tabd = s_u + BZ_TABD, *tabc = s_u + BZ_TABC, *stage = s_u + BZ_STAGE;
            bgzf_make_codes(ll, 286, tabl, s_u, lane);
            bgzf_make_codes(dl, 30, tabd, s_u, lane);
            bgzf_make_codes(cl, 19, tabc, s_u, lane);
            uint32_t* ow = (uint32_t*)z;
            int bitpos = 0;
            {
                u64 v = 0; int nb = 0;
                if (lane == 0) { v = 1u | 2u << 1 | (u64)(hh.hlit - 257) << 3 | (u64)(hh.hdist - 1) << 8 | (u64)(hh.hclen - 4) << 13; nb = 17; }
                else if (lane - 1 < hh.hclen) { v = cl[lh_bgzf_cl_order[lane - 1]]; nb = 3; }
                bgzf_put(stage, ow, bitpos, v, nb, lane);
            }
            for (int i0 = 0; i0 < hh.hlit + hh.hdist; i0 += 64) {
                const int i = i0 + lane;
                u64 v = 0; int nb = 0;
                if (i < hh.hlit + hh.hdist) { const uint32_t t = tabc[i < hh.hlit ? ll[i] : dl[i - hh.hlit]]; v = t >> 4; nb = (int)(t & 15); }
                bgzf_put(stage, ow, bitpos, v, nb, lane);
            }
            const int items = coding == 1 ? n : ntok;
            for (int i0 = 0; i0 < items; i0 += 64) {
                const int i = i0 + lane;
                u64 v = 0; int nb = 0;
                if (i < items) {
                    const uint32_t t = coding == 1 ? (uint32_t)d[i] : tok[i];
                    if (!(t >> 31)) { const uint32_t c = tabl[t & 0xff]; v = c >> 4; nb = (int)(c & 15); }
                    else {
                        int leb, lev, deb, dev;
                        const uint32_t lc = tabl[257 + bgzf_len_code((int)(t & 0xff) + 3, &leb, &lev)];
                        const uint32_t dc = tabd[bgzf_dist_code((int)(t >> 8 & 0x7fff) + 1, &deb, &dev)];
                        v = lc >> 4; nb = (int)(lc & 15);
                        v |= (u64)lev << nb; nb += leb;
                        v |= (u64)(dc >> 4) << nb; nb += (int)(dc & 15);
                        v |= (u64)dev << nb; nb += deb;
                    }
                }
                bgzf_put(stage, ow, bitpos, v, nb, lane);
            }
            {
                const uint32_t c = tabl[256];
                bgzf_put(stage, ow, bitpos, lane == 0 ? (u64)(c >> 4) : 0, lane == 0 ? (int)(c & 15) : 0, lane);
            }
            if (lane == 0 && (bitpos & 31)) ow[bitpos >> 5] = stage[0];
            if (lane == 0 && ((bitpos + 7) >> 3) != zbytes) wd[LH_BGZF_WD_SIZE] = 1;
        }
        WAVE_SYNC();
        if (lane == 0) {
            uint8_t* t = z + zbytes;
            for (int k = 0; k < 4; ++k) { t[k] = (uint8_t)(crc >> (8 * k)); t[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
            out_size[blk] = 18 + zbytes + 8;
        }
        WAVE_SYNC();
    }
}
