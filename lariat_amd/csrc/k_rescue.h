// k_rescue.h — K6's wave-wide Smith-Waterman: BWA's ksw_align2 as mem_matesw calls it (lariat's GoBwaMemMateSW loops,
// go/src/gobwa/gobwa.go:286-325), one wavefront per alignment.  The attempts of a batch run as jobs of k_rescue2.h / k_rescue3.h; k_resc_apply
// calls this one in place for the few attempts that have no job.
//
// ksw_align2 upstream is Farrar's striped SSE2 kernel (ksw_u8): 16 byte lanes x slen segments, with a lazy-F loop that
// repairs H across stripe boundaries but never refreshes E.  Its results are therefore defined by the striping, not by
// the textbook recurrences.  Restated column-parallel (lane = query position, all 64 lanes busy):
//   hnf(k)    = max(H'(i-1,k-1) + S, E(i,k))                       (saturating u8 arithmetic: floors at 0)
//   F_seg(k)  = max-plus prefix scan of (hnf - oe_ins) RESTARTED at every stripe boundary k = L*slen  -> H_main = max(hnf, F_seg)
//   F_full(k) = the same scan over the whole row                                                    -> H'     = max(hnf, F_full)
//   E(i+1,k)  = max(E - e_del, H_main - oe_del)     row maximum is taken over H_main                (what the SSE code does)
// i.e. one segmented and one plain shuffle scan per row.  The early exit of the lazy-F loop only skips no-op work.
#pragma once
#include "k_dedup.h"

struct KswR { int score, te, qe, tb, qb; };

__device__ __forceinline__ int sat0(int x) { return x < 0 ? 0 : x; }

#define LH_SEG_BIG 8192
#define LH_SEG_OFF 256

#define LH_U8_SLAB(T)                                                                                         \
    if (64 * (T) < ncol) {                                                                                    \
        int k = 64 * (T) + lane;                                                                              \
        int in = k < ncol;                                                                                    \
        int hd = wave_shr1_i32(HP##T, hdcarry);             /* H'(i-1,k-1) */                                  \
        hdcarry = wave_readlane(HP##T, 63);                                                                          \
        int qv = qb##T;                                                                                       \
        int sc = k >= qlen ? 0 : ((tb > 3 || qv > 3) ? -1 : (tb == qv ? a_ : -b_));                           \
        int hnf = sat0(hd + sc);                                                                              \
        int e = E##T;                                                                                         \
        hnf = hnf > e ? hnf : e;                                                                              \
        /* gap-open candidates, G-transformed: cand(k) = hnf(k) - oe_ins + (k+1)*e_ins feeds F(k+1) */        \
        int cand = hnf - oe_ins + (k + 1) * e_ins;                                                            \
        int c1 = in ? cand : -0x3fffffff;                                                                     \
        int c2 = in ? cand + LH_SEG_OFF + LH_SEG_BIG * sg##T : -0x3fffffff;   /* stripe id in the high part */ \
        int i1 = wave_scan_max_i32(c1, lane), i2 = wave_scan_max_i32(c2, lane);                               \
        int x1 = wave_shr1_i32(i1, -0x3fffffff), x2 = wave_shr1_i32(i2, -0x3fffffff);                         \
        x1 = x1 > fcarry ? x1 : fcarry;                                                                       \
        x2 = x2 > scarry ? x2 : scarry;                                                                       \
        int l1_ = wave_readlane(i1, 63), l2_ = wave_readlane(i2, 63);                                                       \
        fcarry = fcarry > l1_ ? fcarry : l1_;                                                                 \
        scarry = scarry > l2_ ? scarry : l2_;                                                                 \
        int ffull = sat0(x1 - k * e_ins);                                                                     \
        int fseg = (x2 >= 0 && x2 / LH_SEG_BIG == sg##T) ? sat0(x2 % LH_SEG_BIG - LH_SEG_OFF - k * e_ins) : 0; \
        int hmain = hnf > fseg ? hnf : fseg;                                                                  \
        int hfull = hnf > ffull ? hnf : ffull;                                                                \
        if (!in) { hmain = 0; hfull = 0; }                                                                    \
        int rm = wave_max_i32(hmain);                                                                         \
        imax = imax > rm ? imax : rm;                                                                         \
        int en = sat0(e - e_del), t_ = sat0(hmain - oe_del);                                                  \
        if (in) { E##T = en > t_ ? en : t_; HN##T = hfull; }                                                  \
    }

// one pass of ksw_u8 over target rows [0,tlen): query column k = qarr[qoff + qstep*k] (complemented if qcomp),
// target row i = base at tcoord0 + tstep*i.  endsc: stop when the running maximum reaches it (KSW_XSTOP) or 0x10000.
__device__ __forceinline__ void wave_ksw_u8(const DIndex& ix, const DOpts& o, const uint8_t* qarr, int qoff, int qstep, int qcomp, int qlen, i64 tcoord0,
                                            int tstep, int tlen, int endsc, int lane, int* score_out, int* te_out, int* qe_out, u64* cells) {
    const int a_ = o.a, b_ = o.b, e_del = o.e_del, e_ins = o.e_ins, oe_del = o.o_del + o.e_del, oe_ins = o.o_ins + o.e_ins;
    int slen = (qlen + 15) / 16, ncol = slen * 16;
    int HP0 = 0, HP1 = 0, HP2 = 0, HP3 = 0, HN0 = 0, HN1 = 0, HN2 = 0, HN3 = 0, E0 = 0, E1 = 0, E2 = 0, E3 = 0;
    int HM0 = 0, HM1 = 0, HM2 = 0, HM3 = 0;   // Hmax row
    int qb0, qb1, qb2, qb3, sg0, sg1, sg2, sg3;
#define LH_U8_Q(T)                                                                     \
    {                                                                                  \
        int k = 64 * (T) + lane;                                                       \
        int v = k < qlen ? qarr[qoff + qstep * k] : 4;                                 \
        qb##T = (qcomp && v < 4) ? 3 - v : v;                                          \
        sg##T = k / slen;                                                              \
    }
    LH_U8_Q(0) LH_U8_Q(1) LH_U8_Q(2) LH_U8_Q(3)
#undef LH_U8_Q
    int gmax = 0, te = -1, tchunk = 4;
    u64 ncell = 0;
    for (int i = 0; i < tlen; ++i) {
        if ((i & 63) == 0) {
            int ii = i + lane;
            tchunk = ii < tlen ? dev_ref_base(ix, tcoord0 + (i64)tstep * ii) : 4;
        }
        int tb = wave_readlane(tchunk, i & 63);
        int imax = 0, hdcarry = 0, fcarry = -0x3fffffff, scarry = -0x3fffffff;
        LH_U8_SLAB(0) LH_U8_SLAB(1) LH_U8_SLAB(2) LH_U8_SLAB(3)
        ncell += (u64)ncol;
        HP0 = HN0; HP1 = HN1; HP2 = HN2; HP3 = HN3;
        if (imax > gmax) {
            gmax = imax; te = i;
            HM0 = HN0; HM1 = HN1; HM2 = HN2; HM3 = HN3;
            if (gmax >= endsc) break;
        }
    }
    if (cells) *cells += ncell;
    // qe: the smallest query index among the maxima of the saved row
    int best = -1;
    {
        int m0 = wave_max_i32(lane < ncol ? HM0 : -1), m1 = wave_max_i32(64 + lane < ncol ? HM1 : -1);
        int m2 = wave_max_i32(128 + lane < ncol ? HM2 : -1), m3 = wave_max_i32(192 + lane < ncol ? HM3 : -1);
        best = m0 > m1 ? m0 : m1; best = best > m2 ? best : m2; best = best > m3 ? best : m3;
    }
    int qe = -1;
    {
        u64 b0 = __ballot(lane < ncol && HM0 == best), b1 = __ballot(64 + lane < ncol && HM1 == best);
        u64 b2 = __ballot(128 + lane < ncol && HM2 == best), b3 = __ballot(192 + lane < ncol && HM3 == best);
        if (b0) qe = __ffsll((unsigned long long)b0) - 1;
        else if (b1) qe = 64 + __ffsll((unsigned long long)b1) - 1;
        else if (b2) qe = 128 + __ffsll((unsigned long long)b2) - 1;
        else if (b3) qe = 192 + __ffsll((unsigned long long)b3) - 1;
    }
    *score_out = gmax; *te_out = te; *qe_out = qe;
}

// ksw_align2 with KSW_XSUBO|KSW_XSTART|KSW_XBYTE|minsc (mem_matesw's call); the sub-optimal score (score2) is not
// computed: it only feeds mem_alnreg_t.csub, which nothing lariat reads depends on.
__device__ __forceinline__ KswR wave_ksw_align2(const DIndex& ix, const DOpts& o, const uint8_t* qarr, int qoff, int qstep, int qcomp, int qlen, i64 tcoord0,
                                                int tstep, int tlen, int minsc, int lane, u64* cells) {
    KswR r;
    r.tb = r.qb = -1;
    wave_ksw_u8(ix, o, qarr, qoff, qstep, qcomp, qlen, tcoord0, tstep, tlen, 0x10000, lane, &r.score, &r.te, &r.qe, cells);
    if (r.score < minsc) return r;
    // reverse pass over the prefixes ending at (te, qe) to find the start
    int s2, te2, qe2;
    wave_ksw_u8(ix, o, qarr, qoff + qstep * r.qe, -qstep, qcomp, r.qe + 1, tcoord0 + (i64)tstep * r.te, -tstep, r.te + 1, r.score, lane, &s2, &te2, &qe2, cells);
    if (r.score == s2) { r.tb = r.te - te2; r.qb = r.qe - qe2; }
    return r;
}

__device__ __forceinline__ int dev_infer_dir(i64 l_pac, i64 b1, i64 b2, i64* dist) {
    int r1 = (b1 >= l_pac), r2 = (b2 >= l_pac);
    i64 p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}
