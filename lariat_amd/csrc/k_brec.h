// k_brec.h — N1 on the device: the BAM records of a batch derived and encoded by kernels (lh_brec.inc drives them; lh_bam_set_device_records).
// The specification is the host path and stays there: records.cpp::append_bam says what a record holds (bamwriter.go AppendBam), bamfile.cpp::encode how it
// is laid out.  Every rule below restates one of theirs; the files must come out byte for byte the same.
//
//   k_brec_plan    one lane per PAIR.  AppendBam edits the alignment it is handed (pos = -1, mapq = 0 for an improper low-score one) and later records of the
//                  pair read the edited values, so the lane walks the pair's up to four records in the reference's order (read 0's active, its split, read 1's
//                  active, its split) with the edits as a bit per gathered row.  Per record: the fixed fields, which tags exist, the byte size, the output file.
//   k_brec_keys / k_brec_sorted / k_brec_place   the offsets: every record's place in bc_sorted (a scan of the sizes in input order) and in its position
//                  bucket (a stable sort by file, then a scan: records of one file keep input order, which is what the host's join gives).
//   k_brec_write   a 16-lane group per record, one wave per pair: the lanes stride over the record's bytes and store each to both places.
//   k_brec_f6      the %.6f of the DM tag on its own (lh_diag_format_f6).
//   k_brec_gather_count / k_brec_gather_fill   the rows the kernels above read, gathered from a context's resident result (lh_bam_append_resident) instead of by the
//                  host from a downloaded one: a lane per read counts its CIGAR operations and mismatch loci, two scans place them, a 16-lane group per read fills.
#pragma once
#include "lh_dev.h"
#include "k_rfa.h"   // DCand (k_aln.h), DInf: where a context's result lies

#define LH_BREC_SLOTS 4   // rows gathered per read: the active alignment, its split, the second best, the active's mate
#define LH_BREC_WD_LOOP 1   // watchdog word: a loop over a CIGAR or a mismatch list ran out of its budget
#define LH_BREC_E_FORMAT 1  // err[0] bits: a read name over 254 bytes or more than 65,535 CIGAR operations
#define LH_BREC_E_DM 2      // ... a molecule_difference that is not finite or not below 2^31
#define LH_BREC_E_NOACTIVE 4   // the device gather's own word: a read has no active alignment
#define LH_BREC_E_INDEX 8      // ... a candidate index or a mismatch list's continuation lies outside the result
// which optional tags a record has (BrecPlan::tags)
#define LH_BREC_T_TR 1
#define LH_BREC_T_BC 2
#define LH_BREC_T_RG 4
#define LH_BREC_T_SA 8
#define LH_BREC_T_BX 16
#define LH_BREC_T_DM 32
#define LH_BREC_T_XM 64     // XM is "1"
#define LH_BREC_T_AM 128    // AM is "1"
#define LH_BREC_T_XC 256    // the read has a second best: XC lists its mismatches
#define LH_BREC_T_QUAL 512  // QUAL has SEQ's length (else 0xff fill)
#define LH_BREC_T_CLIP0 1024  // a split's first / last operation is a soft clip: written as a hard clip
#define LH_BREC_T_CLIP1 2048

struct BrecRow {   // one alignment a record reads, gathered by the host from the result's columns
    i64 ci;        // its candidate index (-1: none).  Rows of a pair with equal ci are ONE alignment: an edit of one is seen through all
    i64 pos, aend;
    i64 cig_off, mm_off;   // into BrecIn::cig, BrecIn::mm (pairs)
    double mol_diff;
    int32_t rid, score, mapq, mol_id, n_cig, n_mm;
    uint8_t reversed, is_proper, duplicate, active_mol;
    int32_t pad_;
};
static_assert(sizeof(BrecRow) == 80, "the host gathers into this layout");

struct BrecIn {   // what the kernels read: the gathered rows and the ingest batch's text, as uploaded
    int32_t n_pairs, n_sets, n_contigs, n_out;
    const BrecRow* row;     // [2 * n_pairs][LH_BREC_SLOTS]
    const double* rd;       // [2 * n_pairs][4] second_best_score, as_score, split_second_best, split_score
    const uint32_t* cig;
    const int32_t* mm;      // ref_loc, read_loc per locus
    const uint8_t* seq; const i64* seq_off;
    const int32_t* bc_pair_off; const uint8_t* set_complete;
    const char *name, *qual1, *qual2, *trim_bases, *trim_quals, *bc, *rawbc, *bcqual, *si, *siqual, *rgid;
    const i64 *name_off, *qual1_off, *qual2_off, *trim_off, *bc_off, *rawbc_off, *bcqual_off, *si_off, *siqual_off, *rgid_off;
    const char* cname; const i64* cname_off;            // contig names [n_contigs + 1]
    const int32_t* bucket_off; const int32_t* bucket;   // the writer's bucket[rid][chunk] -> file, flattened
    i64 chunk;
};

struct BrecPlan {   // one record, before its bytes: slot 4 * pair + 2 * mate + is_split
    uint32_t size;   // bytes, block_size word included; 0: the read has no such record
    int32_t file;
    int32_t rid, pos, mrid, mpos, tlen;
    uint32_t bin_mq_nl, flag_nc, l_seq;
    int32_t start, qstart;   // the first base / quality of the slice, in the record's orientation (hard clip of a split)
    uint32_t tags;
    int32_t xs, as, xt;
    int32_t xc_len, ac_len, sa_len;
    int32_t sa_mapq, sa_nm;
    i64 sa_pos;
};

// ------------------------------------------------------------------------------------------------ numbers as text
__device__ __forceinline__ int brec_declen(long long v) {
    u64 u = v < 0 ? 0ull - (u64)v : (u64)v;
    int n = v < 0 ? 2 : 1;
    while (u >= 10) { u /= 10; ++n; }
    return n;
}
// decimal digits of v into b (at most 20 bytes), most significant first; returns their number
__device__ __forceinline__ int brec_dec(char* b, long long v) {
    const int n = brec_declen(v);
    u64 u = v < 0 ? 0ull - (u64)v : (u64)v;
    for (int i = n - 1; i >= (v < 0 ? 1 : 0); --i) { b[i] = (char)('0' + (int)(u % 10)); u /= 10; }
    if (v < 0) b[0] = '-';
    return n;
}
// (int32_t)(long long)x as x86 computes it (cvttsd2si): NaN and values outside int64 give INT64_MIN, whose low word is 0
__device__ __forceinline__ int32_t brec_f2i(double x) {
    if (!(x > -9223372036854775808.0 && x < 9223372036854775808.0)) return 0;
    return (int32_t)(uint32_t)(u64)(i64)x;
}
__device__ __forceinline__ void brec_mul64(u64 a, u64 b, u64* hi, u64* lo) {
#ifdef LH_EMU
    const unsigned __int128 p = (unsigned __int128)a * b;
    *hi = (u64)(p >> 64); *lo = (u64)p;
#else
    *hi = __umul64hi(a, b); *lo = a * b;
#endif
}
// printf("%.6f", v) for finite |v| < 2^31, as glibc prints it: correctly rounded from the exact binary value, ties to even.  The integer part and the fraction
// are both exact in a double; the fraction is M * 2^-s with M < 2^53 and s >= 53, so fraction * 10^6 = (M * 10^6) >> s is a 73-bit product cut at bit s: the six
// digits above the cut, the round bit at s - 1, the sticky bits below.  Returns the length (at most 18), 0: refused.  b holds 24 bytes.
__device__ __forceinline__ int brec_f6(double v, char* b) {
    u64 bits;
    __builtin_memcpy(&bits, &v, 8);
    const int neg = (int)(bits >> 63);
    bits &= ~(1ull << 63);
    double a;
    __builtin_memcpy(&a, &bits, 8);
    if (!(a < 2147483648.0)) return 0;   // NaN, infinity, too large
    u64 ip = (u64)a;
    const double fr = a - (double)ip;
    u64 fb;
    __builtin_memcpy(&fb, &fr, 8);
    const int e = (int)(fb >> 52);
    const u64 m = e ? ((fb & ((1ull << 52) - 1)) | 1ull << 52) : fb;
    const int s = e ? 1075 - e : 1074;
    u64 hi, lo, d = 0;
    brec_mul64(m, 1000000ull, &hi, &lo);
    if (s < 128 && (hi | lo)) {
        // q = P >> (s - 1): the digits and the round bit; sticky = the bits of P below s - 1
        const int t = s - 1;   // 52 .. 126
        u64 q, sticky;
        if (t < 64) { q = lo >> t | hi << (64 - t); sticky = lo & ((1ull << t) - 1); }
        else if (t == 64) { q = hi; sticky = lo; }
        else { q = hi >> (t - 64); sticky = lo | (hi & ((1ull << (t - 64)) - 1)); }
        d = q >> 1;
        if ((q & 1) && (sticky || (d & 1))) ++d;
    }
    if (d >= 1000000ull) { d -= 1000000ull; ++ip; }
    int n = 0;
    if (neg) b[n++] = '-';
    n += brec_dec(b + n, (long long)ip);
    b[n++] = '.';
    for (int i = 5; i >= 0; --i) { b[n + i] = (char)('0' + (int)(d % 10)); d /= 10; }
    return n + 6;
}

__global__ void __launch_bounds__(64) k_brec_f6(int n, const double* __restrict__ v, char* __restrict__ out, int32_t* __restrict__ refused) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    char b[24];
    const int len = brec_f6(v[i], b);
    for (int k = 0; k < 32; ++k) out[(i64)i * 32 + k] = k < len ? b[k] : 0;
    if (!len) atomicOr(refused, (int32_t)1);
}

// ------------------------------------------------------------------------------------------------ the plan
__device__ __forceinline__ int brec_reg2bin(i64 beg, i64 end) {   // SAM spec section 5.3
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
// the bytes of "ref,read,1;" for the loci of a row
__device__ __forceinline__ int brec_mm_len(const BrecIn& in, const BrecRow& r, int32_t* wd, int* budget) {
    int n = 0;
    for (int k = 0; k < r.n_mm; ++k) {
        LH_WATCH(wd, *budget, LH_BREC_WD_LOOP, break)
        n += brec_declen(in.mm[2 * (r.mm_off + k)]) + brec_declen(in.mm[2 * (r.mm_off + k) + 1]) + 4;
    }
    return n;
}
__device__ __forceinline__ char brec_sa_op(uint32_t op, int is_split) { return (op == 3 && !is_split) ? 'H' : (op == 0 ? 'M' : op == 1 ? 'I' : op == 2 ? 'D' : 'S'); }

__global__ void __launch_bounds__(64) k_brec_plan(BrecIn in, BrecPlan* __restrict__ plan, int32_t* __restrict__ err, int32_t* wd) {
    const int pair = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pair >= in.n_pairs) return;
    const BrecRow* rows = in.row + (i64)pair * 2 * LH_BREC_SLOTS;
    int budget = 1 << 20;
    // the pair's set (ReadBarcodeSet's unit): the last one that begins at or before the pair
    int lo = 0, hi = in.n_sets - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (in.bc_pair_off[mid] <= pair) lo = mid; else hi = mid - 1; }
    const int attach_bx = in.n_sets > 0 && in.set_complete[lo] != 0;
    i64 ci[2 * LH_BREC_SLOTS];
    for (int k = 0; k < 2 * LH_BREC_SLOTS; ++k) ci[k] = rows[k].ci;
    uint32_t edited = 0;   // bit k: AppendBam has set row k's pos to -1 and its mapq to 0
#define EPOS(k) ((edited >> (k) & 1) ? (i64)-1 : rows[k].pos)
#define EMAPQ(k) ((edited >> (k) & 1) ? 0 : rows[k].mapq)
    const i64 name_len = in.name_off[pair + 1] - in.name_off[pair];
    for (int rec = 0; rec < 4; ++rec) {
        const int mate = rec >> 1, is_split = rec & 1;
        const int read = 2 * pair + mate;
        const int A = mate * LH_BREC_SLOTS + is_split, P = mate * LH_BREC_SLOTS, SB = P + 2, PM = P + 3;
        BrecPlan& pl = plan[(i64)pair * 4 + rec];
        if (ci[A] < 0) { pl.size = 0; pl.file = in.n_out; continue; }
        const BrecRow& a = rows[A];
        if (!a.is_proper && a.score - 17 < 19)
            for (int k = 0; k < 2 * LH_BREC_SLOTS; ++k) if (ci[k] == ci[A]) edited |= 1u << k;
        int flags = 0;
        int32_t mrid = -1;
        i64 mate_pos = -1, tlen = 0;
        if (ci[PM] >= 0) {
            const BrecRow& pm = rows[PM];
            const BrecRow& pr = rows[P];
            flags |= 1;
            if (a.is_proper) {
                if (!is_split) flags |= 0x2;
                else if (a.reversed != pm.reversed && a.rid == pm.rid) {   // isPair, on the edited positions
                    const i64 dist = a.reversed ? EPOS(A) - EPOS(PM) : EPOS(PM) - EPOS(A);
                    if (dist >= -35 && dist < 750) flags |= 0x2;
                }
            }
            const i64 pmpos = EPOS(PM);
            if (pmpos == -1 || (!pr.is_proper && pm.score - 17 < 19)) flags |= 0x8;
            else {
                if (pm.reversed) flags |= 0x20;
                mrid = (pm.rid >= 0 && pm.rid < in.n_contigs) ? pm.rid : -1;
                mate_pos = pmpos;
            }
            flags |= mate ? 0x80 : 0x40;
            if (a.duplicate) flags |= 0x400;
            if (pmpos == -1) mrid = -1;
            else if (!is_split && a.rid == pm.rid && (pr.is_proper || pm.score - 17 >= 19)) tlen = a.reversed ? -(a.aend - pmpos) : pm.aend - EPOS(A);
        }
        if (is_split) flags |= 256;
        int mq = EMAPQ(A) & 0xff;
        int32_t rid = (a.rid >= 0 && a.rid < in.n_contigs) ? a.rid : -1;
        const i64 pos = EPOS(A);
        if (pos == -1) { flags |= 0x4; mq = 0; rid = -1; }
        if (a.reversed) flags |= 0x10;
        // SEQ / QUAL and the hard clip of a split
        const i64 slen = in.seq_off[read + 1] - in.seq_off[read];
        const i64 qlen = mate ? in.qual2_off[pair + 1] - in.qual2_off[pair] : in.qual1_off[pair + 1] - in.qual1_off[pair];
        i64 start = 0, end = slen, qs = 0, qe = qlen, reflen = 0;
        uint32_t tags = 0;
        for (int k = 0; k < a.n_cig; ++k) {
            LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
            const uint32_t c = in.cig[a.cig_off + k];
            if ((c & 0xf) == 0 || (c & 0xf) == 2) reflen += c >> 4;
        }
        if (is_split) {
            if (a.n_cig >= 1 && (in.cig[a.cig_off] & 0xf) == 3) { start = in.cig[a.cig_off] >> 4; tags |= LH_BREC_T_CLIP0; }
            if (a.n_cig >= 2 && (in.cig[a.cig_off + a.n_cig - 1] & 0xf) == 3) { end -= in.cig[a.cig_off + a.n_cig - 1] >> 4; tags |= LH_BREC_T_CLIP1; }
            if (start > slen) start = slen;
            if (end > slen || end < start) end = start;
            qs = start < qlen ? start : qlen; qe = end < qlen ? end : qlen;
            if (qe < qs) qe = qs;
        }
        const i64 l_seq = end - start;
        if (qe - qs == l_seq) tags |= LH_BREC_T_QUAL;
        if (name_len > 254 || a.n_cig > 65535) { atomicOr(err, (int32_t)LH_BREC_E_FORMAT); atomicMin(err + 1, (int32_t)read); }
        // the tags: RX QX [TR TQ] [BC QT] [RG] XS XC AC AS XM AM XT [SA] [BX [DM]]
        i64 size = 36 + name_len + 1 + 4 * (i64)a.n_cig + (l_seq + 1) / 2 + l_seq;
        size += 4 + (in.rawbc_off[pair + 1] - in.rawbc_off[pair]) + 4 + (in.bcqual_off[pair + 1] - in.bcqual_off[pair]);
        if (!mate) { tags |= LH_BREC_T_TR; size += 2 * (4 + (in.trim_off[pair + 1] - in.trim_off[pair])); }
        if (in.si_off[pair + 1] - in.si_off[pair] > 1) { tags |= LH_BREC_T_BC; size += 4 + (in.si_off[pair + 1] - in.si_off[pair]) + 4 + (in.siqual_off[pair + 1] - in.siqual_off[pair]); }
        if (in.rgid_off[pair + 1] > in.rgid_off[pair]) { tags |= LH_BREC_T_RG; size += 4 + (in.rgid_off[pair + 1] - in.rgid_off[pair]); }
        const int has_sb = !is_split && ci[SB] >= 0;
        pl.xs = brec_f2i(in.rd[(i64)read * 4 + (is_split ? 2 : 0)]);
        pl.as = brec_f2i(in.rd[(i64)read * 4 + (is_split ? 3 : 1)]);
        pl.xc_len = has_sb ? brec_mm_len(in, rows[SB], wd, &budget) : 0;
        pl.ac_len = brec_mm_len(in, a, wd, &budget);
        if (has_sb) tags |= LH_BREC_T_XC;
        if (has_sb && rows[SB].active_mol) tags |= LH_BREC_T_XM;
        if (a.active_mol) tags |= LH_BREC_T_AM;
        pl.xt = (has_sb && a.mol_id == rows[SB].mol_id) ? 1 : 0;
        size += 7 + 4 + pl.xc_len + 4 + pl.ac_len + 7 + 5 + 5 + 7;
        // SA: the split as seen from the primary, or the primary as seen from the split
        const int O = is_split ? P : P + 1;
        pl.sa_len = 0; pl.sa_pos = 0; pl.sa_mapq = 0; pl.sa_nm = 0;
        if (ci[O] >= 0 && EPOS(O) > -1) {
            const BrecRow& o = rows[O];
            i64 indel = 0;
            int n = 0;
            for (int k = 0; k < o.n_cig; ++k) {
                LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
                const uint32_t c = in.cig[o.cig_off + k];
                if ((c & 0xf) == 1 || (c & 0xf) == 2) indel += c >> 4;
                n += brec_declen(c >> 4) + 1;
            }
            pl.sa_pos = EPOS(O); pl.sa_mapq = EMAPQ(O); pl.sa_nm = (int32_t)(o.n_mm + indel);
            if (o.rid >= 0 && o.rid < in.n_contigs) n += (int)(in.cname_off[o.rid + 1] - in.cname_off[o.rid]);
            n += 1 + brec_declen(pl.sa_pos) + 1 + 1 + 1 + 1 + brec_declen(pl.sa_mapq) + 1 + brec_declen((long long)o.n_mm + indel) + 1;
            pl.sa_len = n;
            tags |= LH_BREC_T_SA;
            size += 4 + n;
        }
        if (attach_bx) {
            int dash = 0;
            for (i64 k = in.bc_off[pair]; k < in.bc_off[pair + 1]; ++k) dash |= in.bc[k] == '-';
            if (dash) {
                tags |= LH_BREC_T_BX;
                size += 4 + (in.bc_off[pair + 1] - in.bc_off[pair]);
                if (a.active_mol) {
                    char b[24];
                    const int n = brec_f6(a.mol_diff, b);
                    if (!n) { atomicOr(err, (int32_t)LH_BREC_E_DM); atomicMin(err + 1, (int32_t)read); }
                    tags |= LH_BREC_T_DM;
                    size += 4 + n;
                }
            }
        }
        pl.size = (uint32_t)size;
        pl.rid = rid; pl.pos = (int32_t)pos; pl.mrid = mrid; pl.mpos = (int32_t)mate_pos; pl.tlen = (int32_t)tlen;
        const int bin = pos < 0 ? 4680 : brec_reg2bin(pos, pos + (reflen > 0 ? reflen : 1));
        pl.bin_mq_nl = (uint32_t)bin << 16 | (uint32_t)(mq & 0xff) << 8 | (uint32_t)((name_len + 1) & 0xff);
        pl.flag_nc = (uint32_t)flags << 16 | (uint32_t)(a.n_cig & 0xffff);
        pl.l_seq = (uint32_t)l_seq;
        pl.start = (int32_t)start; pl.qstart = (int32_t)qs;
        pl.tags = tags;
        // AppendBams: the unmapped file, or the contig's bucket of the position (the last one for a position past the contig's end)
        if (pos < 0 || rid < 0) pl.file = in.n_out - 1;
        else {
            const int nb = in.bucket_off[rid + 1] - in.bucket_off[rid];
            const i64 ch = pos / in.chunk;
            pl.file = in.bucket[in.bucket_off[rid] + (int)(ch < nb ? ch : nb - 1)];
        }
    }
#undef EPOS
#undef EMAPQ
}

// ------------------------------------------------------------------------------------------------ the offsets
// n slots: the sort's key (the file; a slot without a record sorts behind all files) and value, and the size for the scan in input order
__global__ void __launch_bounds__(256) k_brec_keys(const BrecPlan* __restrict__ plan, i64 n, uint32_t* __restrict__ key, uint32_t* __restrict__ val, i64* __restrict__ sz) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { sz[i] = 0; return; }   // (the scan's last element is then the total)
    key[i] = (uint32_t)plan[i].file; val[i] = (uint32_t)i; sz[i] = plan[i].size;
}
// the sizes in the sorted order
__global__ void __launch_bounds__(256) k_brec_sorted(const uint32_t* __restrict__ val, const i64* __restrict__ sz, i64 n, i64* __restrict__ ssz) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ssz[i] = sz[val[i]];
}
// a record's offset among the bucket files' records (file by file), and where every file's records end there (file_end: -1 where a file has none)
__global__ void __launch_bounds__(256) k_brec_place(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, const i64* __restrict__ ssz, const i64* __restrict__ sscan, i64 n,
                                                     int n_out, i64* __restrict__ off_file, i64* __restrict__ file_end) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    off_file[val[i]] = sscan[i];
    if ((int)key[i] < n_out && (i + 1 == n || key[i + 1] != key[i])) file_end[key[i]] = sscan[i] + ssz[i];
}

// ------------------------------------------------------------------------------------------------ the bytes
struct BrecDst { uint8_t* out; i64 d0, d1; };   // a record's two places: in bc_sorted and in its bucket file
__device__ __forceinline__ void brec_put(const BrecDst& d, i64 o, int b) { d.out[d.d0 + o] = (uint8_t)b; d.out[d.d1 + o] = (uint8_t)b; }
__device__ __forceinline__ void brec_put32(const BrecDst& d, i64 o, uint32_t v) { for (int k = 0; k < 4; ++k) brec_put(d, o + k, (int)(v >> (8 * k) & 0xff)); }
// a Z tag whose value lies in memory: 3 + n + 1 bytes at o
__device__ __forceinline__ i64 brec_tagz(const BrecDst& d, i64 o, int sub, char t0, char t1, const char* src, i64 n) {
    if (sub == 0) { brec_put(d, o, t0); brec_put(d, o + 1, t1); brec_put(d, o + 2, 'Z'); brec_put(d, o + 3 + n, 0); }
    for (i64 i = sub; i < n; i += 16) brec_put(d, o + 3 + i, src[i]);
    return o + 4 + n;
}
__device__ __forceinline__ i64 brec_tagi(const BrecDst& d, i64 o, int sub, char t0, char t1, int32_t v) {
    if (sub == 0) { brec_put(d, o, t0); brec_put(d, o + 1, t1); brec_put(d, o + 2, 'i'); brec_put32(d, o + 3, (uint32_t)v); }
    return o + 7;
}
__device__ __forceinline__ i64 brec_tagc(const BrecDst& d, i64 o, int sub, char t0, char t1, char c) {   // a Z tag of one character
    if (sub == 0) { brec_put(d, o, t0); brec_put(d, o + 1, t1); brec_put(d, o + 2, 'Z'); brec_put(d, o + 3, c); brec_put(d, o + 4, 0); }
    return o + 5;
}

__global__ void __launch_bounds__(64) k_brec_write(BrecIn in, const BrecPlan* __restrict__ plan, const i64* __restrict__ off_bc, const i64* __restrict__ off_file,
                                                    const i64* __restrict__ file_base, i64 bc_base, uint8_t* __restrict__ out, int32_t* wd) {
    const int pair = (int)blockIdx.x;   // a wave per pair, a 16-lane group per record
    const int rec = LANE() >> 4, sub = LANE() & 15;
    const int mate = rec >> 1, is_split = rec & 1;
    const int read = 2 * pair + mate;
    const i64 slot = (i64)pair * 4 + rec;
    const BrecPlan pl = plan[slot];
    const int present = pl.size != 0;
    const BrecRow* rows = in.row + (i64)pair * 2 * LH_BREC_SLOTS;
    const BrecRow& a = rows[mate * LH_BREC_SLOTS + is_split];
    const BrecRow& sb = rows[mate * LH_BREC_SLOTS + 2];
    BrecDst d;
    d.out = out; d.d0 = 0; d.d1 = 0;
    i64 o = 0, xc_at = 0, ac_at = 0;
    if (present) {
        d.d0 = bc_base + off_bc[slot]; d.d1 = file_base[pl.file] + off_file[slot];
        // the 36 fixed bytes
        if (sub < 9) {
            const uint32_t w = sub == 0 ? pl.size - 4 : sub == 1 ? (uint32_t)pl.rid : sub == 2 ? (uint32_t)pl.pos : sub == 3 ? pl.bin_mq_nl : sub == 4 ? pl.flag_nc : sub == 5 ? pl.l_seq
                             : sub == 6 ? (uint32_t)pl.mrid : sub == 7 ? (uint32_t)pl.mpos : (uint32_t)pl.tlen;
            brec_put32(d, 4 * sub, w);
        }
        o = 36;
        const i64 nl = in.name_off[pair + 1] - in.name_off[pair];
        for (i64 i = sub; i <= nl; i += 16) brec_put(d, o + i, i < nl ? in.name[in.name_off[pair] + i] : 0);
        o += nl + 1;
        // CIGAR: lariat's operations M I D S H are BAM's 0 1 2 4 5; a split's outer soft clips become hard clips
        for (int k = sub; k < a.n_cig; k += 16) {
            const uint32_t c = in.cig[a.cig_off + k];
            uint32_t op = c & 0xf;
            op = op > 4 ? 5 : op >= 3 ? op + 1 : op;
            if ((k == 0 && (pl.tags & LH_BREC_T_CLIP0)) || (k == a.n_cig - 1 && (pl.tags & LH_BREC_T_CLIP1))) op = 5;
            brec_put32(d, o + 4 * (i64)k, (c >> 4) << 4 | op);
        }
        o += 4 * (i64)a.n_cig;
        // SEQ: base j of the record is base start + j of the read in the alignment's orientation
        const uint8_t* sq = in.seq + in.seq_off[read];
        const i64 slen = in.seq_off[read + 1] - in.seq_off[read];
        const i64 l_seq = pl.l_seq;
        for (i64 j = sub; j < (l_seq + 1) / 2; j += 16) {
            int byte = 0;
            for (int h = 0; h < 2; ++h) {
                const i64 i = pl.start + 2 * j + h;
                int nyb = 0;
                if (2 * j + h < l_seq) {
                    int c = a.reversed ? sq[slen - 1 - i] : sq[i];
                    if (c > 3) nyb = 15;
                    else { if (a.reversed) c = 3 - c; nyb = 1 << c; }
                }
                byte = byte << 4 | nyb;
            }
            brec_put(d, o + j, byte);
        }
        o += (l_seq + 1) / 2;
        const char* ql = mate ? in.qual2 + in.qual2_off[pair] : in.qual1 + in.qual1_off[pair];
        const i64 qlen = mate ? in.qual2_off[pair + 1] - in.qual2_off[pair] : in.qual1_off[pair + 1] - in.qual1_off[pair];
        for (i64 j = sub; j < l_seq; j += 16) {
            const i64 i = pl.qstart + j;
            brec_put(d, o + j, (pl.tags & LH_BREC_T_QUAL) ? (int)(uint8_t)((a.reversed ? ql[qlen - 1 - i] : ql[i]) - 33) : 0xff);
        }
        o += l_seq;
        o = brec_tagz(d, o, sub, 'R', 'X', in.rawbc + in.rawbc_off[pair], in.rawbc_off[pair + 1] - in.rawbc_off[pair]);
        o = brec_tagz(d, o, sub, 'Q', 'X', in.bcqual + in.bcqual_off[pair], in.bcqual_off[pair + 1] - in.bcqual_off[pair]);
        if (pl.tags & LH_BREC_T_TR) {
            o = brec_tagz(d, o, sub, 'T', 'R', in.trim_bases + in.trim_off[pair], in.trim_off[pair + 1] - in.trim_off[pair]);
            o = brec_tagz(d, o, sub, 'T', 'Q', in.trim_quals + in.trim_off[pair], in.trim_off[pair + 1] - in.trim_off[pair]);
        }
        if (pl.tags & LH_BREC_T_BC) {
            o = brec_tagz(d, o, sub, 'B', 'C', in.si + in.si_off[pair], in.si_off[pair + 1] - in.si_off[pair]);
            o = brec_tagz(d, o, sub, 'Q', 'T', in.siqual + in.siqual_off[pair], in.siqual_off[pair + 1] - in.siqual_off[pair]);
        }
        if (pl.tags & LH_BREC_T_RG) o = brec_tagz(d, o, sub, 'R', 'G', in.rgid + in.rgid_off[pair], in.rgid_off[pair + 1] - in.rgid_off[pair]);
        o = brec_tagi(d, o, sub, 'X', 'S', pl.xs);
        if (sub == 0) { brec_put(d, o, 'X'); brec_put(d, o + 1, 'C'); brec_put(d, o + 2, 'Z'); brec_put(d, o + 3 + pl.xc_len, 0); }
        xc_at = o + 3;
        o += 4 + pl.xc_len;
        if (sub == 0) { brec_put(d, o, 'A'); brec_put(d, o + 1, 'C'); brec_put(d, o + 2, 'Z'); brec_put(d, o + 3 + pl.ac_len, 0); }
        ac_at = o + 3;
        o += 4 + pl.ac_len;
        o = brec_tagi(d, o, sub, 'A', 'S', pl.as);
        o = brec_tagc(d, o, sub, 'X', 'M', (pl.tags & LH_BREC_T_XM) ? '1' : '0');
        o = brec_tagc(d, o, sub, 'A', 'M', (pl.tags & LH_BREC_T_AM) ? '1' : '0');
        o = brec_tagi(d, o, sub, 'X', 'T', pl.xt);
        if (pl.tags & LH_BREC_T_SA) {
            if (sub == 0) {   // one lane renders it
                const BrecRow& ot = rows[mate * LH_BREC_SLOTS + (is_split ? 0 : 1)];
                i64 p = o;
                char b[24];
                brec_put(d, p++, 'S'); brec_put(d, p++, 'A'); brec_put(d, p++, 'Z');
                if (ot.rid >= 0 && ot.rid < in.n_contigs) for (i64 k = in.cname_off[ot.rid]; k < in.cname_off[ot.rid + 1]; ++k) brec_put(d, p++, in.cname[k]);
                brec_put(d, p++, ',');
                int n = brec_dec(b, pl.sa_pos);
                for (int k = 0; k < n; ++k) brec_put(d, p++, b[k]);
                brec_put(d, p++, ','); brec_put(d, p++, ot.reversed ? '-' : '+'); brec_put(d, p++, ',');
                int budget = 1 << 20;
                for (int k = 0; k < ot.n_cig; ++k) {
                    LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
                    const uint32_t c = in.cig[ot.cig_off + (ot.reversed ? ot.n_cig - 1 - k : k)];
                    n = brec_dec(b, c >> 4);
                    for (int q = 0; q < n; ++q) brec_put(d, p++, b[q]);
                    brec_put(d, p++, brec_sa_op(c & 0xf, is_split));
                }
                brec_put(d, p++, ',');
                n = brec_dec(b, pl.sa_mapq);
                for (int k = 0; k < n; ++k) brec_put(d, p++, b[k]);
                brec_put(d, p++, ',');
                n = brec_dec(b, pl.sa_nm);
                for (int k = 0; k < n; ++k) brec_put(d, p++, b[k]);
                brec_put(d, p++, ';'); brec_put(d, p++, 0);
            }
            o += 4 + pl.sa_len;
        }
        if (pl.tags & LH_BREC_T_BX) o = brec_tagz(d, o, sub, 'B', 'X', in.bc + in.bc_off[pair], in.bc_off[pair + 1] - in.bc_off[pair]);
        if ((pl.tags & LH_BREC_T_DM) && sub == 0) {
            char b[24];
            const int n = brec_f6(a.mol_diff, b);
            brec_put(d, o, 'D'); brec_put(d, o + 1, 'M'); brec_put(d, o + 2, 'Z');
            for (int k = 0; k < n; ++k) brec_put(d, o + 3 + k, b[k]);
            brec_put(d, o + 3 + n, 0);
        }
    }
    // XC and AC, "ref,read,1;" per locus: a lane renders one locus at the offset a prefix sum over the group's lanes gives.  The whole wave runs the same number of
    // rounds (the scan is a cross-lane operation), groups with fewer loci render nothing in the later ones
    for (int list = 0; list < 2; ++list) {
        const BrecRow& r = list ? a : sb;
        const int n_loc = !present ? 0 : list ? a.n_mm : ((pl.tags & LH_BREC_T_XC) ? sb.n_mm : 0);
        const int rounds = wave_max_i32((n_loc + 15) >> 4);
        i64 at = list ? ac_at : xc_at;
        int budget = 1 << 16;
        for (int t = 0; t < rounds; ++t) {
            LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
            const int k = t * 16 + sub;
            char b[28];
            int n = 0;
            if (k < n_loc) {
                n = brec_dec(b, in.mm[2 * (r.mm_off + k)]);
                b[n++] = ',';
                n += brec_dec(b + n, in.mm[2 * (r.mm_off + k) + 1]);
                b[n++] = ','; b[n++] = '1'; b[n++] = ';';
            }
            const int incl = row_scan_add_i32(n);
            const int total = __shfl(incl, (LANE() & ~15) | 15);
            for (int q = 0; q < n; ++q) brec_put(d, at + incl - n + q, b[q]);
            at += total;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the gather from a resident result
// brec_gather (lh_brec.inc) on the device: the stage buffer's rows, doubles, packed CIGARs and packed loci come out as the host's gather and upload leave them, read
// by read and slot by slot.  The kernels read one pipeline's DCand / DInf and write the encoder's buffers alone.
struct BrecSrc {   // one pipeline's part of the batch
    int32_t n_reads;   // of the part
    i64 read0;         // its first read in the batch
    i64 n_cand;        // cand_off[n_reads]: every index below is -1 or smaller than this
    DCand R; DInf S;
};
// the candidates read r's records read (-1: none): the active alignment, its split, the second best, the active's mate.  An index outside the result counts as none
__device__ __forceinline__ void brec_slots(const BrecSrc& s, int r, i64* idx, int32_t* __restrict__ err) {
    idx[0] = s.S.active_idx[r]; idx[1] = s.S.split_idx[r]; idx[2] = s.S.second_best_idx[r];
    for (int k = 0; k < 3; ++k) if (idx[k] < -1 || idx[k] >= s.n_cand) { idx[k] = -1; atomicOr(err, (int32_t)LH_BREC_E_INDEX); }
    idx[3] = idx[0] >= 0 ? s.S.mate[idx[0]] : -1;
    if (idx[3] < -1 || idx[3] >= s.n_cand) { idx[3] = -1; atomicOr(err, (int32_t)LH_BREC_E_INDEX); }
}
__device__ __forceinline__ int brec_n_cig(const BrecSrc& s, i64 a) {   // (a count over the slots has raised LH_ST_CIGAR_OVERFLOW: such a result is refused before)
    const int n = s.R.n_cigar[a];
    return n < 0 ? 0 : n > LH_MAX_CIGAR ? LH_MAX_CIGAR : n;
}
__device__ __forceinline__ int brec_n_mm(const BrecSrc& s, i64 a, int32_t* __restrict__ err) {   // loci past the slots continue in the pool: all of them inside it
    const int n = s.R.n_mm[a];
    if (n <= LH_MAX_MM) return n < 0 ? 0 : n;
    const i64 xo = s.R.mm_xoff[a];
    if (xo < 0 || xo + (n - LH_MAX_MM) > (i64)s.R.mm_xcap) { atomicOr(err, (int32_t)LH_BREC_E_INDEX); return LH_MAX_MM; }
    return n;
}

// a lane per read: its CIGAR operations (slots 0 and 1) and mismatch loci (slots 0 to 2) at its place in the batch; the host path's "a read has no active alignment"
__global__ void __launch_bounds__(256) k_brec_gather_count(BrecSrc s, i64* __restrict__ n_cig, i64* __restrict__ n_mm, int32_t* __restrict__ err) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= s.n_reads) return;
    i64 idx[LH_BREC_SLOTS];
    brec_slots(s, r, idx, err);
    if (idx[0] < 0) { atomicOr(err, (int32_t)LH_BREC_E_NOACTIVE); atomicMin(err + 1, (int32_t)(s.read0 + r)); }
    i64 nc = 0, nm = 0;
    for (int k = 0; k < 3; ++k) {
        if (idx[k] < 0) continue;
        if (k < 2) nc += brec_n_cig(s, idx[k]);
        nm += brec_n_mm(s, idx[k], err);
    }
    n_cig[s.read0 + r] = nc; n_mm[s.read0 + r] = nm;
}

// a 16-lane group per read.  Lanes 0 to 3 write the four rows (brec_gather_row: a whole row zeroed, ci, then the fields), lanes 4 to 7 the four doubles; then the group
// strides the read's lists.  The rows are of fixed width and the lists short (a handful of entries in the mean, 64 and the pool at most), so a read keeps a quarter
// of a wave busy where a wave per read would idle three quarters of it, and the group's stores to a list are consecutive words.
__global__ void __launch_bounds__(256) k_brec_gather_fill(BrecSrc s, const i64* __restrict__ cig_at, const i64* __restrict__ mm_at, BrecRow* __restrict__ row, double* __restrict__ rd,
                                                          uint32_t* __restrict__ cig, int32_t* __restrict__ mm, int32_t* __restrict__ err, int32_t* wd) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = (int)(t >> 4), sub = (int)(t & 15);
    if (r >= s.n_reads) return;
    const i64 read = s.read0 + r;
    i64 idx[LH_BREC_SLOTS];
    brec_slots(s, r, idx, err);
    int nc[2], nm[3];
    for (int k = 0; k < 3; ++k) {
        if (k < 2) nc[k] = idx[k] < 0 ? 0 : brec_n_cig(s, idx[k]);
        nm[k] = idx[k] < 0 ? 0 : brec_n_mm(s, idx[k], err);
    }
    const i64 c0 = cig_at[read], m0 = mm_at[read];
    if (sub < LH_BREC_SLOTS) {
        const i64 a = idx[sub];
        BrecRow o;
        __builtin_memset(&o, 0, sizeof o);
        o.ci = a;
        if (a >= 0) {
            o.pos = s.R.pos[a]; o.aend = s.R.aend[a]; o.rid = s.R.rid[a]; o.score = s.R.score[a]; o.mapq = s.S.mapq[a]; o.mol_id = s.S.molecule_id[a];
            o.mol_diff = s.S.mol_diff[a];
            o.reversed = s.R.reversed[a]; o.is_proper = s.S.is_proper[a]; o.duplicate = s.S.duplicate[a]; o.active_mol = s.S.active_molecule[a];
            if (sub < 2) { o.cig_off = c0 + (sub ? nc[0] : 0); o.n_cig = nc[sub]; }
            if (sub < 3) { o.mm_off = m0 + (sub > 0 ? nm[0] : 0) + (sub > 1 ? nm[1] : 0); o.n_mm = nm[sub]; }
        }
        row[read * LH_BREC_SLOTS + sub] = o;
    } else if (sub < 8) {
        const double* __restrict__ src = sub == 4 ? s.S.second_best_score : sub == 5 ? s.S.as_score : sub == 6 ? s.S.split_second_best : s.S.split_score;
        rd[read * 4 + (sub - 4)] = src[r];
    }
    int budget = 1 << 12;   // (a list is at most a read's bases long, a sixteenth of it per lane)
    i64 c_at = c0, m_at = m0;
    for (int k = 0; k < 3; ++k) {
        const i64 a = idx[k];
        if (a < 0) continue;
        if (k < 2) {
            const uint32_t* __restrict__ src = s.R.cigar + a * LH_MAX_CIGAR;
            for (int j = sub; j < nc[k]; j += 16) {
                LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
                cig[c_at + j] = src[j];
            }
            c_at += nc[k];
        }
        const int32_t* __restrict__ ref = s.R.mm_ref + a * LH_MAX_MM;
        const int32_t* __restrict__ rdl = s.R.mm_read + a * LH_MAX_MM;
        const i64 xo = nm[k] > LH_MAX_MM ? (i64)s.R.mm_xoff[a] - LH_MAX_MM : 0;   // locus j >= LH_MAX_MM is entry mm_xoff[a] + j - LH_MAX_MM of the pool (k_pack_slots)
        for (int j = sub; j < nm[k]; j += 16) {
            LH_WATCH(wd, budget, LH_BREC_WD_LOOP, break)
            mm[2 * (m_at + j)] = j < LH_MAX_MM ? ref[j] : s.R.mm_xref[xo + j];
            mm[2 * (m_at + j) + 1] = j < LH_MAX_MM ? rdl[j] : s.R.mm_xread[xo + j];
        }
        m_at += nm[k];
    }
}
