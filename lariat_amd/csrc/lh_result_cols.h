// lh_result_cols.h — the array columns of lh_result (include/lariat_hip.h), described ONCE: what the host code that produces a result needs to
// know about a column.  The device arrays' allocation (alloc_cand_pools, rfa_alloc), the download (pipe_download_begin: layout of the pinned
// block, device-to-host copies, values of a run without inference, pointers handed out) and the merge of two lanes' results (merge_results) are
// loops over LH_RESULT_COLS.  A column added to lh_result and not entered here fails the static_assert at the end of this file.
// Host side only: kernels take DCand / DInf by value and never see the table.
#pragma once
#include <stddef.h>
#include <string.h>
#include <type_traits>
#include "../../include/lariat_hip.h"
#include "k_rfa.h"   // DCand (k_aln.h), DInf

enum ColLen : uint8_t {   // what a column's length follows
    PER_CAND,        // n_cand
    PER_READ,        // n_reads
    PER_READ_1,      // n_reads + 1
    PER_CAND_1,      // n_cand + 1
    PER_CIGAR_OP,    // cigar_off[n_cand]
    PER_MM_LOCUS     // mm_off[n_cand]
};
enum ColSrc : uint8_t {   // where it is on the device
    FROM_CAND,         // member of DCand at dev_off
    FROM_INF,          // member of DInf at dev_off: written by the inference only, `dflt` is its value in a result without inference
    FROM_CIGAR_OFF, FROM_MM_OFF,              // lh_context::d_cigar_off, d_mm_off (scans of DCand::n_cigar, n_mm at download time)
    FROM_PACK_A, FROM_PACK_B, FROM_PACK_C     // lh_context::d_pack_a, b, c (k_pack_slots: cigar, mm_read, mm_ref without the unused slots)
};
enum ColMerge : uint8_t {   // the second lane's values behind the first lane's
    MERGE_COPY,        // as they are
    MERGE_SHIFT,       // candidate indices: + the first lane's n_cand where >= 0 (-1 = none stays)
    MERGE_CONTINUE     // offset arrays: entries 1.. of the second lane + the first lane's last entry, which replaces its entry 0
};
struct ResultCol {
    uint16_t res_off;        // offsetof(lh_result, member)
    uint8_t elt, dev_elt;    // element size in lh_result / on the device (the same: checked below)
    bool fp;                 // double (else an integer of elt bytes)
    ColLen len;
    ColSrc src;
    uint16_t dev_off;        // offsetof(DCand / DInf, member)
    double dflt;
    ColMerge merge;
};

#define LH_COL(f, dev_elt, len, src, dev_off, dflt, merge) \
    {offsetof(lh_result, f), sizeof(*lh_result::f), dev_elt, std::is_same<decltype(lh_result::f), const double*>::value, len, src, dev_off, dflt, merge}
// a member of DCand; a member of DInf with its Alignment default (lariat.go:1655-1689); a buffer of the context
#define COL_R(f, len, m, merge) LH_COL(f, sizeof(*DCand::m), len, FROM_CAND, offsetof(DCand, m), 0, merge)
#define COL_S(f, len, m, dflt, merge) LH_COL(f, sizeof(*DInf::m), len, FROM_INF, offsetof(DInf, m), dflt, merge)
#define COL_X(f, len, src, merge) LH_COL(f, sizeof(*lh_result::f), len, src, 0, 0, merge)
static constexpr ResultCol LH_RESULT_COLS[] = {
    COL_R(cand_off, PER_READ_1, cand_off, MERGE_CONTINUE),
    COL_R(rid, PER_CAND, rid, MERGE_COPY),
    COL_R(pos, PER_CAND, pos, MERGE_COPY),
    COL_R(aend, PER_CAND, aend, MERGE_COPY),
    COL_R(rb, PER_CAND, rb, MERGE_COPY),
    COL_R(re, PER_CAND, re, MERGE_COPY),
    COL_R(reversed, PER_CAND, reversed, MERGE_COPY),
    COL_R(score, PER_CAND, score, MERGE_COPY),
    COL_R(qb, PER_CAND, qb, MERGE_COPY),
    COL_R(qe, PER_CAND, qe, MERGE_COPY),
    COL_R(nm, PER_CAND, nm, MERGE_COPY),
    COL_R(matches, PER_CAND, matches, MERGE_COPY),
    COL_R(mismatches, PER_CAND, mismatches, MERGE_COPY),
    COL_R(indels, PER_CAND, indels, MERGE_COPY),
    COL_R(soft_clipped, PER_CAND, soft_clipped, MERGE_COPY),
    COL_R(soft_clipped_length, PER_CAND, soft_clipped_length, MERGE_COPY),
    COL_R(in_filtered, PER_CAND, in_filtered, MERGE_COPY),
    COL_X(cigar_off, PER_CAND_1, FROM_CIGAR_OFF, MERGE_CONTINUE),
    COL_X(cigar, PER_CIGAR_OP, FROM_PACK_A, MERGE_COPY),
    COL_X(mm_off, PER_CAND_1, FROM_MM_OFF, MERGE_CONTINUE),
    COL_X(mm_ref_loc, PER_MM_LOCUS, FROM_PACK_C, MERGE_COPY),
    COL_X(mm_read_loc, PER_MM_LOCUS, FROM_PACK_B, MERGE_COPY),
    COL_R(log_alignment_probability, PER_CAND, lap, MERGE_COPY),
    COL_S(active, PER_CAND, active, 0, MERGE_COPY),
    COL_S(is_proper, PER_CAND, is_proper, 0, MERGE_COPY),
    COL_S(bwa_pick, PER_CAND, bwa_pick, 0, MERGE_COPY),
    COL_S(active_molecule, PER_CAND, active_molecule, 0, MERGE_COPY),
    COL_S(duplicate, PER_CAND, duplicate, 0, MERGE_COPY),
    COL_S(molecule_id, PER_CAND, molecule_id, -1, MERGE_COPY),
    COL_S(mapq, PER_CAND, mapq, 0, MERGE_COPY),
    COL_S(molecule_difference, PER_CAND, mol_diff, 0, MERGE_COPY),
    COL_S(molecule_confidence, PER_CAND, mol_conf, 0.00075 * 0.025, MERGE_COPY),
    COL_S(sum_move_probability_change, PER_CAND, sum_move, 1.0, MERGE_COPY),
    COL_S(mate_idx, PER_CAND, mate, -1, MERGE_SHIFT),
    COL_S(active_idx, PER_READ, active_idx, -1, MERGE_SHIFT),
    COL_S(second_best_idx, PER_READ, second_best_idx, -1, MERGE_SHIFT),
    COL_S(second_best_score, PER_READ, second_best_score, 0, MERGE_COPY),
    COL_S(as_score, PER_READ, as_score, 0, MERGE_COPY),
    COL_S(split_idx, PER_READ, split_idx, -1, MERGE_SHIFT),
    COL_S(split_mapq, PER_READ, split_mapq, 0, MERGE_COPY),
    COL_S(split_second_best, PER_READ, split_second_best, 0, MERGE_COPY),
    COL_S(split_score, PER_READ, split_score, 0, MERGE_COPY),
};
#undef LH_COL
#undef COL_R
#undef COL_S
#undef COL_X
constexpr size_t LH_N_COLS = sizeof LH_RESULT_COLS / sizeof LH_RESULT_COLS[0];

// every pointer member of lh_result from cand_off (behind n_cand) to split_score (before the counters) is described exactly once, with the device
// array's element size; shifted and continued columns are 64-bit integers
constexpr bool result_cols_ok() {
    constexpr size_t first = offsetof(lh_result, cand_off), last = offsetof(lh_result, split_score);
    if (first != offsetof(lh_result, n_cand) + sizeof(int64_t) || last + sizeof(void*) != offsetof(lh_result, n_ext)) return false;
    if (LH_N_COLS != (last - first) / sizeof(void*) + 1) return false;
    for (size_t slot = first; slot <= last; slot += sizeof(void*)) {
        int n = 0;
        for (const ResultCol& k : LH_RESULT_COLS) n += k.res_off == slot;
        if (n != 1) return false;
    }
    for (const ResultCol& k : LH_RESULT_COLS) {
        if (k.elt != k.dev_elt || (k.elt != 1 && k.elt != 4 && k.elt != 8) || (k.fp && k.elt != 8)) return false;
        if (k.merge != MERGE_COPY && (k.elt != 8 || k.fp)) return false;
        if ((k.merge == MERGE_CONTINUE) != (k.len == PER_READ_1 || k.len == PER_CAND_1)) return false;
    }
    return true;
}
static_assert(result_cols_ok(), "LH_RESULT_COLS does not match lh_result's array columns (include/lariat_hip.h) or the device arrays' element types");

// the 19 work counters: DCounters (lh_dev.h) lists them in the order of lh_result's counter block, n_ext_exec[3] / n_ktree[3] standing for _p1 .. _p3
constexpr size_t LH_N_CTRS = sizeof(DCounters) / sizeof(uint64_t);
static_assert(LH_N_CTRS == 19 && offsetof(DCounters, n_ext) == 0 && offsetof(DCounters, n_glob_exec) == (LH_N_CTRS - 1) * sizeof(uint64_t), "DCounters: 19 u64, n_ext first, n_glob_exec last");
static_assert(offsetof(lh_result, n_glob_exec) - offsetof(lh_result, n_ext) == offsetof(DCounters, n_glob_exec) && offsetof(lh_result, arena_) - offsetof(lh_result, n_ext) == sizeof(DCounters) &&
                  offsetof(lh_result, n_calls_by_text) - offsetof(lh_result, n_ext) == offsetof(DCounters, n_bt),
              "lh_result's counter block: the same 19 u64, n_ext first, n_glob_exec last");
static inline uint64_t* result_ctrs(lh_result* r) { return (uint64_t*)((char*)r + offsetof(lh_result, n_ext)); }

// a column's number of elements in a result of these sizes
static inline size_t col_count(const ResultCol& k, size_t n_reads, size_t n_cand, size_t n_cigar, size_t n_mm) {
    switch (k.len) {
    case PER_CAND: return n_cand;
    case PER_READ: return n_reads;
    case PER_READ_1: return n_reads + 1;
    case PER_CAND_1: return n_cand + 1;
    case PER_CIGAR_OP: return n_cigar;
    default: return n_mm;
    }
}
// the pointer members of lh_result, DCand and DInf have different types: they are read and written as bytes
static inline void* ptr_at(const void* base, size_t off) { void* p; memcpy(&p, (const char*)base + off, sizeof p); return p; }
static inline void set_ptr_at(void* base, size_t off, const void* p) { memcpy((char*)base + off, &p, sizeof p); }
