// lh_workspace.h — the device workspace of a pipeline (struct lh_context, lh_host.inc), described ONCE: who owns a buffer (DevGroup), what the
// words of a counter block mean, and where the sections of a buffer that several kernels share begin.  Host side only: kernels take the
// pointers the launches derive from these definitions and never see them.  Included by lh_host.inc after the kernel headers and set_err.
#pragma once
#include <stddef.h>
#include <vector>

template <class T> static int dalloc(T** p, size_t n) {
    hipError_t e = hipMalloc((void**)p, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return set_err(LH_E_HIP, std::string("hipMalloc of ") + std::to_string((n ? n : 1) * sizeof(T)) + " bytes: " + hipGetErrorString(e)); }
    return LH_OK;
}

// The device buffers of one lifetime.  A group remembers the ADDRESSES of the pointer variables it allocated into — members of lh_context, of
// DCand / DInf (kernel arguments: they stay plain structs), of a batch slot, or locals — so release() frees each buffer and leaves its pointer
// null: a buffer is never freed twice, and swapping two pointers moves their buffers between the groups that own the variables.  A capacity that
// describes a group's buffers is reset next to release() and set again when every allocation of the regrow has succeeded.
struct DevGroup {
    std::vector<void**> held;
    DevGroup() = default;
    DevGroup(const DevGroup&) = delete;
    DevGroup& operator=(const DevGroup&) = delete;
    ~DevGroup() { release(); }
    // n elements (at least one), p owned by this group from now on.  A group's buffers exist together or not at all: if this allocation fails, the group is released
    template <class T> int alloc(T*& p, size_t n) {
        int rc = dalloc(&p, n);
        if (rc) release(); else held.push_back((void**)&p);
        return rc;
    }
    void release() { for (void** q : held) { hipFree(*q); *q = nullptr; } held.clear(); }
    // for a thread that must not call hipFree (it waits for the whole device): the buffers go to a list that another thread frees
    void release_to(std::vector<void*>& later) { for (void** q : held) { if (*q) later.push_back(*q); *q = nullptr; } held.clear(); }
};
#define DALLOC(g, p, n) do { int rc_ = (g).alloc(p, (size_t)(n)); if (rc_) return rc_; } while (0)

// ------------------------------------------------------------------------------------------------ a batch on the device
// What the kernel sequence reads of its input: the arrays of lh_batch and their sizes.  One value: a slot holds one for its own buffers (lh_context::DevBatch), the
// context holds the selected one (lh_context::b: a slot's, or a round's part of it, lh_host.inc: part_view), and whatever saves, restores or replaces the selection
// copies all of it.  It owns nothing: the arrays belong to a slot's DevGroup or to the rounds' (RoundBufs)
struct BatchView {
    uint8_t* seq = nullptr; i64* seq_off = nullptr;   // the reads' bases, a byte each, and where each read begins [n_reads + 1]
    u64* name_seed = nullptr;                         // per pair
    int32_t* bc_pair_off = nullptr; uint8_t* bc_do_rfa = nullptr;   // per barcode: its first pair [n_bc + 1]; run the inference for it?
    i64 *cen_start = nullptr, *cen_end = nullptr;     // per contig of the index: the centromere's interval (-1: none)
    int n_pairs = 0, n_reads = 0, n_bc = 0; bool has_cen = false; i64 n_bases = 0;
    int max_len = LH_MAXLEN;   // the longest read (K1 stages its queries in that many bases' worth of LDS)
};

// ------------------------------------------------------------------------------------------------ counter blocks (device)
// K1's work counters: cleared as a whole when K1 starts, big_pass again before every second-chance round
struct K1Counters {
    int32_t pass[3];       // the three passes' read counters (k_smem_pass: the next read a lane takes)
    int32_t big_pass[3];   // the same for the second chance (k1_big_round)
    int32_t n_todo;        // reads k_smem_first left to pass 1: the length of lh_context::d_k1_todo
    int32_t n_p2_tasks;    // pass 2's list (k_p2_probe, k_p2_tasks): the length of lh_context::d_p2_tasks
    int32_t n_fin;         // reads k_smem_p3_lock lists for k_smem_fin: the length of lh_context::d_fin_list
};
static_assert(sizeof(K1Counters) == 9 * sizeof(int32_t) && offsetof(K1Counters, big_pass) == 3 * sizeof(int32_t) && sizeof(K1Counters::big_pass) == 3 * sizeof(int32_t),
              "the second chance's counters are cleared as one range");
// k_big_collect addresses these two as count[0] and count[1]
struct K1BigCounts {
    int32_t listed;   // reads given a slot of the big slab in this round: the length of lh_context::d_big_list
    int32_t asked;    // reads that asked for one
};
static_assert(offsetof(K1BigCounts, listed) == 0 && offsetof(K1BigCounts, asked) == sizeof(int32_t) && sizeof(K1BigCounts) == 2 * sizeof(int32_t), "k_big_collect: count[0], count[1]");
// the lengths of the candidate lists K7's kernels hand each other in lh_context::d_aln_r / d_aln_ci and the region scratch (RegsTmpLists).  The lists are shared
// with K3, K5 and K6, which run earlier, and so are two of the counters: the ones a stage uses are cleared when it starts
struct AlnCounts {
    int32_t flat;    // candidates listed by k_aln_flat (k_aln_flat2's input).  After K7: the OR of the status words (k_status_or)
    int32_t grp16;   // what k_aln_flat2 lists for k_aln_grp<16>
    int32_t grp32;   // candidates listed for k_aln_grp<32>
    int32_t full;    // candidates listed for k_aln.  Before K7: the reads k_chain_cl leaves to k_chain
};
static_assert(offsetof(AlnCounts, flat) == 0 && sizeof(AlnCounts) == 4 * sizeof(int32_t), "K7 clears all four, the download the first");
// K8's work counters and overflow counts: cleared as a whole when K8 starts
struct RfaCounters {
    int32_t next;             // work counter of k_rfa's first launch
    int32_t n_ovf;            // barcodes it turned away: the length of lh_context::d_rfa_ovf
    int32_t last_next;        // work counter of k_rfa's last launch (the large slabs)
    int32_t heavy_pairs;      // pairs k_rfa_tag leaves to k_rfa_tag_w: the length of lh_context::d_rfa_hp
    int32_t heavy_reads;      // reads k_rfa leaves to k_rfa_mq_w: the length of lh_context::d_rfa_hr
    int32_t post_next;        // work counter of k_rfa_post's first launch
    int32_t post_n_ovf;       // barcodes it turned away: the length of lh_context::d_rfa_ovf2
    int32_t post_last_next;   // work counter of k_rfa_post's last launch
    struct Tier {             // tier k's launches (RfaOvfMid holds the lists)
        int32_t next, n_ovf;             // k_rfa: work counter, barcodes turned away
        int32_t post_next, post_n_ovf;   // k_rfa_post: the same
    } tier[2];
    int32_t routed_next;      // work counter of the first tier's launch for the barcodes routed there up front (its overflow: tier[0].n_ovf)
    int32_t small_next;       // work counter of the small instance's launch
    int32_t unused[6];
};
static_assert(sizeof(RfaCounters) == 24 * sizeof(int32_t) && offsetof(RfaCounters, tier) == 8 * sizeof(int32_t) && offsetof(RfaCounters, routed_next) == 16 * sizeof(int32_t), "RfaCounters");

// ------------------------------------------------------------------------------------------------ small read-backs (pinned host memory)
// Written by one-thread kernels (k_peek_*, k_resc_offsets), not by copy-engine transfers: those may be busy with the previous result or the next batch.  The host
// reads a value after it has synchronised the stream the kernel ran on.
struct HostPeek {
    struct K1 { i64 seeds, big_asked, p2_drop_probed, p2_unprobed_shares; };
    struct K6 { i64 total, padded, listed, n_long; };
    union {   // the read-back of the moment; every one is consumed before the next is launched
        i64 one;   // k_peek_i32 / k_peek_i64: K4's queued jobs (ext_long_queue), the batch's candidates (stage2_run)
        K1 k1;     // k_peek_k1 (run_front): the batch's seeds; the reads that asked for a slot of the big slab; pass 2's call counts, two to a word (k_smem4.h)
        K6 k6;     // k_resc_offsets (rescue_dir): jobs; their order array's padded length; listed pairs; those with long lists
    };
    // the one value that outlives a batch.  Written by stage2_run's last k_peek_i32 on the auxiliary stream (joined before the batch ends) and by nothing else;
    // read by the NEXT batch's run_front (pass 2 as tasks?) and stage2_run (long queue?) while lh_context::ext_hint_valid
    i64 prev_wave_reads;
    i64 rfa_listed;   // K8: the length of an overflow list (rfa_list_len)
    i64 rfa_routed;   // K8: the barcodes routed to the first tier up front (read with rfa_listed: one synchronisation)
    i64 rfa_classes;  // K8: k_peek_rfa's word (read with rfa_listed too): barcodes listed as small, and << 32 those the small instance turned away
};
static_assert(offsetof(HostPeek, one) == 0 && offsetof(HostPeek, k1.seeds) == 0 && offsetof(HostPeek, k1.big_asked) == 8 && offsetof(HostPeek, k1.p2_drop_probed) == 16 && sizeof(HostPeek::K1) == 32, "k_peek_k1: dst_host[0 .. 3]");
static_assert(offsetof(HostPeek, k6.total) == 0 && offsetof(HostPeek, k6.padded) == 8 && offsetof(HostPeek, k6.listed) == 16 && offsetof(HostPeek, k6.n_long) == 24, "k_resc_offsets: peek_host[0 .. 3]");
static_assert(sizeof(HostPeek) == 64 && offsetof(HostPeek, prev_wave_reads) == 32, "HostPeek");

// ------------------------------------------------------------------------------------------------ rounds (k_rounds.h; lh_host.inc: align_rounds)
// lh_context::round_mem, one group: the plan's prefix array and the view of a part as a batch of its own.  Allocated when a batch first needs a plan (prefix alone:
// lh_last_rounds after a batch that ran whole) or rounds (all four), sized by that batch, regrown as a whole when a later one is larger
struct RoundBufs {
    i64* prefix = nullptr;              // k_round_cost: the seeds before every barcode boundary [cap_bc + 1]
    int32_t* v_bc_pair_off = nullptr;   // k_batch_view: the part's bc_pair_off [cap_bc + 1] ...
    i64* v_seq_off = nullptr;           // ... seq_off [cap_reads + 1] ...
    u64* v_seq = nullptr;               // ... and bases, 8-aligned and padded to a word [cap_bases / 8 + 8]
    i64 cap_bc = 0, cap_reads = 0, cap_bases = 0;   // cap_reads = 0: no view yet
};
// k_round_plan's output in page-locked host memory the device can write: the header, then four arrays of cap_rounds + 1 words
struct RoundPlanBlock {
    char* p = nullptr; i64 cap_rounds = 0;
    static size_t bytes(i64 cap) { return sizeof(RoundPlanHdr) + 4 * (size_t)(cap + 1) * sizeof(i64); }
    RoundPlanHdr* hdr() const { return (RoundPlanHdr*)p; }
    i64* cut_bc() const { return (i64*)(p + sizeof(RoundPlanHdr)); }   // [r]: the first barcode of part r; [n_rounds]: the batch's barcodes
    i64* cut_pair() const { return cut_bc() + (cap_rounds + 1); }      // ... its first pair
    i64* cut_base() const { return cut_pair() + (cap_rounds + 1); }    // ... its first base
    i64* part_seeds() const { return cut_base() + (cap_rounds + 1); }  // [r]: the seeds of part r
};
// what lh_last_rounds reports on a pipeline's last lh_align_resident
struct RoundState {
    int n_rounds = 0;          // 0: the pipeline took no part in the last batch
    bool have_max = false;     // max_bc / max_bc_seeds are known (a batch that ran whole: only once lh_last_rounds has asked the device)
    i64 total_seeds = 0, budget = 0, max_bc = 0, max_bc_seeds = 0;
    std::vector<int32_t> first_bc;
    std::vector<i64> seeds, need;
    void clear() { *this = RoundState(); }
};

// ------------------------------------------------------------------------------------------------ buffers cut into sections
// lh_context::d_ext_u, K4's long queue per chain slot (pool_cap of them): a few int lists, then the units' saved state
struct ExtUnits {
    enum { ULIST, JLIST, JKEY, JORDER, NREG_U, U_READ, EST_U, SECTIONS = EST_U + sizeof(ExtSt) / sizeof(int32_t) };   // in ints per chain slot
    static size_t ints(size_t pool_cap) { return (size_t)SECTIONS * pool_cap; }
    int32_t *ulist;    // the units (free after round 0: then the calls k_ext_wround makes)
    int32_t *jlist, *jkey, *jorder;   // the queued jobs, their keys, their sorted order
    int32_t* nreg_u;   // ExtArgs::nreg_u: regions a unit found
    int32_t* u_read;   // ExtArgs::u_read: a unit's owner read
    ExtSt* est_u;      // ExtArgs::est_u: a unit's saved state
    ExtUnits(int32_t* base, size_t pc) : ulist(base + ULIST * pc), jlist(base + JLIST * pc), jkey(base + JKEY * pc), jorder(base + JORDER * pc), nreg_u(base + NREG_U * pc),
                                         u_read(base + U_READ * pc), est_u((ExtSt*)(base + EST_U * pc)) {}
};
static_assert(ExtUnits::SECTIONS == 10 && sizeof(ExtSt) % sizeof(int32_t) == 0, "ExtUnits");
// lh_context::d_ext_long, the long queue's own read lists (it runs beside the rounds of the other reads), cap_reads entries each
struct ExtLongLists {
    enum { SECTIONS = 4 };
    static size_t ints(size_t cap_reads) { return (size_t)SECTIONS * cap_reads; }
    int32_t* long_list;   // the reads whose chains take the rounds
    int32_t* fb_list;     // the ones k_extend prepares and extends
    int32_t* defer;       // the ones k_ext_merge hands to k_extend
    int32_t* rflag;       // ExtArgs::rflag: per read, "extend me from scratch"
    ExtLongLists(int32_t* base, size_t cap) : long_list(base), fb_list(base + cap), defer(base + 2 * cap), rflag(base + 3 * cap) {}
};
// lh_context::d_regs_tmp while K7 runs (K5's and K6's region scratch, regpool_cap x sizeof(DReg), is dead by then): four candidate lists of regpool_cap ints
struct RegsTmpLists {
    int32_t *wide_r, *wide_ci;   // what k_aln_grp<16> hands on to k_aln_grp<32>
    int32_t *deep_r, *deep_ci;   // (r06) equal spans and five or six mismatches: k_aln_flat2's list for k_aln_grp<16>; it lies behind the other two
    RegsTmpLists(DReg* scratch, size_t regpool_cap) : wide_r((int32_t*)scratch), wide_ci(wide_r + regpool_cap), deep_r(wide_r + 2 * regpool_cap), deep_ci(wide_r + 3 * regpool_cap) {}
};
static_assert(sizeof(DReg) >= 2 * sizeof(int32_t), "two lists in the region scratch");
static_assert(sizeof(DReg) >= 4 * sizeof(int32_t), "four lists in the region scratch");
// lh_context::d_rfa_order, k_rfa_order's output: four barcode lists, largest first, and their lengths
struct RfaOrder {
    static size_t ints(size_t cap_bc) { return 4 * (cap_bc + 4) + 8; }
    int32_t *all, *big, *rest, *small;           // every barcode; those whose tables cannot fit a regular slab; the others; those the small instance of k_rfa takes
    int32_t *n_all, *n_big, *n_rest, *n_small;   // k_rfa_order's counts[0 .. 3] (counts[5]: n_rest as k_rfa_order wrote it; *n_rest itself grows by the barcodes the small instance turns away).  (rest has room for every barcode: the small instance appends those it turns away)
    RfaOrder(int32_t* base, size_t cap_bc) : all(base), big(base + (cap_bc + 4)), rest(base + 2 * (cap_bc + 4)), small(base + 3 * (cap_bc + 4)), n_all(base + 4 * (cap_bc + 4)), n_big(n_all + 1), n_rest(n_all + 2), n_small(n_all + 3) {}
};
// lh_context::d_rfa_ovf_mid, the tiers' overflow lists: what tier k's launch of k_rfa / of k_rfa_post turns away (RfaCounters::tier[k] holds the lengths)
struct RfaOvfMid {
    static size_t ints(size_t cap_bc) { return 4 * (cap_bc + 1); }
    int32_t *rfa[2], *post[2];
    RfaOvfMid(int32_t* base, size_t cap_bc) : rfa{base, base + (cap_bc + 1)}, post{base + 2 * (cap_bc + 1), base + 3 * (cap_bc + 1)} {}
};
// what one launch of k_rfa / k_rfa_post runs on (lh_host_stage2.inc: rfa_tier): a wave per slab, the barcodes taken off a list one by one through a work counter
struct RfaTier { uint8_t* slab; i64 bytes; int grid; int32_t* next; };
// a barcode list on the device and its length: a launch's work list, or where it lists what it turns away (none: the last slabs' verdict is final)
struct RfaList { int32_t *list, *count; };
