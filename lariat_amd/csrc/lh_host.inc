// lh_host.inc — host side of liblariat_hip.so: index upload, per-stream context (workspace pools sized for 288 GB of
// HBM: every intermediate of the per-read pipeline stays resident), kernel sequencing, result download.
// Included by lariat_hip.hip (hipcc, the product) and by tests/hipemu/emu_lib.cpp (g++ -DLH_EMU, test only).
//
// Implements the C-ABI declared in include/lariat_hip.h; the reference interfaces each entry point replaces are cited there.
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <deque>
#include <map>

#include "../../include/lariat_hip.h"
#include "k_smem4.h"
#include "k_chain_lane.h"
#include "k_chain_cl.h"
#include "k_rfa.h"   // pulls in k_seed/k_chain/k_extend/k_global/k_dedup/k_rescue/k_aln
#include "k_rescue3.h"
#include "k_rounds.h"
#include "lh_result_cols.h"

static void lh_print_wd(const int32_t* d_wd) {   // (LH_DEBUG_SYNC builds of a run: the pipeline's watchdog slots after every launch)
    int32_t h[LH_WD_SLOTS];
    if (!d_wd || hipMemcpy(h, d_wd, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int i = 0; i < LH_WD_SLOTS; ++i) if (h[i]) fprintf(stderr, "[lh] watchdog slot %d = %d\n", i, h[i]);
}
static bool lh_debug_sync() { static const bool v = getenv("LH_DEBUG_SYNC") != nullptr; return v; }   // read once: development aid
static thread_local std::string g_err;
static int set_err(int code, const std::string& m) { g_err = m; return code; }
#define HIPCHK(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) { (void)hipGetLastError();   /* HIP's last-error slot is sticky: do not let this failure surface again in a later, unrelated call */ \
            return set_err(LH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); }                      \
    } while (0)
#include "lh_workspace.h"   // DevGroup, the counter blocks, the sectioned buffers


// pinned host blocks that carry results (lh_result_download), recycled between batches
struct PinBlock { char* p = nullptr; size_t cap = 0; };
struct PinPool {
    std::mutex mu;
    std::vector<PinBlock> free_;
    ~PinPool() { for (auto& b : free_) if (b.p) hipHostFree(b.p); }
};
struct lh_index {
    int device = 0;
    DIndex d;   // device pointers
    std::vector<std::string> names;
    std::vector<const char*> name_ptrs;
    std::vector<i64> lens, offs;
    std::vector<uint8_t> h_pac;   // host copy for lh_get_seq
    uint4* d_occ = nullptr; u64* d_sb = nullptr; u64* d_sa = nullptr; u64* d_isa = nullptr; uint32_t* d_tn = nullptr; u64* d_bloom1 = nullptr; u64* d_bloom2 = nullptr; PEnt* d_kmer = nullptr; PEnt* d_ktree = nullptr; uint8_t* d_lcp = nullptr; uint8_t* d_plcp = nullptr; u64* d_rep_t = nullptr; uint8_t* d_pac = nullptr; i64* d_coff = nullptr; int32_t* d_clen = nullptr; int32_t* d_rid_bins = nullptr;
    u64 bwt_words = 0, n_sa = 0;
    int file_sa_intv = 0;
    bool kmer_tables_built = false;
    bool lcp_prebuilt = false; u64* d_ktree_raw = nullptr; int ktree_raw_levels = 0;   // handed over by lh_index_build_device (from its sort keys)
    std::vector<int32_t> n_ambs;                                                     // per contig (.ann)
    std::vector<uint8_t> is_alt; uint8_t* d_alt = nullptr;                            // per contig (.alt); empty: no ALT contigs
    std::vector<i64> hole_off; std::vector<int32_t> hole_len; std::vector<char> hole_char;   // the .amb file's holes
    lh_index_opts io;   // how the index was made resident (defaults filled in)
    u64* d_rep19 = nullptr; u64 n_rep19 = 0;   // lh_index_build_device only, until the sweep filters are built: rows whose suffix shares LH_BLOOM_K bases with the next
};

#define LH_NSTAGE 40
struct lh_context {
    lh_index* idx = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};   // K4's wave kernels run beside its rounds (fork / join around them); (r06) K3's cluster kernels beside each other
    hipStream_t dl_stream = nullptr, up_stream = nullptr;   // the result's device-to-host copies (lh_result_download_begin / _end); uploads into slots that are not selected (lh_batch_stage_slot)
    hipEvent_t ev_pack = nullptr, ev_dl = nullptr;
    bool dl_pending = false, dl_split = false; std::function<int(lh_result**)> dl_finish;
    int sel_slot = 0;
    HostPeek* h_peek = nullptr;   // page-locked, device-writable: small read-backs inside lh_align_resident (lh_workspace.h)
    bool rfa_merge_big = false;    // this batch: k_rfa_order put the big barcodes in front of the rest list (no first-tier slabs to route them to); rfa_prologue decides, rfa_run follows
    i64 rfa_cls[4] = {0, 0, 0, 0}; // lh_last_rfa_classes: the last batch's big, rest and small barcodes as k_rfa_order listed them, and those the small instance turned away
    bool ext_hint_valid = false;   // h_peek->prev_wave_reads holds a previous batch's count
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    i64 cap_pairs = 0, cap_reads = 0, cap_bases = 0, pool_cap = 0, regpool_cap = 0, cap_bc = 0;
    // device memory by lifetime (lh_workspace.h).  mem: the whole context's; seed_mem follows a batch's seed total (pool_cap, regpool_cap: alloc_seed_pools), cand_mem its
    // candidate total (cand_cap: alloc_cand_pools); regrown on their own: K1's big slab and list (big_cap), K6's job arrays (rjob_cap), the download's pack buffers
    // (pack_cap), each K8 tier's slabs (grid_rfa_mid[k]), the rounds' plan array and batch view (rb).  A batch slot's arrays: DevBatch::mem
    DevGroup mem, seed_mem, cand_mem, big_mem, rjob_mem, pack_mem, tier_mem[2], round_mem;
    void free_device() {   // everything this context owns on the device
        for (DevGroup* g : {&mem, &seed_mem, &cand_mem, &big_mem, &rjob_mem, &pack_mem, &tier_mem[0], &tier_mem[1], &round_mem}) g->release();
        for (DevBatch& sl : slots) sl.mem.release();
        for (void* q : free_later) hipFree(q);
        free_later.clear();
    }
    int grid_smem4 = 0; PEnt* d_slab4 = nullptr; K1Counters* d_next_read = nullptr;
    // inputs
    BatchView b;                  // the selected batch: a slot's (select_slot) or, inside align_rounds, a round's part of it
    uint32_t* d_seq4 = nullptr;   // its reads as a 4-bit stream (k_pack_reads), two words of padding in front
    const uint32_t* q4 = nullptr;   // d_seq4 + 2 while the index has the 4-bit text (run_front)
    // K1
    DIntv* d_intv = nullptr; DIntv* d_big_slab = nullptr; int32_t *d_big_slot = nullptr, *d_big_list = nullptr; K1BigCounts* d_big_count = nullptr; int big_cap = 0, big_base = 0;   // reads with more than LH_MAX_INTV intervals (k_smem4.h BIG)
    K1Resume* d_k1_resume = nullptr; int32_t* d_k1_todo = nullptr;   // k_smem_first's hand-over to the state machine (the count: d_next_read->n_todo)
    u64* d_p2_tasks = nullptr; P2Calls* d_p2_calls = nullptr;   // pass 2's list (the count: d_next_read->n_p2_tasks) and what its lister counted, LH_CTR_SLOTS copies
    i64 p2_cls[4] = {0, 0, 0, 0};   // lh_last_p2_calls: the last batch's re-seeding calls dropped, listed probed, listed unprobed, and its reads listed as shares
    int32_t *d_n_intv = nullptr, *d_seed_cnt = nullptr, *d_l_rep = nullptr, *d_status = nullptr;
    int32_t* d_fin_list = nullptr;   // the reads pass 3 leaves to k_smem_fin (the count: d_next_read->n_fin); the others' intervals K2 ranks itself
    // K2/K3
    i64* d_seed_off = nullptr; DSeed* d_seeds = nullptr; int32_t *d_s_rid = nullptr, *d_s_next = nullptr, *d_ord = nullptr, *d_srt = nullptr;
    DChainTmp* d_ct = nullptr; DChain* d_chains = nullptr; DSeed* d_cseeds = nullptr; int32_t* d_n_chains = nullptr;
    DCounters* d_ctr = nullptr; i64* d_tile_sum = nullptr;
    int32_t* d_wd = nullptr;   // this pipeline's watchdog slots (LH_WATCH through DOpts::wd): read back and cleared with its result
    // K4 (k_extend2.h); the region pools follow the seed pools
    i64* d_reg_off = nullptr; DReg* d_regs = nullptr; int32_t* d_n_regs = nullptr; i64* d_chain_rmax = nullptr;
    DReg* d_regs_tmp = nullptr;   // K5's and K6's region scratch; K7's lists (RegsTmpLists)
    int32_t* d_ia = nullptr;
    int32_t *d_ext_defer = nullptr, *d_ext_heavy = nullptr, *d_ext_jlist = nullptr, *d_ext_jkey = nullptr, *d_ext_jorder = nullptr; ExtSt* d_ext_st = nullptr;
    DExtJobs* d_ext_jobs = nullptr; DExtJobs* d_ext_jobs2 = nullptr;   // the rounds' queue; the long queue's own (it runs beside them)
    int32_t* d_ext_long = nullptr;   // the long queue's read lists (ExtLongLists)
    int32_t* d_ext_u = nullptr;      // the long queue per chain slot (ExtUnits)
    // K5, K6 (k_dedup.h, k_rescue2.h)
    int32_t* d_best = nullptr;
    uint8_t* d_reg_clean = nullptr;   // K5's word per read: its list needs no look before K6's replay (k_dedup.h)
    uint8_t* d_dd_done = nullptr;     // K5's lane form ran where the read's extension finished (ExtArgs::dd_done): k_dedup_fast passes over the read
    int32_t* d_dd_list = nullptr;     // the reads K5's lane form leaves to k_dedup (the count: d_ext_jobs->dd_need).  Its own: d_aln_r is being read by K4's long queue while the rounds append here
    int32_t* d_rnj = nullptr; i64* d_rjob_off = nullptr; RMeta* d_rmeta = nullptr; int32_t* d_rkeys = nullptr; int32_t* d_rheavy = nullptr;
    RJob* d_rjobs = nullptr; int32_t *d_rorder = nullptr, *d_rorder2 = nullptr; i64 rjob_cap = 0;   // K6's jobs (k_rescue2.h): they follow the batch
    // K7 (k_aln.h) and the result's candidate arrays
    i64 cand_cap = 0; int grid_aln = 0; DCand R; uint8_t* d_zpool = nullptr;
    int32_t *d_aln_r = nullptr, *d_aln_ci = nullptr; AlnCounts* d_aln_count = nullptr;   // candidate lists and their lengths (K3, K5 and K6 list reads there before)
    i64 *d_cigar_off = nullptr, *d_mm_off = nullptr; uint32_t *d_pack_a = nullptr, *d_pack_b = nullptr, *d_pack_c = nullptr; i64 pack_cap = 0;   // the download's scans and packed arrays
    std::shared_ptr<PinPool> pin_pool = std::make_shared<PinPool>();
    bool dump_stop_after_dedup = false; bool ran_inference = false;
    bool in_round = false;   // the selection is a part of the resident batch (align_rounds)
    // K8 (k_rfa.h)
    DInf S; uint8_t* d_slab = nullptr; i64 slab_bytes = 0; int grid_rfa = 0; RfaCounters* d_bc_next = nullptr;
    uint8_t* d_slab2 = nullptr; i64 slab2_bytes = 0; int grid_rfa2 = 0;
    uint8_t* d_slab_mid[2] = {nullptr, nullptr}; i64 slab_mid_bytes[2] = {0, 0}; int grid_rfa_mid[2] = {0, 0}; int grid_rfa_mid_max[2] = {0, 0};   // (r05) two tiers between the regular slabs and the few large ones
    int32_t* d_rfa_ovf_mid = nullptr;   // the tiers' overflow lists (RfaOvfMid)
    int32_t* d_rfa_order = nullptr;     // k_rfa_order's lists (RfaOrder)
    bool rfa_pre = false;               // K8's prologue (rfa_prologue) was forked onto aux[0] beside K7: rfa_run joins it
    int32_t *d_rfa_ovf = nullptr, *d_rfa_ovf2 = nullptr, *d_rfa_hp = nullptr, *d_rfa_hr = nullptr; double* d_bc_lmp = nullptr;
    // timings
    hipEvent_t ev[LH_NSTAGE + 1];
    const char* tnames[LH_NSTAGE];
    float tms[LH_NSTAGE];
    int n_t = 0;
    bool resident = false, ran = false;
    std::mutex res_mu;   // (the first pipeline's) held by lh_align_resident and lh_stage_dump_resident, and by lh_bam_append_resident while its gather kernels read the result arrays.  Lock order: this, then a compressor's
    // resident input batches: slot 0 holds capacity-sized buffers allocated at creation, further slots own exact-size copies
    struct DevBatch {
        BatchView v;    // the slot's batch (pipe_upload_slot)
        DevGroup mem;   // v's seven arrays
        bool filled = false;
        i64 cap_bases = 0; int cap_reads = 0, cap_bc = 0;   // what the slot's own buffers hold (slots > 0)
    };
    std::deque<DevBatch> slots; std::mutex slot_mu;   // slot_mu: slots' size and `filled`, sel_slot / resident, free_later.  (A deque: growing it does not move the slots another thread holds)
    std::vector<void*> free_later;   // device buffers a staging thread replaced: freed by the aligning thread
    lh_context_opts co;   // launch geometry (defaults filled in)
    // rounds (k_rounds.h, align_rounds): a batch whose seed workspace exceeds the budget is aligned part by part inside one lh_align_resident
    RoundBufs rb; RoundPlanBlock plan; RoundState rounds;
    lh_result* round_result = nullptr;   // the parts' results merged: handed out by the next download
    uint32_t flags = 0;   // lh_opts.flags of the running call
    // lanes > 1 (lh_lanes.inc): further, smaller pipelines owned by this one; a batch is cut at barcode boundaries and the parts
    // run side by side from as many host threads
    std::vector<lh_context*> more;            // lanes 2 .. L
    std::vector<std::vector<int32_t>> slot_cut;   // slot_cut[k] = first barcode of lane 2 .. L's part in slot k (empty: not split)
    int cur_slot = 0;
};

const char* lh_last_error(void) { return g_err.c_str(); }
// for the host-only translation units of the library (ingest.cpp)
extern "C" int lh_set_error_(int code, const char* msg) { return set_err(code, msg ? msg : ""); }

int lh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void lh_opts_init(lh_opts* o) {
    memset(o, 0, sizeof *o);
    o->abi_version = LH_ABI_VERSION;
    o->a = 1; o->b = 4; o->o_del = 6; o->e_del = 1; o->o_ins = 6; o->e_ins = 1;
    o->pen_unpaired = 17; o->pen_clip5 = 5; o->pen_clip3 = 5;
    o->w = 100; o->zdrop = 100; o->T = 30;
    o->min_seed_len = 19; o->min_chain_weight = 0; o->max_chain_extend = 1 << 30;
    o->split_factor = 1.5f; o->split_width = 10; o->max_occ = 500; o->max_chain_gap = 10000; o->max_ins = 10000;
    o->mask_level = 0.50f; o->drop_ratio = 0.50f; o->XA_drop_ratio = 0.80f; o->mask_level_redun = 0.95f;
    o->mapQ_coef_len = 50; o->max_mem_intv = 20; o->max_matesw = 50;
    o->pes_low = -35; o->pes_high = 500;
    o->rescue_score_delta = 25; o->rescue_max_hits = 50; o->aln_score_delta = 17;
    o->improper_pair_penalty = -4.0; o->genome_length = 3200000000.0; o->run_inference = 1;
}

void lh_context_opts_init(lh_context_opts* co) {
    if (!co) return;
    memset(co, 0, sizeof *co);
    co->abi_version = LH_ABI_VERSION;
}

static DOpts to_dopts(const lh_opts* o) {
    DOpts d;
    memset(&d, 0, sizeof d);
    d.a = o->a; d.b = o->b; d.o_del = o->o_del; d.e_del = o->e_del; d.o_ins = o->o_ins; d.e_ins = o->e_ins;
    d.pen_unpaired = o->pen_unpaired; d.pen_clip5 = o->pen_clip5; d.pen_clip3 = o->pen_clip3; d.w = o->w; d.zdrop = o->zdrop; d.T = o->T;
    d.min_seed_len = o->min_seed_len; d.min_chain_weight = o->min_chain_weight; d.max_chain_extend = o->max_chain_extend;
    d.split_width = o->split_width; d.max_occ = o->max_occ; d.max_chain_gap = o->max_chain_gap; d.max_ins = o->max_ins;
    d.max_mem_intv = o->max_mem_intv; d.max_matesw = o->max_matesw;
    d.split_factor = o->split_factor; d.mask_level = o->mask_level; d.drop_ratio = o->drop_ratio; d.XA_drop_ratio = o->XA_drop_ratio;
    d.mask_level_redun = o->mask_level_redun; d.mapQ_coef_len = o->mapQ_coef_len;
    d.pes_low = o->pes_low; d.pes_high = o->pes_high; d.rescue_score_delta = o->rescue_score_delta; d.rescue_max_hits = o->rescue_max_hits;
    d.aln_score_delta = o->aln_score_delta; d.run_inference = o->run_inference;
    d.improper_pair_penalty = o->improper_pair_penalty; d.genome_length = o->genome_length;
    int k = 0;
    for (int i = 0; i < 4; ++i) { for (int j = 0; j < 4; ++j) d.mat[k++] = (int8_t)(i == j ? o->a : -o->b); d.mat[k++] = -1; }
    for (int j = 0; j < 5; ++j) d.mat[k++] = -1;
    return d;
}

#include "lh_index.inc"

// ------------------------------------------------------------------------------------------------ context
#ifndef LH_POOL_FLOOR
#define LH_POOL_FLOOR (1 << 16)   // the seed pools and the candidate pools start with room for this many entries at least
#endif
static int rfa_alloc(lh_context* c);
static void rfa_prologue(lh_context* c, hipStream_t st);
static int rfa_run(lh_context* c, const DOpts& o, int& t);
static int stage2_alloc(lh_context* c);
static int stage2_run(lh_context* c, const DOpts& o, int& t);
#define LH_NEED_ROUNDS (-1)   // run_front, internal: the batch's seed workspace exceeds its budget (pipe_align then aligns it in rounds)

// ---- the seed budget.  The seed, chain and region pools follow a batch's seed total; what they may take is the budget: lh_context_opts.seed_budget_kb, or (0) the
// HBM that is free plus what the pools hold already, less 2 GB for the other buffers that follow a batch.  A batch that needs more is aligned in rounds (align_rounds).
// bytes per entry of the seed pools plus one of the region pools (alloc_seed_pools' arrays; a low-complexity read has up to max_occ seeds per interval: ~0.5 KB each)
static const i64 LH_REG_ENTRY_BYTES = (i64)(2 * sizeof(DReg) + 12);                                                               // per entry of the region pools
static const i64 LH_SEED_ENTRY_BYTES = (i64)(sizeof(DSeed) * 2 + 4 * 4 + sizeof(DChainTmp) + sizeof(DChain) + 16 + 40);            // per entry of the seed pools
static const i64 LH_SEED_POOL_BYTES = LH_SEED_ENTRY_BYTES + LH_REG_ENTRY_BYTES;   // per seed: one of each (the need counts a rescue slot as much: room for the buffers that grow later)
static i64 seed_fixed_slots(const lh_context* c) { return c->cap_reads * LH_RESCUE_SLOTS; }
static i64 seed_need(const lh_context* c, i64 seeds) { return lh_seed_need(seeds, seed_fixed_slots(c), LH_SEED_POOL_BYTES); }
static int seed_budget(const lh_context* c, i64* budget) {
    if (c->co.seed_budget_kb > 0) { *budget = (i64)c->co.seed_budget_kb << 10; return LH_OK; }
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    *budget = (i64)free_b + c->pool_cap * LH_SEED_ENTRY_BYTES + c->regpool_cap * LH_REG_ENTRY_BYTES - 2000000000;   // (what the pools hold is theirs to use again)
    return LH_OK;
}
// the largest pool_cap a fixed budget allows (no fixed budget: no bound)
static i64 pool_cap_limit(const lh_context* c) {
    return c->co.seed_budget_kb > 0 ? ((i64)c->co.seed_budget_kb << 10) / LH_SEED_POOL_BYTES - seed_fixed_slots(c) : INT64_MAX;
}

// pools whose size follows the number of seeds of a batch (pool_cap) or of regions (regpool_cap = seeds + rescue slots)
static int alloc_seed_pools(lh_context* c, i64 pool_cap) {
    DevGroup& g = c->seed_mem;
    g.release(); c->pool_cap = c->regpool_cap = 0;
    const i64 regpool_cap = pool_cap + c->cap_reads * LH_RESCUE_SLOTS;
    DALLOC(g, c->d_seeds, pool_cap); DALLOC(g, c->d_s_rid, pool_cap); DALLOC(g, c->d_s_next, pool_cap);
    DALLOC(g, c->d_ord, pool_cap); DALLOC(g, c->d_srt, pool_cap); DALLOC(g, c->d_ct, pool_cap); DALLOC(g, c->d_chains, pool_cap);
    DALLOC(g, c->d_cseeds, pool_cap);
    DALLOC(g, c->d_regs, regpool_cap); DALLOC(g, c->d_regs_tmp, regpool_cap); DALLOC(g, c->d_ia, regpool_cap + c->cap_reads + 8);
    DALLOC(g, c->d_aln_r, regpool_cap); DALLOC(g, c->d_aln_ci, regpool_cap); DALLOC(g, c->d_chain_rmax, 2 * pool_cap);
    DALLOC(g, c->d_ext_u, ExtUnits::ints((size_t)pool_cap));
    c->pool_cap = pool_cap; c->regpool_cap = regpool_cap;
    return LH_OK;
}
static int alloc_cand_pools(lh_context* c, i64 cand_cap);
// the two pools' sizes in a new context; both grow on demand (run_front, stage2_run: a batch's totals are known before anything is written there)
static i64 first_pool_cap(const lh_context* c) {   // ~10 seeds per 150-base read at hg38 scale; within a fixed seed budget from the first allocation on
    const i64 want = c->cap_reads * 16 > LH_POOL_FLOOR ? c->cap_reads * 16 : LH_POOL_FLOOR, most = pool_cap_limit(c);
    return want < most ? want : most;
}
static i64 first_cand_cap(const lh_context* c) { return c->cap_reads * 3 > LH_POOL_FLOOR ? c->cap_reads * 3 : LH_POOL_FLOOR; }     // ~1.1 candidates/read on unique sequence

static void pipe_free(lh_context* c);
static void select_slot(lh_context* c, const lh_context::DevBatch& sl) { c->b = sl.v; }
struct CtxGuard { lh_context* c; ~CtxGuard() { if (c) pipe_free(c); } };

static int pipe_create(lh_index* idx, int64_t max_pairs, const lh_context_opts* co, lh_context** out) {
    if (!idx || !out || max_pairs <= 0) return set_err(LH_E_ARG, "lh_context_create: bad argument");
    if (co && co->abi_version != LH_ABI_VERSION) return set_err(LH_E_ARG, "lh_context_opts.abi_version does not match LH_ABI_VERSION (use lh_context_opts_init)");
    if (max_pairs >= (int64_t)1 << 29) return set_err(LH_E_LIMIT, "lh_context_create: fewer than 2^29 pairs per batch (K6's list entries keep a pair's index in 29 bits, k_rescue2.h)");
    HIPCHK(hipSetDevice(idx->device));
    lh_context* c = new lh_context();
    CtxGuard guard{c};
    if (co) c->co = *co; else lh_context_opts_init(&c->co);
    if (c->co.smem_grid <= 0) c->co.smem_grid = 6144;
    if (c->co.aln_grid <= 0) c->co.aln_grid = 256 * 40;   // (k_aln at 44 VGPRs: measured 5.6 / 3.8 / 3.6 ms per 2 M pairs with 2560 / 5120 / 10240 waves)
    if (c->co.rfa_grid <= 0) c->co.rfa_grid = 4096;
    if (c->co.rfa_slab_kb <= 0) c->co.rfa_slab_kb = 3072;   // (r06: 2048 before; a 1,000-pair barcode with a twentieth of its pairs on repeat families carves 1 - 2.3 MB, and a barcode sent to a tier only starts when the first launch has ended)
    for (int i = 0; i <= LH_NSTAGE; ++i) c->ev[i] = nullptr;
    c->idx = idx;
    c->cap_pairs = max_pairs; c->cap_reads = 2 * max_pairs;
    c->cap_bases = c->cap_reads * (i64)LH_MAXLEN;
    c->cap_bc = max_pairs;
    HIPCHK(hipStreamCreate(&c->stream));
    for (int i = 0; i < 3; ++i) { HIPCHK(hipStreamCreate(&c->aux[i])); HIPCHK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming)); }
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    {   // the transfer streams get a priority of their own: HIP maps the streams of one priority onto a few hardware queues, and a kernel launch
        // that shares its queue with a 600 MB copy waits for it (measured: 13 ms per batch inside lh_align_resident at hg38 scale)
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&c->dl_stream, hipStreamNonBlocking, lo));
        HIPCHK(hipStreamCreateWithPriority(&c->up_stream, hipStreamNonBlocking, lo));
    }
    HIPCHK(hipHostMalloc((void**)&c->h_peek, sizeof(HostPeek), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_dl, hipEventDisableTiming));
    i64 N = c->cap_reads;
    DevGroup& g = c->mem;
    DALLOC(g, c->d_seq4, c->cap_bases / 8 + 16); HIPCHK(hipMemset(c->d_seq4, 0x44, 16));
    {
        lh_context::DevBatch& s0 = c->slots.emplace_back();
        DALLOC(s0.mem, s0.v.seq, c->cap_bases + 64); DALLOC(s0.mem, s0.v.seq_off, N + 1); DALLOC(s0.mem, s0.v.name_seed, max_pairs);
        DALLOC(s0.mem, s0.v.bc_pair_off, c->cap_bc + 1); DALLOC(s0.mem, s0.v.bc_do_rfa, c->cap_bc);
        DALLOC(s0.mem, s0.v.cen_start, idx->names.size()); DALLOC(s0.mem, s0.v.cen_end, idx->names.size());
        select_slot(c, s0);
    }
    DALLOC(g, c->d_intv, N * LH_MAX_INTV); DALLOC(g, c->d_n_intv, N);
    c->big_cap = c->co.big_slots > 0 ? c->co.big_slots : LH_MAX_INTV < 16 ? (int)N : (int)(N / 256 > 64 ? N / 256 : 64);   // (a test build with tiny regular slots sends most reads there)
    DALLOC(g, c->d_k1_resume, N); DALLOC(g, c->d_k1_todo, N); DALLOC(g, c->d_p2_tasks, (size_t)LH_P2_SPLIT * N); DALLOC(g, c->d_p2_calls, LH_CTR_SLOTS);
    DALLOC(c->big_mem, c->d_big_slab, (size_t)c->big_cap * 2 * LH_BIG_INTV); DALLOC(g, c->d_big_slot, N); DALLOC(c->big_mem, c->d_big_list, c->big_cap); DALLOC(g, c->d_big_count, 1);
    DALLOC(g, c->d_seed_cnt, N); DALLOC(g, c->d_l_rep, N); DALLOC(g, c->d_status, N); DALLOC(g, c->d_fin_list, N);
    {   // persistent-lane K1: 64 reads per wave in flight, as many waves as the device keeps resident (tunable for experiments)
        int want = c->co.smem_grid;
        i64 need = (c->cap_reads + 63) / 64;
        c->grid_smem4 = (int)(need < want ? need : want);
        DALLOC(g, c->d_slab4, (size_t)c->grid_smem4 * 64 * 2 * (LH_MAXLEN + 2));
        DALLOC(g, c->d_next_read, 1);
    }
    DALLOC(g, c->d_seed_off, N + 1); DALLOC(g, c->d_n_chains, N);
    if (c->co.seed_budget_kb < 0 || pool_cap_limit(c) < 1)
        return set_err(LH_E_ARG, "lh_context_opts.seed_budget_kb = " + std::to_string(c->co.seed_budget_kb) + ": the rescue slots of " + std::to_string(max_pairs) +
                                     " pairs alone take " + std::to_string((seed_need(c, 0) >> 10) + 1) + " KiB");
    { int rc = alloc_seed_pools(c, first_pool_cap(c)); if (rc) return rc; }
    DALLOC(g, c->d_ctr, LH_CTR_SLOTS);
    DALLOC(g, c->d_wd, LH_WD_SLOTS);
    HIPCHK(hipMemset(c->d_wd, 0, LH_WD_SLOTS * sizeof(int32_t)));
    { int rc = stage2_alloc(c); if (rc) return rc; }
    for (int i = 0; i <= LH_NSTAGE; ++i) HIPCHK(hipEventCreate(&c->ev[i]));
    guard.c = nullptr;
    *out = c;
    return LH_OK;
}

static void pipe_free(lh_context* c) {
    if (!c) return;
    c->free_device();
    for (int i = 0; i <= LH_NSTAGE; ++i) if (c->ev[i]) hipEventDestroy(c->ev[i]);
    for (int i = 0; i < 3; ++i) { if (c->aux[i]) hipStreamDestroy(c->aux[i]); if (c->ev_join[i]) hipEventDestroy(c->ev_join[i]); }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->dl_pending) { lh_result* r = nullptr; if (c->dl_finish && c->dl_finish(&r) == LH_OK) lh_result_free(r); c->dl_pending = false; }
    if (c->h_peek) hipHostFree(c->h_peek);
    if (c->plan.p) hipHostFree(c->plan.p);
    if (c->round_result) lh_result_free(c->round_result);
    if (c->dl_stream) hipStreamDestroy(c->dl_stream);
    if (c->up_stream) hipStreamDestroy(c->up_stream);
    if (c->ev_pack) hipEventDestroy(c->ev_pack);
    if (c->ev_dl) hipEventDestroy(c->ev_dl);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

static int pipe_upload_slot(lh_context* c, int32_t slot, const lh_batch* b, bool staged) {
    if (!c || !b || !b->seq_off || !b->seq || !b->bc_pair_off) return set_err(LH_E_ARG, "lh_batch_upload: null argument");
    if (slot < 0 || slot > 4096) return set_err(LH_E_ARG, "lh_batch_upload_slot: slot out of range");
    hipStream_t us = staged ? c->up_stream : c->stream;
    if (b->n_pairs <= 0 || b->n_pairs > c->cap_pairs) return set_err(LH_E_CAPACITY, "batch larger than the context capacity");
    if (b->n_barcodes <= 0 || b->n_barcodes > c->cap_bc) return set_err(LH_E_ARG, "bad barcode count");
    if (b->bc_pair_off[0] != 0 || b->bc_pair_off[b->n_barcodes] != b->n_pairs) return set_err(LH_E_ARG, "bc_pair_off must cover [0,n_pairs]");
    HIPCHK(hipSetDevice(c->idx->device));
    int n_reads = 2 * b->n_pairs;
    i64 nb = b->seq_off[n_reads];
    if (nb > c->cap_bases) return set_err(LH_E_CAPACITY, "too many bases for the context");
    if (b->seq_off[0] != 0) return set_err(LH_E_ARG, "seq_off must start at 0");
    i64 lmax = 0;
    for (int r = 0; r < n_reads; ++r) {
        i64 l = b->seq_off[r + 1] - b->seq_off[r];
        if (l < 0) return set_err(LH_E_ARG, "seq_off must be non-decreasing (read " + std::to_string(r) + ")");
        if (l > LH_MAX_READ_LEN) return set_err(LH_E_LIMIT, "read " + std::to_string(r) + " is longer than LH_MAX_READ_LEN");
        lmax = l > lmax ? l : lmax;
    }
    for (int k = 0; k < b->n_barcodes; ++k)
        if (b->bc_pair_off[k + 1] < b->bc_pair_off[k]) return set_err(LH_E_ARG, "bc_pair_off must be non-decreasing (barcode " + std::to_string(k) + ")");
    size_t nc = c->idx->names.size();
    lh_context::DevBatch* slp;
    {
        std::lock_guard<std::mutex> g(c->slot_mu);
        if (staged && c->resident && slot == c->sel_slot) return set_err(LH_E_ARG, "lh_batch_stage_slot: that slot is the selected one (stage into another, then lh_batch_select)");
        while ((size_t)slot >= c->slots.size()) c->slots.emplace_back();
        slp = &c->slots[(size_t)slot];
        slp->filled = false;   // not selectable while its contents are being replaced (a failed copy leaves it so)
    }
    lh_context::DevBatch& sl = *slp;
    BatchView& v = sl.v;
    if (slot > 0 && (nb > sl.cap_bases || n_reads > sl.cap_reads || b->n_barcodes > sl.cap_bc)) {
        // buffers of its own (slot 0 uses the capacity-sized ones), kept while the next batch fits.  hipFree waits for the whole device: from
        // the staging thread it would sit behind the kernels the upload is meant to run beside, so the old buffers are handed to the thread
        // that aligns (pipe_align frees them before its first launch) or to lh_context_free
        if (staged) { std::lock_guard<std::mutex> g(c->slot_mu); sl.mem.release_to(c->free_later); }
        else sl.mem.release();
        sl.cap_bases = 0; sl.cap_reads = 0; sl.cap_bc = 0;
        const i64 cap_bases = nb + nb / 16;
        DevGroup& g = sl.mem;
        DALLOC(g, v.seq, (size_t)cap_bases + 64); DALLOC(g, v.seq_off, (size_t)n_reads + 1); DALLOC(g, v.name_seed, (size_t)b->n_pairs);
        DALLOC(g, v.bc_pair_off, (size_t)b->n_barcodes + 1); DALLOC(g, v.bc_do_rfa, (size_t)b->n_barcodes); DALLOC(g, v.cen_start, nc); DALLOC(g, v.cen_end, nc);
        sl.cap_bases = cap_bases; sl.cap_reads = n_reads; sl.cap_bc = b->n_barcodes;
    }
    v.n_pairs = b->n_pairs; v.n_reads = n_reads; v.n_bc = b->n_barcodes; v.n_bases = nb; v.max_len = (int)lmax;
    HIPCHK(hipMemcpyAsync(v.seq, b->seq, (size_t)nb, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(v.seq_off, b->seq_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, us));
    std::vector<u64> seeds;
    const u64* ns = (const u64*)b->name_seed;
    if (!ns) { seeds.assign(b->n_pairs, 1); ns = seeds.data(); }
    HIPCHK(hipMemcpyAsync(v.name_seed, ns, (size_t)b->n_pairs * 8, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(v.bc_pair_off, b->bc_pair_off, (size_t)(b->n_barcodes + 1) * 4, hipMemcpyHostToDevice, us));
    std::vector<uint8_t> rfa;
    const uint8_t* pr = b->bc_do_rfa;
    if (!pr) { rfa.assign(b->n_barcodes, 1); pr = rfa.data(); }
    HIPCHK(hipMemcpyAsync(v.bc_do_rfa, pr, (size_t)b->n_barcodes, hipMemcpyHostToDevice, us));
    v.has_cen = b->cen_start && b->cen_end;
    std::vector<i64> neg(nc, -1);
    HIPCHK(hipMemcpyAsync(v.cen_start, v.has_cen ? b->cen_start : neg.data(), nc * 8, hipMemcpyHostToDevice, us));
    HIPCHK(hipMemcpyAsync(v.cen_end, v.has_cen ? b->cen_end : neg.data(), nc * 8, hipMemcpyHostToDevice, us));
    HIPCHK(hipStreamSynchronize(us));
    std::lock_guard<std::mutex> g(c->slot_mu);
    sl.filled = true;
    if (!staged) {   // (a staged batch is selected later: lh_batch_select)
        select_slot(c, sl);
        c->sel_slot = slot;
        c->resident = true; c->ran = false;
    }
    return LH_OK;
}


static int pipe_select(lh_context* c, int32_t slot) {
    if (!c) return set_err(LH_E_ARG, "lh_batch_select: null context");
    std::lock_guard<std::mutex> g(c->slot_mu);
    if (slot < 0 || (size_t)slot >= c->slots.size() || !c->slots[(size_t)slot].filled) return set_err(LH_E_ARG, "lh_batch_select: no batch resident in that slot");
    select_slot(c, c->slots[(size_t)slot]);
    c->sel_slot = slot;
    c->resident = true; c->ran = false;
    return LH_OK;
}

#define T_BEGIN(name) do { c->tnames[t] = name; HIPCHK(hipEventRecord(c->ev[t], c->stream)); } while (0)
#define T_END()                                                                                  \
    do {                                                                                         \
        if (lh_debug_sync()) {                                                                   \
            fprintf(stderr, "[lh] launched %s ...", c->tnames[t]); fflush(stderr);               \
            hipError_t e_ = hipStreamSynchronize(c->stream);                                     \
            fprintf(stderr, " done (%s)\n", e_ == hipSuccess ? "ok" : hipGetErrorString(e_)); fflush(stderr); \
            lh_print_wd(c->d_wd);                                                                    \
        }                                                                                        \
        ++t;                                                                                     \
    } while (0)

static int run_scan(lh_context* c, int n, const int32_t* in, int add, int at_least, i64* out, i64* out2 = nullptr, int add2 = 0) {
    int nt = (n + LH_SCAN_TILE - 1) / LH_SCAN_TILE;
    LH_LAUNCH(k_scan_partial, nt, 256, c->stream, n, in, add, at_least, c->d_tile_sum);
    LH_LAUNCH(k_scan_tiles, 1, 256, c->stream, nt, c->d_tile_sum);
    LH_LAUNCH(k_scan_final, nt, 256, c->stream, n, in, add, at_least, c->d_tile_sum, nt, out, out2, add2);
    return LH_OK;
}

static inline bool dedup_fused(const lh_context* c) { return !(c->flags & (LH_F_TAIL_PASSES | LH_F_EXT_WAVE)); }
static ExtArgs ext_args(lh_context* c) {
    ExtArgs A;
    A.seq = c->b.seq; A.q4 = c->q4; A.seq_off = c->b.seq_off; A.seed_off = c->d_seed_off; A.chains = c->d_chains; A.cseeds = c->d_cseeds; A.n_chains = c->d_n_chains;
    A.sorder = c->d_srt; A.sdone = c->d_ord; A.chain_rmax = c->d_chain_rmax; A.reg_off = c->d_reg_off; A.regs = c->d_regs; A.n_regs = c->d_n_regs; A.est = c->d_ext_st;
    const ExtUnits U(c->d_ext_u, (size_t)c->pool_cap);
    A.nreg_u = U.nreg_u; A.u_read = U.u_read; A.est_u = U.est_u; A.rflag = ExtLongLists(c->d_ext_long, (size_t)c->cap_reads).rflag;
    // K5 on the lane that finishes a read (not when K5 runs as a pass of its own, nor when no lane extends: LH_F_EXT_WAVE)
    A.dd_best = c->d_best; A.dd_clean = c->d_reg_clean; A.dd_done = dedup_fused(c) ? c->d_dd_done : nullptr; A.dd_list = c->d_dd_list; A.dd_count = &c->d_ext_jobs->dd_need;
    return A;
}

#include "lh_host_trace.inc"   // the development aids' read-outs (LH_K1_TRACE, LH_RFA_PROF, LH_RA_HIST)

// one pass of K1's state machine (k_smem4.h) on `grid` waves.  PASS names its read counter, the second chance's if BIG; QW: the instance by query staging; big: the
// second chance's slab (BIG), else the list the pass works from (k_smem_first's reads, pass 2's tasks; none: every read)
template <int PASS, bool BIG, int QW = 32> static void smem_pass(lh_context* c, const DIndex& ix4, const DOpts& o, int N, int grid, const K1Big& big) {
    int32_t* const next = BIG ? &c->d_next_read->big_pass[PASS - 1] : &c->d_next_read->pass[PASS - 1];
    LH_LAUNCH((k_smem_pass<PASS, BIG, QW>), grid, 64, c->stream, ix4, o, N, c->b.seq, c->b.seq_off, c->d_intv, c->d_n_intv, c->d_status, c->d_slab4, next, c->d_ctr, big);
}

// K1's second chance: the reads whose intervals outgrew their LH_MAX_INTV regular slots run the three passes again into slots of the big slab
// (BWA's interval vector grows: no read is refused).  base = 0: the round inside K1; base > 0: a further round for the reads that found the slab
// full, after run_front has grown it.
static int k1_big_round(lh_context* c, const DOpts& o, const DIndex& ix4, int N, int base) {
    const int g4 = (N + 63) / 64 < c->grid_smem4 ? (N + 63) / 64 : c->grid_smem4;
    const int gb = g4 < 64 ? g4 : 64;   // a handful of reads, if any (the kernels read the count on the device: no host round trip)
    HIPCHK(hipMemsetAsync(c->d_big_count, 0, sizeof(K1BigCounts), c->stream));
    HIPCHK(hipMemsetAsync(c->d_next_read->big_pass, 0, sizeof c->d_next_read->big_pass, c->stream));
    K1Big big; big.list = c->d_big_list; big.count = &c->d_big_count->listed; big.slot = c->d_big_slot; big.slab = c->d_big_slab; big.resume = nullptr;
    LH_LAUNCH(k_big_collect, (N + 255) / 256, 256, c->stream, N, c->d_status, c->d_n_intv, c->d_big_slot, c->d_big_list, &c->d_big_count->listed, base, c->big_cap - base);
    smem_pass<1, true>(c, ix4, o, N, gb, big);
    smem_pass<2, true>(c, ix4, o, N, gb, big);
    if (o.max_mem_intv > 0) smem_pass<3, true>(c, ix4, o, N, gb, big);
    LH_LAUNCH(k_smem_fin_big, gb, 64, c->stream, o, big, (const int32_t*)c->d_n_intv, c->d_seed_cnt, c->d_l_rep);
    return LH_OK;
}

// the regular slots' intervals sorted, seed counts, l_rep: of the reads pass 3 listed (it has counted the others), or of every read
static int smem_fin(lh_context* c, const DOpts& o, int N, bool listed) {
    const int all = (N * 16 + 255) / 256;
    LH_LAUNCH(k_smem_fin, listed && all > LH_FIN_GRID ? LH_FIN_GRID : all, 256, c->stream, o, N, c->d_intv, (const int32_t*)c->d_n_intv, c->d_seed_cnt, c->d_l_rep, (const int32_t*)c->d_big_slot,
              (const int32_t*)(listed ? c->d_fin_list : nullptr), (const int32_t*)(listed ? &c->d_next_read->n_fin : nullptr));
#ifdef LH_FIN_TRACE   // a development build's read-out (it waits for the stream): how many reads pass 3 listed
    if (listed) {
        int32_t n_fin = 0;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(&n_fin, &c->d_next_read->n_fin, sizeof n_fin, hipMemcpyDeviceToHost));
        fprintf(stderr, "[lh] k_smem_fin: %d of %d reads listed\n", (int)n_fin, N);
    }
#endif
    return LH_OK;
}

// the batch's seed total, the reads that asked for a slot of the big slab and pass 2's call counts, on the host (h_peek->k1)
static int peek_seed_total(lh_context* c, int N) {
    LH_LAUNCH(k_peek_k1, 1, 64, c->stream, (const i64*)(c->d_seed_off + N), (const int32_t*)&c->d_big_count->asked, (const P2Calls*)c->d_p2_calls, &c->h_peek->k1.seeds);   // (not a copy-engine transfer: those may be busy with the previous result / the next batch)
    HIPCHK(hipStreamSynchronize(c->stream));
    const u64 dp = (u64)c->h_peek->k1.p2_drop_probed, us = (u64)c->h_peek->k1.p2_unprobed_shares;
    c->p2_cls[0] = (i64)(dp & 0xffffffffu); c->p2_cls[1] = (i64)(dp >> 32); c->p2_cls[2] = (i64)(us & 0xffffffffu); c->p2_cls[3] = (i64)(us >> 32);
    return LH_OK;
}

static inline int ext_long_min(int N);   // (lh_host_stage2.inc)
// K1'S TAIL, what runs between pass 1 and k_smem_fin: the batch's plan.  A choice of path and never of result.
// Pass 2 runs over a list (k_smem4.h: P2TASK).  By default the probe makes it: every re-seeding call judged in lockstep, the calls that can contribute listed one
// by one with the probe's answer, a read with more than LH_P2_SPLIT of them as shares.  LH_F_P2_TASKS: every read with a call as shares, up to LH_P2_SPLIT lanes
// scanning and probing a read's calls themselves (k_p2_tasks; pass 2 45 -> 31 ms on the repeat input, but 4.7 -> 5.4 ms on unique sequence).  LH_F_P2_SCAN: the
// sequence before the probe kernel — the state machine over every read, or k_p2_tasks after a repeat-rich batch (the wave-chained reads of the context's PREVIOUS
// batch, the sign K4 chooses its path by).  (A list needs N < 2^27 and the call entry's four bits of min_intv.)
// Pass 3 in lockstep is the last to touch a read's regular slots and walks them anyway: it counts the read's seeds and lists the few reads that need their
// intervals sorted in memory (k_smem_fin); K2 ranks the others' inside its groups.  Every other path — no pass 3, the state machine's, the lane-per-seed
// K2, the trace build — keeps k_smem_fin over all reads.
// The default, where the probe and the counting pass 3 both run: ONE lockstep kernel behind pass 1 does the probe's work and pass 3's (k_p23_lock: one scan
// of the pass-1 intervals serves both; pass 3's walks need nothing of pass 2), pass 2 then appends behind pass 3's intervals and adds its own counts, and
// k_p2_close ends it.  The bracket "k_smem4_p3" then comes FIRST and holds k_p23_lock — the probe's time with it — and "k_smem4_p2" holds pass 2 and k_p2_close.
// LH_F_P3_LAST keeps the separate sequence: probe, pass 2, clamp, pass 3.
struct K1Tail {
    bool probe;       // k_p2_probe's list (or, fused, k_p23_lock's)
    bool tasks;       // k_p2_tasks' list
    bool list;        // pass 2 runs over one of the two
    bool p3_lock;     // forward-only walks: one thread per read, in lockstep
    bool p3_counts;   // ... which counts the seeds and lists the reads for k_smem_fin
    bool fused;       // k_p23_lock, pass 2, k_p2_close
};
static K1Tail k1_tail_plan(const lh_context* c, const DOpts& o, int N, bool packed_reads) {
    K1Tail t;
    const bool list_ok = N < (1 << 27);
    t.probe = list_ok && !(c->flags & (LH_F_P2_TASKS | LH_F_P2_SCAN)) && o.split_width < LH_P2_MAX_MIN_INTV;
    t.p3_lock = o.max_mem_intv > 0 && packed_reads;
    t.p3_counts = t.p3_lock && !(c->flags & LH_F_SEED_LANE);
#ifdef LH_K1_TRACE   // (the trace build's list-length histograms are the state machine's, and its k_smem_fin runs over all reads)
    t.probe = t.p3_counts = false;
#endif
    t.tasks = list_ok && !t.probe && ((c->flags & LH_F_P2_TASKS) || (c->ext_hint_valid && c->h_peek->prev_wave_reads >= ext_long_min(N)));
    t.list = t.probe || t.tasks;
    t.fused = t.probe && t.p3_counts && !(c->flags & LH_F_P3_LAST);
    return t;
}
static int run_front(lh_context* c, const DOpts& o, int& t) {
    int N = c->b.n_reads;
    const DIndex& ix = c->idx->d;
    HIPCHK(hipMemsetAsync(c->d_ctr, 0, sizeof(DCounters) * LH_CTR_SLOTS, c->stream));
    const uint32_t* q4 = nullptr;
    if (ix.tn) {   // the diagonal scans of K3 / K4 compare eight bases at a time against the 4-bit text
        LH_LAUNCH(k_pack_reads, 4096, 256, c->stream, (const uint8_t*)c->b.seq, c->b.n_bases, c->d_seq4 + 2);
        q4 = c->d_seq4 + 2;
    }
    c->q4 = q4;
    DIndex ix4 = ix;
    if (c->flags & LH_F_NO_SWEEP_FILTER) ix4.bloom1 = ix4.bloom2 = nullptr;   // n_ext then counts every bwt_extend of the reference
    {   // K1: persistent lanes, one launch per pass of mem_collect_intv (k_smem4.h)
        const int g4 = (N + 63) / 64 < c->grid_smem4 ? (N + 63) / 64 : c->grid_smem4;
        HIPCHK(hipMemsetAsync(c->d_next_read, 0, sizeof(K1Counters), c->stream));
        K1Big nobig; nobig.list = nullptr; nobig.count = nullptr; nobig.slot = nullptr; nobig.slab = nullptr; nobig.resume = nullptr;
        K1Big first = nobig; first.list = c->d_k1_todo; first.count = &c->d_next_read->n_todo; first.resume = c->d_k1_resume;
        const int g3 = (N + 63) / 64 < 2 * c->grid_smem4 ? (N + 63) / 64 : 2 * c->grid_smem4;   // pass 3 keeps no interval lists: the slab is not touched
        T_BEGIN("k_smem4");
        // every read's first bwt_smem1a call in lockstep, one thread per read; what it does not settle goes on in the state machine
        LH_LAUNCH(k_smem_first, (N + 255) / 256, 256, c->stream, ix4, o, N, q4, (const i64*)c->b.seq_off, c->d_intv, c->d_n_intv, c->d_status, c->d_k1_resume, c->d_k1_todo, &c->d_next_read->n_todo, c->d_ctr);
#ifdef LH_K1_TRACE
        K1Trace trace;
        { int rc = k1_trace_begin(c, trace, g4); if (rc) return rc; }
#endif
        // the instance whose query staging holds the batch's longest read: the LDS it leaves is the lists' ring (k_smem4.h: LH_K1_QW_SMALL)
        const bool qw_small = c->b.max_len <= 8 * LH_K1_QW_SMALL;
        if (qw_small) smem_pass<1, false, LH_K1_QW_SMALL>(c, ix4, o, N, g4, first);
        else smem_pass<1, false>(c, ix4, o, N, g4, first);
        T_END();
#ifdef LH_K1_TRACE
        { int rc = k1_trace_replay(c, trace, N, g4); if (rc) return rc; }
#endif
        HIPCHK(hipMemsetAsync(c->d_p2_calls, 0, sizeof(P2Calls) * LH_CTR_SLOTS, c->stream));
        const K1Tail tail = k1_tail_plan(c, o, N, q4 != nullptr);
        K1Big p2 = nobig;
        if (tail.list) { p2.list = (const int32_t*)c->d_p2_tasks; p2.count = &c->d_next_read->n_p2_tasks; p2.slot = c->d_k1_todo; }   // (slot: the reads' numbers of pass-1 intervals; pass 1's to-do list is spent)
        if (tail.fused) {
            T_BEGIN("k_smem4_p3");
            LH_LAUNCH(k_p23_lock, (N + 255) / 256, 256, c->stream, ix4, o, N, (const uint8_t*)c->b.seq, q4, (const i64*)c->b.seq_off, c->d_intv, c->d_n_intv, c->d_ctr, c->d_seed_cnt, c->d_p2_tasks,
                      &c->d_next_read->n_p2_tasks, c->d_k1_todo, c->d_p2_calls);
            T_END();
            T_BEGIN("k_smem4_p2");
            p2.p2_cnt = c->d_seed_cnt;
            if (qw_small) smem_pass<2, false, LH_K1_QW_SMALL>(c, ix4, o, N, g4, p2);
            else smem_pass<2, false>(c, ix4, o, N, g4, p2);
            LH_LAUNCH(k_p2_close, (N + 255) / 256, 256, c->stream, N, c->d_n_intv, c->d_status, c->d_seed_cnt, c->d_l_rep, c->d_fin_list, &c->d_next_read->n_fin);
            T_END();
#ifdef LH_P3_KINDS   // a development build's read-out (it waits for the stream): k_smem4.h, lh_p3_kinds
            {
                unsigned long long k[16], zero[16] = {0};
                HIPCHK(hipStreamSynchronize(c->stream));
                HIPCHK(hipMemcpyFromSymbol(k, HIP_SYMBOL(lh_p3_kinds), sizeof k));
                HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_p3_kinds), zero, sizeof zero));
                fprintf(stderr, "[lh] p3_kinds:");
                for (int i = 0; i < 14; ++i) fprintf(stderr, " %llu", k[i]);
                fprintf(stderr, "\n");
            }
#endif
        } else {
            T_BEGIN("k_smem4_p2");
            if (tail.probe)
                LH_LAUNCH(k_p2_probe, (N + 255) / 256, 256, c->stream, ix4, o, N, (const uint8_t*)c->b.seq, (const i64*)c->b.seq_off, (const DIntv*)c->d_intv, (const int32_t*)c->d_n_intv, c->d_p2_tasks,
                          &c->d_next_read->n_p2_tasks, c->d_k1_todo, c->d_p2_calls);
            else if (tail.tasks)
                LH_LAUNCH(k_p2_tasks, (N + 255) / 256, 256, c->stream, o, N, (const DIntv*)c->d_intv, (const int32_t*)c->d_n_intv, c->d_p2_tasks, &c->d_next_read->n_p2_tasks, c->d_k1_todo, c->d_p2_calls);
            if (qw_small) smem_pass<2, false, LH_K1_QW_SMALL>(c, ix4, o, N, g4, p2);
            else smem_pass<2, false>(c, ix4, o, N, g4, p2);
            if (tail.list) LH_LAUNCH(k_p2_clamp, (N + 255) / 256, 256, c->stream, N, c->d_n_intv);
            T_END();
#ifdef LH_K1_TRACE
            { int rc = k1_trace_lens(c, trace); if (rc) return rc; }
#endif
            T_BEGIN("k_smem4_p3");
            if (tail.p3_lock)
                LH_LAUNCH(k_smem_p3_lock, (N + 255) / 256, 256, c->stream, ix4, o, N, q4, (const i64*)c->b.seq_off, c->d_intv, c->d_n_intv, c->d_status, c->d_ctr,
                          tail.p3_counts ? c->d_seed_cnt : nullptr, tail.p3_counts ? c->d_l_rep : nullptr, tail.p3_counts ? c->d_fin_list : nullptr, tail.p3_counts ? &c->d_next_read->n_fin : nullptr);
            else if (o.max_mem_intv > 0)
                smem_pass<3, false>(c, ix4, o, N, g3, nobig);
            T_END();
        }
        T_BEGIN("k_smem_fin");
        // reads whose intervals outgrew their LH_MAX_INTV slots: the three passes again into the big slab (BWA's vectors grow: no read is refused)
        { int rc = k1_big_round(c, o, ix4, N, 0); if (rc) return rc; }
        { int rc = smem_fin(c, o, N, tail.p3_counts); if (rc) return rc; }
        T_END();
    }
    T_BEGIN("k_scan_seeds");
    // ... and with them the region slots of a read, one per seed + the rescue slots: reg_off[i] = seed_off[i] + i * LH_RESCUE_SLOTS
    { int rc = run_scan(c, N, c->d_seed_cnt, 0, 0, c->d_seed_off, c->d_reg_off, LH_RESCUE_SLOTS); if (rc) return rc; }
    T_END();
    {   // the seed pools (and the region pools derived from them) follow the batch: grow them before anything writes there
        { int rc = peek_seed_total(c, N); if (rc) return rc; }
        while (c->h_peek->k1.big_asked > (i64)(c->big_cap - c->big_base)) {
            // more reads asked for a slot of the big slab than it had (a batch of low-complexity reads): the slab grows by what is missing, the
            // reads left out run their second chance into the new slots, and the seed counts are scanned again.  (The loop ends: a round lists
            // every read that is still without a slot.)
            const i64 asked = c->h_peek->k1.big_asked, old_cap = c->big_cap, new_cap = old_cap + asked + asked / 8 + 16;
            if (new_cap > (1 << 30)) return set_err(LH_E_CAPACITY, "too many reads with more than LH_MAX_INTV SMEM intervals for one batch: split the batch");
            DIntv* slab = nullptr; int32_t* list = nullptr;
            DevGroup grown;   // the new slab and list; once they are swapped in, the old ones
            DALLOC(grown, slab, (size_t)new_cap * 2 * LH_BIG_INTV); DALLOC(grown, list, (size_t)new_cap);
            HIPCHK(hipMemcpyAsync(slab, c->d_big_slab, (size_t)old_cap * 2 * LH_BIG_INTV * sizeof(DIntv), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));   // (the slab is copied before the old one is released)
            std::swap(c->d_big_slab, slab); std::swap(c->d_big_list, list);   // (a buffer goes with the variable that holds it: DevGroup)
            grown.release();
            c->big_base = (int)old_cap; c->big_cap = (int)new_cap;
            { int rc = k1_big_round(c, o, ix4, N, c->big_base); if (rc) return rc; }
            { int rc = run_scan(c, N, c->d_seed_cnt, 0, 0, c->d_seed_off, c->d_reg_off, LH_RESCUE_SLOTS); if (rc) return rc; }
            { int rc = peek_seed_total(c, N); if (rc) return rc; }
        }
        c->big_base = 0;
        const i64 total = c->h_peek->k1.seeds;
        if (!c->in_round) c->rounds.total_seeds = total;
        if (total > c->pool_cap || c->co.seed_budget_kb > 0) {
            // the pools follow the batch as far as their budget allows.  What does not fit is aligned in rounds of whole barcodes (align_rounds: this pass is discarded);
            // a stage dump shows one pass over the whole batch, so there it stays a capacity error with its size, never a per-read refusal
            const i64 need = seed_need(c, total);
            i64 budget = 0;
            { int rc = seed_budget(c, &budget); if (rc) return rc; }
            if (!c->in_round) c->rounds.budget = budget;
            if (need > budget) {
                if (!c->dump_stop_after_dedup && !c->in_round) return LH_NEED_ROUNDS;
                return set_err(LH_E_CAPACITY, "the batch has " + std::to_string(total) + " seeds: their workspace (" + std::to_string((long long)(need / 1000000000)) + " GB) does not fit the " +
                                                  std::to_string((long long)(budget / 1000000000)) + " GB of its budget (seed_budget_kb, or the HBM that is free): split the batch");
            }
            if (total > c->pool_cap) {
                int rc = alloc_seed_pools(c, total + total / 4);
                if (rc) return rc;
            }
        }
    }
    T_BEGIN("k_seed");
    if (c->flags & LH_F_SEED_LANE) {   // one lane per seed (the A/B leg)
        int g2 = (int)((i64)N * 8 / 256 + 1); if (g2 > 2048) g2 = 2048;
        LH_LAUNCH(k_seed_owner, (N + 255) / 256 < 8192 ? (N + 255) / 256 : 8192, 256, c->stream, N, (const i64*)c->d_seed_off, c->pool_cap, c->d_s_next);   // d_s_next is K3's: free until then
        LH_LAUNCH(k_seed, g2, 256, c->stream, ix, o, N, c->d_seed_off, c->pool_cap, c->d_intv, c->d_n_intv, c->d_seeds, c->d_s_rid, c->d_ctr, (const int32_t*)c->d_s_next, (const int32_t*)c->d_big_slot, (const DIntv*)c->d_big_slab);
    } else {   // a 16-lane group per read, four reads to a wave
        const int items = (N + 3) / 4;
        LH_LAUNCH(k_seed_grp, items < LH_K2_GRID ? items : LH_K2_GRID, 64, c->stream, ix, o, N, (const i64*)c->d_seed_off, c->pool_cap, (const DIntv*)c->d_intv, (const int32_t*)c->d_n_intv, c->d_seeds, c->d_s_rid, c->d_ctr,
                  (const int32_t*)c->d_big_slot, (const DIntv*)c->d_big_slab);
    }
    T_END();
    T_BEGIN("k_chain");
    HIPCHK(hipMemsetAsync(c->d_ext_jobs, 0, sizeof(DExtJobs), c->stream));
    {
        ExtArgs A = ext_args(c);
        const int fuse = (c->flags & LH_F_EXT_WAVE) ? 0 : 1;
        // reads with few seeds and chains: chained by a lane, which then starts their extension (round 0 of K4); the others are listed for the wave kernels
        LH_LAUNCH(k_chain_lane, (N + 63) / 64, 64, c->stream, ix, o, N, c->pool_cap, c->d_seeds, c->d_s_rid, c->d_l_rep, c->d_chains, c->d_cseeds, c->d_n_chains, c->d_status,
                  c->d_aln_r, c->d_ext_jobs->wave_range + 1, c->d_srt, c->d_chain_rmax, c->d_ctr, A, fuse, c->d_ext_jobs->count + 1, c->d_ext_jlist, c->d_ext_jkey,
                  c->d_ext_jobs->heavy_range + 1, c->d_ext_heavy);
        // the listed reads: chained cluster by cluster (k_chain_cl.h: three instances by seed count); what those leave — a cluster too large for a lane, more
        // seeds than the larger instance holds — by the wave-per-seed kernel, which takes any read (d_aln_ci, K7's list, is free until then)
        const int32_t* wlist = c->d_aln_r;
        const int32_t* wcount = c->d_ext_jobs->wave_range + 1;
        if (!(c->flags & LH_F_CHAIN_WAVE)) {
            int32_t* const fb_count = &c->d_aln_count->full;   // (K7's counter: free until then)
            HIPCHK(hipMemsetAsync(fb_count, 0, sizeof(int32_t), c->stream));
            // (r06) the three instances take disjoint reads of the list (by seed count) and share nothing but the list of what they leave: side by side on three streams
            // (mixed input: 22.0 -> 20.5 ms; each instance alone already holds most of the waves its LDS use allows)
#define LH_K3_CL(CAP_, GRID_, LO_, LAST_, ST_)                                                                                                                         \
            LH_LAUNCH((k_chain_cl<CAP_>), N < (GRID_) ? N : (GRID_), 64, ST_, ix, o, (const i64*)c->b.seq_off, (const i64*)c->d_seed_off, c->pool_cap, (const DSeed*)c->d_seeds, \
                      (const int32_t*)c->d_s_rid, (const int32_t*)c->d_l_rep, c->d_chains, c->d_cseeds, c->d_n_chains, c->d_status, wlist, wcount, LO_, LAST_, c->d_aln_ci, fb_count)
            HIPCHK(hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0)); HIPCHK(hipStreamWaitEvent(c->aux[2], c->ev_fork, 0));
            LH_K3_CL(LH_CHAIN_CL_CAP_C, 2048, LH_CHAIN_CL_CAP_B, 1, c->aux[2]);
            LH_K3_CL(LH_CHAIN_CL_CAP_B, 8192, LH_CHAIN_CL_CAP_A, 0, c->aux[1]);
            LH_K3_CL(LH_CHAIN_CL_CAP_A, 16384, 0, 0, c->stream);
            HIPCHK(hipEventRecord(c->ev_join[1], c->aux[1])); HIPCHK(hipEventRecord(c->ev_join[2], c->aux[2]));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[1], 0)); HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[2], 0));
#undef LH_K3_CL
            wlist = c->d_aln_ci; wcount = fb_count;
#ifdef LH_RFA_PROF
            { int rc = prof_chain_cl(c); if (rc) return rc; }
#endif
            if (lh_debug_sync()) {
                int32_t nl = 0, nf = 0;
                if (hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(&nl, c->d_ext_jobs->wave_range + 1, 4, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(&nf, fb_count, 4, hipMemcpyDeviceToHost) == hipSuccess)
                    fprintf(stderr, "[lh] K3: %d reads listed for the wave kernels, %d of them left to k_chain by k_chain_cl\n", nl, nf);
            }
        }
        LH_LAUNCH(k_chain, N < 16384 ? N : 16384, 64, c->stream, ix, o, N, c->b.seq_off, c->d_seed_off, c->pool_cap, c->d_seeds, c->d_s_rid, c->d_l_rep, c->d_s_next, c->d_ct,
                  c->d_ord, c->d_srt, c->d_chains, c->d_cseeds, c->d_n_chains, c->d_status, wlist, wcount);
    }
    T_END();
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ rounds
// the plan's prefix array for n_bc barcodes and, with view, the buffers of a part as a batch of its own (at most the whole batch); the plan block for as many cuts
static int round_mem_for(lh_context* c, int n_bc, bool view, i64 n_reads, i64 n_bases) {
    RoundBufs& rb = c->rb;
    if (n_bc > rb.cap_bc || (view && (n_reads > rb.cap_reads || n_bases > rb.cap_bases))) {
        HIPCHK(hipStreamSynchronize(c->stream));
        c->round_mem.release();
        const bool v = view || rb.cap_reads > 0;
        const i64 cb = n_bc > rb.cap_bc ? n_bc : rb.cap_bc, cr = !v ? 0 : n_reads > rb.cap_reads ? n_reads : rb.cap_reads, cs = !v ? 0 : n_bases > rb.cap_bases ? n_bases : rb.cap_bases;
        rb = RoundBufs();
        DevGroup& g = c->round_mem;
        DALLOC(g, rb.prefix, cb + 1);
        if (v) { DALLOC(g, rb.v_bc_pair_off, cb + 1); DALLOC(g, rb.v_seq_off, cr + 1); DALLOC(g, rb.v_seq, cs / 8 + 8); }
        rb.cap_bc = cb; rb.cap_reads = cr; rb.cap_bases = cs;
    }
    if (n_bc > c->plan.cap_rounds) {
        if (c->plan.p) { HIPCHK(hipStreamSynchronize(c->stream)); hipHostFree(c->plan.p); }
        c->plan = RoundPlanBlock();
        HIPCHK(hipHostMalloc((void**)&c->plan.p, RoundPlanBlock::bytes(n_bc), hipHostMallocDefault));
        c->plan.cap_rounds = n_bc;
    }
    return LH_OK;
}
// the selected batch's seeds (d_seed_off: k_scan_seeds has run) cut into parts within `budget`: the plan in c->plan once the stream is synchronised
static int round_plan(lh_context* c, i64 budget, bool view) {
    { int rc = round_mem_for(c, c->b.n_bc, view, c->b.n_reads, c->b.n_bases); if (rc) return rc; }
    LH_LAUNCH(k_round_cost, (c->b.n_bc + 256) / 256, 256, c->stream, c->b.n_bc, (const int32_t*)c->b.bc_pair_off, (const i64*)c->d_seed_off, c->rb.prefix);
    LH_LAUNCH(k_round_plan, 1, 64, c->stream, c->b.n_bc, (const i64*)c->rb.prefix, (const int32_t*)c->b.bc_pair_off, (const i64*)c->b.seq_off, budget, seed_fixed_slots(c),
              LH_SEED_POOL_BYTES, (int)c->plan.cap_rounds, c->plan.hdr(), c->plan.cut_bc(), c->plan.cut_pair(), c->plan.cut_base(), c->plan.part_seeds(), c->d_wd);
    return LH_OK;
}

// Part r of the plan as a batch of its own, once k_batch_view has filled the round buffers: its reads and its barcodes' pair offsets are the buffers' copies
// (they begin at 0), its name seeds and inference flags the whole batch's from the part's first pair and barcode on.  What is per contig or chooses a kernel instance
// it inherits from the whole batch: has_cen and the centromere arrays, and max_len — K1's query-staging instance stays the one the whole batch chose
static BatchView part_view(const BatchView& whole, const RoundBufs& rb, const RoundPlanBlock& P, i64 r) {
    const i64 b0 = P.cut_bc()[r], p0 = P.cut_pair()[r];
    BatchView v = whole;
    v.seq = (uint8_t*)rb.v_seq; v.seq_off = rb.v_seq_off; v.bc_pair_off = rb.v_bc_pair_off;
    v.name_seed = whole.name_seed + p0; v.bc_do_rfa = whole.bc_do_rfa + b0;
    v.n_bc = (int)(P.cut_bc()[r + 1] - b0); v.n_pairs = (int)(P.cut_pair()[r + 1] - p0); v.n_reads = 2 * v.n_pairs; v.n_bases = P.cut_base()[r + 1] - P.cut_base()[r];
    return v;
}

// an error return may come between a fork onto an auxiliary stream (K3's cluster kernels, K4's wave kernels beside the rounds, K6's long-list replay, K8's prologue beside K7 and its routed
// barcodes) and its join: nothing of the call may still be running on the context's buffers when the caller frees or reuses them
static void quiesce(lh_context* c) {
    for (int i = 0; i < 3; ++i) hipStreamSynchronize(c->aux[i]);
    hipStreamSynchronize(c->stream);
}

static int merge_results(lh_result* a, lh_result* b, lh_result** out);   // (lh_lanes.inc)
static int merge_into(lh_result*& acc, lh_result* part);                 // (lh_lanes.inc)
static int pipe_download(lh_context* c, lh_result** out);                // (lh_host_stage2.inc)
struct TimeSums {   // per-kernel times summed over the rounds, in the order of their first appearance
    const char* names[LH_NSTAGE]; float ms[LH_NSTAGE]; int n = 0;
    void add(const char* name, float v) {
        int i = 0;
        while (i < n && strcmp(names[i], name)) ++i;
        if (i == n) { if (n == LH_NSTAGE) return; names[n] = name; ms[n] = 0; ++n; }
        ms[i] += v;
    }
};
// the times of the t entries just run (the stream is synchronised)
static int add_times(lh_context* c, int t, TimeSums& sums, const char* as_one) {
    for (int i = 0; i < t; ++i) {
        float v = 0;
        HIPCHK(hipEventElapsedTime(&v, c->ev[i], c->ev[i + 1]));
        sums.add(as_one ? as_one : c->tnames[i], v);
    }
    return LH_OK;
}

// The selected batch does not fit its seed budget as a whole: align it part by part.  The K1 pass that found out is discarded (re-running K1 per part costs that one
// pass in the overflow case and nothing otherwise); every part is a batch view (k_batch_view) that runs the unchanged kernel sequence and downloads, and the parts'
// results are merged column by column as the lanes' are (merge_results) before the next part's kernels reuse the result arrays.  t: the discarded pass's entries.
static int align_rounds(lh_context* c, const DOpts& o, int t) {
    TimeSums sums;
    HIPCHK(hipEventRecord(c->ev[t], c->stream));
    const i64 total = c->rounds.total_seeds;
    // the view's buffers take HBM too: with the budget read from the free memory, plan after they exist
    { int rc = round_mem_for(c, c->b.n_bc, true, c->b.n_reads, c->b.n_bases); if (rc) return rc; }
    i64 budget = 0;
    { int rc = seed_budget(c, &budget); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->ev[LH_NSTAGE - 1], c->stream));
    { int rc = round_plan(c, budget, true); if (rc) return rc; }
    HIPCHK(hipEventRecord(c->ev[LH_NSTAGE], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    { int rc = add_times(c, t, sums, "k1_discarded"); if (rc) return rc; }
    { float v = 0; HIPCHK(hipEventElapsedTime(&v, c->ev[LH_NSTAGE - 1], c->ev[LH_NSTAGE])); sums.add("k_round_plan", v); }
    const RoundPlanBlock& P = c->plan;
    RoundState& R = c->rounds;
    R.budget = budget; R.have_max = true; R.max_bc = P.hdr()->max_barcode; R.max_bc_seeds = P.hdr()->max_barcode_seeds;
    const i64 n_rounds = P.hdr()->n_rounds;
    if (n_rounds == 0)
        return set_err(LH_E_CAPACITY, "barcode " + std::to_string(R.max_bc) + " has " + std::to_string(R.max_bc_seeds) + " seeds: their workspace (" + std::to_string(seed_need(c, R.max_bc_seeds)) +
                                          " bytes) does not fit the budget of " + std::to_string(budget) + " bytes (seed_budget_kb, or the HBM that is free), and a barcode is never split");
    bool ok = n_rounds > 0 && n_rounds <= c->b.n_bc && P.hdr()->total_seeds == total && P.cut_bc()[0] == 0 && P.cut_bc()[n_rounds] == c->b.n_bc && P.cut_pair()[n_rounds] == c->b.n_pairs &&
              P.cut_base()[n_rounds] == c->b.n_bases;
    for (i64 r = 0; ok && r < n_rounds; ++r)
        ok = P.cut_bc()[r] < P.cut_bc()[r + 1] && P.cut_pair()[r] < P.cut_pair()[r + 1] && P.cut_base()[r] <= P.cut_base()[r + 1] && seed_need(c, P.part_seeds()[r]) <= budget;
    if (!ok) return set_err(LH_E_HIP, "the round plan is inconsistent (k_round_plan, watchdog slot " + std::to_string(LH_WD_ROUND_PLAN) + ")");
    R.first_bc.assign(P.cut_bc(), P.cut_bc() + n_rounds + 1);
    R.seeds.assign(P.part_seeds(), P.part_seeds() + n_rounds);
    R.need.clear();
    for (i64 s : R.seeds) R.need.push_back(seed_need(c, s));
    // a download the host began for the PREVIOUS batch and has not collected: its copies must have ended before a part's download reuses the copy stream's event;
    // it stays pending for the host while the parts' downloads come and go
    const bool host_pending = c->dl_pending;
    std::function<int(lh_result**)> host_finish;
    if (host_pending) { HIPCHK(hipEventSynchronize(c->ev_dl)); host_finish = std::move(c->dl_finish); c->dl_pending = false; }
    const BatchView whole = c->b;
    struct Restore {   // the batch's own selection and the host's pending download, back in place however this ends
        lh_context* c; const BatchView& whole; bool pending; std::function<int(lh_result**)>& finish;
        ~Restore() {
            c->b = whole; c->in_round = false;
            if (pending) { c->dl_pending = true; c->dl_finish = std::move(finish); }
        }
    } restore{c, whole, host_pending, host_finish};
    c->in_round = true;
    lh_result* acc = nullptr;
    for (i64 r = 0; r < n_rounds; ++r) {
        const int b0 = (int)P.cut_bc()[r], p0 = (int)P.cut_pair()[r];
        const i64 s0 = P.cut_base()[r];
        const BatchView part = part_view(whole, c->rb, P, r);
        int rt = 0;
        HIPCHK(hipEventRecord(c->ev[LH_NSTAGE - 1], c->stream));
        {
            const i64 work = part.n_bases / 8 > part.n_reads ? part.n_bases / 8 : part.n_reads;
            LH_LAUNCH(k_batch_view, (int)(work / 256 + 1 < 4096 ? work / 256 + 1 : 4096), 256, c->stream, part.n_bc, part.n_reads, part.n_bases, b0, p0, s0, (const int32_t*)whole.bc_pair_off,
                      (const i64*)whole.seq_off, (const uint8_t*)whole.seq, c->rb.v_bc_pair_off, c->rb.v_seq_off, c->rb.v_seq);
        }
        HIPCHK(hipEventRecord(c->ev[LH_NSTAGE], c->stream));
        c->b = part;
        int rc = run_front(c, o, rt);
        if (!rc) rc = stage2_run(c, o, rt);
        lh_result* res = nullptr;
        if (!rc) {
            hipError_t e = hipEventRecord(c->ev[rt], c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = set_err(LH_E_HIP, std::string("round ") + std::to_string(r) + ": " + hipGetErrorString(e));
        }
        if (!rc) rc = add_times(c, rt, sums, nullptr);
        if (!rc) { float v = 0; hipEventElapsedTime(&v, c->ev[LH_NSTAGE - 1], c->ev[LH_NSTAGE]); sums.add("k_batch_view", v); }
        if (!rc) {
            c->ran = true;
            rc = pipe_download(c, &res);   // (the watchdog slots are read and cleared with every part's result)
            c->ran = false;
            if (rc) rc = set_err(rc, "round " + std::to_string(r) + " of " + std::to_string(n_rounds) + " (its reads start at read " + std::to_string(2 * (i64)p0) + " of the batch): " + g_err);
        }
        if (!rc) rc = merge_into(acc, res);
        if (rc) {
            const std::string why = g_err;
            quiesce(c);
            if (acc) lh_result_free(acc);
            return set_err(rc, why);
        }
    }
    c->round_result = acc;
    R.n_rounds = (int)n_rounds;
    c->n_t = sums.n;
    for (int i = 0; i < sums.n; ++i) { c->tnames[i] = sums.names[i]; c->tms[i] = sums.ms[i]; }
    return LH_OK;
}

static int pipe_align(lh_context* c, const lh_opts* opts) {
    if (!c || !opts) return set_err(LH_E_ARG, "lh_align_resident: null argument");
    if (!c->resident) return set_err(LH_E_ARG, "no batch resident: call lh_batch_upload first");
    if (opts->abi_version != LH_ABI_VERSION) return set_err(LH_E_ARG, "lh_opts.abi_version does not match LH_ABI_VERSION (use lh_opts_init)");
    if (opts->flags & ~(LH_F_NO_SWEEP_FILTER | LH_F_EXT_WAVE | LH_F_EXT_SERIAL | LH_F_CHAIN_WAVE | LH_F_P2_TASKS | LH_F_RESCUE_FULL | LH_F_SEED_LANE | LH_F_TAIL_PASSES | LH_F_RFA_SLAB | LH_F_P2_SCAN | LH_F_P3_LAST)) return set_err(LH_E_ARG, "lh_opts.flags: unknown bit set");
    HIPCHK(hipSetDevice(c->idx->device));
    {
        std::vector<void*> fl;
        { std::lock_guard<std::mutex> g(c->slot_mu); fl.swap(c->free_later); }
        for (void* q : fl) hipFree(q);
    }
    if (c->round_result) { lh_result_free(c->round_result); c->round_result = nullptr; }   // (an earlier batch's, never downloaded)
    c->rounds.clear();
    c->ran = false;
    // a regrow that failed in an earlier call left the context without that group's buffers (capacity 0): start again with the sizes of a new context
    if (!c->pool_cap) { int rc = alloc_seed_pools(c, first_pool_cap(c)); if (rc) return rc; }
    if (!c->cand_cap) { int rc = alloc_cand_pools(c, first_cand_cap(c)); if (rc) return rc; }
    DOpts o = to_dopts(opts);
    o.wd = c->d_wd;
    c->flags = opts->flags;
    int t = 0;
    int rc = run_front(c, o, t);
    const bool in_rounds = rc == LH_NEED_ROUNDS;
    if (in_rounds) rc = align_rounds(c, o, t);
    else if (!rc) rc = stage2_run(c, o, t);
    if (rc) { quiesce(c); return rc; }
    if (!in_rounds) {
        HIPCHK(hipEventRecord(c->ev[t], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipGetLastError());
        c->n_t = t;
        for (int i = 0; i < t; ++i) HIPCHK(hipEventElapsedTime(&c->tms[i], c->ev[i], c->ev[i + 1]));
        c->rounds.n_rounds = 1;
    }
    c->ran = true;
    return LH_OK;
}

int lh_last_timings(lh_context* c, int32_t* n, const char* const** names, const float** ms) {
    if (!c) return set_err(LH_E_ARG, "null context");
    if (n) *n = c->n_t;
    if (names) *names = c->tnames;
    if (ms) *ms = c->tms;
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ stage dump
struct DumpArenaH {
    lh_stage_dump d;
    std::vector<i64> intv_off, seed_off, seed_rbeg, chain_off, chain_pos, reg_off, reg_rb, reg_re;
    std::vector<u64> intv;
    std::vector<int32_t> seed_qbeg, seed_len, seed_rid, chain_nseeds, chain_rid, chain_w, chain_kept, reg_qb, reg_qe, reg_rid, reg_score, reg_truesc,
        reg_w, reg_seedcov, reg_seedlen0, reg_csub, reg_secondary;
};

template <class T> static int d2h(std::vector<T>& v, const T* d, size_t n) {
    v.resize(n);
    if (n && hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return set_err(LH_E_HIP, "hipMemcpy D2H failed");
    return LH_OK;
}
#define D2H(v, d, n) do { int rc_ = d2h(v, d, (size_t)(n)); if (rc_) return rc_; } while (0)

static int stage2_dump_regs(lh_context* c, DumpArenaH* A);
static bool lanes_split(const lh_context* c);   // (lh_lanes.inc)

int lh_stage_dump_resident(lh_context* c, const lh_opts* opts, lh_stage_dump** out) {
    if (!c || !opts || !out) return set_err(LH_E_ARG, "lh_stage_dump_resident: null argument");
    std::lock_guard<std::mutex> res_lock(c->res_mu);   // (the dump reruns the front half over the result arrays: as lh_align_resident, not under lh_bam_append_resident's gather)
    {   // the dump shows mem_align1_core's output, i.e. BEFORE mate rescue: rerun the front half only
        if (lanes_split(c))
            return set_err(LH_E_ARG, "lh_stage_dump_resident: the resident batch is split over several lanes (create the context with lanes = 1 for stage dumps)");
        c->dump_stop_after_dedup = true;
        int rc = pipe_align(c, opts);
        c->dump_stop_after_dedup = false;
        c->ran = false;
        if (rc) return rc;
    }
    int N = c->b.n_reads;
    DumpArenaH* A = new DumpArenaH();
    std::vector<int32_t> n_intv, n_chains, s_rid, status;
    std::vector<DIntv> intv;
    std::vector<i64> seed_off;
    std::vector<DSeed> seeds;
    std::vector<DChain> chains;
    K1Big big; big.list = c->d_big_list; big.count = &c->d_big_count->listed; big.slot = c->d_big_slot; big.slab = c->d_big_slab; big.resume = nullptr;
    {   // the dump shows a read's intervals sorted; the default path leaves that to K2's groups.  Seeds and chains are that path's: this sorts for the display only (and writes the same counts again)
        DOpts o = to_dopts(opts);
        o.wd = c->d_wd;
        int rc = smem_fin(c, o, N, false);
        if (rc) return rc;
    }
    LH_LAUNCH(k_intv_rows, (N + 255) / 256, 256, c->stream, c->idx->d, N, c->d_intv, (const int32_t*)c->d_n_intv, big);   // K1 stores unique intervals by text position: the dump shows rows, like bwt_smem1a
    HIPCHK(hipStreamSynchronize(c->stream));
    D2H(n_intv, c->d_n_intv, N); D2H(intv, c->d_intv, (size_t)N * LH_MAX_INTV); D2H(seed_off, c->d_seed_off, N + 1); D2H(status, c->d_status, N);
    i64 tot = seed_off[N] < c->pool_cap ? seed_off[N] : c->pool_cap;
    D2H(seeds, c->d_seeds, tot); D2H(s_rid, c->d_s_rid, tot); D2H(n_chains, c->d_n_chains, N); D2H(chains, c->d_chains, tot);
    for (int r = 0; r < N; ++r)
        if (status[r] & (LH_ST_INTV_OVERFLOW | LH_ST_POOL_OVERFLOW)) { delete A; return set_err(LH_E_CAPACITY, "workspace overflow in the front end"); }
    A->intv_off.push_back(0); A->seed_off.push_back(0); A->chain_off.push_back(0);
    std::vector<int32_t> big_slot;
    std::vector<DIntv> big_slab;
    D2H(big_slot, c->d_big_slot, N);
    { bool any = false; for (int r = 0; r < N; ++r) any = any || big_slot[r] >= 0; if (any) D2H(big_slab, c->d_big_slab, (size_t)c->big_cap * 2 * LH_BIG_INTV); }
    for (int r = 0; r < N; ++r) {
        for (int t = 0; t < n_intv[r]; ++t) {
            const DIntv& p = big_slot[r] >= 0 ? big_slab[((size_t)big_slot[r] * 2 + 1) * LH_BIG_INTV + t] : intv[(size_t)r * LH_MAX_INTV + t];
            A->intv.push_back(p.x0); A->intv.push_back(p.x1); A->intv.push_back(p.x2); A->intv.push_back(p.info);
        }
        A->intv_off.push_back((i64)A->intv.size() / 4);
        for (i64 s = seed_off[r]; s < seed_off[r + 1]; ++s) {
            A->seed_rbeg.push_back(seeds[s].rbeg); A->seed_qbeg.push_back(seeds[s].qbeg); A->seed_len.push_back(seeds[s].len); A->seed_rid.push_back(s_rid[s]);
        }
        A->seed_off.push_back((i64)A->seed_rbeg.size());
        for (int k = 0; k < n_chains[r]; ++k) {
            const DChain& ch = chains[seed_off[r] + k];
            A->chain_nseeds.push_back(ch.n); A->chain_rid.push_back(ch.rid); A->chain_w.push_back(ch.w); A->chain_kept.push_back(ch.kept); A->chain_pos.push_back(ch.pos);
        }
        A->chain_off.push_back((i64)A->chain_rid.size());
    }
    A->reg_off.assign(N + 1, 0);
    { int rc = stage2_dump_regs(c, A); if (rc) { delete A; return rc; } }
    lh_stage_dump& d = A->d;
    memset(&d, 0, sizeof d);
    d.n_reads = N;
    d.intv_off = A->intv_off.data(); d.intv = (const uint64_t*)A->intv.data();
    d.seed_off = A->seed_off.data(); d.seed_rbeg = A->seed_rbeg.data(); d.seed_qbeg = A->seed_qbeg.data(); d.seed_len = A->seed_len.data(); d.seed_rid = A->seed_rid.data();
    d.chain_off = A->chain_off.data(); d.chain_nseeds = A->chain_nseeds.data(); d.chain_rid = A->chain_rid.data(); d.chain_w = A->chain_w.data();
    d.chain_kept = A->chain_kept.data(); d.chain_pos = A->chain_pos.data();
    d.reg_off = A->reg_off.data(); d.reg_rb = A->reg_rb.data(); d.reg_re = A->reg_re.data(); d.reg_qb = A->reg_qb.data(); d.reg_qe = A->reg_qe.data();
    d.reg_rid = A->reg_rid.data(); d.reg_score = A->reg_score.data(); d.reg_truesc = A->reg_truesc.data(); d.reg_w = A->reg_w.data();
    d.reg_seedcov = A->reg_seedcov.data(); d.reg_seedlen0 = A->reg_seedlen0.data(); d.reg_csub = A->reg_csub.data(); d.reg_secondary = A->reg_secondary.data();
    d.arena_ = A;
    *out = &A->d;
    return LH_OK;
}
void lh_stage_dump_free(lh_stage_dump* d) { if (d) delete (DumpArenaH*)d->arena_; }

#include "lh_host_stage2.inc"

#include "lh_lanes.inc"

#include "lh_bgzf.inc"   // the device compressor of BGZF members (lh_bgzf_*), an object of its own
#include "lh_brec.inc"   // the device encoder of BAM records (lh_bam_set_device_records), on the compressor's device
