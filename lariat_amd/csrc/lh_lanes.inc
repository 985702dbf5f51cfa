// lh_lanes.inc — the public context entry points over one or two pipelines ("lanes").
//
// A pipeline (struct lh_context, lh_host.inc / lh_host_stage2.inc) runs the kernel sequence K1..K8 for one resident batch on
// its own streams and workspaces.  Kernels are launched back to back; each leaves the GPU partly idle while its last waves
// finish, and a register-bound kernel (K1) cannot share a CU with more of itself but can with a kernel of another stage.
// With lh_context_opts.lanes = L > 1 the context owns L - 1 further, smaller pipelines: every batch is cut at the barcode
// boundaries nearest to k / L of its pairs — barcodes are independent work units (lariat.go:461-547) — and the parts are
// aligned side by side from L host threads; the results are merged into one lh_result (candidate indices of the later parts
// shifted).  Nothing else changes: same kernels, same per-barcode arithmetic, same results as with one lane.
#include <atomic>
#include <thread>

#define LH_MAX_LANES 4

int lh_context_create(lh_index* idx, int64_t max_pairs, const lh_context_opts* co, lh_context** out) {
    const int lanes = co && co->lanes ? co->lanes : 1;
    if (lanes < 1 || lanes > LH_MAX_LANES) return set_err(LH_E_ARG, "lh_context_opts.lanes must be 1 .. 4");
    lh_context* c = nullptr;
    int rc = pipe_create(idx, max_pairs, co, &c);
    if (rc) return rc;
    for (int k = 1; k < lanes && max_pairs >= 2 * lanes; ++k) {
        lh_context_opts c2 = *co;
        c2.lanes = 1;
        {   // a further lane takes its share of a batch's barcodes: its share of K8's waves (and slabs) too
            const int g = (c2.rfa_grid > 0 ? c2.rfa_grid : 4096) / lanes;
            c2.rfa_grid = g > 1024 ? g : 1024;
        }
        // a part is at most its share of the pairs plus one barcode; the reader caps a barcode at 30,000 pairs (reader.go:205): batches
        // with larger work units simply stay on the first lane
        int64_t cap = max_pairs / lanes + 30000 < max_pairs ? max_pairs / lanes + 30000 : max_pairs;
        lh_context* p = nullptr;
        rc = pipe_create(idx, cap, &c2, &p);
        if (rc) { lh_context_free(c); return rc; }
        c->more.push_back(p);
    }
    *out = c;
    return LH_OK;
}

void lh_context_free(lh_context* c) {
    if (!c) return;
    for (lh_context* p : c->more) pipe_free(p);
    pipe_free(c);
}

int lh_batch_upload_slot(lh_context* c, int32_t slot, const lh_batch* b) {
    if (!c || !b) return set_err(LH_E_ARG, "lh_batch_upload: null argument");
    if (slot < 0 || slot > 4096) return set_err(LH_E_ARG, "lh_batch_upload_slot: slot out of range");
    if ((size_t)slot >= c->slot_cut.size()) c->slot_cut.resize((size_t)slot + 1);
    c->slot_cut[(size_t)slot].clear();
    c->cur_slot = slot;
    const int L = 1 + (int)c->more.size();
    std::vector<int32_t> cut;   // first barcode of lanes 2 .. L
    if (L > 1 && b->bc_pair_off && b->seq_off && b->n_barcodes >= L && b->n_pairs >= L && b->bc_pair_off[0] == 0 && b->bc_pair_off[b->n_barcodes] == b->n_pairs) {
        const int32_t* off = b->bc_pair_off;
        bool ok = true;
        for (int32_t k = 0; ok && k < b->n_barcodes; ++k) ok = off[k + 1] >= off[k];   // let the pipeline report a malformed batch
        for (int k = 1; ok && k < L; ++k) {   // the barcode boundary nearest to k / L of the pairs
            const int64_t want = (int64_t)b->n_pairs * k / L;
            int32_t lo = 1, hi = b->n_barcodes - 1;
            while (lo < hi) { int32_t m = (lo + hi) >> 1; if (off[m] < want) lo = m + 1; else hi = m; }
            int32_t at = lo;
            if (at > 1 && want - off[at - 1] < off[at] - want) --at;
            if (!cut.empty() && at <= cut.back()) at = cut.back() + 1;
            if (at >= b->n_barcodes) { ok = false; break; }
            cut.push_back(at);
        }
        for (int k = 1; ok && k < L; ++k) {   // every part non-empty and within its lane's capacity
            const int32_t b0 = cut[(size_t)k - 1], b1 = k + 1 < L ? cut[(size_t)k] : b->n_barcodes;
            if (off[b1] - off[b0] <= 0 || off[b1] - off[b0] > c->more[(size_t)k - 1]->cap_pairs || b1 - b0 > c->more[(size_t)k - 1]->cap_bc) ok = false;   // (empty barcodes count against cap_bc)
        }
        if (ok && off[cut[0]] <= 0) ok = false;
        if (!ok) cut.clear();
    }
    if (cut.empty()) return pipe_upload_slot(c, slot, b, false);
    for (int k = 0; k < L; ++k) {
        const int32_t b0 = k ? cut[(size_t)k - 1] : 0, b1 = k + 1 < L ? cut[(size_t)k] : b->n_barcodes;
        const int32_t p0 = b->bc_pair_off[b0], p1 = b->bc_pair_off[b1];
        lh_batch part = *b;
        part.n_barcodes = b1 - b0; part.n_pairs = p1 - p0;
        std::vector<int32_t> off1((size_t)part.n_barcodes + 1);
        for (int32_t q = 0; q <= part.n_barcodes; ++q) off1[(size_t)q] = b->bc_pair_off[b0 + q] - p0;
        const int64_t s0 = b->seq_off[2 * (int64_t)p0];
        std::vector<int64_t> so1((size_t)(2 * (int64_t)part.n_pairs + 1));
        for (size_t q = 0; q < so1.size(); ++q) so1[q] = b->seq_off[2 * (int64_t)p0 + (int64_t)q] - s0;
        part.bc_pair_off = off1.data();
        part.bc_do_rfa = b->bc_do_rfa ? b->bc_do_rfa + b0 : nullptr;
        part.seq_off = so1.data();
        part.seq = b->seq + s0;
        part.name_seed = b->name_seed ? b->name_seed + p0 : nullptr;
        int rc = pipe_upload_slot(k ? c->more[(size_t)k - 1] : c, slot, &part, false);
        if (rc) {   // no lane may keep a part of a batch that is not resident as a whole: the slot is empty again everywhere
            const std::string why = g_err;
            for (int q = 0; q < L; ++q) {
                lh_context* p = q ? c->more[(size_t)q - 1] : c;
                if ((size_t)slot < p->slots.size()) p->slots[(size_t)slot].filled = false;
                p->resident = false; p->ran = false;
            }
            return set_err(rc, why);
        }
    }
    c->slot_cut[(size_t)slot] = cut;   // committed only now: the split exists in every lane
    return LH_OK;
}

int lh_batch_upload(lh_context* c, const lh_batch* b) { return lh_batch_upload_slot(c, 0, b); }

static bool lanes_split(const lh_context* c) {
    return !c->more.empty() && (size_t)c->cur_slot < c->slot_cut.size() && !c->slot_cut[(size_t)c->cur_slot].empty();
}

int lh_batch_select(lh_context* c, int32_t slot) {
    if (!c) return set_err(LH_E_ARG, "lh_batch_select: null context");
    int rc = pipe_select(c, slot);
    if (rc) return rc;
    c->cur_slot = slot;
    if (lanes_split(c))
        for (lh_context* p : c->more) { rc = pipe_select(p, slot); if (rc) return rc; }
    return LH_OK;
}

int lh_align_resident(lh_context* c, const lh_opts* opts) {
    if (!c || !opts) return set_err(LH_E_ARG, "lh_align_resident: null argument");
    std::lock_guard<std::mutex> res_lock(c->res_mu);   // (lh_bam_append_resident's gather may still be reading the previous result)
    if (!lanes_split(c)) {
        for (lh_context* p : c->more) p->rounds.clear();   // (lh_last_rounds: they took no part)
        return pipe_align(c, opts);
    }
    const size_t M = c->more.size();
    std::vector<int> rcs(M, LH_OK);
    std::vector<std::string> errs(M);
    std::vector<std::thread> th;
    for (size_t k = 0; k < M; ++k) th.emplace_back([&, k]() { rcs[k] = pipe_align(c->more[k], opts); if (rcs[k]) errs[k] = g_err; });   // g_err is per thread
    int rc = pipe_align(c, opts);
    for (auto& t : th) t.join();
    if (rc) return rc;
    for (size_t k = 0; k < M; ++k) if (rcs[k]) return set_err(rcs[k], errs[k]);
    return LH_OK;
}

// How a lane ran the last lh_align_resident (rounds live inside a pipeline: every lane plans its own part against its own budget).  Barcode indices are the
// batch's.  For a part that ran whole, the barcode with the most seeds is asked of the device here (the seed offsets of the run are still there), not in the run.
int lh_last_rounds(lh_context* c, int32_t lane, lh_round_info* out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_last_rounds: null argument");
    if (lane < 0 || lane > (int32_t)c->more.size()) return set_err(LH_E_ARG, "lh_last_rounds: no such lane");
    lh_context* p = lane ? c->more[(size_t)lane - 1] : c;
    RoundState& R = p->rounds;
    memset(out, 0, sizeof *out);
    if (R.n_rounds == 0) {
        if (lane == 0 || !c->ran) return set_err(LH_E_ARG, "lh_last_rounds: call lh_align_resident first (and ask before the next upload, select or stage dump)");
        return LH_OK;   // a lane that took no part in the batch: n_rounds = 0
    }
    if (!p->ran) return set_err(LH_E_ARG, "lh_last_rounds: call lh_align_resident first (and ask before the next upload, select or stage dump)");
    if (!R.have_max) {   // ran whole: one part, every barcode
        HIPCHK(hipSetDevice(p->idx->device));
        if (!R.budget) { int rc = seed_budget(p, &R.budget); if (rc) return rc; }
        { int rc = round_plan(p, INT64_MAX, false); if (rc) return rc; }
        HIPCHK(hipStreamSynchronize(p->stream));
        R.max_bc = p->plan.hdr()->max_barcode; R.max_bc_seeds = p->plan.hdr()->max_barcode_seeds;
        if (p->plan.hdr()->n_rounds != 1 || p->plan.hdr()->total_seeds != R.total_seeds) return set_err(LH_E_HIP, "lh_last_rounds: the plan of a batch that ran whole is inconsistent");
        R.first_bc.assign({0, p->b.n_bc}); R.seeds.assign(1, R.total_seeds); R.need.assign(1, seed_need(p, R.total_seeds));
        R.have_max = true;
    }
    const int32_t b0 = lane && lanes_split(c) ? c->slot_cut[(size_t)c->cur_slot][(size_t)lane - 1] : 0;
    if (b0 && R.first_bc[0] == 0) { for (int32_t& b : R.first_bc) b += b0; R.max_bc += b0; }   // (once: the arrays are the pipeline's until its next run)
    out->n_rounds = R.n_rounds; out->max_barcode = (int32_t)R.max_bc;
    out->first_barcode = R.first_bc.data(); out->round_seeds = R.seeds.data(); out->round_need_bytes = R.need.data();
    out->need_bytes = seed_need(p, R.total_seeds); out->budget_bytes = R.budget; out->max_barcode_need_bytes = seed_need(p, R.max_bc_seeds);
    return LH_OK;
}

// K8's classes in the first pipeline's last run (a batch in rounds or lanes: its last part there)
int lh_last_rfa_classes(lh_context* c, int64_t* out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_last_rfa_classes: null argument");
    if (!c->ran_inference) return set_err(LH_E_ARG, "lh_last_rfa_classes: call lh_align_resident with run_inference first");
    for (int i = 0; i < 4; ++i) out[i] = c->rfa_cls[i];
    return LH_OK;
}

// pass 2's calls as the lister of the first pipeline's last K1 counted them
int lh_last_p2_calls(lh_context* c, int64_t* out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_last_p2_calls: null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->p2_cls[i];
    return LH_OK;
}

// the reads the first pipeline's last K1 listed for k_smem_fin (the list lives until the pipeline's next K1)
int lh_last_fin_list(lh_context* c, int32_t* out, int64_t cap, int64_t* n) {
    if (!c || !n || cap < 0 || (cap && !out)) return set_err(LH_E_ARG, "lh_last_fin_list: null argument");
    if (!c->d_fin_list || !c->d_next_read) return set_err(LH_E_ARG, "lh_last_fin_list: call lh_align_resident or lh_stage_dump_resident first");
    HIPCHK(hipSetDevice(c->idx->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    int32_t n_fin = 0;
    HIPCHK(hipMemcpy(&n_fin, &c->d_next_read->n_fin, sizeof n_fin, hipMemcpyDeviceToHost));
    *n = n_fin;
    const int64_t k = n_fin < cap ? n_fin : cap;
    if (k > 0) HIPCHK(hipMemcpy(out, c->d_fin_list, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost));
    return LH_OK;
}

// part behind acc (the first part becomes acc): merged into a new result, and both are freed whatever the outcome.  The rounds' parts and the lanes' fold this way
static int merge_into(lh_result*& acc, lh_result* part) {
    if (!acc) { acc = part; return LH_OK; }
    lh_result* m = nullptr;
    const int rc = merge_results(acc, part, &m);
    lh_result_free(acc); lh_result_free(part);
    acc = m;
    return rc;
}
// b's arrays behind a's in one block, column by column as LH_RESULT_COLS says (lh_result_cols.h): candidate / CIGAR / mismatch indices of b shifted by a's totals
static int merge_results(lh_result* a, lh_result* b, lh_result** out) {
    const size_t Ca = (size_t)a->n_cand, Cb = (size_t)b->n_cand;
    size_t total = 0;
    auto reserve = [&](size_t bytes) { size_t o = total; total += (bytes + 63) & ~(size_t)63; return o; };
    std::array<size_t, LH_N_COLS> na, nb, off;   // per column: a's and b's elements, place in the block
    for (size_t i = 0; i < LH_N_COLS; ++i) {
        const ResultCol& k = LH_RESULT_COLS[i];
        na[i] = col_count(k, (size_t)a->n_reads, Ca, (size_t)a->cigar_off[Ca], (size_t)a->mm_off[Ca]);
        nb[i] = col_count(k, (size_t)b->n_reads, Cb, (size_t)b->cigar_off[Cb], (size_t)b->mm_off[Cb]);
        off[i] = reserve((na[i] + nb[i] - (k.merge == MERGE_CONTINUE)) * k.elt);   // (b's entry 0 of an offset array is a's last)
    }
    char* B = (char*)malloc(total + 64);
    if (!B) return set_err(LH_E_ARG, "out of memory merging the lanes' results");
    {   // a's part of every column and b's of the plain ones, a few host threads
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (size_t i = next++; i < LH_N_COLS; i = next++) {
                const ResultCol& k = LH_RESULT_COLS[i];
                if (na[i]) memcpy(B + off[i], ptr_at(a, k.res_off), na[i] * k.elt);
                if (nb[i] && k.merge == MERGE_COPY) memcpy(B + off[i] + na[i] * k.elt, ptr_at(b, k.res_off), nb[i] * k.elt);
            }
        };
        std::vector<std::thread> th;
        for (int t = 0; t < 7; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    ResultArenaH* A = new ResultArenaH();
    A->merged = B;
    lh_result& r = A->r;
    memset(&r, 0, sizeof r);
    r.arena_ = A;
    r.abi_version = LH_ABI_VERSION; r.n_reads = a->n_reads + b->n_reads; r.n_cand = (int64_t)(Ca + Cb);
    for (size_t i = 0; i < LH_N_COLS; ++i) {
        const ResultCol& k = LH_RESULT_COLS[i];
        set_ptr_at(&r, k.res_off, B + off[i]);
        if (k.merge == MERGE_COPY) continue;
        i64* dst = (i64*)(B + off[i]) + na[i];
        const i64* src = (const i64*)ptr_at(b, k.res_off);
        if (k.merge == MERGE_SHIFT)
            for (size_t q = 0; q < nb[i]; ++q) dst[q] = src[q] < 0 ? src[q] : src[q] + (i64)Ca;
        else {
            const i64 last = dst[-1];   // a's last entry = b's entry 0
            for (size_t q = 1; q < nb[i]; ++q) dst[q - 1] = src[q] + last;
        }
    }
    for (size_t q = 0; q < LH_N_CTRS; ++q) result_ctrs(&r)[q] = result_ctrs(a)[q] + result_ctrs(b)[q];
    *out = &A->r;
    return LH_OK;
}

// the download in two steps (lh_host_stage2.inc): begin enqueues the copies of every lane's part, end collects and merges them
int lh_result_download_begin(lh_context* c) {
    if (!c) return set_err(LH_E_ARG, "lh_result_download_begin: null context");
    c->dl_split = lanes_split(c);
    int rc = pipe_download_begin(c);
    if (rc || !c->dl_split) return rc;
    for (size_t k = 0; k < c->more.size(); ++k) {
        rc = pipe_download_begin(c->more[k]);
        if (rc) {   // collect what was started: no half-begun download stays behind
            const std::string why = g_err;
            lh_result* r = nullptr;
            if (pipe_download_end(c, &r) == LH_OK) lh_result_free(r);
            for (size_t q = 0; q < k; ++q) { r = nullptr; if (pipe_download_end(c->more[q], &r) == LH_OK) lh_result_free(r); }
            return set_err(rc, "lane " + std::to_string(k + 2) + ": " + why);
        }
    }
    return LH_OK;
}
int lh_result_download_end(lh_context* c, lh_result** out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_result_download_end: null argument");
    if (!c->dl_split) return pipe_download_end(c, out);
    const size_t M = c->more.size();
    std::vector<lh_result*> rs(M + 1, nullptr);
    std::vector<int> rcs(M + 1, LH_OK);
    std::vector<std::string> errs(M + 1);
    for (size_t k = 0; k <= M; ++k) { rcs[k] = pipe_download_end(k ? c->more[k - 1] : c, &rs[k]); if (rcs[k]) errs[k] = g_err; }
    int64_t first_read = 0;
    for (size_t k = 0; k <= M; ++k) {
        if (rcs[k]) {
            for (lh_result* r : rs) if (r) lh_result_free(r);
            return set_err(rcs[k], k ? "lane " + std::to_string(k + 1) + " (its reads start at read " + std::to_string(first_read) + " of the batch): " + errs[k] : errs[0]);
        }
        first_read += rs[k]->n_reads;
    }
    lh_result* acc = nullptr;
    for (size_t k = 0; k <= M; ++k) {
        int rc = merge_into(acc, rs[k]);
        if (rc) { for (size_t q = k + 1; q <= M; ++q) lh_result_free(rs[q]); return rc; }
    }
    *out = acc;
    return LH_OK;
}
int lh_result_download(lh_context* c, lh_result** out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_result_download: null argument");
    int rc = lh_result_download_begin(c);
    return rc ? rc : lh_result_download_end(c, out);
}

void* lh_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { set_err(LH_E_HIP, "lh_host_alloc: hipHostMalloc failed"); return nullptr; }
    return p;
}
void lh_host_free(void* p) { if (p) hipHostFree(p); }

// a batch into a slot that is NOT the selected one, on the context's upload stream: may be called from a second host thread while
// lh_align_resident runs on the selected slot (the reference's reader goroutine fills the next work unit the same way, lariat.go:333)
int lh_batch_stage_slot(lh_context* c, int32_t slot, const lh_batch* b) {
    if (!c || !b) return set_err(LH_E_ARG, "lh_batch_stage_slot: null argument");
    if (!c->more.empty()) return set_err(LH_E_ARG, "lh_batch_stage_slot: contexts with several lanes upload through lh_batch_upload_slot");
    if ((size_t)slot < c->slot_cut.size()) c->slot_cut[(size_t)slot].clear();
    return pipe_upload_slot(c, slot, b, true);
}

int lh_align_barcodes(lh_context* c, const lh_opts* opts, const lh_batch* b, lh_result** out) {
    int rc = lh_batch_upload(c, b);
    if (rc) return rc;
    rc = lh_align_resident(c, opts);
    if (rc) return rc;
    return lh_result_download(c, out);
}
