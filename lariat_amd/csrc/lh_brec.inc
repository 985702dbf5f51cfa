// lh_brec.inc — the device record encoder behind lh_bam_set_device_records (include/lariat_hip.h): the BAM records of a batch by k_brec.h, compressed where
// they lie by k_bgzf.h.  Included from lh_host.inc after lh_bgzf.inc: the encoder's buffers belong to the lh_bgzf object, its work runs on the compressor's first
// stream under the compressor's mutex.
//
// One lh_bam_append: the host gathers the few rows of the result a record reads (at most four candidates per read) into page-locked staging and uploads them with
// the ingest batch's text as it is; k_brec_plan sizes every record; the offsets (rocPRIM's radix sort by file and two scans; std::stable_sort under the emulator) give
// every record its place in bc_sorted and in its bucket file; k_brec_write stores the bytes behind each file's `pending` bytes in one device buffer, a region per file;
// k_bgzf compresses every whole block of every region from there.  Only the members and each file's last partial block come back.
// One lh_bam_append_resident: the same, but the staging buffer's contents are produced on the device, by k_brec_gather_count, two scans and k_brec_gather_fill from
// the arrays lh_align_resident left in the context; the result is not downloaded, and everything behind the staging buffer is shared.
#include "k_brec.h"
#include "brec_internal.h"
#include <chrono>
#include <thread>

struct lh_brec_bufs {
    struct Dev { void* p = nullptr; size_t cap = 0; };
    Dev text, stage, plan, work, tmp, out;
    void* h_stage = nullptr; size_t h_stage_cap = 0;   // page-locked: the gathered rows
    i64* h_small = nullptr; size_t h_small_cap = 0;    // page-locked: what comes back between the offsets and the write (file_end, the total, err, watchdog)
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // upload begins / ends, plan begins, offsets end, write begins / ends, the device gather begins / ends
};
static void brec_free(lh_brec_bufs* b) {
    if (!b) return;
    for (lh_brec_bufs::Dev* d : {&b->text, &b->stage, &b->plan, &b->work, &b->tmp, &b->out}) if (d->p) (void)hipFree(d->p);
    if (b->h_stage) (void)hipHostFree(b->h_stage);
    if (b->h_small) (void)hipHostFree(b->h_small);
    for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
    delete b;
}
// a buffer of at least `need` bytes; its contents are not kept.  The new one is allocated before the old one is freed (a hipFree waits for the whole device: it then comes
// after the allocation that could fail, and once per growth)
static int brec_dev(lh_brec_bufs::Dev& d, size_t need) {
    if (need <= d.cap && d.p) return LH_OK;
    const size_t cap = need + need / 4 + 4096;
    uint8_t* p = nullptr;
    const int rc = dalloc(&p, cap);
    if (rc) return rc;
    if (d.p) (void)hipFree(d.p);
    d.p = p; d.cap = cap;
    return LH_OK;
}
static int brec_pinned(void** h, size_t* have, size_t need) {
    if (need <= *have && *h) return LH_OK;
    const size_t cap = need + need / 4 + 4096;
    void* p = nullptr;
    HIPCHK(hipHostMalloc(&p, cap, hipHostMallocDefault));
    if (*h) (void)hipHostFree(*h);
    *h = p; *have = cap;
    return LH_OK;
}

namespace {
struct BrecLayout {   // sections of one buffer, 16-byte aligned
    size_t total = 0;
    size_t add(size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; }
};
struct BrecUpload { size_t at; const void* src; size_t bytes; };

// the resident variant of bgzf_submit: the chunk's blocks lie in device memory already (d_in + blk_off[first + i]); no staging copy, no upload but the descriptors'
int bgzf_submit_resident(lh_bgzf* z, lh_bgzf::Set& s, const uint8_t* d_in, const std::vector<BgzfBlk>& blks, const std::vector<i64>& blk_off, size_t first, int nb) {
    i64* off = (i64*)s.h_desc; int32_t* len = (int32_t*)(s.h_desc + (size_t)z->max_blocks * 8);
    for (int i = 0; i < nb; ++i) { off[i] = blk_off[first + (size_t)i]; len[i] = blks[first + (size_t)i].len; }
    s.nb = nb; s.first = first;
    HIPCHK(hipEventRecord(s.ev[0], s.st));
    HIPCHK(hipMemcpyAsync(s.d_desc, s.h_desc, (size_t)z->max_blocks * 12, hipMemcpyHostToDevice, s.st));
    HIPCHK(hipEventRecord(s.ev[1], s.st));
    LH_LAUNCH(k_bgzf, nb < z->waves ? nb : z->waves, 64, s.st, d_in, (const i64*)s.d_desc, (const int32_t*)(s.d_desc + (size_t)z->max_blocks * 8), nb, s.d_out, s.d_meta,
              s.d_tok, (const uint32_t*)z->d_consts, s.d_meta + z->max_blocks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev[2], s.st));
    HIPCHK(hipMemcpyAsync(s.h_out, s.d_out, (size_t)nb * LH_BGZF_SLOT, hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipMemcpyAsync(s.h_meta, s.d_meta, ((size_t)z->max_blocks + LH_WD_SLOTS) * sizeof(int32_t), hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipEventRecord(s.ev[3], s.st));
    return LH_OK;
}

double brec_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the rows a read's records read: the active alignment, its split, the second best, the active's mate
void brec_gather_row(const lh_result* r, i64 a, BrecRow& o, i64& cig_at, i64& mm_at, bool want_cig, bool want_mm, uint32_t* cig, int32_t* mm) {
    memset(&o, 0, sizeof o);
    o.ci = a;
    if (a < 0) return;
    o.pos = r->pos[a]; o.aend = r->aend[a]; o.rid = r->rid[a]; o.score = r->score[a]; o.mapq = r->mapq[a]; o.mol_id = r->molecule_id[a];
    o.mol_diff = r->molecule_difference[a];
    o.reversed = r->reversed[a]; o.is_proper = r->is_proper[a]; o.duplicate = r->duplicate[a]; o.active_mol = r->active_molecule[a];
    if (want_cig) {
        o.cig_off = cig_at; o.n_cig = (int32_t)(r->cigar_off[a + 1] - r->cigar_off[a]);
        if (cig) memcpy(cig + cig_at, r->cigar + r->cigar_off[a], (size_t)o.n_cig * 4);
        cig_at += o.n_cig;
    }
    if (want_mm) {
        o.mm_off = mm_at; o.n_mm = (int32_t)(r->mm_off[a + 1] - r->mm_off[a]);
        if (mm) for (i64 k = 0; k < o.n_mm; ++k) { mm[2 * (mm_at + k)] = r->mm_ref_loc[r->mm_off[a] + k]; mm[2 * (mm_at + k) + 1] = r->mm_read_loc[r->mm_off[a] + k]; }
        mm_at += o.n_mm;
    }
}
// reads [r0, r1): counts only (rows == null) or fills, from the given places of the packed arrays on
void brec_gather(const lh_result* r, i64 r0, i64 r1, BrecRow* rows, double* rd, uint32_t* cig, int32_t* mm, i64& cig_at, i64& mm_at) {
    BrecRow scratch;
    for (i64 read = r0; read < r1; ++read) {
        const i64 a = r->active_idx[read];
        const i64 idx[LH_BREC_SLOTS] = {a, r->split_idx[read], r->second_best_idx[read], a >= 0 ? r->mate_idx[a] : -1};
        for (int k = 0; k < LH_BREC_SLOTS; ++k) brec_gather_row(r, idx[k], rows ? rows[read * LH_BREC_SLOTS + k] : scratch, cig_at, mm_at, k < 2, k < 3, rows ? cig : nullptr, rows ? mm : nullptr);
        if (rd) { rd[read * 4] = r->second_best_score[read]; rd[read * 4 + 1] = r->as_score[read]; rd[read * 4 + 2] = r->split_second_best[read]; rd[read * 4 + 3] = r->split_score[read]; }
    }
}

// srcs == null: the stage buffer comes from c->res by the host's gather and one upload.  Else the device gathers it from the pipelines' resident results (`srcs`, a part
// of the batch each); ctx_lock holds the context's mutex and is released once the gather kernels have completed
int brec_encode(lh_bgzf* z, LhBrecCall* c, lh_brec_bufs* B, const std::vector<BrecSrc>* srcs, std::unique_lock<std::mutex>* ctx_lock) {
    const lh_result* res = c->res;
    const lh_ingest_batch* in = c->in;
    const i64 n_pairs = in->batch.n_pairs, n_reads = 2 * n_pairs, n_slots = 4 * n_pairs;
    const int n_out = (int)c->pending.size(), n_contigs = (int)c->names->size();
    lh_bgzf::Set& s0 = z->set[0];
    hipStream_t st = s0.st;
    for (hipEvent_t& e : B->ev) if (!e) HIPCHK(hipEventCreate(&e));
    c->seg_off.assign((size_t)n_out + 1, 0);
    c->rest.assign((size_t)n_out, std::string());
    std::vector<i64> rec_bytes((size_t)n_out, 0), region((size_t)n_out, 0), file_base((size_t)n_out, 0);
    i64 total = 0;
    z->t_up = z->t_kernel = z->t_down = 0;
    if (n_pairs > 0) {
        // the work buffer's sections (laid out first: the device gather keeps its counts and scans there)
        BrecLayout wl;
        const size_t N = (size_t)n_slots;
        const size_t w_key0 = wl.add(N * 4), w_key1 = wl.add(N * 4), w_val0 = wl.add(N * 4), w_val1 = wl.add(N * 4);
        const size_t w_sz = wl.add((N + 1) * 8), w_offbc = wl.add((N + 1) * 8), w_ssz = wl.add((N + 1) * 8), w_sscan = wl.add((N + 1) * 8), w_offf = wl.add(N * 8);
        const size_t w_fend = wl.add((size_t)n_out * 8), w_fbase = wl.add((size_t)n_out * 8), w_err = wl.add(16), w_wd = wl.add(LH_WD_SLOTS * 4);
        const size_t R1 = srcs ? (size_t)n_reads + 1 : 0;   // the device gather's: per read the CIGAR operations and loci, their scans, its error and watchdog words
        const size_t w_gnc = wl.add(R1 * 8), w_gnm = wl.add(R1 * 8), w_gcs = wl.add(R1 * 8), w_gms = wl.add(R1 * 8), w_gerr = wl.add(srcs ? 16 + LH_WD_SLOTS * 4 : 0);
        const size_t small_words = (size_t)n_out + 1 + 2 + LH_WD_SLOTS / 2, small_gather = 2 + LH_WD_SLOTS / 2;   // (page-locked words; the gather's behind the others)
        BrecLayout sl;
        size_t s_row = 0, s_rd = 0, s_cig = 0, s_mm = 0;
        uint8_t* hs = nullptr;
        int rc = LH_OK;
        if (srcs) {
            // ---- 1. gather on the device, from the context's arrays: counts per read, two scans (read order, then slot order: the order the host's threads produce), fill
            rc = brec_dev(B->work, wl.total);
            if (!rc) rc = brec_pinned((void**)&B->h_small, &B->h_small_cap, (small_words + small_gather) * 8);
            size_t g_tmp = 16;
#ifndef LH_EMU
            { size_t b = 0; HIPCHK(rocprim::exclusive_scan(nullptr, b, (const i64*)nullptr, (i64*)nullptr, (i64)0, R1, rocprim::plus<i64>(), st)); g_tmp = b + 16; }
#endif
            if (!rc) rc = brec_dev(B->tmp, g_tmp);
            if (rc) return rc;
            uint8_t* gw = (uint8_t*)B->work.p;
            i64 *g_nc = (i64*)(gw + w_gnc), *g_nm = (i64*)(gw + w_gnm), *g_cs = (i64*)(gw + w_gcs), *g_ms = (i64*)(gw + w_gms);
            int32_t *g_err = (int32_t*)(gw + w_gerr), *g_wd = g_err + 4;
            HIPCHK(hipEventRecord(B->ev[6], st));
            HIPCHK(hipMemsetAsync(g_nc, 0, R1 * 8, st));   // (entry n_reads stays 0: the scan's last element is then the total)
            HIPCHK(hipMemsetAsync(g_nm, 0, R1 * 8, st));
            HIPCHK(hipMemsetAsync(g_err, 0, 16 + LH_WD_SLOTS * 4, st));
            const int32_t g_err_init[4] = {0, 0x7fffffff, 0, 0};
            HIPCHK(hipMemcpyAsync(g_err, g_err_init, 16, hipMemcpyHostToDevice, st));
            for (const BrecSrc& s : *srcs) if (s.n_reads > 0) LH_LAUNCH(k_brec_gather_count, (s.n_reads + 255) / 256, 256, st, s, g_nc, g_nm, g_err);
            HIPCHK(hipGetLastError());
#ifdef LH_EMU
            { i64 rc_ = 0, rm_ = 0; for (size_t i = 0; i < R1; ++i) { g_cs[i] = rc_; rc_ += g_nc[i]; g_ms[i] = rm_; rm_ += g_nm[i]; } }
#else
            {
                size_t tb = B->tmp.cap;
                HIPCHK(rocprim::exclusive_scan(B->tmp.p, tb, (const i64*)g_nc, g_cs, (i64)0, R1, rocprim::plus<i64>(), st));
                tb = B->tmp.cap;
                HIPCHK(rocprim::exclusive_scan(B->tmp.p, tb, (const i64*)g_nm, g_ms, (i64)0, R1, rocprim::plus<i64>(), st));
            }
#endif
            i64* gh = B->h_small;   // the two totals, the error words
            HIPCHK(hipMemcpyAsync(gh, g_cs + n_reads, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(gh + 1, g_ms + n_reads, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(gh + 2, g_err, 16, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const int32_t* gh_err = (const int32_t*)(gh + 2);
            if (gh_err[0] & LH_BREC_E_INDEX) return set_err(LH_E_HIP, "lh_bam_append_resident: the context's result holds a candidate index or a mismatch list outside its arrays; nothing was appended");
            if (gh_err[0] & LH_BREC_E_NOACTIVE) return set_err(LH_E_ARG, "lh_bam_append_resident: a read has no active alignment (read " + std::to_string(gh_err[1]) + "); nothing was appended");
            if (gh[0] < 0 || gh[1] < 0) return set_err(LH_E_HIP, "lh_bam_append_resident: the gather's totals are negative");
            s_row = sl.add((size_t)n_reads * LH_BREC_SLOTS * sizeof(BrecRow)); s_rd = sl.add((size_t)n_reads * 4 * sizeof(double));
            s_cig = sl.add((size_t)gh[0] * 4); s_mm = sl.add((size_t)gh[1] * 8);
            rc = brec_dev(B->stage, sl.total);
            if (rc) return rc;
            uint8_t* gs = (uint8_t*)B->stage.p;
            for (const BrecSrc& s : *srcs)
                if (s.n_reads > 0)
                    LH_LAUNCH(k_brec_gather_fill, (int)(((i64)s.n_reads * 16 + 255) / 256), 256, st, s, (const i64*)g_cs, (const i64*)g_ms, (BrecRow*)(gs + s_row), (double*)(gs + s_rd), (uint32_t*)(gs + s_cig),
                              (int32_t*)(gs + s_mm), g_err, g_wd);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(B->ev[7], st));
        } else {
            // ---- 1. gather: counts, then the rows, by ranges of reads
            const double tg0 = brec_now();
            int nt = c->threads < 1 ? 1 : c->threads;
            if ((i64)nt > (n_pairs + 255) / 256) nt = (int)((n_pairs + 255) / 256);
            std::vector<i64> cig_at((size_t)nt + 1, 0), mm_at((size_t)nt + 1, 0);
            auto each = [&](const std::function<void(int)>& f) {
                std::vector<std::thread> th;
                for (int t = 1; t < nt; ++t) th.emplace_back(f, t);
                f(0);
                for (auto& t : th) t.join();
            };
            each([&](int t) { i64 ca = 0, ma = 0; brec_gather(res, n_reads * t / nt, n_reads * (t + 1) / nt, nullptr, nullptr, nullptr, nullptr, ca, ma); cig_at[(size_t)t + 1] = ca; mm_at[(size_t)t + 1] = ma; });
            for (int t = 0; t < nt; ++t) { cig_at[(size_t)t + 1] += cig_at[(size_t)t]; mm_at[(size_t)t + 1] += mm_at[(size_t)t]; }
            s_row = sl.add((size_t)n_reads * LH_BREC_SLOTS * sizeof(BrecRow)); s_rd = sl.add((size_t)n_reads * 4 * sizeof(double));
            s_cig = sl.add((size_t)cig_at[(size_t)nt] * 4); s_mm = sl.add((size_t)mm_at[(size_t)nt] * 8);
            rc = brec_pinned(&B->h_stage, &B->h_stage_cap, sl.total);
            if (!rc) rc = brec_dev(B->stage, sl.total);
            if (rc) return rc;
            hs = (uint8_t*)B->h_stage;
            each([&](int t) {
                i64 ca = cig_at[(size_t)t], ma = mm_at[(size_t)t];
                brec_gather(res, n_reads * t / nt, n_reads * (t + 1) / nt, (BrecRow*)(hs + s_row), (double*)(hs + s_rd), (uint32_t*)(hs + s_cig), (int32_t*)(hs + s_mm), ca, ma);
            });
            c->t[0] = brec_now() - tg0;
        }
        // ---- 2. upload: the rows in one copy, the batch's text arenas and offsets as they are, the writer's small tables
        std::vector<i64> cname_off((size_t)n_contigs + 1, 0);
        std::string cname;
        std::vector<int32_t> bucket_off((size_t)n_contigs + 1, 0), bucket;
        for (int k = 0; k < n_contigs; ++k) {
            cname += (*c->names)[(size_t)k]; cname_off[(size_t)k + 1] = (i64)cname.size();
            for (int f : (*c->bucket)[(size_t)k]) bucket.push_back(f);
            bucket_off[(size_t)k + 1] = (int32_t)bucket.size();
        }
        BrecLayout tl;
        std::vector<BrecUpload> ups;
        auto sec = [&](const void* src, size_t bytes) { const size_t at = tl.add(bytes); ups.push_back(BrecUpload{at, src, bytes}); return at; };
        const size_t P = (size_t)n_pairs;
        const size_t a_seq_off = sec(in->batch.seq_off, (2 * P + 1) * 8), a_seq = sec(in->batch.seq, (size_t)in->batch.seq_off[2 * P]);
        const size_t a_bcp = sec(in->batch.bc_pair_off, ((size_t)in->n_sets + 1) * 4), a_setc = sec(in->set_complete, (size_t)in->n_sets);
        struct Col { const char* base; const int64_t* off; size_t a_base, a_off; };
        Col cols[11] = {{in->name, in->name_off, 0, 0}, {in->qual1, in->qual1_off, 0, 0}, {in->qual2, in->qual2_off, 0, 0}, {in->trim_bases, in->trim_off, 0, 0}, {in->trim_quals, in->trim_off, 0, 0},
                        {in->bc, in->bc_off, 0, 0}, {in->rawbc, in->rawbc_off, 0, 0}, {in->bcqual, in->bcqual_off, 0, 0}, {in->si, in->si_off, 0, 0}, {in->siqual, in->siqual_off, 0, 0},
                        {in->rgid, in->rgid_off, 0, 0}};
        for (Col& q : cols) { q.a_off = sec(q.off, (P + 1) * 8); q.a_base = sec(q.base, (size_t)q.off[P]); }
        const size_t a_cname = sec(cname.data(), cname.size()), a_cname_off = sec(cname_off.data(), cname_off.size() * 8);
        const size_t a_boff = sec(bucket_off.data(), bucket_off.size() * 4), a_bucket = sec(bucket.data(), bucket.size() * 4);
        rc = brec_dev(B->text, tl.total);
        if (!rc) rc = brec_dev(B->plan, (size_t)n_slots * sizeof(BrecPlan));
        if (!rc) rc = brec_dev(B->work, wl.total);   // (after a device gather: the buffer it allocated with this size, so this keeps it and the counts and scans in it; the same for h_small below)
        size_t tmp_bytes = 16;
#ifndef LH_EMU
        {
            size_t b1 = 0, b2 = 0;
            rocprim::double_buffer<uint32_t> kb((uint32_t*)nullptr, (uint32_t*)nullptr), vb((uint32_t*)nullptr, (uint32_t*)nullptr);
            HIPCHK(rocprim::radix_sort_pairs(nullptr, b1, kb, vb, N, 0u, 32u, st));
            HIPCHK(rocprim::exclusive_scan(nullptr, b2, (const i64*)nullptr, (i64*)nullptr, (i64)0, N + 1, rocprim::plus<i64>(), st));
            tmp_bytes = (b1 > b2 ? b1 : b2) + 16;
        }
#endif
        if (!rc) rc = brec_dev(B->tmp, tmp_bytes);
        if (!rc) rc = brec_pinned((void**)&B->h_small, &B->h_small_cap, (small_words + (srcs ? small_gather : 0)) * 8);
        if (rc) return rc;
        uint8_t* dt = (uint8_t*)B->text.p; uint8_t* ds = (uint8_t*)B->stage.p; uint8_t* dw = (uint8_t*)B->work.p;
        HIPCHK(hipEventRecord(B->ev[0], st));
        if (!srcs) HIPCHK(hipMemcpyAsync(ds, hs, sl.total, hipMemcpyHostToDevice, st));
        for (const BrecUpload& u : ups) if (u.bytes) HIPCHK(hipMemcpyAsync(dt + u.at, u.src, u.bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(dw + w_fend, 0xff, (size_t)n_out * 8, st));
        HIPCHK(hipMemsetAsync(dw + w_err, 0, 16 + LH_WD_SLOTS * 4, st));   // (err and the watchdog words are neighbours)
        static_assert(LH_WD_SLOTS * 4 % 16 == 0, "sections");
        const int32_t err_init[4] = {0, 0x7fffffff, 0, 0};
        HIPCHK(hipMemcpyAsync(dw + w_err, err_init, 16, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(B->ev[1], st));
        BrecIn di;
        memset(&di, 0, sizeof di);
        di.n_pairs = (int32_t)n_pairs; di.n_sets = in->n_sets; di.n_contigs = n_contigs; di.n_out = n_out;
        di.row = (const BrecRow*)(ds + s_row); di.rd = (const double*)(ds + s_rd); di.cig = (const uint32_t*)(ds + s_cig); di.mm = (const int32_t*)(ds + s_mm);
        di.seq = dt + a_seq; di.seq_off = (const i64*)(dt + a_seq_off); di.bc_pair_off = (const int32_t*)(dt + a_bcp); di.set_complete = dt + a_setc;
        const char** cb[11] = {&di.name, &di.qual1, &di.qual2, &di.trim_bases, &di.trim_quals, &di.bc, &di.rawbc, &di.bcqual, &di.si, &di.siqual, &di.rgid};
        const i64** co[11] = {&di.name_off, &di.qual1_off, &di.qual2_off, &di.trim_off, &di.trim_off, &di.bc_off, &di.rawbc_off, &di.bcqual_off, &di.si_off, &di.siqual_off, &di.rgid_off};
        for (int k = 0; k < 11; ++k) { *cb[k] = (const char*)(dt + cols[k].a_base); *co[k] = (const i64*)(dt + cols[k].a_off); }
        di.cname = (const char*)(dt + a_cname); di.cname_off = (const i64*)(dt + a_cname_off);
        di.bucket_off = (const int32_t*)(dt + a_boff); di.bucket = (const int32_t*)(dt + a_bucket);
        di.chunk = c->chunk;
        // ---- 3. plan and offsets
        BrecPlan* d_plan = (BrecPlan*)B->plan.p;
        uint32_t *key0 = (uint32_t*)(dw + w_key0), *key1 = (uint32_t*)(dw + w_key1), *val0 = (uint32_t*)(dw + w_val0), *val1 = (uint32_t*)(dw + w_val1);
        i64 *sz = (i64*)(dw + w_sz), *off_bc = (i64*)(dw + w_offbc), *ssz = (i64*)(dw + w_ssz), *sscan = (i64*)(dw + w_sscan), *off_f = (i64*)(dw + w_offf);
        i64 *d_fend = (i64*)(dw + w_fend), *d_fbase = (i64*)(dw + w_fbase);
        int32_t *d_err = (int32_t*)(dw + w_err), *d_wd = (int32_t*)(dw + w_wd);
        HIPCHK(hipEventRecord(B->ev[2], st));
        LH_LAUNCH(k_brec_plan, (int)((n_pairs + 63) / 64), 64, st, di, d_plan, d_err, d_wd);
        LH_LAUNCH(k_brec_keys, (int)((n_slots + 1 + 255) / 256), 256, st, (const BrecPlan*)d_plan, n_slots, key0, val0, sz);
        HIPCHK(hipGetLastError());
        uint32_t *key = key0, *val = val0;
#ifdef LH_EMU
        {   // the same offsets by host loops: the stable sort stands in for rocPRIM's
            std::vector<uint32_t> ord(N);
            for (size_t i = 0; i < N; ++i) ord[i] = (uint32_t)i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return key0[x] < key0[y]; });
            for (size_t i = 0; i < N; ++i) { key1[i] = key0[ord[i]]; val1[i] = val0[ord[i]]; }
            key = key1; val = val1;
            i64 run = 0;
            for (size_t i = 0; i <= N; ++i) { off_bc[i] = run; run += sz[i]; }
        }
#else
        {
            rocprim::double_buffer<uint32_t> kb(key0, key1), vb(val0, val1);
            size_t tb = B->tmp.cap;
            HIPCHK(rocprim::radix_sort_pairs(B->tmp.p, tb, kb, vb, N, 0u, 32u, st));
            key = kb.current(); val = vb.current();
            tb = B->tmp.cap;
            HIPCHK(rocprim::exclusive_scan(B->tmp.p, tb, (const i64*)sz, off_bc, (i64)0, N + 1, rocprim::plus<i64>(), st));
        }
#endif
        LH_LAUNCH(k_brec_sorted, (int)((n_slots + 255) / 256), 256, st, (const uint32_t*)val, (const i64*)sz, n_slots, ssz);
#ifdef LH_EMU
        { i64 run = 0; for (size_t i = 0; i < N; ++i) { sscan[i] = run; run += ssz[i]; } }
#else
        { size_t tb = B->tmp.cap; HIPCHK(rocprim::exclusive_scan(B->tmp.p, tb, (const i64*)ssz, sscan, (i64)0, N, rocprim::plus<i64>(), st)); }
#endif
        LH_LAUNCH(k_brec_place, (int)((n_slots + 255) / 256), 256, st, (const uint32_t*)key, (const uint32_t*)val, (const i64*)ssz, (const i64*)sscan, n_slots, n_out, off_f, d_fend);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(B->ev[3], st));
        i64* hsm = B->h_small;   // file_end [n_out], the total, err (2 words), the watchdog words
        HIPCHK(hipMemcpyAsync(hsm, d_fend, (size_t)n_out * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hsm + n_out, off_bc + N, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hsm + n_out + 1, d_err, 16 + LH_WD_SLOTS * 4, hipMemcpyDeviceToHost, st));
        if (srcs) {
            HIPCHK(hipMemcpyAsync(hsm + small_words, dw + w_gerr, 16 + LH_WD_SLOTS * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventSynchronize(B->ev[7]));   // the gather kernels have read the context's arrays: its next align may overwrite them
            if (ctx_lock && ctx_lock->owns_lock()) ctx_lock->unlock();
        }
        HIPCHK(hipStreamSynchronize(st));
        if (srcs) {
            const int32_t* g = (const int32_t*)(hsm + small_words);
            for (int k = 0; k < LH_WD_SLOTS; ++k) if (g[4 + k]) return set_err(LH_E_HIP, "lh_bam_append_resident: watchdog word " + std::to_string(k) + " of k_brec_gather_fill tripped");
            if (g[0] & LH_BREC_E_INDEX) return set_err(LH_E_HIP, "lh_bam_append_resident: the context's result changed under the gather");
        }
        const int32_t* h_err = (const int32_t*)(hsm + n_out + 1);
        const int32_t* h_wd = h_err + 4;
        for (int k = 0; k < LH_WD_SLOTS; ++k) if (h_wd[k]) return set_err(LH_E_HIP, "lh_bam_append: watchdog word " + std::to_string(k) + " of k_brec_plan tripped");
        if (h_err[0]) {   // found in the plan pass: no byte has been written
            const i64 read = h_err[1], pair = read >> 1;
            if (h_err[0] & LH_BREC_E_FORMAT)
                return set_err(LH_E_LIMIT, "lh_bam_append: a record does not fit the BAM format (read " + std::to_string(read) + ": read name of " + std::to_string(in->name_off[pair + 1] - in->name_off[pair]) +
                                               " bytes: at most 254; CIGAR operations: at most 65535); nothing was appended");
            return set_err(LH_E_LIMIT, "lh_bam_append: the molecule_difference of read " + std::to_string(read) + "'s alignment is not a finite value below 2^31 (the device's %.6f of the DM tag); nothing was appended");
        }
        total = hsm[n_out];
        // ---- 4. the layout: a region per file, its pending bytes in front of its records
        if (n_out < 2 || hsm[0] >= 0) return set_err(LH_E_HIP, "lh_bam_append: the device's plan put records into bc_sorted's bucket");
        i64 prev_end = 0, cursor = 0;
        rec_bytes[0] = total;
        for (int o = 0; o < n_out; ++o) {
            const i64 pend = (i64)c->pending[(size_t)o]->size();
            region[(size_t)o] = cursor;
            if (o == 0) { file_base[0] = pend; cursor += pend + total; continue; }
            const i64 end = hsm[o] < 0 ? prev_end : hsm[o];
            if (end < prev_end) return set_err(LH_E_HIP, "lh_bam_append: the bucket files' offsets are not in order");
            rec_bytes[(size_t)o] = end - prev_end;
            file_base[(size_t)o] = cursor + pend - prev_end;
            cursor += pend + rec_bytes[(size_t)o];
            prev_end = end;
        }
        if (prev_end != total) return set_err(LH_E_HIP, "lh_bam_append: the bucket files hold " + std::to_string(prev_end) + " bytes of records, bc_sorted " + std::to_string(total));
        rc = brec_dev(B->out, (size_t)cursor + 64);
        if (rc) return rc;
        uint8_t* d_out = (uint8_t*)B->out.p;
        for (int o = 0; o < n_out; ++o) {
            const std::string& p = *c->pending[(size_t)o];
            if (!p.empty()) HIPCHK(hipMemcpyAsync(d_out + region[(size_t)o], p.data(), p.size(), hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(d_fbase, file_base.data(), (size_t)n_out * 8, hipMemcpyHostToDevice, st));
        // ---- 5. the bytes
        HIPCHK(hipEventRecord(B->ev[4], st));
        LH_LAUNCH(k_brec_write, (int)n_pairs, 64, st, di, (const BrecPlan*)d_plan, (const i64*)off_bc, (const i64*)off_f, (const i64*)d_fbase, file_base[0], d_out, d_wd);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(B->ev[5], st));
        HIPCHK(hipMemcpyAsync(hsm, d_wd, LH_WD_SLOTS * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < LH_WD_SLOTS; ++k) if (((const int32_t*)hsm)[k]) return set_err(LH_E_HIP, "lh_bam_append: watchdog word " + std::to_string(k) + " of k_brec_write tripped");
        float ms[3] = {0, 0, 0};
        HIPCHK(hipEventElapsedTime(&ms[0], B->ev[0], B->ev[1])); HIPCHK(hipEventElapsedTime(&ms[1], B->ev[2], B->ev[3])); HIPCHK(hipEventElapsedTime(&ms[2], B->ev[4], B->ev[5]));
        c->t[1] = ms[0] * 1e-3; c->t[2] = ms[1] * 1e-3; c->t[3] = ms[2] * 1e-3;
        if (srcs) { float g = 0; HIPCHK(hipEventElapsedTime(&g, B->ev[6], B->ev[7])); c->t[0] = g * 1e-3; }   // (the read-back of the totals between the two kernels included)
    } else {   // an empty batch: the pending bytes alone (whole blocks of them are written, as the host path's flush does)
        i64 cursor = 0;
        for (int o = 0; o < n_out; ++o) { region[(size_t)o] = cursor; cursor += (i64)c->pending[(size_t)o]->size(); }
        int rc = brec_dev(B->out, (size_t)cursor + 64);
        if (rc) return rc;
        for (int o = 0; o < n_out; ++o) {
            const std::string& p = *c->pending[(size_t)o];
            if (!p.empty()) HIPCHK(hipMemcpyAsync((uint8_t*)B->out.p + region[(size_t)o], p.data(), p.size(), hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    // ---- 6. compress in place: every whole block of every file, cut from the file's start as flush_device cuts `pending`; each file's rest comes back as it is
    const uint8_t* d_out = (const uint8_t*)B->out.p;
    std::vector<BgzfBlk> blks;
    std::vector<i64> blk_off;
    i64 bound = 0;
    for (int o = 0; o < n_out; ++o) {
        const i64 len = (i64)c->pending[(size_t)o]->size() + rec_bytes[(size_t)o], whole = len / LH_BGZF_DATA * LH_BGZF_DATA;
        for (i64 at = 0; at < whole; at += LH_BGZF_DATA) { blks.push_back(BgzfBlk{nullptr, LH_BGZF_DATA, o}); blk_off.push_back(region[(size_t)o] + at); }
        bound += lh_bgzf_bound(whole);
        std::string& rest = c->rest[(size_t)o];
        rest.resize((size_t)(len - whole));
        if (len > whole) HIPCHK(hipMemcpyAsync(&rest[0], d_out + region[(size_t)o] + whole, (size_t)(len - whole), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (bound > *c->zbuf_cap) { c->zbuf->reset(); *c->zbuf_cap = 0; c->zbuf->reset(new uint8_t[(size_t)bound]); *c->zbuf_cap = bound; }
    std::vector<i64> seg_off((size_t)n_out + 1, -1);
    i64 pos = 0;
    int rc = LH_OK;
    size_t chunk = 0;
    for (size_t first = 0; first < blks.size() && !rc; first += (size_t)z->max_blocks, ++chunk) {
        lh_bgzf::Set& s = z->set[chunk & 1];
        if (s.nb) rc = bgzf_collect(z, s, blks, c->zbuf->get(), *c->zbuf_cap, pos, seg_off.data());
        if (!rc) rc = bgzf_submit_resident(z, s, d_out, blks, blk_off, first, (int)(blks.size() - first < (size_t)z->max_blocks ? blks.size() - first : (size_t)z->max_blocks));
    }
    for (size_t k = 0; k < 2 && !rc; ++k) {
        lh_bgzf::Set& s = z->set[(chunk + k) & 1];
        if (s.nb) rc = bgzf_collect(z, s, blks, c->zbuf->get(), *c->zbuf_cap, pos, seg_off.data());
    }
    if (rc) return rc;
    seg_off[(size_t)n_out] = pos;
    for (int k = n_out - 1; k >= 0; --k) if (seg_off[(size_t)k] < 0) seg_off[(size_t)k] = seg_off[(size_t)k + 1];
    c->seg_off = seg_off;
    return LH_OK;
}
}   // namespace

// lh_bam_append_resident: the pipelines that hold the batch's result, each with its part's place in the batch (the first lane's reads first, as lh_result_download_end
// merges them), after the checks a download makes before it trusts a result.  The caller holds the context's mutex
static int brec_resident_srcs(lh_bgzf* z, lh_context* ctx, const lh_ingest_batch* in, std::vector<BrecSrc>* srcs) {
    const char* const F = "lh_bam_append_resident: ";
    if (!ctx->ran) return set_err(LH_E_ARG, std::string(F) + "nothing was aligned yet: call lh_align_resident first; nothing was appended");
    std::vector<lh_context*> pipes(1, ctx);
    if (lanes_split(ctx)) for (lh_context* p : ctx->more) pipes.push_back(p);
    i64 n_reads = 0;
    for (lh_context* p : pipes) {
        if (!p->ran) return set_err(LH_E_ARG, std::string(F) + "nothing was aligned yet: call lh_align_resident first; nothing was appended");
        if (p->rounds.n_rounds > 1)
            return set_err(LH_E_ARG, std::string(F) + "the last batch was aligned in rounds: its parts' results were merged on the host already, none is resident as a whole; lh_result_download + "
                                                      "lh_bam_append cost nothing extra there; nothing was appended");
        if (!p->ran_inference) return set_err(LH_E_ARG, std::string(F) + "the last lh_align_resident ran without inference (lh_opts.run_inference): no read has an active alignment; nothing was appended");
        n_reads += p->b.n_reads;
    }
    if (n_reads != 2 * (i64)in->batch.n_pairs)
        return set_err(LH_E_ARG, std::string(F) + "the ingest batch has " + std::to_string(in->batch.n_pairs) + " pairs, the batch the context aligned " + std::to_string(n_reads / 2) + "; nothing was appended");
    if (ctx->idx->device != z->device)
        return set_err(LH_E_ARG, std::string(F) + "the context's result is on device " + std::to_string(ctx->idx->device) + ", the writer's compressor on device " + std::to_string(z->device) + "; nothing was appended");
    i64 read0 = 0;
    for (size_t k = 0; k < pipes.size(); ++k) {
        lh_context* p = pipes[k];
        BrecSrc s;
        s.n_reads = p->b.n_reads; s.read0 = read0; s.n_cand = 0; s.R = p->R; s.S = p->S;
        const int rc = pipe_result_check(p, &s.n_cand);
        if (rc) { const std::string why = g_err; return set_err(rc, std::string(F) + (k ? "lane " + std::to_string(k + 1) + ": " : "") + why + "; nothing was appended"); }
        srcs->push_back(s);
        read0 += p->b.n_reads;
    }
    return LH_OK;
}

extern "C" int lh_brec_encode_(lh_bgzf* z, LhBrecCall* c) {
    if (!z || !c || (!c->res && !c->ctx) || !c->in || !c->names || !c->bucket || !c->zbuf || !c->zbuf_cap) return set_err(LH_E_ARG, "lh_bam_append: null argument");
    if (c->ctx) {
        // Lock order: the context's mutex, then the compressor's (the appends from a downloaded result take the compressor's alone).  The context's is held until the
        // gather kernels have completed (brec_encode releases it on their event), so that no next lh_align_resident overwrites the arrays under them; a download in
        // flight reads the same arrays and is no conflict
        std::unique_lock<std::mutex> ctx_lock(c->ctx->res_mu);
        std::vector<BrecSrc> srcs;
        // (an ingest batch without pairs, the end of the input, has no resident counterpart: a context holds no empty batch.  It reads nothing of the context)
        if (c->in->batch.n_pairs > 0) { const int rc = brec_resident_srcs(z, c->ctx, c->in, &srcs); if (rc) { c->refused = true; return rc; } }
        std::lock_guard<std::mutex> lock(z->mu);
        HIPCHK(hipSetDevice(z->device));
        if (!z->enc) z->enc = new lh_brec_bufs();
        const int rc = brec_encode(z, c, z->enc, &srcs, &ctx_lock);
        if (rc) {   // nothing of this call stays in flight (the context's mutex is still held, or the gather has completed)
            const std::string why = g_err;
            for (lh_bgzf::Set& s : z->set) { (void)hipStreamSynchronize(s.st); s.nb = 0; }
            (void)hipGetLastError();
            return set_err(rc, why);
        }
        return LH_OK;
    }
    const lh_result* res = c->res;
    if (res->n_reads != 2 * c->in->batch.n_pairs) return set_err(LH_E_ARG, "lh_bam_append: result and batch describe different reads");
    for (int64_t read = 0; read < res->n_reads; ++read)
        if (res->active_idx[read] < 0) return set_err(LH_E_ARG, "lh_bam_append: a read has no active alignment (inference was not run?)");
    std::lock_guard<std::mutex> lock(z->mu);
    HIPCHK(hipSetDevice(z->device));
    if (!z->enc) z->enc = new lh_brec_bufs();
    const int rc = brec_encode(z, c, z->enc, nullptr, nullptr);
    if (rc) {   // nothing of this call stays in flight
        const std::string why = g_err;
        for (lh_bgzf::Set& s : z->set) { (void)hipStreamSynchronize(s.st); s.nb = 0; }
        (void)hipGetLastError();
        return set_err(rc, why);
    }
    return LH_OK;
}

int lh_diag_format_f6(int device, int32_t n, const double* v, char* out) {
    if (n < 0 || (n && (!v || !out))) return set_err(LH_E_ARG, "lh_diag_format_f6: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    if (device < 0 || device >= lh_device_count()) return set_err(LH_E_ARG, "lh_diag_format_f6: no such device");
    if (!n) return LH_OK;
    HIPCHK(hipSetDevice(device));
    DevGroup g;
    double* d_v = nullptr; char* d_out = nullptr; int32_t* d_ref = nullptr;
    DALLOC(g, d_v, n); DALLOC(g, d_out, (size_t)n * 32); DALLOC(g, d_ref, 1);
    HIPCHK(hipMemcpy(d_v, v, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_ref, 0, 4));
    LH_LAUNCH(k_brec_f6, (n + 63) / 64, 64, (hipStream_t)0, (int)n, (const double*)d_v, d_out, d_ref);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    int32_t refused = 0;
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * 32, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&refused, d_ref, 4, hipMemcpyDeviceToHost));
    if (refused) return set_err(LH_E_LIMIT, "lh_diag_format_f6: a value is not finite or not below 2^31 in magnitude (its 32 bytes are zero)");
    return LH_OK;
}
