// lh_host_stage2.inc — back half of the resident pipeline: extension, dedup/patch, mate rescue, region->alignment,
// per-barcode inference, and the result download.  Included by lh_host.inc.

static int ext_alloc(lh_context* c);
static int stage2_alloc(lh_context* c) {
    i64 N = c->cap_reads;
    DevGroup& g = c->mem;
    DALLOC(g, c->d_reg_off, N + 1);
    DALLOC(g, c->d_n_regs, N); DALLOC(g, c->d_best, N);
    DALLOC(g, c->d_reg_clean, N + 1); DALLOC(g, c->d_dd_done, N + 1); DALLOC(g, c->d_dd_list, N + 1); DALLOC(g, c->d_rnj, N / 2 + 1); DALLOC(g, c->d_rjob_off, N / 2 + 2); DALLOC(g, c->d_rmeta, 1); DALLOC(g, c->d_rheavy, N / 2 + 1); DALLOC(g, c->d_rkeys, 3 * LH_RC_KEYS);
    c->grid_aln = c->co.aln_grid;   // 92 VGPRs: 5 waves per SIMD
    DALLOC(g, c->d_zpool, (size_t)c->grid_aln * LH_ZSLAB);
    DALLOC(g, c->d_aln_count, 1);
    DALLOC(g, c->R.cand_off, N + 1);
    { int rc = alloc_cand_pools(c, first_cand_cap(c)); if (rc) return rc; }
    { int rc = ext_alloc(c); if (rc) return rc; }
    { int rc = rfa_alloc(c); if (rc) return rc; }
    return LH_OK;
}

// a result column's array on the device
static void* col_dev(lh_context* c, const ResultCol& k) {
    switch (k.src) {
    case FROM_CAND: return ptr_at(&c->R, k.dev_off);
    case FROM_INF: return ptr_at(&c->S, k.dev_off);
    case FROM_CIGAR_OFF: return c->d_cigar_off;
    case FROM_MM_OFF: return c->d_mm_off;
    case FROM_PACK_A: return c->d_pack_a;
    case FROM_PACK_B: return c->d_pack_b;
    default: return c->d_pack_c;
    }
}
// n elements of a column set to its value in a result without inference
static void fill_col(void* p, size_t n, const ResultCol& k) {
    if (k.elt == 1) memset(p, (int)k.dflt, n);
    else if (k.fp) std::fill_n((double*)p, n, k.dflt);
    else if (k.elt == 8) std::fill_n((i64*)p, n, (i64)k.dflt);
    else std::fill_n((int32_t*)p, n, (int32_t)k.dflt);
}
// the members of DCand / DInf that are result columns of one length class, with room for n elements
static int alloc_result_cols(lh_context* c, DevGroup& g, ColLen len, size_t n) {
    for (const ResultCol& k : LH_RESULT_COLS)
        if (k.len == len && (k.src == FROM_CAND || k.src == FROM_INF)) {
            uint8_t*& member = *(uint8_t**)((char*)(k.src == FROM_CAND ? (void*)&c->R : (void*)&c->S) + k.dev_off);
            DALLOC(g, member, n * k.elt);
        }
    return LH_OK;
}

// the download's staging buffers for the packed CIGAR / mismatch arrays: they follow the candidates, and grow on their own when a batch has more than 8 entries per candidate
static int alloc_pack(lh_context* c, i64 pack_cap) {
    DevGroup& g = c->pack_mem;
    g.release(); c->pack_cap = 0;
    DALLOC(g, c->d_pack_a, pack_cap); DALLOC(g, c->d_pack_b, pack_cap); DALLOC(g, c->d_pack_c, pack_cap);
    c->pack_cap = pack_cap;
    return LH_OK;
}
// everything sized by the number of candidates of a batch (cand_cap); DCand::cand_off is per read and stays
static int alloc_cand_pools(lh_context* c, i64 C) {
    DCand& R = c->R;
    DevGroup& g = c->cand_mem;
    g.release(); c->cand_cap = 0;
    DALLOC(g, c->d_cigar_off, C + 1); DALLOC(g, c->d_mm_off, C + 1);
    { int rc = alloc_pack(c, C * 8); if (rc) { g.release(); return rc; } }
    DALLOC(g, c->d_tile_sum, C / LH_SCAN_TILE + 8);   // scans run over reads and over candidates
    DALLOC(g, R.n_cigar, C); DALLOC(g, R.cigar, C * LH_MAX_CIGAR); DALLOC(g, R.n_mm, C); DALLOC(g, R.mm_ref, C * LH_MAX_MM); DALLOC(g, R.mm_read, C * LH_MAX_MM); DALLOC(g, R.read_len, C);
    R.mm_xcap = 1 << 22;   // loci beyond a candidate's slots: room for ~20,000 candidates that need it
    DALLOC(g, R.mm_xoff, C); DALLOC(g, R.mm_xref, R.mm_xcap); DALLOC(g, R.mm_xread, R.mm_xcap); DALLOC(g, R.mm_xctr, 1);
    DALLOC(g, c->S.cand_read, C);
    { int rc = alloc_result_cols(c, g, PER_CAND, C); if (rc) return rc; }   // the per-candidate columns of the result (DCand's and DInf's)
    c->cand_cap = C;
    return LH_OK;
}

// K6 once its jobs exist (the emitting pass of rescue_dir; lh_diag_rescue_sw's own): which rows of its window a job's forward pass has to run (r06, k_rescue3.h:
// k_resc_cert, a certificate per job and no DP; not with full), the jobs in the order (striping, rows) — an order by striping alone that the emitting pass left is
// replaced — the forward Smith-Waterman, the jobs that reached min_seed_len in the order of THEIR striping, the reverse Smith-Waterman.  order: `padded` ints, what
// the first order takes (fewer jobs after the certificates, the same padding); order2: cap2 ints, every job with each bucket padded to 8.  meta: bstart / hist2 cleared
static int rescue_sw(hipStream_t st, const DIndex& ix, const DOpts& o, i64 total, RJob* jobs, const uint8_t* seq, RMeta* meta, int32_t* keys, int32_t* order, i64 padded,
                     int32_t* order2, i64 cap2, DCounters* ctr, bool full, int weaken) {
    const int gb = (int)((total + 4095) / 4096 < 1024 ? (total + 4095) / 4096 : 1024), minsc = o.min_seed_len * o.a;
    int32_t *const hist1 = keys, *const bstart1 = keys + LH_RC_KEYS, *const bcur1 = keys + 2 * LH_RC_KEYS;
    if (!full) LH_LAUNCH(k_resc_cert, (int)((total + 15) / 16 < 65536 ? (total + 15) / 16 : 65536), 64, st, ix, o, total, jobs, seq, weaken);
    HIPCHK(hipMemsetAsync(hist1, 0, sizeof(int32_t) * LH_RC_KEYS, st));
    LH_LAUNCH((k_resc_bucket1<false>), gb, 256, st, total, (const RJob*)jobs, hist1, bcur1, (const int32_t*)bstart1, order, ctr);
    LH_LAUNCH(k_resc_offsets1, 1, 1, st, meta, (const int32_t*)hist1, bstart1, bcur1, (i64*)nullptr);
    HIPCHK(hipMemsetAsync(order, 0xff, (size_t)padded * 4, st));
    LH_LAUNCH((k_resc_bucket1<true>), gb, 256, st, total, (const RJob*)jobs, hist1, bcur1, (const int32_t*)bstart1, order, ctr);
    LH_LAUNCH((k_resc_sw<false>), (int)(padded / 8), 64, st, ix, o, jobs, (const int32_t*)order, seq, meta);
    LH_LAUNCH((k_resc_bucket2<false>), gb, 256, st, total, (const RJob*)jobs, minsc, meta, order2);
    LH_LAUNCH(k_resc_offsets, 1, 1, st, meta, 1, (i64*)nullptr, (const i64*)nullptr);
    HIPCHK(hipMemsetAsync(order2, 0xff, (size_t)cap2 * 4, st));
    LH_LAUNCH((k_resc_bucket2<true>), gb, 256, st, total, (const RJob*)jobs, minsc, meta, order2);
    LH_LAUNCH((k_resc_sw<true>), (int)(cap2 / 8), 64, st, ix, o, jobs, (const int32_t*)order2, seq, meta);
    return LH_OK;
}

// K6 (k_rescue2.h): per direction, the attempts that need a Smith-Waterman become jobs for the packed systolic kernel; a wave per pair then
// replays gobwa.go's loop with their results.  One host round trip per direction: the job arrays follow the batch.
template <int DIR> static int rescue_dir(lh_context* c, const DOpts& o, const DIndex& ix) {
    const int P = c->b.n_pairs;
    const uint8_t* const seq = c->b.seq;
    // the enumeration, a lane per pair and a wave per heavy pair; emit (std::true_type, after the scan of the counts): write the jobs and their places in the order array
    auto resc_enum = [&](auto emit, int grid) {
        constexpr bool EMIT = decltype(emit)::value;
        const i64* const job_off = EMIT ? c->d_rjob_off : nullptr; RJob* const jobs = EMIT ? c->d_rjobs : nullptr; int32_t* const order = EMIT ? c->d_rorder : nullptr;
        LH_LAUNCH((k_resc_enum<DIR, EMIT>), grid, 256, c->stream, ix, o, P, seq, (const i64*)c->b.seq_off, (const i64*)c->d_reg_off, (const DReg*)c->d_regs,
                  (const int32_t*)c->d_n_regs, (const int32_t*)c->d_best, c->d_rnj, job_off, jobs, order, c->d_rmeta, c->d_aln_r, c->d_rheavy);
        LH_LAUNCH((k_resc_enum_w<DIR, EMIT>), P < 8192 ? P : 8192, 64, c->stream, ix, o, P, seq, (const i64*)c->b.seq_off, (const i64*)c->d_reg_off, (const DReg*)c->d_regs,
                  (const int32_t*)c->d_n_regs, (const int32_t*)c->d_best, c->d_rnj, job_off, jobs, order, c->d_rmeta, c->d_aln_r, (const int32_t*)c->d_rheavy);
    };
    // the replay, a wave per listed pair; cap (std::integral_constant): the instance by the list entries its LDS holds
    auto resc_apply = [&](auto cap, int grid, hipStream_t st) {
        LH_LAUNCH((k_resc_apply<DIR, decltype(cap)::value>), grid, 64, st, ix, o, P, seq, (const i64*)c->b.seq_off, (const i64*)c->d_reg_off, c->d_regs,
                  c->d_regs_tmp, c->d_ia, c->d_n_regs, (const int32_t*)c->d_best, (const uint8_t*)c->d_reg_clean, c->d_ctr, (const int32_t*)c->d_aln_r, c->d_rmeta, (const int32_t*)c->d_rnj,
                  (const i64*)c->d_rjob_off, (const RJob*)c->d_rjobs);
    };
    HIPCHK(hipMemsetAsync(c->d_rmeta, 0, sizeof(RMeta), c->stream));
    resc_enum(std::false_type(), (P + 255) / 256);
    { int rc = run_scan(c, P, c->d_rnj, 0, 0, c->d_rjob_off); if (rc) return rc; }
    LH_LAUNCH(k_resc_offsets, 1, 1, c->stream, c->d_rmeta, 0, &c->h_peek->k6.total, (const i64*)(c->d_rjob_off + P));
    HIPCHK(hipStreamSynchronize(c->stream));
    const i64 total = c->h_peek->k6.total, padded = c->h_peek->k6.padded, listed = c->h_peek->k6.listed, n_long = c->h_peek->k6.n_long;
    if (listed == 0) return LH_OK;
    if (total > 0) {
        if (total > c->rjob_cap) {
            DevGroup& g = c->rjob_mem;
            g.release(); c->rjob_cap = 0;
            const i64 cap = total + total / 4 + 1024;
            DALLOC(g, c->d_rjobs, cap); DALLOC(g, c->d_rorder, cap + 8 * LH_RJ_NB); DALLOC(g, c->d_rorder2, cap + 8 * LH_RJ_NB);
            c->rjob_cap = cap;
        }
        HIPCHK(hipMemsetAsync(c->d_rorder, 0xff, (size_t)padded * 4, c->stream));
        resc_enum(std::true_type(), (int)((listed + 255) / 256));
        { int rc = rescue_sw(c->stream, ix, o, total, c->d_rjobs, seq, c->d_rmeta, c->d_rkeys, c->d_rorder, padded, c->d_rorder2, total + 8 * LH_RJ_NB, c->d_ctr,
                             (c->flags & LH_F_RESCUE_FULL) != 0, 0); if (rc) return rc; }
        LH_LAUNCH(k_resc_cells2, (int)((total + 4095) / 4096 < 1024 ? (total + 4095) / 4096 : 1024), 256, c->stream, total, (const RJob*)c->d_rjobs, o.min_seed_len * o.a, c->d_ctr);
    }
    // the few pairs with long lists (LH_RA_CAP_BIG entries of LDS per wave) beside the others: disjoint pairs, and a single long pair can take as long as all the short ones
    if (n_long > 0) {
        HIPCHK(hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
        resc_apply(std::integral_constant<int, LH_RA_CAP_BIG>(), (int)(listed < 2048 ? listed : 2048), c->aux[0]);
        HIPCHK(hipEventRecord(c->ev_join[0], c->aux[0]));
    }
    resc_apply(std::integral_constant<int, LH_RA_CAP>(), (int)(listed < 16384 ? listed : 16384), c->stream);
    if (n_long > 0) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[0], 0));
    return LH_OK;
}
static int rescue_run(lh_context* c, const DOpts& o, const DIndex& ix) {
    { int rc = rescue_dir<0>(c, o, ix); if (rc) return rc; }   // read 1 from read 2's hits (gobwa.go:286-301)
    { int rc = rescue_dir<1>(c, o, ix); if (rc) return rc; }   // read 2 from read 1's hits, the rescued ones among them (gobwa.go:309-325)
#ifdef LH_RFA_PROF
    { int rc = prof_rescue(c); if (rc) return rc; }
#endif
#ifdef LH_RA_HIST
    { int rc = hist_rescue(c); if (rc) return rc; }
#endif
    return LH_OK;
}

// K4 for the reads the wave kernel chained (k_extend2.h, THE LONG QUEUE), on stream st (the rounds of the other reads run beside it)
#ifndef LH_EXT_LONG_DIV
#define LH_EXT_LONG_DIV 8        // fewer listed reads than 1 / 8 of the batch AND fewer than LH_EXT_LONG_MIN: the wave-per-read kernel, as before
#endif
#ifndef LH_EXT_LONG_MIN
#define LH_EXT_LONG_MIN 16384    // (r05) ... an absolute count: a batch in which 5 % of the pairs lie on repeat copies lists 150 k reads of 4 M — the wave-per-read
#endif                           // kernel took as long for them (154 ms) as the long queue takes for the 600 k of a batch that has nothing else
static inline int ext_long_min(int N) { const int a = N / LH_EXT_LONG_DIV; return a < LH_EXT_LONG_MIN ? a : LH_EXT_LONG_MIN; }
#ifndef LH_EXT_LONG_TAIL
#define LH_EXT_LONG_TAIL 1024    // the rounds stop when fewer jobs than this are queued (a round costs its slowest DP whatever it holds)
#endif
#ifndef LH_EXT_LONG_GROUP
#define LH_EXT_LONG_GROUP 4      // rounds between two looks at the queue
#endif
// k_extend, the wave-per-read kernel (k_extend.h), for the reads of a list on the device (range: its bounds); no list: every read of the batch, a wave each.
// count: the chains of these reads are not in the counters yet
static void launch_extend(lh_context* c, const DOpts& o, hipStream_t st, const int32_t* list, const int32_t* range, int count) {
    const int N = c->b.n_reads;
    LH_LAUNCH(k_extend, list && N > 16384 ? 16384 : N, 64, st, c->idx->d, o, N, list, range, c->b.seq, c->q4, c->b.seq_off, c->d_seed_off, c->d_chains, c->d_cseeds, c->d_n_chains,
              c->d_srt, c->d_ord, c->d_reg_off, c->d_regs, c->d_n_regs, c->d_ctr, count);
}
// the jobs queued in J->count[cur] (keys and list: jkey, jlist) sorted by kind and size into jorder, for k_ext_round; other: the queue the round fills (the long queue's
// two take turns), or -1
static void ext_sort_jobs(hipStream_t st, int grid, DExtJobs* J, int cur, int other, const int32_t* jkey, const int32_t* jlist, int32_t* jorder) {
    LH_LAUNCH(k_extj_count, grid, 256, st, (const int32_t*)(J->count + cur), jkey, J);
    LH_LAUNCH(k_extj_offsets, 1, 256, st, J, cur, other);
    LH_LAUNCH(k_extj_scatter, grid, 256, st, (const int32_t*)(J->count + cur), jkey, jlist, J, jorder);
}
static int ext_long_queue(lh_context* c, const DOpts& o, hipStream_t st) {
    const int N = c->b.n_reads;
    const DIndex& ix = c->idx->d;
    const ExtLongLists Q(c->d_ext_long, (size_t)c->cap_reads);
    const ExtUnits U(c->d_ext_u, (size_t)c->pool_cap);
    DExtJobs* J = c->d_ext_jobs2;
    ExtArgs A = ext_args(c);
    const int gw = N < 16384 ? N : 16384;
    HIPCHK(hipMemsetAsync(J, 0, sizeof(DExtJobs), st));
    // J->wave_range[1]: the reads whose chains take the rounds; J->heavy_range: the ones k_extend prepares and extends (all of them when they are few);
    // J->defer_range: the ones k_ext_merge hands to k_extend; J->count[0]: the units; J->count[1], [2]: the queued jobs, in turn; J->count[3]: the calls for k_ext_wround
    LH_LAUNCH(k_ext_prep, gw, 64, st, ix, o, (const int32_t*)c->d_aln_r, (const int32_t*)c->d_ext_jobs->wave_range, ext_long_min(N), A, c->d_srt, c->d_chain_rmax,
              U.u_read, Q.long_list, J->wave_range + 1, Q.fb_list, J->heavy_range + 1, U.ulist, J->count, c->d_ctr);
    // (before the host looks at the queue: with few listed reads — the usual batch — this is all there is, and it should start at once)
    launch_extend(c, o, st, Q.fb_list, J->heavy_range, 1);
    LH_LAUNCH(k_ext_round0, 2560, 64, st, ix, o, (const int32_t*)U.ulist, (const int32_t*)J->count, A, J->count + 1, U.jlist, U.jkey, c->d_ctr);
    int cur = 1;
    for (int rounds = 0;; rounds += LH_EXT_LONG_GROUP) {
        LH_LAUNCH(k_peek_i32, 1, 1, st, (const int32_t*)(J->count + cur), &c->h_peek->one);
        HIPCHK(hipStreamSynchronize(st));
        const i64 n_jobs = c->h_peek->one;
        if (lh_debug_sync()) fprintf(stderr, "[lh] K4 long queue: %lld jobs queued after %d rounds\n", (long long)n_jobs, rounds);
        if (n_jobs < LH_EXT_LONG_TAIL || rounds >= 4096) {
            if (n_jobs > 0) LH_LAUNCH(k_ext_flush, (int)((n_jobs + 255) / 256), 256, st, (const int32_t*)(J->count + cur), (const int32_t*)U.jlist, A);
            break;
        }
        const int gs = (int)((n_jobs + 1023) / 1024 < 256 ? (n_jobs + 1023) / 1024 : 256);
        for (int u = 0; u < LH_EXT_LONG_GROUP; ++u) {
            const int other = cur ^ 3;
            ext_sort_jobs(st, gs, J, cur, other, U.jkey, U.jlist, U.jorder);
            LH_LAUNCH(k_ext_round<true>, 2560, 64, st, ix, o, (const int32_t*)(J->range + 2 * cur), J->next + cur, (const int32_t*)U.jorder, A, J->count + other, U.jlist, U.jkey,
                      J->count + 3, U.ulist, c->d_ctr);   // (a unit's verdict 2: its call is made by a whole wave, next; the unit list is free after round 0)
            LH_LAUNCH(k_ext_wround, gw, 64, st, ix, o, (const int32_t*)U.ulist, (const int32_t*)(J->count + 3), &J->wnext, A, J->count + other, U.jlist, U.jkey, c->d_ctr);
            cur = other;
        }
    }
    LH_LAUNCH(k_ext_merge, gw, 64, st, o, (const int32_t*)Q.long_list, (const int32_t*)(J->wave_range + 1), A, c->d_regs_tmp, J->defer_range + 1, Q.defer, J->kinds);
    if (lh_debug_sync()) {
        DExtJobs hj;
        if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(&hj, J, sizeof hj, hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[lh] K4 long queue: %d reads as %d chain units, %d reads left to k_extend before and %d after the rounds; (still queued: %d, more than %d regions: %d, a seed inside an earlier chain's region: %d); jobs: narrow %d + %d, live-interval %d + %d, short full-band %d + %d\n",
                    hj.wave_range[1], hj.count[0], hj.heavy_range[1], hj.defer_range[1], hj.kinds[0], LH_EXT_MERGE_CAP, hj.kinds[1], hj.kinds[2], hj.kinds[3], hj.kinds[6], hj.kinds[4], hj.kinds[7], hj.kinds[5], hj.kinds[8]);
    }
    launch_extend(c, o, st, Q.defer, J->defer_range, 0);
    return LH_OK;
}

static int stage2_run(lh_context* c, const DOpts& o, int& t) {
    int N = c->b.n_reads;
    const DIndex& ix = c->idx->d;
    c->ran_inference = false;
    if (c->flags & LH_F_EXT_WAVE) {   // wave-per-read extension (k_extend.h), kept for A/B measurements
        T_BEGIN("k_extend");
        launch_extend(c, o, c->stream, nullptr, nullptr, 1);
        T_END();
    } else {   // a read's control flow on one lane (round 0 ran at the end of k_chain_lane), its DPs in rounds of sorted jobs (k_extend2.h)
        if ((i64)LH_MAXLEN * o.a + (o.pen_clip5 > o.pen_clip3 ? o.pen_clip5 : o.pen_clip3) >= 8192)
            return set_err(LH_E_LIMIT, "match score too large for the packed DP cells of the lane DP (need 250*a + clip bonus < 8192)");
        const int gl = (N + 63) / 64;
        const int gs = (N + 1023) / 1024 < 256 ? (N + 1023) / 1024 : 256, glr = gl < 2560 ? gl : 2560;   // persistent / grid-stride kernels (16 KB of LDS per wave: 10 waves per CU): a round without jobs costs a few microseconds
        bool long_q = true;
        const bool serial = (c->flags & LH_F_EXT_SERIAL) != 0;   // per-round timings: the wave-chained reads first, on the same stream
        ExtArgs A = ext_args(c);
        DExtJobs* const J = c->d_ext_jobs;
        // reads with many seeds or chains (chained by the wave kernel): extended by the wave-per-read kernel (parallel over seeds and
        // columns), beside the rounds of the others (disjoint reads; ONE auxiliary stream: with more, two contexts of a process exceed
        // the hardware queues and serialise each other)
        if (serial) {
            T_BEGIN("k_extend(wave-chained)");
            { int rc = ext_long_queue(c, o, c->stream); if (rc) return rc; }
            T_END();
            T_BEGIN("k_extend(heavy)");
            launch_extend(c, o, c->stream, c->d_ext_heavy, J->heavy_range, 0);   // a long side behind an indel or many mismatches (round 0's verdict)
            T_END();
        } else {
            T_BEGIN("k_extend(rounds)");
            HIPCHK(hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
            // the reads the wave kernel chained, beside the rounds below.  Through the long queue or by the wave-per-read kernel: both give the same
            // regions, so the choice may rest on the PREVIOUS batch of this context — few such reads there (unique sequence) -> the wave-per-read
            // kernel at once; otherwise the long queue, after the rounds have been queued (the host looks at its length as it goes)
            const i64 hint = c->ext_hint_valid ? c->h_peek->prev_wave_reads : -1;
            long_q = !(hint >= 0 && hint < ext_long_min(N));
            if (!long_q) launch_extend(c, o, c->aux[0], c->d_aln_r, J->wave_range, 1);
            launch_extend(c, o, c->aux[0], c->d_ext_heavy, J->heavy_range, 0);   // a long side behind an indel or many mismatches (round 0's verdict)
        }
        static const char* const round_names[8] = {"k_ext_round 1", "k_ext_round 2", "k_ext_round 3", "k_ext_round 4", "k_ext_round 5", "k_ext_round 6", "k_ext_round 7", "k_ext_round 8"};
        for (int k = 1; k <= LH_EXT_ROUNDS; ++k) {
            if (serial) T_BEGIN(round_names[k - 1 < 8 ? k - 1 : 7]);
            ext_sort_jobs(c->stream, gs, J, k, -1, c->d_ext_jkey, c->d_ext_jlist, c->d_ext_jorder);
            // the round queues what needs a further DP for the next one; after the last round that is the wave kernel's list
            const bool last = k == LH_EXT_ROUNDS;
            LH_LAUNCH(k_ext_round<false>, glr, 64, c->stream, ix, o, (const int32_t*)(J->range + 2 * k), J->next + k, (const int32_t*)c->d_ext_jorder, A, last ? J->defer_range + 1 : J->count + k + 1,
                      last ? c->d_ext_defer : c->d_ext_jlist, last ? (int32_t*)nullptr : c->d_ext_jkey, J->defer_range + 1, c->d_ext_defer, c->d_ctr);
            if (serial) T_END();
        }
        if (!serial) {
            if (long_q) { int rc = ext_long_queue(c, o, c->aux[0]); if (rc) return rc; }
            LH_LAUNCH(k_peek_i32, 1, 1, c->aux[0], (const int32_t*)(c->d_ext_jobs->wave_range + 1), &c->h_peek->prev_wave_reads);
            c->ext_hint_valid = true;
            HIPCHK(hipEventRecord(c->ev_join[0], c->aux[0]));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[0], 0));
            T_END();
        }
        T_BEGIN("k_extend(deferred)");
        launch_extend(c, o, c->stream, c->d_ext_defer, J->defer_range, 0);   // reads the rounds left to the wave kernel (their chains were counted by k_chain_lane)
        T_END();
    }
    if (lh_debug_sync()) {   // development aid: sanity of k_extend's output before the order-dependent stages
        std::vector<int32_t> nr, sc;
        std::vector<i64> ro;
        D2H(nr, c->d_n_regs, N); D2H(sc, c->d_seed_cnt, N); D2H(ro, c->d_reg_off, N + 1);
        int mx = 0, bad = 0; long tot = 0;
        for (int r = 0; r < N; ++r) { if (nr[r] > mx) mx = nr[r]; if (nr[r] < 0 || nr[r] > sc[r]) bad++; tot += nr[r]; }
        fprintf(stderr, "[lh] after k_extend: max n_regs=%d total=%ld reads_with_bad_count=%d\n", mx, tot, bad);
        if (!(c->flags & LH_F_EXT_WAVE)) {
            DExtJobs hj;
            if (hipMemcpy(&hj, c->d_ext_jobs, sizeof hj, hipMemcpyDeviceToHost) == hipSuccess) {
                fprintf(stderr, "[lh] K4: %d reads chained and extended by the wave kernels, %d / %d left to the wave extension kernel by round 0 / the later rounds\n", hj.wave_range[1], hj.heavy_range[1], hj.defer_range[1]);
                for (int k = 1; k <= LH_EXT_ROUNDS; ++k)
                    fprintf(stderr, "[lh] K4 round %d: %d jobs (narrow %d, live-interval %d, short full-band %d)\n", k, hj.count[k], hj.kinds[3 * k], hj.kinds[3 * k + 1], hj.kinds[3 * k + 2]);
            }
        }
    }
    T_BEGIN("k_dedup");
    // the lane form for the reads that did not get it where their extension finished (every read: LH_F_TAIL_PASSES, LH_F_EXT_WAVE), then the wave kernel over what
    // either listed.  The list's counter was cleared with K4's job block before K3 (run_front) and has been appended to since round 0
    int32_t* const dd_count = &c->d_ext_jobs->dd_need;
    LH_LAUNCH(k_dedup_fast, (N + 255) / 256, 256, c->stream, ix, o, N, (const i64*)c->d_reg_off, c->d_regs, c->d_n_regs, c->d_best, c->d_dd_list, dd_count, c->d_reg_clean,
              (const uint8_t*)(dedup_fused(c) ? c->d_dd_done : nullptr));
    LH_LAUNCH(k_dedup, N < 16384 ? N : 16384, 64, c->stream, ix, o, N, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->d_regs_tmp, c->d_ia, c->d_n_regs, c->d_best, c->d_ctr,
              (const int32_t*)c->d_dd_list, (const int32_t*)dd_count, c->d_reg_clean);
    T_END();
    if (c->dump_stop_after_dedup) return LH_OK;
    T_BEGIN("k_rescue");
    { int rc = rescue_run(c, o, ix); if (rc) return rc; }
    T_END();
    T_BEGIN("k_scan_cands");
    if (c->dl_pending) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_dl, 0));   // the previous batch's result is still on its way to the host: its arrays are written from here on
    { int rc = run_scan(c, N, c->d_n_regs, 0, 1, c->R.cand_off); if (rc) return rc; }
    T_END();
    i64 total = 0;   // the batch's candidates (a read without a region has one: its placeholder)
    {   // the candidate arrays follow the batch: grow them before K7 writes there
        LH_LAUNCH(k_peek_i64, 1, 1, c->stream, (const i64*)(c->R.cand_off + N), &c->h_peek->one);
        HIPCHK(hipStreamSynchronize(c->stream));
        total = c->h_peek->one;
        if (total > c->cand_cap) {
            if (c->dl_pending) HIPCHK(hipEventSynchronize(c->ev_dl));   // (the arrays about to be replaced are being copied)
            int rc = alloc_cand_pools(c, total + total / 4);
            if (rc) return rc;
        }
    }
    T_BEGIN("k_aln_fast");
    HIPCHK(hipMemsetAsync(c->d_aln_count, 0, sizeof(AlnCounts), c->stream));
    HIPCHK(hipMemsetAsync(c->R.mm_xctr, 0, sizeof(int32_t), c->stream));
    {   // (K5's and K6's per-read best scores are dead by now: d_best holds K7's; the read of every candidate slot goes where K8 will write the same numbers)
        const i64 n_cand = total < c->cand_cap ? total : c->cand_cap;
        LH_LAUNCH(k_aln_prep, (N + 255) / 256, 256, c->stream, o, N, c->b.seq_off, c->d_reg_off, c->d_regs, c->d_n_regs, c->R, c->cand_cap, c->d_status, c->d_best, c->S.cand_read);
        if (n_cand > 0)
            LH_LAUNCH(k_aln_flat, (int)((n_cand + 255) / 256), 256, c->stream, ix, o, n_cand, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->R, c->d_status, c->d_aln_r, c->d_aln_ci,
                      &c->d_aln_count->flat, c->d_ctr, c->q4, (const int32_t*)c->d_best, (const int32_t*)c->S.cand_read);
    }
    // K8's prologue needs the candidate offsets and nothing else: the defaults of the inference columns and the barcodes' order run on the auxiliary stream beside
    // K7's DP kernels, which touch none of what they write (rfa_run joins them before k_rfa_tag).  They start behind k_aln_flat — two passes over memory side by
    // side only share its bandwidth — and are launched when K7's own launches are out, so that the device never waits for the host to issue them
    c->rfa_pre = o.run_inference != 0 && !(c->flags & LH_F_TAIL_PASSES);
    if (c->rfa_pre) HIPCHK(hipEventRecord(c->ev_fork, c->stream));
    const int g7 = N < c->grid_aln ? N : c->grid_aln;
    T_END();
    T_BEGIN("k_aln");
    const RegsTmpLists T7(c->d_regs_tmp, (size_t)c->regpool_cap);   // (K5's and K6's region scratch is dead by now: the lists of the candidates K7's kernels hand on)
    AlnCounts* const n7 = c->d_aln_count;
    // (r06) equal spans and five or six mismatches: a second, longer look without the DP (aln_deep_check) at what k_aln_flat listed
    LH_LAUNCH(k_aln_flat2, g7 < 2048 ? g7 : 2048, 256, c->stream, ix, o, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->R, c->d_status, (const int32_t*)c->d_aln_r, (const int32_t*)c->d_aln_ci,
              (const int32_t*)&n7->flat, T7.deep_r, T7.deep_ci, &n7->grp16, c->d_ctr, c->q4, (const int32_t*)c->d_best);
    LH_LAUNCH(k_aln_grp<16>, g7, 64, c->stream, ix, o, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->d_n_regs, c->R, c->d_status, c->d_ctr, (const int32_t*)T7.deep_r,
              (const int32_t*)T7.deep_ci, (const int32_t*)&n7->grp16, T7.wide_r, T7.wide_ci, &n7->grp32);
    // (r05) what four-per-wave in a band of 7 could not settle: two per wave in a band of 15; the first kernel's input list is free by now and takes what is still left for k_aln
    LH_LAUNCH(k_aln_grp<32>, g7, 64, c->stream, ix, o, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->d_n_regs, c->R, c->d_status, c->d_ctr, (const int32_t*)T7.wide_r,
              (const int32_t*)T7.wide_ci, (const int32_t*)&n7->grp32, c->d_aln_r, c->d_aln_ci, &n7->full);
    LH_LAUNCH(k_aln, g7, 64, c->stream, ix, o, N, c->b.seq, c->b.seq_off, c->d_reg_off, c->d_regs, c->d_n_regs, c->R, c->cand_cap, c->d_zpool, c->d_status, c->d_ctr,
              (const int32_t*)c->d_aln_r, (const int32_t*)c->d_aln_ci, (const int32_t*)&n7->full);
    if (c->rfa_pre) {
        HIPCHK(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
        rfa_prologue(c, c->aux[0]);
        HIPCHK(hipEventRecord(c->ev_join[0], c->aux[0]));
    }
    T_END();
    if (o.run_inference) { int rc = rfa_run(c, o, t); if (rc) return rc; }
    return LH_OK;
}

static int stage2_dump_regs(lh_context* c, DumpArenaH* A) {
    int N = c->b.n_reads;
    std::vector<i64> reg_off;
    std::vector<int32_t> n_regs;
    std::vector<DReg> regs;
    D2H(reg_off, c->d_reg_off, N + 1); D2H(n_regs, c->d_n_regs, N);
    i64 tot = reg_off[N] < c->regpool_cap ? reg_off[N] : c->regpool_cap;
    D2H(regs, c->d_regs, tot);
    A->reg_off.assign(1, 0);
    for (int r = 0; r < N; ++r) {
        for (int i = 0; i < n_regs[r]; ++i) {
            const DReg& g = regs[reg_off[r] + i];
            A->reg_rb.push_back(g.rb); A->reg_re.push_back(g.re); A->reg_qb.push_back(g.qb); A->reg_qe.push_back(g.qe); A->reg_rid.push_back(g.rid);
            A->reg_score.push_back(g.score); A->reg_truesc.push_back(g.truesc); A->reg_w.push_back(g.w); A->reg_seedcov.push_back(g.seedcov);
            A->reg_seedlen0.push_back(g.seedlen0); A->reg_csub.push_back(g.csub); A->reg_secondary.push_back(g.secondary);
        }
        A->reg_off.push_back((i64)A->reg_rb.size());
    }
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ result download
// dst[off[i] + k] = src[i*stride + k] for k < n[i]; entries past the slots (k >= stride) come from xsrc[xoff[i] + k - stride] (DCand::mm_x*)
__global__ void __launch_bounds__(256) k_pack_slots(int n_items, const int32_t* __restrict__ n, const i64* __restrict__ off, const uint32_t* __restrict__ src, int stride,
                                                     uint32_t* __restrict__ dst, const int32_t* __restrict__ xoff, const uint32_t* __restrict__ xsrc) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    int m = n[i];
    i64 o = off[i];
    const uint32_t* s = src + (size_t)i * stride;
    for (int k = 0; k < m && k < stride; ++k) dst[o + k] = s[k];
    if (m > stride) { const uint32_t* x = xsrc + xoff[i]; for (int k = stride; k < m; ++k) dst[o + k] = x[k - stride]; }
}

// The result lives in ONE pinned host block per batch: every array is copied device -> its final place by an asynchronous
// copy on the context's stream (no staging copy, no per-array synchronisation), and blocks are recycled between batches
// (pinning ~350 MB per million pairs costs more than copying them).
struct ResultArenaH {
    lh_result r;
    PinBlock blk;
    std::shared_ptr<PinPool> pool;
    void* merged = nullptr;   // a result merged from two lanes owns one malloc'ed block instead of a pinned one
};

__global__ void __launch_bounds__(256) k_status_or(int n, const int32_t* __restrict__ status, int32_t* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int v = i < n ? status[i] : 0;
    for (int m = 32; m >= 1; m >>= 1) v |= __shfl_xor(v, m);
    if (LANE() == 0 && v) atomicOr(out, v);
}
// What a pipeline's result must pass before anything reads it, the download (pipe_download_begin) and the BAM encoder's device gather (lh_bam_append_resident) alike:
// no read over a per-read limit (named in the message), no overflowed workspace, a candidate total within the pools, no watchdog word.  *n_cand: the candidate total
static int pipe_result_check(lh_context* c, i64* n_cand) {
    HIPCHK(hipSetDevice(c->idx->device));
    const int N = c->b.n_reads;
    // two small read-backs first: the OR of the status words, the candidate total
    int32_t* const status_or = &c->d_aln_count->flat;   // (K7's counter: free by now)
    HIPCHK(hipMemsetAsync(status_or, 0, sizeof(int32_t), c->stream));
    if (N > 0) LH_LAUNCH(k_status_or, (N + 255) / 256, 256, c->stream, N, (const int32_t*)c->d_status, status_or);
    int32_t bad = 0;
    i64 C = 0;
    HIPCHK(hipMemcpyAsync(&bad, status_or, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&C, c->R.cand_off + N, sizeof C, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad & (LH_ST_INTV_OVERFLOW | LH_ST_CIGAR_OVERFLOW | LH_ST_MM_OVERFLOW | LH_ST_TOO_LONG)) {
        // a per-read / per-candidate slot limit: splitting the batch cannot help, so name the read (the host can route it elsewhere)
        std::vector<int32_t> st(N);
        HIPCHK(hipMemcpy(st.data(), c->d_status, (size_t)N * 4, hipMemcpyDeviceToHost));
        int first = -1, n_bad = 0;
        for (int r = 0; r < N; ++r)
            if (st[r] & (LH_ST_INTV_OVERFLOW | LH_ST_CIGAR_OVERFLOW | LH_ST_MM_OVERFLOW | LH_ST_TOO_LONG)) { if (first < 0) first = r; ++n_bad; }
        return set_err(LH_E_LIMIT, "read " + std::to_string(first) + " (pair " + std::to_string(first / 2) + ") exceeds a per-read limit (status bits " + std::to_string(first >= 0 ? st[first] : bad) +
                                       ": 1 = more than " + std::to_string(LH_BIG_INTV) + " SMEM intervals, 2 = reference span over 704, 4 = more than 64 CIGAR operations, 8 = more than 64 mismatch loci); " +
                                       std::to_string(n_bad) + " such reads in the batch");
    }
    if (bad & LH_ST_POOL_OVERFLOW)
        return set_err(LH_E_CAPACITY, "a per-batch device workspace overflowed: split the batch");
    if (C > c->cand_cap) return set_err(LH_E_CAPACITY, "candidate pool overflow");
    {   // watchdog slots of the kernels' bounded loops: any trip means this result may be incomplete.  The slots belong to THIS pipeline (its
        // kernels get them through DOpts::wd), so a trip fails the download of the batch it happened in and no other; they are cleared once
        // reported, so one bad batch does not fail every later one.
        int32_t h[LH_WD_SLOTS];
        HIPCHK(hipMemcpyAsync(h, c->d_wd, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < LH_WD_SLOTS; ++i)
            if (h[i]) {
                HIPCHK(hipMemsetAsync(c->d_wd, 0, sizeof h, c->stream));
                return set_err(LH_E_HIP, "a kernel watchdog tripped (slot " + std::to_string(i) + "): the batch's results are not trustworthy");
            }
    }
    *n_cand = C;
    return LH_OK;
}
// The result leaves in two steps so that a host with ONE context can have batch k's download under batch k + 1's kernels (the reference
// double-buffers its work units the same way: lariat.go:333, bamwriter.go:188): pipe_download_begin checks the batch's status, packs the
// variable-length arrays and ENQUEUES the device-to-host copies on the context's copy stream; pipe_download_end waits for them and hands
// out the result.  In between the host may call lh_align_resident for the next batch: its kernels up to the mate rescue do not touch the
// result arrays, and it waits for the copies (ev_dl) before the first one that does.
static int pipe_download_begin(lh_context* c) {
    if (!c) return set_err(LH_E_ARG, "lh_result_download: null argument");
    if (!c->ran) return set_err(LH_E_ARG, "nothing to download: call lh_align_resident first");
    if (c->dl_pending) return set_err(LH_E_ARG, "lh_result_download_begin: the previous download has not been collected (lh_result_download_end)");
    if (c->rounds.n_rounds > 1) {   // a batch aligned in rounds: every part was downloaded and merged inside lh_align_resident, nothing is left to enqueue
        if (!c->round_result) return set_err(LH_E_ARG, "lh_result_download: the result of a batch aligned in rounds is handed out once");
        lh_result* r = c->round_result;
        c->round_result = nullptr;
        c->dl_pending = true;
        c->dl_finish = [r](lh_result** out) -> int { *out = r; return LH_OK; };
        return LH_OK;
    }
    const int N = c->b.n_reads;
    i64 C = 0;
    { int rc = pipe_result_check(c, &C); if (rc) return rc; }
    { int rc = run_scan(c, (int)C, c->R.n_cigar, 0, 0, c->d_cigar_off); if (rc) return rc; }
    { int rc = run_scan(c, (int)C, c->R.n_mm, 0, 0, c->d_mm_off); if (rc) return rc; }
    i64 tc = 0, tm = 0;
    HIPCHK(hipMemcpyAsync(&tc, c->d_cigar_off + C, sizeof tc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tm, c->d_mm_off + C, sizeof tm, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (tc > c->pack_cap || tm > c->pack_cap) {   // more than 8 entries per candidate on average: grow the staging buffers
        int rc = alloc_pack(c, (tc > tm ? tc : tm) + 1024);
        if (rc) return rc;
    }
    // layout of the pinned block: the columns of LH_RESULT_COLS (lh_result_cols.h), then the counters' slots
    size_t total = 0;
    auto reserve = [&](size_t bytes) { size_t o = total; total += (bytes + 63) & ~(size_t)63; return o; };
    const bool inf = c->ran_inference;
    std::array<size_t, LH_N_COLS> cnt, off;   // per column: elements, place in the block
    for (size_t i = 0; i < LH_N_COLS; ++i) {
        cnt[i] = col_count(LH_RESULT_COLS[i], (size_t)N, (size_t)C, (size_t)tc, (size_t)tm);
        off[i] = reserve(cnt[i] * LH_RESULT_COLS[i].elt);
    }
    DCand& R = c->R;
    const size_t o_ctr = reserve(sizeof(DCounters) * LH_CTR_SLOTS);
    total += 64;
    ResultArenaH* A = new ResultArenaH();
    A->pool = c->pin_pool;
    {
        std::lock_guard<std::mutex> g(c->pin_pool->mu);
        for (size_t i = 0; i < c->pin_pool->free_.size(); ++i)
            if (c->pin_pool->free_[i].cap >= total) { A->blk = c->pin_pool->free_[i]; c->pin_pool->free_.erase(c->pin_pool->free_.begin() + (long)i); break; }
    }
    if (!A->blk.p) {
        size_t cap = total + total / 8;
        if (hipHostMalloc((void**)&A->blk.p, cap, hipHostMallocDefault) != hipSuccess) { delete A; return set_err(LH_E_HIP, "hipHostMalloc failed for the result block"); }
        A->blk.cap = cap;
    }
    char* B = A->blk.p;
#define LH_FAIL(expr) do { if ((expr) != hipSuccess) { lh_result_free(&A->r); return set_err(LH_E_HIP, #expr " failed"); } } while (0)
    A->r.arena_ = A;
    // the counters first, on the compute stream (the next batch clears them when it starts)
    LH_FAIL(hipMemcpyAsync(B + o_ctr, c->d_ctr, sizeof(DCounters) * LH_CTR_SLOTS, hipMemcpyDeviceToHost, c->stream));
    if (C > 0) {   // CIGAR ops and mismatch loci: packed on the device (only the used entries cross PCIe), each into its own staging buffer
        int g = (int)((C + 255) / 256);
        LH_LAUNCH(k_pack_slots, g, 256, c->stream, (int)C, (const int32_t*)R.n_cigar, (const i64*)c->d_cigar_off, (const uint32_t*)R.cigar, LH_MAX_CIGAR, c->d_pack_a, (const int32_t*)nullptr, (const uint32_t*)nullptr);
        LH_LAUNCH(k_pack_slots, g, 256, c->stream, (int)C, (const int32_t*)R.n_mm, (const i64*)c->d_mm_off, (const uint32_t*)R.mm_read, LH_MAX_MM, c->d_pack_b, (const int32_t*)R.mm_xoff, (const uint32_t*)R.mm_xread);
        LH_LAUNCH(k_pack_slots, g, 256, c->stream, (int)C, (const int32_t*)R.n_mm, (const i64*)c->d_mm_off, (const uint32_t*)R.mm_ref, LH_MAX_MM, c->d_pack_c, (const int32_t*)R.mm_xoff, (const uint32_t*)R.mm_xref);
    }
    LH_FAIL(hipEventRecord(c->ev_pack, c->stream));
    LH_FAIL(hipStreamWaitEvent(c->dl_stream, c->ev_pack, 0));
    for (size_t i = 0; i < LH_N_COLS; ++i) {   // every column straight to its place (an inference column only if the inference ran)
        const ResultCol& k = LH_RESULT_COLS[i];
        if (cnt[i] && (inf || k.src != FROM_INF)) LH_FAIL(hipMemcpyAsync(B + off[i], col_dev(c, k), cnt[i] * k.elt, hipMemcpyDeviceToHost, c->dl_stream));
    }
    LH_FAIL(hipEventRecord(c->ev_dl, c->dl_stream));
    LH_FAIL(hipStreamSynchronize(c->stream));   // (the counters and the pack kernels: short)
#undef LH_FAIL
    c->dl_pending = true;
    c->dl_finish = [=](lh_result** out) -> int {
    if (hipEventSynchronize(c->ev_dl) != hipSuccess) { lh_result_free(&A->r); return set_err(LH_E_HIP, "the result's device-to-host copies failed"); }
    lh_result& r = A->r;
    void* keep = r.arena_;
    memset(&r, 0, sizeof r);
    r.arena_ = keep;
    r.abi_version = LH_ABI_VERSION; r.n_reads = N; r.n_cand = C;
    for (size_t i = 0; i < LH_N_COLS; ++i) {
        const ResultCol& k = LH_RESULT_COLS[i];
        if (!inf && k.src == FROM_INF) fill_col(B + off[i], cnt[i], k);   // candidate generation only: the inference fields hold the Alignment defaults (lariat.go:1655-1689)
        set_ptr_at(&r, k.res_off, B + off[i]);
    }
    const uint64_t* slots = (const uint64_t*)(B + o_ctr);   // LH_CTR_SLOTS copies of DCounters: their sums are the result's counters
    uint64_t* ctr = result_ctrs(&r);
    for (size_t i = 0; i < LH_CTR_SLOTS; ++i)
        for (size_t q = 0; q < LH_N_CTRS; ++q) ctr[q] += slots[i * LH_N_CTRS + q];
    *out = &A->r;
    return LH_OK;
    };
    return LH_OK;
}
static int pipe_download_end(lh_context* c, lh_result** out) {
    if (!c || !out) return set_err(LH_E_ARG, "lh_result_download: null argument");
    if (!c->dl_pending) return set_err(LH_E_ARG, "lh_result_download_end: no download in flight (lh_result_download_begin)");
    HIPCHK(hipSetDevice(c->idx->device));
    c->dl_pending = false;
    auto fin = std::move(c->dl_finish);
    c->dl_finish = nullptr;
    return fin(out);
}
static int pipe_download(lh_context* c, lh_result** out) {
    if (!out) return set_err(LH_E_ARG, "lh_result_download: null argument");
    int rc = pipe_download_begin(c);
    return rc ? rc : pipe_download_end(c, out);
}

void lh_result_free(lh_result* r) {
    if (!r) return;
    ResultArenaH* A = (ResultArenaH*)r->arena_;
    free(A->merged);
    if (A->blk.p) {
        std::lock_guard<std::mutex> g(A->pool->mu);
        if (A->pool->free_.size() < 4) A->pool->free_.push_back(A->blk);
        else hipHostFree(A->blk.p);
    }
    delete A;
}

// ------------------------------------------------------------------------------------------------ inference (K8)
static int ext_alloc(lh_context* c) {
    DevGroup& g = c->mem;
    DALLOC(g, c->d_ext_defer, c->cap_reads); DALLOC(g, c->d_ext_heavy, c->cap_reads);
    DALLOC(g, c->d_ext_st, c->cap_reads); DALLOC(g, c->d_ext_jlist, c->cap_reads); DALLOC(g, c->d_ext_jkey, c->cap_reads); DALLOC(g, c->d_ext_jorder, c->cap_reads); DALLOC(g, c->d_ext_jobs, 1);
    DALLOC(g, c->d_ext_jobs2, 1); DALLOC(g, c->d_ext_long, ExtLongLists::ints((size_t)c->cap_reads));
    return LH_OK;
}

static int rfa_alloc(lh_context* c) {
    i64 N = c->cap_reads;
    DevGroup& g = c->mem;
    { int rc = alloc_result_cols(c, g, PER_READ, N); if (rc) return rc; }   // the per-read columns of the result (DInf's)
    int want = c->co.rfa_grid;   // 16 single-wave blocks per CU = 4 waves per SIMD
    c->grid_rfa = c->cap_bc < want ? (int)c->cap_bc : want;
    c->slab_bytes = (i64)c->co.rfa_slab_kb << 10;
    DALLOC(g, c->d_slab, (size_t)c->grid_rfa * (size_t)c->slab_bytes);
    // second-chance slabs for barcodes that outgrow the regular ones (up to the reader's 30,000-pair work units)
    // (a 30,000-pair barcode holds 60,000 reads; its molecule x read table is the large one: 1.5 GB = 6,000 molecules)
    c->slab2_bytes = (i64)c->cap_reads * 2048 + ((i64)16 << 20);
    c->grid_rfa2 = 4;
    if (c->slab2_bytes > ((i64)512 << 20)) { c->grid_rfa2 = 2; if (c->slab2_bytes > ((i64)1536 << 20)) c->slab2_bytes = (i64)1536 << 20; }
    DALLOC(g, c->d_slab2, (size_t)c->grid_rfa2 * (size_t)c->slab2_bytes);
    // (r05) between the two: the molecule x read table grows with the square of a barcode's size on repeat families (every candidate position a molecule), and the step from 4,096
    // waves to 4 was a cliff — 2,000 barcodes of 200 pairs on the copies of repeat families, which outgrow 2 MiB, took 38 s instead of 0.1 s.  Up to 1,024 waves x 16 MiB, then
    // up to 64 x 128 MiB (tiers that would not be smaller than the last one are left out: small contexts).  (r06) The tiers' slabs are allocated when a batch first lists a
    // barcode for them, as many as the list is long (rfa_tier_slabs): a context that only ever sees 100-pair barcodes on unique sequence holds none of the 24 GiB.
    {
        static const int def_kb[2] = {16 << 10, 128 << 10}, def_grid[2] = {1024, 64};
        for (int k = 0; k < 2; ++k) {
            c->slab_mid_bytes[k] = 0; c->grid_rfa_mid[k] = 0; c->grid_rfa_mid_max[k] = 0; c->d_slab_mid[k] = nullptr;
            if (c->co.rfa_tier_kb[k] < 0) continue;
            const i64 bytes = (i64)(c->co.rfa_tier_kb[k] > 0 ? c->co.rfa_tier_kb[k] : def_kb[k]) << 10;
            if (bytes <= c->slab_bytes || bytes * 2 > c->slab2_bytes) continue;
            if (k == 1 && c->slab_mid_bytes[0] && bytes <= c->slab_mid_bytes[0]) continue;
            i64 gk = ((i64)c->cap_reads << 15) / bytes;   // (a tier's slabs together: at most 32 KiB per read of the context's capacity)
            const i64 gmax = c->co.rfa_tier_grid[k] > 0 ? c->co.rfa_tier_grid[k] : def_grid[k];
            gk = gk < 1 ? 1 : gk > gmax ? gmax : gk;
            c->slab_mid_bytes[k] = bytes;
            c->grid_rfa_mid_max[k] = c->cap_bc < gk ? (int)c->cap_bc : (int)gk;
        }
    }
    DALLOC(g, c->d_rfa_ovf_mid, RfaOvfMid::ints((size_t)c->cap_bc));
    DALLOC(g, c->d_bc_next, 1);
    DALLOC(g, c->d_rfa_ovf, c->cap_bc + 1); DALLOC(g, c->d_rfa_ovf2, c->cap_bc + 1); DALLOC(g, c->d_rfa_order, RfaOrder::ints((size_t)c->cap_bc));
    DALLOC(g, c->d_rfa_hp, N / 2 + 1); DALLOC(g, c->d_rfa_hr, 2 * N + 2); DALLOC(g, c->d_bc_lmp, c->cap_bc + 1);
    return LH_OK;
}

// the length of an overflow list, read back by a one-thread kernel into mapped host memory (not a copy-engine transfer: those may be busy with the previous result)
static int rfa_list_len(lh_context* c, const int32_t* count, i64* n) {
    LH_LAUNCH(k_peek_i32, 1, 1, c->stream, count, &c->h_peek->rfa_listed);
    HIPCHK(hipStreamSynchronize(c->stream));
    *n = c->h_peek->rfa_listed;
    return LH_OK;
}
// tier k has slabs for a list of `listed` barcodes: as many as the list is long (a wave per slab takes the barcodes off the list one by one, so fewer only cost time),
// grown when a later batch lists more than twice as many
static int rfa_tier_slabs(lh_context* c, int k, i64 listed, bool a_slab_each = false) {
    i64 want = listed < c->grid_rfa_mid_max[k] ? listed : c->grid_rfa_mid_max[k];
    if (want < 1) want = 1;
    // (a_slab_each: the barcodes routed to the tier up front are a batch's largest — two of them in turn on one wave is the launch's duration doubled)
    if (c->d_slab_mid[k] && want <= (a_slab_each ? 1 : 2) * (i64)c->grid_rfa_mid[k]) return LH_OK;
    i64 gk = want + want / 2 + 4;
    gk = gk > c->grid_rfa_mid_max[k] ? c->grid_rfa_mid_max[k] : gk;
    // The new slabs are allocated BEFORE the old ones are freed, and fewer are tried when they do not fit (this runs in the middle of a batch, and of a round): a tier
    // that has slabs keeps them if no larger set can be had — fewer slabs only cost time — and only a tier that cannot get a single slab fails the batch
    const i64 have = c->d_slab_mid[k] ? c->grid_rfa_mid[k] : 0;
    uint8_t* fresh = nullptr;
    DevGroup grown;   // the new slabs; once they are swapped in, the old ones
    DevGroup& into = have ? grown : c->tier_mem[k];
    uint8_t*& slot = have ? fresh : c->d_slab_mid[k];
    for (;; gk = gk / 2 > have ? gk / 2 : have + 1) {
        if (gk <= have) { g_err.clear(); return LH_OK; }
        if (into.alloc(slot, (size_t)gk * (size_t)c->slab_mid_bytes[k]) == LH_OK) break;
        if (gk <= have + 1) { if (have) { g_err.clear(); return LH_OK; } return LH_E_HIP; }   // (the message: dalloc's)
    }
    if (have) {
        HIPCHK(hipStreamSynchronize(c->stream));   // (the launches that use the old slabs)
        std::swap(c->d_slab_mid[k], fresh);        // (a buffer goes with the variable that holds it: DevGroup)
        grown.release();
    }
    c->grid_rfa_mid[k] = (int)gk;
    return LH_OK;
}

// The slabs a launch of k_rfa (post: of k_rfa_post) runs on, with that launch's work counter.  The regular slabs take a wave per barcode up to grid_rfa; a barcode
// that does not fit a tier's slab is listed for the next — the middle tiers 0 and 1, then the few large slabs of the last one: fewer waves, larger slabs
enum { RFA_REGULAR = -1, RFA_LAST = 2 };
static RfaTier rfa_tier(const lh_context* c, int k, bool post) {
    RfaCounters* const n = c->d_bc_next;
    if (k == RFA_REGULAR) return {c->d_slab, c->slab_bytes, c->b.n_bc < c->grid_rfa ? c->b.n_bc : c->grid_rfa, post ? &n->post_next : &n->next};
    if (k == RFA_LAST) return {c->d_slab2, c->slab2_bytes, c->grid_rfa2, post ? &n->post_last_next : &n->last_next};
    return {c->d_slab_mid[k], c->slab_mid_bytes[k], c->grid_rfa_mid[k], post ? &n->tier[k].post_next : &n->tier[k].next};
}
static void launch_rfa_small(lh_context* c, const DOpts& o, const RfaTier& T, hipStream_t st, RfaList in, RfaList out) {
    LH_LAUNCH(k_rfa<1>, T.grid, 64, st, c->idx->d, o, c->b.n_bc, c->b.bc_pair_off, c->b.bc_do_rfa, c->b.name_seed, c->b.cen_start, c->b.cen_end, c->R, c->S, c->cand_cap, T.slab, T.bytes,
              c->d_status, T.next, (const int32_t*)in.list, (const int32_t*)in.count, out.list, out.count, c->d_rfa_hr, &c->d_bc_next->heavy_reads, c->d_bc_lmp);
}
static void launch_rfa(lh_context* c, const DOpts& o, const RfaTier& T, hipStream_t st, RfaList in, RfaList out) {
    LH_LAUNCH(k_rfa<0>, T.grid, 64, st, c->idx->d, o, c->b.n_bc, c->b.bc_pair_off, c->b.bc_do_rfa, c->b.name_seed, c->b.cen_start, c->b.cen_end, c->R, c->S, c->cand_cap, T.slab, T.bytes,
              c->d_status, T.next, (const int32_t*)in.list, (const int32_t*)in.count, out.list, out.count, c->d_rfa_hr, &c->d_bc_next->heavy_reads, c->d_bc_lmp);
}
static void launch_rfa_post(lh_context* c, const DOpts& o, const RfaTier& T, hipStream_t st, RfaList in, RfaList out) {
    LH_LAUNCH(k_rfa_post, T.grid, 64, st, c->idx->d, o, c->b.n_bc, c->b.bc_pair_off, (const i64*)c->b.cen_start, (const i64*)c->b.cen_end, c->R, c->S, c->cand_cap, T.slab, T.bytes,
              c->d_status, T.next, (const int32_t*)in.list, (const int32_t*)in.count, out.list, out.count);
}
// The `listed` barcodes a launch turned away (in), through the middle tiers from k_first on and then the last slabs: only the last one's verdict is final.  (r06) The
// host looks at a list's length before it launches the tier that takes it (one small read-back; nothing is launched for an empty list — the usual batch) and makes
// sure the tier has slabs (rfa_tier_slabs)
static int rfa_cascade(lh_context* c, const DOpts& o, bool post, RfaList in, i64 listed, int k_first) {
    const RfaOvfMid mid(c->d_rfa_ovf_mid, (size_t)c->cap_bc);
    const auto launch = post ? launch_rfa_post : launch_rfa;
    for (int k = k_first; k < 2 && listed > 0; ++k) {
        if (!c->slab_mid_bytes[k]) continue;
        { int rc = rfa_tier_slabs(c, k, listed); if (rc) return rc; }
        RfaCounters::Tier* const n = &c->d_bc_next->tier[k];
        const RfaList out{post ? mid.post[k] : mid.rfa[k], post ? &n->post_n_ovf : &n->n_ovf};
        launch(c, o, rfa_tier(c, k, post), c->stream, in, out);
        in = out;
        { int rc = rfa_list_len(c, in.count, &listed); if (rc) return rc; }
    }
    if (listed > 0) launch(c, o, rfa_tier(c, RFA_LAST, post), c->stream, in, RfaList{nullptr, nullptr});
    return LH_OK;
}

// the first tier has slabs (an earlier batch needed them): the barcodes that cannot fit a regular slab start there at once, beside the first launch
static bool rfa_routes_big(const lh_context* c) { return c->slab_mid_bytes[0] && c->d_slab_mid[0] && c->grid_rfa_mid[0] > 0; }
// K8's prologue: the defaults of the inference columns and the order in which the barcode programs take their barcodes.  Both read the candidate offsets alone
static void rfa_prologue(lh_context* c, hipStream_t st) {
    const RfaOrder ord(c->d_rfa_order, (size_t)c->cap_bc);
    c->rfa_merge_big = !(c->flags & LH_F_RFA_SLAB) && !rfa_routes_big(c);
    LH_LAUNCH(k_rfa_init, 4096, 256, st, c->b.n_reads, c->R, c->S, c->cand_cap);
    LH_LAUNCH(k_rfa_order, 1, 256, st, c->b.n_bc, (const int32_t*)c->b.bc_pair_off, c->R, ord.all, ord.big, ord.rest, (c->flags & LH_F_RFA_SLAB) ? (int32_t*)nullptr : ord.small, c->rfa_merge_big ? 1 : 0, ord.n_all, c->slab_bytes, c->idx->d.n_contigs + 2);
}

static int rfa_run(lh_context* c, const DOpts& o, int& t) {
    RfaCounters* const ctr = c->d_bc_next;
    HIPCHK(hipMemsetAsync(ctr, 0, sizeof(RfaCounters), c->stream));
    T_BEGIN("k_rfa");
    const int N = c->b.n_reads, P = c->b.n_pairs;
    // the wave kernels' scratch: the barcode program's slabs while they fit a pair's lists and Go's generator state (a context made with tiny slabs: the large ones)
    const bool small_ok = c->slab_bytes >= ((i64)1 << 20);
    uint8_t* const wslab = small_ok ? c->d_slab : c->d_slab2;
    const i64 wslab_bytes = small_ok ? c->slab_bytes : c->slab2_bytes;
    const int wgrid = small_ok ? c->grid_rfa : c->grid_rfa2;
    if (c->rfa_pre) { HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[0], 0)); c->rfa_pre = false; }
    else rfa_prologue(c, c->stream);
    LH_LAUNCH(k_rfa_tag, (P + 255) / 256, 256, c->stream, o, P, (const u64*)c->b.name_seed, c->R, c->S, c->cand_cap, c->d_rfa_hp, &ctr->heavy_pairs);
    LH_LAUNCH(k_rfa_tag_w, wgrid, 64, c->stream, o, (const u64*)c->b.name_seed, c->R, c->S, wslab, wslab_bytes, (const int32_t*)c->d_rfa_hp, (const int32_t*)&ctr->heavy_pairs, c->d_status);
    // (r06) most candidates first; the barcodes whose tables cannot fit a regular slab apart (k_rfa_order)
    const RfaOrder ord(c->d_rfa_order, (size_t)c->cap_bc);
    const RfaList all{ord.all, ord.n_all}, big{ord.big, ord.n_big}, rest{ord.rest, ord.n_rest};
    {
        // the first tier has slabs (an earlier batch needed them): the barcodes that cannot fit a regular slab start there at once, on a second stream, beside the first launch;
        // what they leave goes to the list the tier's own launch leaves its overflow in.  No slabs yet: the first launch sees every barcode and turns those away, as before
        const bool pre = rfa_routes_big(c);
        RfaList ovf{c->d_rfa_ovf, &ctr->n_ovf};
        const RfaList routed_ovf{RfaOvfMid(c->d_rfa_ovf_mid, (size_t)c->cap_bc).rfa[0], &ctr->tier[0].n_ovf};
        if (pre) {
            HIPCHK(hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
            RfaTier routed = rfa_tier(c, 0, false);
            routed.next = &ctr->routed_next;
            launch_rfa(c, o, routed, c->aux[0], big, routed_ovf);
            HIPCHK(hipEventRecord(c->ev_join[0], c->aux[0]));
        }
        if (c->flags & LH_F_RFA_SLAB) launch_rfa(c, o, rfa_tier(c, RFA_REGULAR, false), c->stream, pre ? rest : all, ovf);   // every barcode through the regular instance (no small list)
        else {
            // (r13) the small barcodes through the small instance, on the regular slabs; what it turns away (more molecules than its on-chip tables hold) joins the
            // rest list, whose launch follows on the same slabs and reads the list's length when it starts: no look from the host in between.  Without first-tier
            // slabs k_rfa_order has put the big barcodes in front of that list (rfa_merge_big), to be turned away into ovf as before
            RfaTier sm = rfa_tier(c, RFA_REGULAR, false);
            sm.next = &ctr->small_next;
            launch_rfa_small(c, o, sm, c->stream, RfaList{ord.small, ord.n_small}, rest);
            launch_rfa(c, o, rfa_tier(c, RFA_REGULAR, false), c->stream, rest, ovf);
        }
        if (pre) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join[0], 0));
        i64 listed = 0;
        LH_LAUNCH(k_peek_i32, 1, 1, c->stream, (const int32_t*)ord.n_big, &c->h_peek->rfa_routed);   // (read with the list's length below: one synchronisation)
        LH_LAUNCH(k_peek_rfa, 1, 1, c->stream, (const int32_t*)ord.n_all, &c->h_peek->rfa_classes);
        { int rc = rfa_list_len(c, ovf.count, &listed); if (rc) return rc; }
        const i64 n_routed = c->h_peek->rfa_routed;
        c->rfa_cls[0] = n_routed; c->rfa_cls[2] = c->h_peek->rfa_classes & 0xffffffffll; c->rfa_cls[3] = c->h_peek->rfa_classes >> 32;
        c->rfa_cls[1] = (i64)c->b.n_bc - c->rfa_cls[0] - c->rfa_cls[2];
        int k_first = 0;
        if (pre && listed == 0) {   // nothing for the first tier's own launch: what the routed barcodes left there is the next tier's list
            ovf = routed_ovf;
            { int rc = rfa_list_len(c, ovf.count, &listed); if (rc) return rc; }
            k_first = 1;
        }
        { int rc = rfa_cascade(c, o, false, ovf, listed, k_first); if (rc) return rc; }
        // the next batch's routed barcodes each want a slab of the first tier: as many as this batch routed (the tier grows when that is more than twice what it has)
        if (c->slab_mid_bytes[0] && n_routed > 0) { int rc = rfa_tier_slabs(c, 0, n_routed, true); if (rc) return rc; }
    }
    LH_LAUNCH(k_rfa_mq_w, wgrid, 64, c->stream, o, (const i64*)c->b.cen_start, (const i64*)c->b.cen_end, c->R, c->S, wslab, wslab_bytes, (const int32_t*)c->d_rfa_hr,
              (const int32_t*)&ctr->heavy_reads, (const double*)c->d_bc_lmp, c->d_status);
    {
        const RfaList ovf{c->d_rfa_ovf2, &ctr->post_n_ovf};
        launch_rfa_post(c, o, rfa_tier(c, RFA_REGULAR, true), c->stream, all, ovf);
        i64 listed = 0;
        { int rc = rfa_list_len(c, ovf.count, &listed); if (rc) return rc; }
        { int rc = rfa_cascade(c, o, true, ovf, listed, 0); if (rc) return rc; }
    }
    T_END();
#ifdef LH_RFA_PROF
    { int rc = prof_rfa(c); if (rc) return rc; }
#endif
#ifdef LH_RA_HIST
    { int rc = hist_rfa(c); if (rc) return rc; }
#endif
    c->ran_inference = true;
    return LH_OK;
}

// ------------------------------------------------------------------------------------------------ diagnostics
#include "k_diag.h"
int lh_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes) {
    if (!free_bytes || !total_bytes) return set_err(LH_E_ARG, "lh_device_memory: null argument");
    HIPCHK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f; *total_bytes = (int64_t)t;
    return LH_OK;
}

int lh_diag_random_read(int device, int64_t table_bytes, int32_t granule_bytes, int64_t n_access, double* gbps, double* ms_out) {
    if (table_bytes <= 0 || granule_bytes < 16 || granule_bytes % 16 || n_access <= 0) return set_err(LH_E_ARG, "lh_diag_random_read: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    uint8_t* tab = nullptr; uint32_t* sink = nullptr;
    HIPCHK(hipMalloc(&tab, (size_t)table_bytes)); HIPCHK(hipMalloc(&sink, 64));
    HIPCHK(hipMemset(tab, 1, (size_t)table_bytes));
    u64 n_blocks = (u64)table_bytes / (u64)granule_bytes;
    int per_thread = 64;
    i64 threads = (n_access + per_thread - 1) / per_thread;
    int grid = (int)((threads + 255) / 256);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    hipStream_t st = nullptr;
    LH_LAUNCH(k_diag_random_read, grid, 256, st, (const uint4*)tab, n_blocks, granule_bytes / 16, per_thread, (u64)12345, sink);   // warm-up
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(e0, st));
    LH_LAUNCH(k_diag_random_read, grid, 256, st, (const uint4*)tab, n_blocks, granule_bytes / 16, per_thread, (u64)777, sink);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    double bytes = (double)grid * 256.0 * per_thread * granule_bytes;
    if (gbps) *gbps = bytes / (ms * 1e-3) / 1e9;
    if (ms_out) *ms_out = ms;
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(tab); hipFree(sink);
    return LH_OK;
}

#include "k_valu_rate.h"
int lh_diag_valu_rate(int device, int32_t op, int32_t waves_per_simd, int32_t iters, double* out, int32_t n_out) {
    if (op < 0 || waves_per_simd < 1 || waves_per_simd > 8 || iters < 1 || !out || n_out < 10) return set_err(LH_E_ARG, "lh_diag_valu_rate: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
#ifdef LH_EMU
    return set_err(LH_E_NODEVICE, "lh_diag_valu_rate measures the hardware: not under the emulator");
#else
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t pr;
    HIPCHK(hipGetDeviceProperties(&pr, device));
    const int grid = pr.multiProcessorCount * waves_per_simd, n_waves = grid * 4;
    DevTmp tmp;
    uint32_t* sink = nullptr; unsigned long long* rec = nullptr;
    HIPCHK(tmp.alloc(&sink, 64)); HIPCHK(tmp.alloc(&rec, (size_t)n_waves * 32));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    hipStream_t st = nullptr;
    LH_LAUNCH(k_diag_valu_rate, grid, 256, st, (int)op, (int)iters, sink, rec);   // warm-up (clock ramp, code fetch)
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipEventRecord(e0, st));
    LH_LAUNCH(k_diag_valu_rate, grid, 256, st, (int)op, (int)iters, sink, rec);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    std::vector<unsigned long long> h((size_t)n_waves * 4);
    HIPCHK(hipMemcpy(h.data(), rec, h.size() * 8, hipMemcpyDeviceToHost));
    const double instr_per_wave = 64.0 * iters;
    std::vector<double> mhz, cpi;
    std::map<u64, int> per_simd;
    for (int w = 0; w < n_waves; ++w) {
        const double dc = (double)h[(size_t)w * 4], dr = (double)h[(size_t)w * 4 + 1];
        if (dr > 0) mhz.push_back(dc / dr * 100.0);
        cpi.push_back(dc / instr_per_wave);
        const u64 id = h[(size_t)w * 4 + 2];
        per_simd[(id >> 32) << 16 | (id & 0xff30u)]++;   // XCC | SE, SH, CU, SIMD of HW_ID (wave slot, pipe, queue and VM bits masked)
    }
    std::sort(mhz.begin(), mhz.end()); std::sort(cpi.begin(), cpi.end());
    int lo = 1 << 30, hi = 0;
    for (auto& kv : per_simd) { lo = kv.second < lo ? kv.second : lo; hi = kv.second > hi ? kv.second : hi; }
    const double total = instr_per_wave * n_waves, clk = mhz.empty() ? 0.0 : mhz[mhz.size() / 2];
    out[0] = ms; out[1] = total; out[2] = total / (ms * 1e-3) / 1e9; out[3] = clk; out[4] = cpi[cpi.size() / 2];
    out[5] = ms * 1e-3 * clk * 1e6 * (pr.multiProcessorCount * 4.0) / total;   // cycles per wave-instruction per SIMD, chip-wide, from the event time
    out[6] = (double)per_simd.size(); out[7] = lo; out[8] = hi; out[9] = mhz.empty() ? 0.0 : mhz[0];
    return LH_OK;
#endif
}

int lh_diag_go_rand(int device, int64_t seed, int32_t n, uint64_t* out_fast, uint64_t* out_ring, double* out_f64) {
    if (n <= 0 || !out_fast || !out_ring || !out_f64) return set_err(LH_E_ARG, "lh_diag_go_rand: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    u64 *ring = nullptr, *a = nullptr, *b = nullptr; double* f = nullptr;
    HIPCHK(hipMalloc(&ring, LH_GO_RING_BYTES)); HIPCHK(hipMalloc(&a, (size_t)n * 8)); HIPCHK(hipMalloc(&b, (size_t)n * 8)); HIPCHK(hipMalloc(&f, (size_t)n * 8));
    HIPCHK(hipMemset(a, 0, (size_t)n * 8));
    LH_LAUNCH(k_diag_go_rand, 1, 64, (hipStream_t)0, (u64)seed, (int)n, ring, a, b, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_fast, a, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_ring, b, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_f64, f, (size_t)n * 8, hipMemcpyDeviceToHost));
    hipFree(ring); hipFree(a); hipFree(b); hipFree(f);
    return LH_OK;
}

int lh_diag_gosort(int device, int32_t n_sorts, const int32_t* first, const int64_t* keys, int32_t* perm_serial, int32_t* perm_wave) {
    if (n_sorts <= 0 || !first || !keys || !perm_serial || !perm_wave) return set_err(LH_E_ARG, "lh_diag_gosort: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    const int n = first[n_sorts];
    if (n <= 0) return set_err(LH_E_ARG, "lh_diag_gosort: nothing to sort");
    std::vector<int32_t> id((size_t)n);
    for (int i = 0; i < n; ++i) id[(size_t)i] = i - first[0];
    for (int k = 0; k < n_sorts; ++k) for (int i = first[k]; i < first[k + 1]; ++i) id[(size_t)i] = i - first[k];   // the identity of every index space
    DevTmp tmp;
    int32_t *d_first = nullptr, *pa = nullptr, *pb = nullptr, *q0 = nullptr, *q1 = nullptr, *q2 = nullptr, *sa = nullptr, *sb = nullptr;
    i64 *ka = nullptr, *kb = nullptr;
    HIPCHK(tmp.alloc(&sa, (size_t)n * 4 + 64)); HIPCHK(tmp.alloc(&sb, (size_t)n * 4 + 64));
    HIPCHK(tmp.alloc(&d_first, (size_t)(n_sorts + 1) * 4)); HIPCHK(tmp.alloc(&pa, (size_t)n * 4)); HIPCHK(tmp.alloc(&pb, (size_t)n * 4));
    HIPCHK(tmp.alloc(&q0, ((size_t)n > 3 * LH_GOSORT_STK * 64 ? (size_t)n : 3 * LH_GOSORT_STK * 64) * 4 + 64));   // (the serial sorts' stacks first, then the wave sort's queue)
    HIPCHK(tmp.alloc(&q1, (size_t)n * 4 + 64)); HIPCHK(tmp.alloc(&q2, (size_t)n * 4 + 64));
    HIPCHK(tmp.alloc(&ka, (size_t)n * 8)); HIPCHK(tmp.alloc(&kb, (size_t)n * 8));
    HIPCHK(hipMemcpy(d_first, first, (size_t)(n_sorts + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ka, keys, (size_t)n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(kb, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pa, id.data(), (size_t)n * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(pb, id.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    LH_LAUNCH(k_diag_gosort, 1, 64, (hipStream_t)0, (int)n_sorts, (const int32_t*)d_first, ka, pa, kb, pb, q0, q1, q2, sa, sb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(perm_serial, pa, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(perm_wave, pb, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_diag_gosort_split(int device, int32_t n, const int64_t* keys, int32_t* perm, int32_t limit) {
    if (n <= 0 || !keys || !perm || limit < 13) return set_err(LH_E_ARG, "lh_diag_gosort_split: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    std::vector<int32_t> id((size_t)n);
    for (int i = 0; i < n; ++i) id[(size_t)i] = i;
    DevTmp tmp;
    int32_t *p = nullptr, *q0 = nullptr, *q1 = nullptr, *q2 = nullptr, *sa = nullptr, *sb = nullptr;
    i64* k = nullptr;
    const size_t qn = (size_t)n + (size_t)n / 16 + 128;
    HIPCHK(tmp.alloc(&p, (size_t)n * 4)); HIPCHK(tmp.alloc(&k, (size_t)n * 8));
    HIPCHK(tmp.alloc(&q0, qn * 4)); HIPCHK(tmp.alloc(&q1, qn * 4)); HIPCHK(tmp.alloc(&q2, qn * 4));
    HIPCHK(tmp.alloc(&sa, (size_t)n * 4 + 64)); HIPCHK(tmp.alloc(&sb, (size_t)n * 4 + 64));
    HIPCHK(hipMemcpy(k, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(p, id.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    LH_LAUNCH(k_diag_gosort_split, 1, 64, (hipStream_t)0, (int)n, k, p, (int)limit, q0, q1, q2, sa, sb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(perm, p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_diag_bitonic(int device, int32_t n, const uint64_t* keys, uint64_t* sorted, int32_t block) {
    if (n <= 0 || !keys || !sorted || (block != 0 && block != 64 && block != 1024)) return set_err(LH_E_ARG, "lh_diag_bitonic: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    DevTmp tmp;
    u64* a = nullptr;
    HIPCHK(tmp.alloc(&a, (size_t)n * 8 + 64));
    HIPCHK(hipMemcpy(a, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    LH_LAUNCH(k_diag_bitonic, 1, 64, (hipStream_t)0, (int)n, a, (int)block);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(sorted, a, (size_t)n * 8, hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_diag_introsort(int device, int32_t n_sorts, const int32_t* first, const int64_t* keys, int32_t* perm_serial, int32_t* perm_wave) {
    if (n_sorts <= 0 || !first || !keys || !perm_serial || !perm_wave) return set_err(LH_E_ARG, "lh_diag_introsort: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    const int n = first[n_sorts];
    if (n <= 0) return set_err(LH_E_ARG, "lh_diag_introsort: nothing to sort");
    for (int k = 0; k < n_sorts; ++k) if (first[k + 1] - first[k] > LH_DIAG_ISORT_MAX) return set_err(LH_E_ARG, "lh_diag_introsort: at most 1024 elements per sort");
    DevTmp tmp;
    int32_t *d_first = nullptr, *pa = nullptr, *pb = nullptr, *d_wd = nullptr;
    i64* ka = nullptr;
    HIPCHK(tmp.alloc(&d_first, (size_t)(n_sorts + 1) * 4)); HIPCHK(tmp.alloc(&pa, (size_t)n * 4)); HIPCHK(tmp.alloc(&pb, (size_t)n * 4)); HIPCHK(tmp.alloc(&ka, (size_t)n * 8));
    HIPCHK(tmp.alloc(&d_wd, LH_WD_SLOTS * 4));
    HIPCHK(hipMemset(d_wd, 0, LH_WD_SLOTS * 4));
    HIPCHK(hipMemcpy(d_first, first, (size_t)(n_sorts + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ka, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    LH_LAUNCH(k_diag_introsort, n_sorts < 1024 ? n_sorts : 1024, 64, (hipStream_t)0, (int)n_sorts, (const int32_t*)d_first, (const i64*)ka, pa, pb, d_wd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    int32_t wd[2] = {0, 0};
    HIPCHK(hipMemcpy(wd, d_wd, sizeof wd, hipMemcpyDeviceToHost));
    if (wd[0] || wd[1]) return set_err(LH_E_LIMIT, "lh_diag_introsort: the device sort gave up (watchdog / stack)");
    HIPCHK(hipMemcpy(perm_serial, pa, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(perm_wave, pb, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_diag_rescue_dedup(int device, int32_t n_cases, const int32_t* first, const int64_t* regions, const int64_t* added, int32_t max_chain_gap, int32_t* verdict, int32_t* n_out) {
    if (n_cases <= 0 || !first || !regions || !added || !verdict || !n_out) return set_err(LH_E_ARG, "lh_diag_rescue_dedup: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)first[n_cases], slots = n + 2 * (size_t)n_cases + 64;
    lh_opts ho;
    lh_opts_init(&ho);
    ho.max_chain_gap = max_chain_gap;
    DOpts o = to_dopts(&ho);
    DIndex ix;
    memset(&ix, 0, sizeof ix);
    DevTmp tmp;
    int32_t *d_first = nullptr, *d_ia = nullptr, *d_v = nullptr, *d_n = nullptr, *d_wd = nullptr;
    i64 *d_vals = nullptr, *d_b = nullptr;
    DReg *ra = nullptr, *rb = nullptr, *rt = nullptr;
    HIPCHK(tmp.alloc(&d_first, (size_t)(n_cases + 1) * 4)); HIPCHK(tmp.alloc(&d_ia, slots * 4)); HIPCHK(tmp.alloc(&d_v, (size_t)n_cases * 4)); HIPCHK(tmp.alloc(&d_n, (size_t)n_cases * 4));
    HIPCHK(tmp.alloc(&d_wd, LH_WD_SLOTS * 4)); HIPCHK(tmp.alloc(&d_vals, (n ? n : 1) * 48)); HIPCHK(tmp.alloc(&d_b, (size_t)n_cases * 48));
    HIPCHK(tmp.alloc(&ra, slots * sizeof(DReg))); HIPCHK(tmp.alloc(&rb, slots * sizeof(DReg))); HIPCHK(tmp.alloc(&rt, slots * sizeof(DReg)));
    HIPCHK(hipMemset(d_wd, 0, LH_WD_SLOTS * 4));
    o.wd = d_wd;
    HIPCHK(hipMemcpy(d_first, first, (size_t)(n_cases + 1) * 4, hipMemcpyHostToDevice));
    if (n) HIPCHK(hipMemcpy(d_vals, regions, n * 48, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_b, added, (size_t)n_cases * 48, hipMemcpyHostToDevice));
    LH_LAUNCH(k_diag_resc_dedup, n_cases < 4096 ? n_cases : 4096, 64, (hipStream_t)0, ix, o, (int)n_cases, (const int32_t*)d_first, (const i64*)d_vals, (const i64*)d_b, ra, rb, rt, d_ia, d_v, d_n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(verdict, d_v, (size_t)n_cases * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, d_n, (size_t)n_cases * 4, hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_diag_rescue_sw(int device, int32_t n_cases, const int32_t* q_off, const uint8_t* q, const int32_t* t_off, const uint8_t* t, int32_t full, int32_t weaken, int32_t* out) {
    if (n_cases <= 0 || !q_off || !q || !t_off || !t || !out) return set_err(LH_E_ARG, "lh_diag_rescue_sw: bad argument");
    if (lh_device_count() <= 0) return set_err(LH_E_NODEVICE, "no HIP device");
    HIPCHK(hipSetDevice(device));
    const size_t nq = (size_t)q_off[n_cases], nt = (size_t)t_off[n_cases];
    std::vector<uint8_t> mate(nq + 8, 0), pac(nt / 4 + 8, 0);
    std::vector<RJob> jobs((size_t)n_cases);
    for (int c = 0; c < n_cases; ++c) {
        const int ql = q_off[c + 1] - q_off[c], tl = t_off[c + 1] - t_off[c];
        if (ql < 1 || ql > LH_MAXLEN || tl < 1 || tl > LH_RJ_TMAX) return set_err(LH_E_ARG, "lh_diag_rescue_sw: a query of 1..250 and a window of 1..LH_RJ_TMAX bases per case");
        for (int k = 0; k < ql; ++k) { if (q[q_off[c] + k] > 3) return set_err(LH_E_ARG, "lh_diag_rescue_sw: bases 0..3"); mate[(size_t)q_off[c] + (size_t)(ql - 1 - k)] = (uint8_t)(3 - q[q_off[c] + k]); }
        for (int i = 0; i < tl; ++i) { const size_t p = (size_t)t_off[c] + (size_t)i; if (t[p] > 3) return set_err(LH_E_ARG, "lh_diag_rescue_sw: bases 0..3"); pac[p >> 2] |= (uint8_t)(t[p] << ((~p & 3) << 1)); }
        RJob& jb = jobs[(size_t)c];
        memset(&jb, 0, sizeof jb);
        jb.t0 = t_off[c]; jb.q0 = q_off[c] + ql - 1; jb.pair = c; jb.qlen = (int16_t)ql; jb.tlen = (int16_t)tl; jb.anchor = 0;
        jb.score = 0; jb.te = -1; jb.qe = -1; jb.tb = -1; jb.qb = -1; jb.rows2 = 0; jb.rlo = 0; jb.rn = jb.tlen;
    }
    lh_opts ho;
    lh_opts_init(&ho);
    DOpts o = to_dopts(&ho);
    DIndex ix;
    memset(&ix, 0, sizeof ix);
    DevTmp tmp;
    uint8_t *d_mate = nullptr, *d_pac = nullptr;
    RJob* d_jobs = nullptr; RMeta* d_meta = nullptr; DCounters* d_ctr = nullptr;
    int32_t *d_keys = nullptr, *d_ord = nullptr, *d_ord2 = nullptr;
    const size_t ocap = (size_t)n_cases + 8 * LH_RJ_NB + 8;
    HIPCHK(tmp.alloc(&d_mate, mate.size())); HIPCHK(tmp.alloc(&d_pac, pac.size())); HIPCHK(tmp.alloc(&d_jobs, sizeof(RJob) * (size_t)n_cases)); HIPCHK(tmp.alloc(&d_meta, sizeof(RMeta)));
    HIPCHK(tmp.alloc(&d_ctr, sizeof(DCounters) * LH_CTR_SLOTS)); HIPCHK(tmp.alloc(&d_keys, sizeof(int32_t) * 3 * LH_RC_KEYS)); HIPCHK(tmp.alloc(&d_ord, ocap * 4)); HIPCHK(tmp.alloc(&d_ord2, ocap * 4));
    HIPCHK(hipMemcpy(d_mate, mate.data(), mate.size(), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_pac, pac.data(), pac.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_jobs, jobs.data(), sizeof(RJob) * (size_t)n_cases, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_meta, 0, sizeof(RMeta))); HIPCHK(hipMemset(d_ctr, 0, sizeof(DCounters) * LH_CTR_SLOTS));
    ix.pac = d_pac; ix.l_pac = (i64)nt;
    // what rescue_dir runs after its emitting pass, on jobs made here (no order by striping exists yet: both order arrays are whole and padded alike)
    { int rc = rescue_sw((hipStream_t)0, ix, o, n_cases, d_jobs, d_mate, d_meta, d_keys, d_ord, (i64)ocap, d_ord2, (i64)ocap, d_ctr, full != 0, (int)weaken); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(jobs.data(), d_jobs, sizeof(RJob) * (size_t)n_cases, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_cases; ++c) {
        const RJob& jb = jobs[(size_t)c];
        int32_t* r = out + (size_t)c * 8;
        r[0] = jb.score; r[1] = jb.te; r[2] = jb.qe; r[3] = jb.tb; r[4] = jb.qb; r[5] = jb.rlo; r[6] = jb.rn; r[7] = jb.rows2;
    }
    return LH_OK;
}

int lh_diag_index_check(const lh_index* ix, uint64_t stride, uint64_t* n_checked, uint64_t* n_bad_order, uint64_t* n_bad_lf) {
    if (!ix || stride == 0 || !n_checked || !n_bad_order || !n_bad_lf) return set_err(LH_E_ARG, "lh_diag_index_check: bad argument");
    if (ix->d.sa_intv != 1) return set_err(LH_E_ARG, "lh_diag_index_check needs a fully resident suffix array (sa_intv 1)");
    HIPCHK(hipSetDevice(ix->device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc(&d, 32));
    HIPCHK(hipMemset(d, 0, 32));
    u64 rows = (ix->d.seq_len + stride - 1) / stride;
    int grid = (int)((rows + 255) / 256 < 8192 ? (rows + 255) / 256 : 8192);
    LH_LAUNCH(k_diag_index_check, grid, 256, (hipStream_t)0, ix->d, (u64)stride, d);
    unsigned long long h[3] = {0, 0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h, d, 24, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return set_err(LH_E_HIP, std::string("lh_diag_index_check: ") + hipGetErrorString(e));
    *n_checked = h[0]; *n_bad_order = h[1]; *n_bad_lf = h[2];
    return LH_OK;
}

int lh_diag_index_digest(const lh_index* ix, uint64_t* lcp_digest, uint64_t* ktree_digest, int32_t* ktree_levels) {
    if (!ix || !lcp_digest || !ktree_digest) return set_err(LH_E_ARG, "lh_diag_index_digest: null argument");
    HIPCHK(hipSetDevice(ix->device));
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc(&d, 16));
    HIPCHK(hipMemset(d, 0, 16));
    u64 n_lcp = ix->d_lcp ? ix->d.seq_len + 2 : 0;
    u64 n_tree = ix->d_ktree ? (((1ull << (2 * (ix->d.ktree_levels + 1))) - 4) / 3) * 2 : 0;
    LH_LAUNCH(k_diag_digest, 4096, 256, (hipStream_t)0, (const uint8_t*)ix->d_lcp, n_lcp, (const u64*)ix->d_ktree, n_tree, d);
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h, d, 16, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return set_err(LH_E_HIP, std::string("lh_diag_index_digest: ") + hipGetErrorString(e));
    *lcp_digest = h[0]; *ktree_digest = h[1];
    if (ktree_levels) *ktree_levels = ix->d_ktree ? ix->d.ktree_levels : 0;
    return LH_OK;
}
