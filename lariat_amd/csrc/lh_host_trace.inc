// lh_host_trace.inc — what the development builds read back and print between the launches (-DLH_K1_TRACE: tools/k1_trace.py; -DLH_RFA_PROF,
// -DLH_RA_HIST: tools/prof_rfa.sh).  Each function is called under its #ifdef at the point of the pipeline its numbers belong to (run_front,
// rescue_run, rfa_run); the tools parse the lines, so their text is fixed.  Included by lh_host.inc; nothing here is compiled into the product.

#ifdef LH_K1_TRACE
// the request trace of K1's pass 1 and the list-length histograms of passes 1 and 2, while LH_K1_TRACE is set in the environment
struct K1Trace {
    const bool on = getenv("LH_K1_TRACE") != nullptr;
    const uint32_t cap = 4096;
    DevGroup mem;   // (released with the object: an error return of run_front does not lose the buffers)
    u64* d_trace = nullptr; uint32_t* d_trace_n = nullptr;
    unsigned long long* d_lens = nullptr;   // list lengths, passes 1 and 2 (k_smem4.h: K1_LEN)
};
// before pass 1: the buffers, and the device symbols that switch the recording on
static int k1_trace_begin(lh_context* c, K1Trace& T, int g4) {
    if (!T.on) return LH_OK;
    const size_t Tl = (size_t)g4 * 64;
    DALLOC(T.mem, T.d_trace, Tl * T.cap); DALLOC(T.mem, T.d_trace_n, Tl); DALLOC(T.mem, T.d_lens, 2 * 3 * 64);
    HIPCHK(hipMemsetAsync(T.d_trace_n, 0, Tl * 4, c->stream));
    HIPCHK(hipMemsetAsync(T.d_lens, 0, 2 * 3 * 64 * 8, c->stream));
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_lens), &T.d_lens, sizeof T.d_lens, 0, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_trace), &T.d_trace, sizeof T.d_trace, 0, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_trace_cap), &T.cap, sizeof T.cap, 0, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_trace_n), &T.d_trace_n, sizeof T.d_trace_n, 0, hipMemcpyHostToDevice, c->stream));
    return LH_OK;
}
// after pass 1: the request stream's own floor: the same sequences, the same geometry, nothing in between (tools/k1_trace.py reads the line)
static int k1_trace_replay(lh_context* c, K1Trace& T, int N, int g4) {
    if (!T.on) return LH_OK;
    u64* const d_trace = T.d_trace; uint32_t* const d_trace_n = T.d_trace_n; const uint32_t trace_cap = T.cap;
    u64* nul = nullptr;
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_trace), &nul, sizeof nul, 0, hipMemcpyHostToDevice, c->stream));
    u64* d_sink = nullptr; unsigned long long* d_hist = nullptr;
    DevGroup tmp;
    DALLOC(tmp, d_sink, 1); DALLOC(tmp, d_hist, 2 * K1T_N + 2);
    HIPCHK(hipMemsetAsync(d_hist, 0, (2 * K1T_N + 2) * 8, c->stream));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    auto replay = [&](float& best, float& sum) -> int {
        best = 1e30f; sum = 0;
        for (int rep_ = 0; rep_ < 4; ++rep_) {
            HIPCHK(hipEventRecord(e0, c->stream));
            LH_LAUNCH(k_k1_replay, g4, 64, c->stream, (const u64*)d_trace, (const uint32_t*)d_trace_n, trace_cap, d_sink);
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            if (rep_) { sum += ms; best = ms < best ? ms : best; }   // (the first launch warms the trace's pages)
        }
        return LH_OK;
    };
    float best = 1e30f, sum = 0;
    { int rc = replay(best, sum); if (rc) return rc; }
    LH_LAUNCH(k_k1_trace_hist, 2048, 256, c->stream, (const u64*)d_trace, (const uint32_t*)d_trace_n, trace_cap, (uint32_t)(g4 * 64), d_hist);
    unsigned long long h[2 * K1T_N + 2];
    HIPCHK(hipMemcpyAsync(h, d_hist, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // LH_K1_REPLAY_SKIP = masks of tables (bit = K1T_*) separated by commas, each a superset of the one before: the replay again without them
    std::string skip_js;
    if (const char* sk = getenv("LH_K1_REPLAY_SKIP")) {
        for (const char* q = sk; *q;) {
            char* end = nullptr;
            const unsigned long m = strtoul(q, &end, 0);
            if (end == q) break;
            LH_LAUNCH(k_k1_trace_skip, 2048, 256, c->stream, d_trace, d_trace_n, trace_cap, (uint32_t)(g4 * 64), (uint32_t)m);
            float b_ = 0, s_ = 0;
            { int rc = replay(b_, s_); if (rc) return rc; }
            skip_js += std::string(skip_js.empty() ? "" : ", ") + "{\"skip_mask\": " + std::to_string(m) + ", \"replay_ms_avg\": " + std::to_string(s_ / 3) + ", \"replay_ms_min\": " + std::to_string(b_) + "}";
            q = *end == ',' ? end + 1 : end;
        }
    }
    static const char* const tn[K1T_N] = {"occurrence", "tree", "bloom1", "bloom2", "rep_t", "plcp", "text", "sa", "isa", "interval_slab_read", "interval_slab_write", "interval_out_write", "reads"};
    std::string js = "{\"pairs\": " + std::to_string(N / 2) + ", \"lanes\": " + std::to_string((long long)g4 * 64) + ", \"replay_ms_avg\": " + std::to_string(sum / 3) + ", \"replay_ms_min\": " + std::to_string(best) +
                     ", \"dropped_requests\": " + std::to_string(h[2 * K1T_N]) + ", \"requests_by_table\": {";
    for (int i = 0; i < K1T_N; ++i) js += std::string(i ? ", " : "") + "\"" + tn[i] + "\": [" + std::to_string(h[2 * i]) + ", " + std::to_string(h[2 * i + 1]) + "]";
    js += "}, \"replay_without\": [" + skip_js + "]}";
    fprintf(stderr, "[lh] K1TRACE %s\n", js.c_str());
    hipEventDestroy(e0); hipEventDestroy(e1);
    return LH_OK;
}
// after pass 2: the list lengths of passes 1 and 2 (tools/k1_trace.py reads the line)
static int k1_trace_lens(lh_context* c, K1Trace& T) {
    if (!T.on) return LH_OK;
    unsigned long long* const d_lens = T.d_lens;
    unsigned long long* nul = nullptr;
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(lh_k1_lens), &nul, sizeof nul, 0, hipMemcpyHostToDevice, c->stream));
    unsigned long long hl[2 * 3 * 64];
    HIPCHK(hipMemcpyAsync(hl, d_lens, sizeof hl, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    static const char* const kn[3] = {"ncurr_at_push", "nprev_at_read", "stored_position_read"};
    std::string js = "{";
    for (int ps = 0; ps < 2; ++ps)
        for (int k = 0; k < 3; ++k) {
            js += std::string(ps || k ? ", " : "") + "\"pass" + std::to_string(ps + 1) + "_" + kn[k] + "\": [";
            for (int v = 0; v < 64; ++v) js += std::string(v ? ", " : "") + std::to_string(hl[(ps * 3 + k) * 64 + v]);
            js += "]";
        }
    js += "}";
    fprintf(stderr, "[lh] K1LENS %s\n", js.c_str());
    return LH_OK;
}
#endif

#ifdef LH_RFA_PROF
// after K3's cluster kernels
static int prof_chain_cl(lh_context* c) {
    static const char* const names[8] = {"load + keys", "bitonic sort", "clusters", "cluster walks (lane per cluster)", "order + weights", "introsort", "greedy scan", "emit"};
    unsigned long long h[16];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(lh_chain_prof), sizeof h));
    unsigned long long tot = 0;
    for (int i = 0; i < 8; ++i) tot += h[i];
    fprintf(stderr, "[lh] k_chain_cl phases (%llu reads, %.1f k clocks per read):\n", h[15], h[15] ? (double)tot / 1e3 / (double)h[15] : 0.0);
    for (int i = 0; i < 8; ++i) fprintf(stderr, "[lh]   %-36s %6.2f %%\n", names[i], tot ? 100.0 * (double)h[i] / (double)tot : 0.0);
    memset(h, 0, sizeof h);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_chain_prof), h, sizeof h));
    return LH_OK;
}
// after K6's two directions
static int prof_rescue(lh_context* c) {
    static const char* const names[8] = {"first test against the current list", "window + job result", "first look at the list (clean?)", "incremental dedup", "insert into the memory list", "mem_sort_dedup_patch as written", "reload + ties", "store"};
    unsigned long long h[24];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(lh_resc_prof), sizeof h));
    unsigned long long tot = 0;
    for (int i = 0; i < 8; ++i) tot += h[i];
    fprintf(stderr, "[lh] k_resc_apply (both directions): %llu pairs replayed, %llu attempts; first look dirty %llu; calls decided incrementally %llu, declined (equal keys) %llu, as written %llu; lists left in memory: tie %llu, too long %llu; %.1f k clocks per pair\n",
            h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15], h[8] ? (double)tot / 1e3 / (double)h[8] : 0.0);
    tot += h[16] + h[17];
    for (int i = 0; i < 8; ++i) fprintf(stderr, "[lh]   %-36s %6.2f %%\n", names[i], tot ? 100.0 * (double)h[i] / (double)tot : 0.0);
    fprintf(stderr, "[lh]   %-36s %6.2f %%\n[lh]   %-36s %6.2f %%   (%llu attempts without a job)\n", "loop head (anchors, job cursor)", tot ? 100.0 * (double)h[16] / (double)tot : 0.0,
            "Smith-Waterman in place (no job)", tot ? 100.0 * (double)h[17] / (double)tot : 0.0, h[18]);
    memset(h, 0, sizeof h);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_resc_prof), h, sizeof h));
    return LH_OK;
}
// after K8
static int prof_rfa(lh_context* c) {
    static const char* const names[15] = {"(k_rfa_init)", "  sort: loop head + lists of up to 64", "  probability sums: the reads' sums", "carve + contig grouping", "position sort", "inferMolecules + markBest step 1",
                                           "scrapMolecules + markBest step 2", "optimizer", "moleculeMapqProbabilitySums (the sinks' scores)", "molecule status + penalty", "mate links + lists",
                                           "estimateMapQualities (lane per read)", "(k_rfa_mq_w)", "(k_rfa_post)", "(k_rfa_post)"};
    unsigned long long h[24];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(lh_rfa_prof), sizeof h));
    unsigned long long tot = 0;
    for (int i = 0; i < 24; ++i) tot += h[i];
    fprintf(stderr, "[lh] k_rfa phases (shader clocks summed over waves, %d barcodes):\n", c->b.n_bc);
    for (int i = 0; i < 15; ++i) fprintf(stderr, "[lh]   %-44s %6.2f %%  %10.1f k clocks per barcode\n", names[i], tot ? 100.0 * (double)h[i] / (double)tot : 0.0, (double)h[i] / 1e3 / (c->b.n_bc ? c->b.n_bc : 1));
    {   // parts of the two phases above, when their markers are compiled in (their clocks are NOT in the phase's own line then)
        static const char* const sub[8] = {"  inferMolecules", "  step 1: staging a tile", "  step 1: the entries of a tile", "  sort: network", "  sort: tie check + copy", "  sort: Go's algorithm on ranks", "  sort: smallest position", "  sort: keys"};
        for (int i = 16; i < 24; ++i) if (h[i]) fprintf(stderr, "[lh]   %-44s %6.2f %%  %10.1f k clocks per barcode\n", sub[i - 16], tot ? 100.0 * (double)h[i] / (double)tot : 0.0, (double)h[i] / 1e3 / (c->b.n_bc ? c->b.n_bc : 1));
    }
    memset(h, 0, sizeof h);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_rfa_prof), h, sizeof h));
    return LH_OK;
}
#endif

#ifdef LH_RA_HIST
// after K6's two directions
static int hist_rescue(lh_context* c) {
    unsigned long long hh[66];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyFromSymbol(hh, HIP_SYMBOL(lh_resc_hist), sizeof hh));
    for (int kind = 0; kind < 2; ++kind) {
        fprintf(stderr, "[lh] k_resc_apply, time per pair, %s (longest %.3f ms):", kind ? "pairs with a call run as written" : "pairs decided incrementally", (double)hh[64 + kind] / 1e5);
        for (int b = 0; b < 32; ++b) if (hh[kind * 32 + b]) fprintf(stderr, " <%.4g ms: %llu", (double)(2ull << b) / 1e5, hh[kind * 32 + b]);
        fprintf(stderr, "\n");
    }
    memset(hh, 0, sizeof hh);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_resc_hist), hh, sizeof hh));
    return LH_OK;
}
// after K8
static int hist_rfa(lh_context* c) {
    unsigned long long hh[40];
    HIPCHK(hipStreamSynchronize(c->stream));
    {
        RfaCounters bn;
        HIPCHK(hipMemcpy(&bn, c->d_bc_next, sizeof bn, hipMemcpyDeviceToHost));
        fprintf(stderr, "[lh] k_rfa tiers: %d barcodes; listed for the 16 MiB tier %d (of %d waves), for the 128 MiB tier %d (of %d), for the last launch %d; k_rfa_post: %d / %d / %d\n", c->b.n_bc, bn.n_ovf,
                c->grid_rfa_mid[0], c->grid_rfa_mid[0] ? bn.tier[0].n_ovf : 0, c->grid_rfa_mid[1], c->grid_rfa_mid[1] ? bn.tier[1].n_ovf : (c->grid_rfa_mid[0] ? bn.tier[0].n_ovf : bn.n_ovf), bn.post_n_ovf,
                bn.tier[0].post_n_ovf, bn.tier[1].post_n_ovf);
    }
    HIPCHK(hipMemcpyFromSymbol(hh, HIP_SYMBOL(lh_rfa_hist), sizeof hh));
    fprintf(stderr, "[lh] k_rfa, time per barcode (longest %.3f ms, sum %.1f ms over %d barcodes):", (double)hh[32] / 1e5, (double)hh[33] / 1e5, c->b.n_bc);
    for (int b = 0; b < 32; ++b) if (hh[b]) fprintf(stderr, " <%.4g ms: %llu", (double)(2ull << b) / 1e5, hh[b]);
    {
        unsigned long long nb = 0;
        for (int b = 0; b < 32; ++b) nb += hh[b];
        if (nb) fprintf(stderr, "; per finished barcode: %.0f candidates (%.0f filtered), %.0f molecules, carve %.0f KB, molecule x read table %.0f K words", (double)hh[34] / nb, (double)hh[35] / nb,
                        (double)hh[36] / nb, (double)hh[37] / nb / 1024.0, (double)hh[38] / nb / 1024.0);
    }
    fprintf(stderr, "\n");
    memset(hh, 0, sizeof hh);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_rfa_hist), hh, sizeof hh));
    {
        unsigned long long h2[8];
        HIPCHK(hipMemcpyFromSymbol(h2, HIP_SYMBOL(lh_rfa_hist2), sizeof h2));
        fprintf(stderr, "[lh] k_rfa position sort (large barcodes): %llu contig lists, longest %llu, longer than %d: %llu, longer than %d: %llu, with two equal positions: %llu, sum of squares %.3g\n", h2[0], h2[1],
                LH_RFA_SORT_LDS, h2[2], LH_RFA_LDS_BYTES / 4, h2[3], h2[5], (double)h2[4]);
        memset(h2, 0, sizeof h2);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_rfa_hist2), h2, sizeof h2));
        static int bs[4096][8];
        HIPCHK(hipMemcpyFromSymbol(bs, HIP_SYMBOL(lh_rfa_bcstat), sizeof bs));
        std::vector<int> ord(4096);
        for (int i = 0; i < 4096; ++i) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](int x, int y) { return bs[x][0] > bs[y][0]; });
        for (int k = 0; k < 6; ++k) { const int* b = bs[ord[k == 5 ? 2000 : k]]; fprintf(stderr, "[lh]   %s barcode: %.2f ms, %d candidates (%d filtered), %d raw molecules (largest %d), %d contigs (longest list %d), %d molecules\n", k == 5 ? "a median" : "slow", b[0] / 1e5, b[1], b[2], b[3], b[4], b[5], b[7], b[6]); }
        memset(bs, 0, sizeof bs);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(lh_rfa_bcstat), bs, sizeof bs));
    }
    return LH_OK;
}
#endif
