// lh_bgzf.inc — the device compressor behind lh_bgzf_* (include/lariat_hip.h): BGZF members by k_bgzf.h.  Included from lh_host.inc.
//
// A compressor is its own object, not part of an lh_context: a writer thread uses it while another thread aligns.  It owns two buffer sets, each with a
// stream of its own at the priority of the contexts' transfer streams (streams of one priority share hardware queues: its launches do not hold align kernels
// back).  An input of more than max_blocks blocks goes through in chunks that alternate between the sets: while the device works on chunk k, the host stages
// chunk k + 1 into the other set's pinned memory and starts its upload, and gathers chunk k - 1's members from where they were downloaded.
#include "k_bgzf.h"

#define LH_BGZF_DEFAULT_BLOCKS 2048   // a launch of that many waves fills the device: 8 single-wave workgroups per CU (the kernel's LDS and registers) on 256 CUs
#define LH_BGZF_MAX_WAVES 2048   // waves of one launch (each owns a token scratch of LH_BGZF_DATA words); more blocks: a wave takes several

struct lh_brec_bufs;                       // the record encoder's buffers (lh_brec.inc): created by its first use, freed with the compressor
static void brec_free(lh_brec_bufs* b);

struct lh_bgzf {
    int device = 0, max_blocks = 0, waves = 0;
    std::mutex mu;
    struct Set {
        hipStream_t st = nullptr;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // before the upload, after it, after the kernel, after the download
        uint8_t *h_in = nullptr, *h_out = nullptr;   // pinned: the blocks, LH_BGZF_DATA apart; the output slots
        char* h_desc = nullptr;                      // pinned: i64 offset[max_blocks], then int32 length[max_blocks]
        int32_t* h_meta = nullptr;                   // pinned: int32 size[max_blocks], then the watchdog words
        uint8_t *d_in = nullptr, *d_out = nullptr; char* d_desc = nullptr; int32_t* d_meta = nullptr; uint32_t* d_tok = nullptr;
        int nb = 0;                                  // blocks in flight
        size_t first = 0;                            // ... the first one's index in the call's list
    } set[2];
    uint32_t* d_consts = nullptr;
    DevGroup mem;   // every device buffer of the compressor
    double t_up = 0, t_kernel = 0, t_down = 0;   // the last lh_bgzf_compress's phases, seconds (device time, summed over its chunks)
    lh_brec_bufs* enc = nullptr;
    ~lh_bgzf() {
        brec_free(enc);
        for (Set& s : set) {
            if (s.st) { (void)hipStreamSynchronize(s.st); (void)hipStreamDestroy(s.st); }
            for (hipEvent_t e : s.ev) if (e) (void)hipEventDestroy(e);
            if (s.h_in) (void)hipHostFree(s.h_in);
            if (s.h_out) (void)hipHostFree(s.h_out);
            if (s.h_desc) (void)hipHostFree(s.h_desc);
            if (s.h_meta) (void)hipHostFree(s.h_meta);
        }
    }
};

static int bgzf_create(int device, int32_t max_blocks, lh_bgzf* z) {
    z->device = device;
    z->max_blocks = max_blocks > 0 ? max_blocks : LH_BGZF_DEFAULT_BLOCKS;
    z->waves = z->max_blocks < LH_BGZF_MAX_WAVES ? z->max_blocks : LH_BGZF_MAX_WAVES;
    const size_t mb = (size_t)z->max_blocks;
    HIPCHK(hipSetDevice(device));
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    uint32_t consts[LH_BGZF_CONST_WORDS];
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? LH_BGZF_POLY : 0u); consts[i] = c; }
    consts[256] = 0x00800000u;   // x^8
    for (int k = 1; k < 16; ++k) consts[256 + k] = bgzf_mulmod(consts[256 + k - 1], consts[256 + k - 1]);
    DALLOC(z->mem, z->d_consts, LH_BGZF_CONST_WORDS);
    for (lh_bgzf::Set& s : z->set) {
        DALLOC(z->mem, s.d_in, mb * LH_BGZF_DATA); DALLOC(z->mem, s.d_out, mb * LH_BGZF_SLOT); DALLOC(z->mem, s.d_desc, mb * 12);
        DALLOC(z->mem, s.d_meta, mb + LH_WD_SLOTS); DALLOC(z->mem, s.d_tok, (size_t)z->waves * LH_BGZF_DATA);
        HIPCHK(hipStreamCreateWithPriority(&s.st, hipStreamNonBlocking, lo));
        for (hipEvent_t& e : s.ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipHostMalloc((void**)&s.h_in, mb * LH_BGZF_DATA, hipHostMallocDefault)); HIPCHK(hipHostMalloc((void**)&s.h_out, mb * LH_BGZF_SLOT, hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void**)&s.h_desc, mb * 12, hipHostMallocDefault)); HIPCHK(hipHostMalloc((void**)&s.h_meta, (mb + LH_WD_SLOTS) * sizeof(int32_t), hipHostMallocDefault));
        HIPCHK(hipMemset(s.d_meta, 0, (mb + LH_WD_SLOTS) * sizeof(int32_t)));
    }
    HIPCHK(hipMemcpy(z->d_consts, consts, sizeof consts, hipMemcpyHostToDevice));
    return LH_OK;
}

int lh_bgzf_create(int device, int32_t max_blocks, lh_bgzf** out) {
    if (!out || max_blocks < 0) return set_err(LH_E_ARG, "lh_bgzf_create: bad argument");
    *out = nullptr;
    const int n_dev = lh_device_count();
    if (n_dev < 1) return set_err(LH_E_NODEVICE, "lh_bgzf_create: no HIP device (the compressor has no CPU fallback; a writer without one compresses with zlib)");
    if (device < 0 || device >= n_dev) return set_err(LH_E_ARG, "lh_bgzf_create: no such device");
    lh_bgzf* z = new lh_bgzf();
    const int rc = bgzf_create(device, max_blocks, z);
    if (rc) { delete z; return rc; }   // (the group frees what was allocated, the destructor the rest)
    *out = z;
    return LH_OK;
}
void lh_bgzf_free(lh_bgzf* z) { delete z; }

int64_t lh_bgzf_bound(int64_t n) { return n <= 0 ? 0 : n + (n + LH_BGZF_DATA - 1) / LH_BGZF_DATA * 31; }   // a stored member: 26 bytes of framing, 5 of block header

int lh_bgzf_timings(const lh_bgzf* z, double* upload_s, double* kernel_s, double* download_s) {
    if (!z) return set_err(LH_E_ARG, "lh_bgzf_timings: null compressor");
    if (upload_s) *upload_s = z->t_up;
    if (kernel_s) *kernel_s = z->t_kernel;
    if (download_s) *download_s = z->t_down;
    return LH_OK;
}

namespace {
struct BgzfBlk { const uint8_t* src; int32_t len; int32_t seg; };
// chunk -> set: stage, upload, launch, download; nothing waits
int bgzf_submit(lh_bgzf* z, lh_bgzf::Set& s, const std::vector<BgzfBlk>& blks, size_t first, int nb) {
    i64* off = (i64*)s.h_desc; int32_t* len = (int32_t*)(s.h_desc + (size_t)z->max_blocks * 8);
    for (int i = 0; i < nb; ++i) {
        const BgzfBlk& b = blks[first + (size_t)i];
        memcpy(s.h_in + (size_t)i * LH_BGZF_DATA, b.src, (size_t)b.len);
        off[i] = (i64)i * LH_BGZF_DATA; len[i] = b.len;
    }
    s.nb = nb; s.first = first;
    HIPCHK(hipEventRecord(s.ev[0], s.st));
    HIPCHK(hipMemcpyAsync(s.d_in, s.h_in, (size_t)nb * LH_BGZF_DATA, hipMemcpyHostToDevice, s.st));
    HIPCHK(hipMemcpyAsync(s.d_desc, s.h_desc, (size_t)z->max_blocks * 12, hipMemcpyHostToDevice, s.st));
    HIPCHK(hipEventRecord(s.ev[1], s.st));
    LH_LAUNCH(k_bgzf, nb < z->waves ? nb : z->waves, 64, s.st, (const uint8_t*)s.d_in, (const i64*)s.d_desc, (const int32_t*)(s.d_desc + (size_t)z->max_blocks * 8), nb, s.d_out, s.d_meta,
              s.d_tok, (const uint32_t*)z->d_consts, s.d_meta + z->max_blocks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s.ev[2], s.st));
    HIPCHK(hipMemcpyAsync(s.h_out, s.d_out, (size_t)nb * LH_BGZF_SLOT, hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipMemcpyAsync(s.h_meta, s.d_meta, ((size_t)z->max_blocks + LH_WD_SLOTS) * sizeof(int32_t), hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipEventRecord(s.ev[3], s.st));
    return LH_OK;
}
// waits for the set's chunk and appends its members to out
int bgzf_collect(lh_bgzf* z, lh_bgzf::Set& s, const std::vector<BgzfBlk>& blks, uint8_t* out, int64_t out_cap, int64_t& pos, int64_t* seg_off) {
    const int nb = s.nb;
    s.nb = 0;
    HIPCHK(hipEventSynchronize(s.ev[3]));
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(&ms[k], s.ev[k], s.ev[k + 1]));
    z->t_up += ms[0] * 1e-3; z->t_kernel += ms[1] * 1e-3; z->t_down += ms[2] * 1e-3;
    const int32_t* wd = s.h_meta + z->max_blocks;
    for (int k = 0; k < LH_WD_SLOTS; ++k)
        if (wd[k]) {
            (void)hipMemsetAsync(s.d_meta + z->max_blocks, 0, LH_WD_SLOTS * sizeof(int32_t), s.st);
            return set_err(LH_E_HIP, "lh_bgzf_compress: watchdog word " + std::to_string(k) + " of k_bgzf tripped");
        }
    for (int i = 0; i < nb; ++i) {
        const BgzfBlk& b = blks[s.first + (size_t)i];
        const int32_t size = s.h_meta[i];
        if (size < 26 + 1 || size > 0x10000 || pos + size > out_cap) return set_err(LH_E_HIP, "lh_bgzf_compress: a member of " + std::to_string(size) + " bytes came back");
        if (seg_off && (s.first + (size_t)i == 0 || blks[s.first + (size_t)i - 1].seg != b.seg)) seg_off[b.seg] = pos;
        memcpy(out + pos, s.h_out + (size_t)i * LH_BGZF_SLOT + LH_BGZF_PAD, (size_t)size);
        pos += size;
    }
    return LH_OK;
}
}   // namespace

// what lh_bgzf_compress does, for several inputs at once (the BAM writer's files, bamfile.cpp): every segment is cut into blocks on its own, all blocks go to the
// device together, the members lie in `out` segment by segment; seg_off (n_seg + 1 entries, may be null): where each segment's members begin, and the end
extern "C" int lh_bgzf_compress_segs_(lh_bgzf* z, int32_t n_seg, const uint8_t* const* seg, const int64_t* seg_len, uint8_t* out, int64_t out_cap, int64_t* out_len, int64_t* seg_off) {
    if (!z || n_seg < 0 || (n_seg && (!seg || !seg_len)) || !out_len) return set_err(LH_E_ARG, "lh_bgzf_compress: null argument");
    int64_t bound = 0;
    for (int k = 0; k < n_seg; ++k) {
        if (seg_len[k] < 0 || (seg_len[k] && !seg[k])) return set_err(LH_E_ARG, "lh_bgzf_compress: bad argument");
        bound += lh_bgzf_bound(seg_len[k]);
    }
    if (out_cap < bound || (bound && !out)) return set_err(LH_E_ARG, "lh_bgzf_compress: out_cap " + std::to_string(out_cap) + " is below the bound, " + std::to_string(bound));
    std::vector<BgzfBlk> blks;
    for (int k = 0; k < n_seg; ++k)
        for (int64_t o = 0; o < seg_len[k]; o += LH_BGZF_DATA) blks.push_back(BgzfBlk{seg[k] + o, (int32_t)(seg_len[k] - o < LH_BGZF_DATA ? seg_len[k] - o : LH_BGZF_DATA), k});
    std::lock_guard<std::mutex> lock(z->mu);
    HIPCHK(hipSetDevice(z->device));
    z->t_up = z->t_kernel = z->t_down = 0;
    int64_t pos = 0;
    if (seg_off) for (int k = 0; k < n_seg; ++k) seg_off[k] = -1;
    int rc = LH_OK;
    size_t chunk = 0;
    for (size_t first = 0; first < blks.size() && !rc; first += (size_t)z->max_blocks, ++chunk) {
        lh_bgzf::Set& s = z->set[chunk & 1];
        if (s.nb) rc = bgzf_collect(z, s, blks, out, out_cap, pos, seg_off);   // chunk - 2: its buffers are this chunk's
        if (!rc) rc = bgzf_submit(z, s, blks, first, (int)(blks.size() - first < (size_t)z->max_blocks ? blks.size() - first : (size_t)z->max_blocks));
    }
    for (size_t k = 0; k < 2 && !rc; ++k) {   // the last two, in order
        lh_bgzf::Set& s = z->set[(chunk + k) & 1];
        if (s.nb) rc = bgzf_collect(z, s, blks, out, out_cap, pos, seg_off);
    }
    if (rc) {   // nothing of this call stays in flight
        const std::string why = g_err;
        for (lh_bgzf::Set& s : z->set) { (void)hipStreamSynchronize(s.st); s.nb = 0; }
        (void)hipGetLastError();
        return set_err(rc, why);
    }
    if (seg_off) {   // an empty segment begins where the next one does
        seg_off[n_seg] = pos;
        for (int k = n_seg - 1; k >= 0; --k) if (seg_off[k] < 0) seg_off[k] = seg_off[k + 1];
    }
    *out_len = pos;
    return LH_OK;
}

int lh_bgzf_compress(lh_bgzf* z, const uint8_t* data, int64_t n, uint8_t* out, int64_t out_cap, int64_t* out_len) {
    if (n < 0 || (n && !data)) return set_err(LH_E_ARG, "lh_bgzf_compress: bad argument");
    return lh_bgzf_compress_segs_(z, n ? 1 : 0, &data, &n, out, out_cap, out_len, nullptr);
}
