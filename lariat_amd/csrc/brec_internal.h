// brec_internal.h — what the BAM writer (bamfile.cpp) hands the device record encoder (lh_brec.inc) for one lh_bam_append.  Internal to the library.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "../../include/lariat_hip.h"

struct LhBrecCall {
    // in: the batch and the writer's layout
    const lh_result* res = nullptr;   // the downloaded result (the host gathers), or
    lh_context* ctx = nullptr;        // ... the context that holds it (lh_bam_append_resident: the device gathers)
    const lh_ingest_batch* in = nullptr;
    const std::vector<std::string>* names = nullptr;        // contig names
    const std::vector<std::vector<int>>* bucket = nullptr;  // [contig][chunk] -> file
    int64_t chunk = 0;
    int threads = 1;
    std::vector<const std::string*> pending;   // per file: the uncompressed bytes the writer still holds (they go in front of the file's records)
    // in / out: the members' buffer, kept by the writer between appends
    std::unique_ptr<uint8_t[]>* zbuf = nullptr;
    int64_t* zbuf_cap = nullptr;
    // out
    bool refused = false;             // the context's result was turned away before anything ran (whatever the code): nothing was appended, the writer goes on
    std::vector<int64_t> seg_off;     // [n files + 1] where each file's members begin in *zbuf, and the end
    std::vector<std::string> rest;    // per file: the bytes behind its last whole block, the writer's next `pending`
    double t[4] = {0, 0, 0, 0};       // gather (the host's, or the device's by events), upload, plan kernels (offsets included), write kernel: seconds
};
// LH_OK: members and rests are ready, nothing of the writer has changed yet.  LH_E_LIMIT / LH_E_ARG: the batch cannot be written, nothing is ready
extern "C" int lh_brec_encode_(lh_bgzf* z, LhBrecCall* c);
