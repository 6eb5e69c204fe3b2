// The resident SAM handle (np2_sam_t): filled by np2_sam_host.cpp, read there and by the BAM writer (np2_bamout_host.cpp).
#pragma once
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_sam_core.hpp"

struct np2_sam {
    int device = 0;
    np2sam::Refs refs;
    // resident: records and tids in sorted order, their CIGAR words in that order, SEQ bytes as they were met
    DevBuf<uint32_t> recs; // SAM_REC_WORDS words a record
    DevBuf<int32_t> tids;
    DevBuf<uint32_t> cigar;
    DevBuf<uint8_t> seq4;
    // NP2_SAM_KEEP_NAMES: the QNAME bytes as they were met, and per record, in sorted order, offset << 8 | length
    bool has_names = false;
    DevBuf<uint8_t> names;
    DevBuf<uint64_t> name_ref;
    uint64_t n_recs = 0, n_cigar = 0, seq_bytes = 0, name_bytes = 0;
    std::vector<uint64_t> keys; // sorted
    np2_sam_stats_t stats{};
    np2_sam() { recs.cached = tids.cached = cigar.cached = seq4.cached = names.cached = name_ref.cached = true; } // (released when nothing reads them any more)
    ~np2_sam() { (void)hipSetDevice(device); }
};
