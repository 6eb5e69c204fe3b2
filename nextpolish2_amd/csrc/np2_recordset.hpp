// A reference's alignment records wherever a reader left them: what the readers of a BAM (np2_bamread.cpp) and of caller-supplied
// arrays hand to the front end (np2_frontend.cpp) and to the depth report.
#pragma once
#include "../../include/np2_io.h"

#include <vector>

namespace np2h {

struct RecordSet {
    // records and CIGAR words on the host: pinned blocks of the handle's device reader (good until its next fetch), the vectors
    // below, or a caller's arrays
    const np2_bamrec_t *recs = nullptr;
    const uint32_t *cigar = nullptr;
    uint32_t n_recs = 0;
    // ... and on the device, where the reader left them there (else null)
    const np2_bamrec_t *d_recs = nullptr;
    const uint32_t *d_cigar = nullptr;
    // SEQ, which np2_bamrec_t::seq_off indexes: seq_bytes bytes on the host, or on the device already
    const uint8_t *seq4 = nullptr, *d_seq = nullptr;
    uint64_t seq_bytes = 0;
    std::vector<uint64_t> voffs; // the records' BGZF virtual offsets, where asked for
    bool from_device = false;    // extracted on the device (the profile line says which reader it was)
    std::vector<np2_bamrec_t> own_recs; // the host reader's records
    std::vector<uint32_t> own_cigar;
    RecordSet() = default;
    RecordSet(RecordSet &&) = default; // (a copy's pointers would still mean the original's vectors)
    // SEQ that is on the device: without records there is nothing to read, and the pointer may be anything
    void device_seq(const uint8_t *d, uint64_t bytes) { d_seq = n_recs ? d : nullptr, seq_bytes = n_recs ? bytes : 0; }
};

} // namespace np2h
