// The resident SAM handle (np2_sam_t): filled by np2_sam_host.cpp, read there and by the BAM writer (np2_bamout_host.cpp).
#pragma once
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_sam_core.hpp"
#include "np2_samtail_core.hpp"

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
    // NP2_SAM_KEEP_ALL: the tails as they were met (np2_samtail_core.hpp: mate fields, aux_len, quality bytes, optional fields), per
    // record, in sorted order, offset << 1 | has_qual, and the header lines of the input other than @HD and @SQ ('\n' after each)
    bool has_tails = false;
    DevBuf<uint8_t> tails;
    DevBuf<uint64_t> tail_ref;
    uint64_t tail_bytes = 0;
    std::string extra_header, header_text; // header_text: what the full stream carries
    float tail_len_ms = 0.f, tail_emit_ms = 0.f; // k_sam_tail_len and its scan; k_sam_tail_emit (HIP events, summed over the pieces)
    uint64_t n_recs = 0, n_cigar = 0, seq_bytes = 0, name_bytes = 0;
    std::vector<uint64_t> keys; // sorted
    np2_sam_stats_t stats{};
    np2_bamin_stats_t bamin{}; // of the inputs that were BAM (np2_sam_bamin_stats)
    np2_sam() { recs.cached = tids.cached = cigar.cached = seq4.cached = names.cached = name_ref.cached = tails.cached = tail_ref.cached = true; } // (released when nothing reads them any more)
    ~np2_sam() { (void)hipSetDevice(device); }
};

namespace np2h {
// the text of the BAM header: @HD, one @SQ line per reference, then `extra` (whole lines, '\n' after each)
std::string bam_header_text(const np2sam::Refs &refs, const std::string &extra);
// The alignment line text[0, e) (no '\r', no '\n') has a bad mate field, QUAL or optional field: throws what tail_line says of
// it, `at` in front, with the field's name or TAG.  Returns when the tail is good or the lean parse refuses the line.
void throw_tail_error(const uint8_t *line, uint32_t e, const np2sam::NameTab &nt, const std::string &at);
// BAM input (np2_bamin_host.cpp).  Is the file's first BGZF block one that inflates to "BAM\1"?  (false when it cannot be read)
bool is_bam_file(const std::string &path);
// The header of the BAM open as fd, inflated on the host: its reference list, the lines of its text other than @HD and @SQ, and
// where the first record lies: `skip` inflated bytes into the BGZF block at file offset *first_block (the file's length when
// the header ends the file).  A damaged header throws NP2_E_ARG with `name` in front.
void bam_read_header(int fd, uint64_t file_len, const std::string &name, np2sam::Refs &refs, std::vector<std::string> &extra, uint64_t *first_block,
                     uint32_t *skip);
} // namespace np2h
