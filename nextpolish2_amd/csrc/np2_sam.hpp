// Launchers of the SAM kernels (np2_sam.hip) for the host driver (np2_sam_host.cpp), and the door np2_frontend.cpp opens for it.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "../../include/np2_io.h"
#include "np2_lookback.hpp"
#include "np2_sam_core.hpp"
#include "np2_samtail_core.hpp"

namespace np2 {

static constexpr uint32_t SAM_BLOCK = 256;                          // lanes of a block
static constexpr uint32_t SAM_STRETCH = 16;                         // text bytes a lane of k_sam_lines owns: one 16-byte load
static constexpr uint32_t SAM_TILE = SAM_BLOCK * SAM_STRETCH;       // ... and its block
static constexpr uint32_t SAM_TEXT_PAD = 64;                        // bytes behind a piece that may be read (and are zero)
static constexpr uint32_t SAM_REC_WORDS = sizeof(np2_bamrec_t) / 4; // a record goes out as ten 32-bit words, padding included
static_assert(sizeof(np2_bamrec_t) == 40, "np2_bamrec_t is written word by word");

// counters of one piece, set by the caller before the first launch (first_err = 0xFFFFFFFF, the others 0)
struct SamCtr {
    uint32_t n_lines;   // k_sam_lines
    uint32_t first_err; // the first line of the piece (0-based) with an error
    uint32_t n_empty;   // lines without a byte
    uint32_t err;       // LB_ERR: a look-back wait gave up
};

inline uint32_t sam_line_blocks(uint64_t n) { return (uint32_t)((n + SAM_TILE - 1) / SAM_TILE); }

// The piece text[0, n) (16-byte aligned, zero up to n + SAM_TEXT_PAD, n below 2^31) ends with '\n'.  line_end[i] = the offset of the '\n'
// that ends line i, in order (room for n entries); ctr->n_lines.  lb: sam_line_blocks(n) blocks.
void launch_sam_lines(hipStream_t s, const Lookback &lb, const uint8_t *text, uint32_t n, uint32_t *line_end, SamCtr *ctr);
// One wavefront per line: lines[i], and for the scans kept[i] (1 for a record that is kept), n_cig[i], n_seq[i] (its CIGAR
// words and packed SEQ bytes, 0 when it is not kept); entry n_lines of the three is set to 0.
void launch_sam_fields(hipStream_t s, const uint8_t *text, const uint32_t *line_end, uint32_t n_lines, np2sam::NameTab nt,
                       np2sam::Line *lines, uint32_t *kept, uint32_t *n_cig, uint32_t *n_seq, SamCtr *ctr);
// One wavefront per line, at work for a kept one: record rec_base + kept_off[i] (input order), its CIGAR words from
// cig_base + cig_off[i] on, its SEQ bytes from seq_base + seq_off[i] on, its tid and its sort key.
void launch_sam_pack(hipStream_t s, const uint8_t *text, const np2sam::Line *lines, uint32_t n_lines, const uint32_t *kept_off,
                     const uint32_t *cig_off, const uint32_t *seq_off, uint64_t rec_base, uint64_t cig_base, uint64_t seq_base,
                     uint32_t tie_by_strand, uint32_t *recs, int32_t *tids, uint64_t *keys, uint32_t *cigar, uint8_t *seq4);
// vals[i] = i
void launch_sam_iota(hipStream_t s, uint32_t *vals, uint32_t n);
// n_cig[i] = the CIGAR words of record order[i]; n_cig[n] = 0
void launch_sam_sorted_sizes(hipStream_t s, const uint32_t *recs_in, const uint32_t *order, uint32_t n, uint32_t *n_cig);
// One wavefront per record of the sorted order: record i = input record order[i] with its CIGAR words moved to cig_off[i]
void launch_sam_gather(hipStream_t s, const uint32_t *recs_in, const int32_t *tids_in, const uint32_t *cigar_in, const uint32_t *order,
                       const uint32_t *cig_off, uint32_t n, uint32_t *recs, int32_t *tids, uint32_t *cigar);

// NP2_SAM_KEEP_NAMES, after launch_sam_fields.  One wavefront per line: n_name[i] = the bytes of a kept line's QNAME (those
// before its first tab), 0 for a line that is not kept; entry n_lines is set to 0.  A kept line whose QNAME is empty or longer
// than 254 bytes: *first_bad = min(*first_bad, i).
void launch_sam_name_len(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                         uint32_t *n_name, uint32_t *first_bad);
// ... and after the scan: a kept line's QNAME to names + name_base + name_off[i], and for its record (input order)
// name_ref[rec_base + kept_off[i]] = offset << 8 | length
void launch_sam_name_copy(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                          const uint32_t *kept_off, const uint32_t *name_off, uint64_t rec_base, uint64_t name_base, uint8_t *names,
                          uint64_t *name_ref);
// NP2_SAM_KEEP_ALL, after launch_sam_fields.  One wavefront per line: t_size[i] = the bytes of a kept line's tail (np2_samtail_core.hpp),
// padded to a multiple of 4, 0 for a line that is not kept; t_aux[i] = its aux_len | has_qual << 31; entry n_lines of both is set
// to 0.  A kept line with a bad mate field, QUAL or optional field: *first_bad = min(*first_bad, i).
void launch_sam_tail_len(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                         np2sam::NameTab nt, uint32_t *t_size, uint32_t *t_aux, uint32_t *first_bad);
// ... and after the scan: a kept line's tail to tails + tail_base + tail_off[i] (tail_base a multiple of 4), and for its record
// (input order) tail_ref[rec_base + kept_off[i]] = offset << 1 | has_qual
void launch_sam_tail_emit(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                          np2sam::NameTab nt, const uint32_t *kept_off, const uint32_t *tail_off, const uint32_t *t_aux, uint64_t rec_base,
                          uint64_t tail_base, uint8_t *tails, uint64_t *tail_ref);
// out[i] = in[order[i]]
void launch_sam_gather_u64(hipStream_t s, const uint64_t *in, const uint32_t *order, uint32_t n, uint64_t *out);

} // namespace np2

struct np2_ctx;
struct np2_contig;
namespace np2h {
// np2_contig_from_records over records and CIGAR words on the host and SEQ bytes that are on cx's device already (d_seq4:
// seq4_bytes bytes, complete; seq_off indexes it).  np2_frontend.cpp, next to the front end.
void contig_from_device_seq(np2_ctx *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                            const uint8_t *d_seq4, uint64_t seq4_bytes, const np2_front_opts_t *opts, np2_contig **out);
} // namespace np2h
