// The read front end (np2_frontend.cpp): a reference's records -> admission -> the columnariser on the device -> an np2_contig.
#pragma once
#include "np2_ctx.hpp"
#include "np2_recordset.hpp"

namespace np2h {

// A reference-interval shard built straight from its BAM records (np2_shard_bam_*): the pileup covers the sub-contig
// [sub_lo, sub_hi) of a contig of L_glob positions; `renumber` turns the pushed records (local order, with the index of
// their input record) into the shard's read list in contig-wide numbering (holes for the contig's reads the shard does
// not hold) once the ranks have exchanged their counts.
struct ShardSpec {
    uint32_t sub_lo = 0, sub_hi = 0, zone_lo = 0, zone_hi = 0;
};
// state between the two halves of the front end: admission + GPU columnariser + keep / drop (front_begin), then the
// clip filter and the contig bookkeeping (front_finish).  A shard renumbers `reads` in between (contig-wide numbers,
// holes for the reads it does not hold) once the ranks have exchanged their records' file offsets.
struct FrontWork {
    np2_contig *c = nullptr;
    std::vector<np2_read_t> reads; // [0] = the (sub-)contig; then the pushed records in file order
    std::vector<uint8_t> lable;
    std::vector<uint32_t> rec_of;  // input record of reads[i]
    uint64_t nib_bytes = 0;
    uint32_t L = 0, L_glob = 0, sub_lo = 0;
    ~FrontWork() { delete c; }
};
// rs.seq4: the records' SEQ bytes on the host (uploaded here) — or, with rs.d_seq, already on the device, on this context's stream
void front_begin(np2_ctx *cx, const uint8_t *ref_glob, uint32_t L_in, const RecordSet &rs, const np2_front_opts_t *o, const ShardSpec *sp,
                 FrontWork &fw);
void front_finish(np2_ctx *cx, FrontWork &fw, np2_contig **out);

} // namespace np2h
