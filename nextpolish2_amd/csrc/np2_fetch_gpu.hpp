// Read extraction on the device (np2_fetch_gpu.cpp), as np2_bamread.cpp sees it.
#pragma once
#include "np2_bamfile.hpp"
#include "np2_recordset.hpp"

namespace np2h {

// Does this reference take the device path?  (read per contig, not per pass: a tool may switch between two reads of the same file)
bool gpu_fetch_wanted(const np2_bam *bam, int tid);
// The records of reference `tid` (all of them: fetch(tid, 0, L)).  false: this BAM / index cannot take the device path
// (no linear index, an index entry that is not a record start) — the caller reads it the host way.
// zone [zone_lo, zone_hi): (0, L) for the whole contig, or a shard's interval; `voffs` (optional) receives the records' BGZF
// virtual offsets: what the ranks exchange to number their reads contig-wide.
bool fetch_records_gpu(np2_bam *bam, int tid, uint32_t L, uint32_t zone_lo, uint32_t zone_hi, hipStream_t s, RecordSet &out, std::vector<uint64_t> *voffs);

} // namespace np2h
