// Launcher of the short-read quality filter (np2_srqc.hip) for the host drivers (np2_srqc_host.cpp, np2_kcount_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "../../include/np2_io.h"
#include "np2_srqc_core.hpp"

static_assert(sizeof(np2_srqc_opts_t) == sizeof(np2srqc::Opts), "np2_srqc_opts_t is np2srqc::Opts");
static_assert(sizeof(np2_srqc_stats_t) == 8 * np2srqc::N_TOTALS, "np2_srqc_stats_t is the seven totals");

namespace np2 {

// One piece: `seq` / `qual` point at the first of its bytes, 4-byte aligned, with 8 readable bytes before and 16 behind
// the last; ends[i] is the offset of read i's separator (the last byte of the piece is one).  Masks `seq` in place, writes
// reads[i] (or nothing: nullptr) and adds to totals[N_TOTALS].
void launch_srqc(hipStream_t s, uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, const np2srqc::Opts &o,
                 np2_srqc_read_t *reads, uint64_t *totals);

} // namespace np2
