// Launcher of the short-read adapter trimmer (np2_sradapt.hip) for the host drivers (np2_sradapt_host.cpp, np2_kcount_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "../../include/np2_io.h"
#include "np2_sradapt_core.hpp"

static_assert(sizeof(np2_sradapt_read_t) == sizeof(np2sradapt::Read), "np2_sradapt_read_t is np2sradapt::Read");
static_assert(sizeof(np2_sradapt_stats_t) == 8 * np2sradapt::N_TOTALS, "np2_sradapt_stats_t is the fourteen totals");

namespace np2 {

// One piece as launch_srqc takes it (np2_srqc.hpp); in pair mode reads 2r and 2r + 1 are mates and n_reads is even.  Masks
// `seq` in place, writes reads[i] (or nothing: nullptr) and adds to totals[np2sradapt::N_TOTALS].
void launch_sradapt(hipStream_t s, uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, const np2srqc::Opts &qc,
                    const np2sradapt::Opts &o, np2_sradapt_read_t *reads, uint64_t *totals);

} // namespace np2
