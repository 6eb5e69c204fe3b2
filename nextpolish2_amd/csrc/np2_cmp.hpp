// Launchers of the k-mer completeness join (np2_cmp.hip) for its host driver (np2_cmp_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_kcount_core.hpp"

namespace np2 {

static constexpr uint32_t CMP_BLOCK = 256;                        // lanes of a block
static constexpr uint32_t CMP_GROUP = 8;                          // slots a lane streams per turn = probes it has in flight
static constexpr uint32_t CMP_CLASSES = 6;                        // min(copy number, 5): read-only, 1 .. 4, more than 4
static constexpr uint32_t CMP_COUNTS = np2kc::COUNT_MAX + 1;      // stored counts 0 .. 1023
static constexpr uint32_t CMP_SPECTRA = CMP_CLASSES * CMP_COUNTS; // counters of the spectrum
static constexpr uint32_t CMP_ASM_CTR = 1 + CMP_CLASSES;          // n_asm, then asm_only[6]

// One direction of the join of two tables of the same k in YakDev's layout (1024 sub-tables of 1 << cap_log2 slots, 16-byte
// aligned, without repeated keys): every slot of `scan` is streamed, its word dropped when it is EMPTY or its count is
// below scan_min, and looked up in `probe` by yak_get's rule; a found count below probe_min reads as 0.
struct CmpJoin {
    const uint64_t *scan, *probe;
    uint32_t scan_cap_log2, probe_cap_log2;
    uint32_t scan_min, probe_min;
    unsigned long long *out; // added to (zeroed by the caller)
};
// scan = the reads' table, probe = the assembly's: out[cls * 1024 + c] = live read words with stored count c whose
// assembly count cn has min(cn, 5) == cls (CMP_SPECTRA counters)
void launch_cmp_join(hipStream_t s, const CmpJoin &q, uint32_t blocks);
// scan = the assembly's table, probe = the reads': out[0] = live assembly words, out[1 + cls] = those of them whose read
// count is 0, by cls = min(their own count, 5) (CMP_ASM_CTR counters)
void launch_cmp_asm_only(hipStream_t s, const CmpJoin &q, uint32_t blocks);

} // namespace np2
