// Launchers of the k-mer counting kernels (np2_kcount.hip) for the host driver (np2_kcount_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include <memory>
#include <string>

namespace np2 {

// A counting table: sub-tables [bucket_lo, bucket_hi) of the 1024 (one bucket range of a multi-pass run, or all of them),
// each 1 << cap_log2 slots, `table` pointing at sub-table bucket_lo.  Layout and slot words are YakDev's.
struct KcTable {
    uint64_t *table;
    uint32_t cap_log2, bucket_lo, bucket_hi;
};
// device counters of one table (uint64_t each)
enum : uint32_t { KC_CLAIMED = 0, KC_SPILLED = 1, KC_KMERS = 2, KC_REHASH_FAIL = 3, KC_N_CTR = 4 };

static constexpr uint32_t KC_BLOCK = 256;                   // lanes of a block
static constexpr uint32_t KC_STRETCH = 32;                  // bytes a lane owns
static constexpr uint32_t KC_TILE = KC_BLOCK * KC_STRETCH;  // bytes a block owns

// `in`: HALO bytes of the stream before the piece, then the piece's n bytes, padded with '\n' to a multiple of 16; 16-byte
// aligned.  `spill` has room for n hashes.
void launch_kcount(hipStream_t s, const uint8_t *in, uint64_t n, uint32_t k, const KcTable &t, uint64_t *ctr, uint64_t *spill);
void launch_kcount_insert_hashes(hipStream_t s, const uint64_t *hashes, uint64_t n, const KcTable &t, uint64_t *ctr, uint64_t *spill);
void launch_kcount_rehash(hipStream_t s, const KcTable &from, const KcTable &to, uint64_t *ctr);
void launch_kcount_bucket_sizes(hipStream_t s, const KcTable &t, uint32_t min_count, uint32_t *sizes);
// one block per sub-table: its slots with count >= min_count -> (bucket << 52 | slot key, count) at off[b] .. off[b + 1]
// (off: prefix sums of launch_kcount_bucket_sizes' counts for the same min_count), in any order inside the bucket
void launch_kcount_emit(hipStream_t s, const KcTable &t, uint32_t min_count, const uint64_t *off, uint64_t *keys, uint32_t *counts);
// sorted (key, count) pairs -> file words
void launch_kcount_words(hipStream_t s, const uint64_t *keys, const uint32_t *counts, uint64_t n, uint64_t *words);

} // namespace np2

namespace np2h {
// the I/O entry points' message slot (np2_io_last_error); returns `code`
int io_set_error(int code, const std::string &msg);

// One separator stream in host memory counted for one k into a table that STAYS in HBM (np2_cmp_host.cpp's second table):
// all 1024 sub-tables in YakDev's layout, every word's count at least 1 and capped at 1023, `distinct` words.  Counted on
// `stream` of `device` within the counter's default memory budget, in one pass: NP2_E_NOMEM otherwise.  The stream has
// been drained when the call returns; the run's figures are np2_kcount_last_stats'.
template <class T> struct DevBuf;
struct ResidentCount {
    std::shared_ptr<DevBuf<uint64_t>> table;
    uint32_t cap_log2;
    uint64_t distinct;
};
ResidentCount kcount_resident(int device, hipStream_t stream, const uint8_t *sep_stream, uint64_t n, uint32_t k);
} // namespace np2h
