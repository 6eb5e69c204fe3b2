// K-mer completeness and copy-number spectrum: a hash join of two HBM-resident k-mer tables of the same k, the reads'
// (YakDev) and one counted from the assembly (np2_kcount_host.cpp's resident table, the same layout).  Where k_qv_scan,
// k_trio_scan and k_bin_scan stream SEQUENCE and probe a table, this kernel streams a TABLE, every slot of it, and probes
// the other table with each live word:
//
//   k_cmp_join      reads' slots -> assembly table: spectra[min(cn, 5)][stored read count]
//   k_cmp_asm_only  assembly's slots -> reads' table: n_asm and asm_only[min(cn, 5)]
//
// (one body, cmp_scan<JOIN>, for both: they differ in what a live word's answer is added to)
//
// Stream: a block takes turns of CMP_BLOCK * CMP_GROUP consecutive slots; a lane loads CMP_GROUP / 2 times 16 bytes (two
// slots), the lanes of a wavefront 1 KiB in a row per load.  A slot's bucket is its index >> cap_log2; its word is
// key << 10 | count with key = hash >> 10, so the hash is (w >> 10) << 10 | bucket and no base is ever looked at.  EMPTY
// words and words below the threshold are dropped (a table is at most half full: about every other slot and more).
//
// Probes: the probe contract of np2_kmerscan.hpp on the other table: the lane's CMP_GROUP first-slot loads back to back
// before any word is looked at, then the words that met another key one more slot each per round, again together.  The
// loop is this kernel's own, on (key, bucket) pairs with a slot index per word: next to a stream of slots, with no hashing
// to hide it behind, probe_settle's 64-bit slot arithmetic per round made the two kernels 8 % slower (0.403 -> 0.434 ms on
// the 12 Mb assembly's tables, k = 21), and probe_settle with this loop's slot indices costs k_trio_scan a wavefront per
// SIMD in registers.
//
// Cost: the scanned table's bytes once, in order, plus one random sector of the probed table per live word (and a few
// more where a probe chain is longer than one slot).
//
// Counters: the spectrum is a histogram in LDS (6 x 1024 x 4 B = 24 KiB per block), flushed once per block with 64-bit
// atomics; n_read and n_found are sums over it and are not counted a second time.  A cell cannot overflow 32 bits: a
// block streams fewer than 2^32 slots (launch_cmp: at most 2^20 turns of 2^11 slots), and a cell counts slots.  The other
// direction needs seven counters: per-lane registers, summed over the wavefront, one LDS add per wavefront and one atomic
// per block and counter.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "np2_cmp.hpp"
#include "np2_kmerscan.hpp"

namespace np2 {
using namespace np2kc;

namespace {

static constexpr uint32_t CMP_LOADS = CMP_GROUP / 2;                 // 16-byte loads of a lane per turn
static constexpr uint32_t CMP_TURN_VEC = CMP_BLOCK * CMP_LOADS;      // 16-byte pieces of a turn
static constexpr uint64_t CMP_MAX_TURNS = 1ull << 20;                // turns of one block: 2^20 * 2^11 slots < 2^32
static_assert(CMP_MAX_TURNS * CMP_BLOCK * CMP_GROUP < (1ull << 32), "a block's slots fit a 32-bit counter");

template <bool JOIN> __device__ __forceinline__ void cmp_scan(const CmpJoin &q) {
    __shared__ uint32_t s_hist[JOIN ? CMP_SPECTRA : CMP_ASM_CTR];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (JOIN ? CMP_SPECTRA : CMP_ASM_CTR); i += CMP_BLOCK) s_hist[i] = 0;
    __syncthreads();

    const uint64_t n_vec = ((uint64_t)N_BUCKETS << q.scan_cap_log2) >> 1; // 16-byte pieces of the scanned table
    const uint64_t n_turns = (n_vec + CMP_TURN_VEC - 1) / CMP_TURN_VEC;
    const uint64_t capm = (1ULL << q.probe_cap_log2) - 1;
    const uint4 *src = reinterpret_cast<const uint4 *>(q.scan);
    uint32_t n_live = 0, only[CMP_CLASSES] = {0, 0, 0, 0, 0, 0}; // (k_cmp_asm_only; indexed by constants only)

    for (uint64_t turn = blockIdx.x; turn < n_turns; turn += gridDim.x) {
        uint64_t key[CMP_GROUP];
        uint32_t bkt[CMP_GROUP], c[CMP_GROUP], cn[CMP_GROUP];
        uint32_t valid = 0;
        uint4 x[CMP_LOADS];
#pragma unroll
        for (uint32_t l = 0; l < CMP_LOADS; ++l) { // (the table's last turn may be a partial one)
            const uint64_t v = turn * CMP_TURN_VEC + l * CMP_BLOCK + tid;
            x[l] = v < n_vec ? src[v] : make_uint4(~0u, ~0u, ~0u, ~0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < CMP_GROUP; ++j) {
            const uint4 &xv = x[j >> 1];
            const uint64_t w = (j & 1u) ? ((uint64_t)xv.w << 32 | xv.z) : ((uint64_t)xv.y << 32 | xv.x);
            const uint64_t slot = 2 * (turn * CMP_TURN_VEC + (j >> 1) * CMP_BLOCK + tid) + (j & 1u);
            c[j] = (uint32_t)(w & COUNT_MAX);
            const bool live = w != YAK_EMPTY && c[j] >= q.scan_min;
            key[j] = live ? w >> COUNT_BITS : 0;
            bkt[j] = live ? (uint32_t)(slot >> q.scan_cap_log2) : 0u; // (< 1024: a live word lies inside the table)
            cn[j] = 0;
            valid |= (live ? 1u : 0u) << j;
        }
        // round 0: every first-slot load is issued before any word is looked at (the scheduling barriers: np2_qv.hip)
        uint64_t w[CMP_GROUP];
        uint32_t s[CMP_GROUP];
        const uint64_t *at[CMP_GROUP];
#pragma unroll
        for (uint32_t j = 0; j < CMP_GROUP; ++j) {
            s[j] = (uint32_t)(key[j] & capm);
            at[j] = q.probe + (((uint64_t)bkt[j] << q.probe_cap_log2) + s[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t j = 0; j < CMP_GROUP; ++j) w[j] = *at[j];
        __builtin_amdgcn_sched_barrier(0);
        uint32_t pend = 0;
#pragma unroll
        for (uint32_t j = 0; j < CMP_GROUP; ++j) {
            const bool hit = (w[j] >> COUNT_BITS) == key[j]; // (EMPTY >> 10 is no key: a hash has 62 bits at most)
            if (hit) cn[j] = (uint32_t)(w[j] & COUNT_MAX);
            pend |= (((valid >> j) & 1u) && !hit && w[j] != YAK_EMPTY ? 1u : 0u) << j;
        }
        // the words whose slot held another key: one more slot each per round, loaded together (a settled one loads its
        // last slot again, a cache hit)
        for (uint64_t probe = 1; pend && probe <= capm; ++probe) {
#pragma unroll
            for (uint32_t j = 0; j < CMP_GROUP; ++j) {
                s[j] = (uint32_t)((s[j] + ((pend >> j) & 1u)) & capm);
                w[j] = q.probe[((uint64_t)bkt[j] << q.probe_cap_log2) + s[j]];
            }
#pragma unroll
            for (uint32_t j = 0; j < CMP_GROUP; ++j)
                if ((pend >> j) & 1u) {
                    const bool hit = (w[j] >> COUNT_BITS) == key[j];
                    if (hit) cn[j] = (uint32_t)(w[j] & COUNT_MAX);
                    if (hit || w[j] == YAK_EMPTY) pend &= ~(1u << j);
                }
        }
#pragma unroll
        for (uint32_t j = 0; j < CMP_GROUP; ++j) {
            const bool live = (valid >> j) & 1u;
            const uint32_t found = cn[j] >= q.probe_min ? cn[j] : 0u; // (a dropped slot's cn is never looked at)
            if (JOIN) {
                if (live) atomicAdd(&s_hist[(found < CMP_CLASSES - 1 ? found : CMP_CLASSES - 1) * CMP_COUNTS + c[j]], 1u);
            } else {
                n_live += live ? 1u : 0u;
                const uint32_t cls = c[j] < CMP_CLASSES - 1 ? c[j] : CMP_CLASSES - 1;
#pragma unroll
                for (uint32_t k = 1; k < CMP_CLASSES; ++k) only[k] += (live && found == 0u && cls == k) ? 1u : 0u;
            }
        }
    }

    if (JOIN) {
        __syncthreads();
        for (uint32_t i = tid; i < CMP_SPECTRA; i += CMP_BLOCK) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&q.out[i], (unsigned long long)v);
        }
    } else {
        only[0] = n_live; // (asm_only[0] is always 0: a live word's own count is at least 1)
#pragma unroll
        for (uint32_t k = 0; k < CMP_CLASSES; ++k) {
            const uint32_t a = wave_sum(only[k]);
            if ((tid & 63u) == 0 && a) atomicAdd(&s_hist[k == 0 ? 0 : 1 + k], a);
        }
        __syncthreads();
        if (tid < CMP_ASM_CTR && s_hist[tid]) atomicAdd(&q.out[tid], (unsigned long long)s_hist[tid]);
    }
}

} // namespace

__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_join(CmpJoin q) { cmp_scan<true>(q); }
__global__ __launch_bounds__(CMP_BLOCK) void k_cmp_asm_only(CmpJoin q) { cmp_scan<false>(q); }

namespace {

template <bool JOIN> void launch_cmp(hipStream_t s, const CmpJoin &q, uint32_t blocks) {
    const uint64_t n_vec = ((uint64_t)N_BUCKETS << q.scan_cap_log2) >> 1;
    const uint64_t n_turns = (n_vec + CMP_TURN_VEC - 1) / CMP_TURN_VEC;
    // the grid: what the caller sized to the device, no more blocks than turns, and enough of them that a block's share of
    // the slots fits the 32-bit cells of its LDS histogram
    uint64_t grid = std::max<uint64_t>(blocks ? blocks : 1u, (n_turns + CMP_MAX_TURNS - 1) / CMP_MAX_TURNS);
    grid = std::min<uint64_t>(grid, n_turns);
    hipLaunchKernelGGL(JOIN ? k_cmp_join : k_cmp_asm_only, dim3((uint32_t)grid), dim3(CMP_BLOCK), 0, s, q);
}

} // namespace

void launch_cmp_join(hipStream_t s, const CmpJoin &q, uint32_t blocks) { launch_cmp<true>(s, q, blocks); }
void launch_cmp_asm_only(hipStream_t s, const CmpJoin &q, uint32_t blocks) { launch_cmp<false>(s, q, blocks); }

} // namespace np2
