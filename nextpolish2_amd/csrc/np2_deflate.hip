// BGZF output on the GPU (gfx950, wave64): host bytes -> BGZF blocks, the mirror of np2_inflate.hip.  The reference's
// recipe compresses its outputs with gzip on the host (sr.R1.clean.fastq.gz); a zlib thread at level 1 does a few tens of
// MB/s, behind kernels that run at tens of GB/s.
//
// k_bgzf_deflate — one wavefront per block of at most 65280 input bytes, every lane running np2def::deflate_block
//   (np2_deflate_core.hpp: the phases, and why the bytes do not depend on timing).  The lanes walk the block in stripes of
//   64 x 64 bytes; per round a lane reads its 8 bytes and the candidate's from memory (L2 / the CU's cache: the block's
//   64 KB are not kept in LDS), the hash slot from LDS, and enters its position with an LDS atomic max.  LDS per
//   wavefront: the 16 KB hash table — whose place the Huffman builder's arrays and the segments' bit counts take once the
//   tokens stand —, two histograms and a third for the code length code (1.4 KB), the three codes and their lengths
//   (1.0 KB): 18.9 KB, eight wavefronts per CU, as for the inflater.  Tokens (a word per input byte) go through a scratch
//   buffer in memory; a lane reads back only what it wrote itself.  The bit stream is assembled in the slot: the words of
//   the stream are zeroed by the kernel, a lane ORs the two words it may share with its neighbours (atomics at L2) and
//   stores the words in between.  Behind the stream the leader writes the 18 header bytes (BSIZE is known only now), the
//   CRC32 word k_bgzf_crc32 computed over the input piece, and ISIZE.
// k_deflate_pieces — the piece table k_bgzf_crc32 takes.
// k_deflate_offsets / k_deflate_pack — exclusive sums of the slots' sizes (one workgroup: np2_blockscan.hpp), then every
//   slot's bytes to its place in one contiguous stream.
#include <hip/hip_runtime.h>
#include "np2_deflate_core.hpp"
#include "np2_deflate.hpp"
#include "np2_abi.hpp"
#include "np2_blockscan.hpp"

namespace np2 {

__device__ __forceinline__ void def_sync() { // LDS written by this wavefront is read by this wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void def_sync_memory() { // ... and its stores and atomics to memory have arrived
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

struct DefMachine {
    struct Lane {
        uint32_t skip, h;
    };
    Lane st;
    uint32_t lane_;
    template <class F> __device__ __forceinline__ void lanes(F f) {
        f(lane_);
        def_sync();
    }
    template <class F> __device__ __forceinline__ void lead(F f) {
        if (lane_ == 0) f();
        def_sync();
    }
    __device__ __forceinline__ Lane &priv(uint32_t) { return st; }
    __device__ __forceinline__ void hist_add(uint32_t *p) { atomicAdd(p, 1u); }
    __device__ __forceinline__ void slot_max(uint32_t *p, uint32_t v) { atomicMax(p, v); }
    __device__ __forceinline__ void word_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ void word_set(uint32_t *p, uint32_t v) { *p = v; }
    __device__ __forceinline__ void zeroed() { def_sync_memory(); }
};

__global__ __launch_bounds__(64) void k_bgzf_deflate(const uint8_t *__restrict__ in, uint64_t total, uint32_t block_bytes, uint32_t n_blk,
                                                     const uint32_t *__restrict__ crc, uint8_t *slots, uint32_t *tok, uint32_t *__restrict__ sizes) {
    __shared__ __attribute__((aligned(16))) np2def::Shared S;
    const uint32_t b = blockIdx.x;
    if (b >= n_blk) return;
    const uint64_t off = (uint64_t)b * block_bytes;
    if (block_bytes > np2def::MAX_BLOCK || off > total) return; // (the launcher has refused both)
    const uint32_t n = (uint32_t)(total - off < block_bytes ? total - off : block_bytes);
    uint8_t *slot = slots + (size_t)b * np2def::SLOT_BYTES;
    DefMachine m;
    m.st.skip = 0, m.st.h = 0xFFFFFFFFu;
    m.lane_ = threadIdx.x;
    const uint32_t k = np2def::deflate_block(m, S, in + off, n, reinterpret_cast<uint32_t *>(slot), np2def::HDR_BYTES * 8u,
                                             tok + (size_t)b * np2def::TOK_WORDS);
    def_sync_memory(); // (bytes 16 and 17 share a word with the stream's first bits)
    if (threadIdx.x == 0) {
        const uint32_t bsize = np2def::HDR_BYTES + k + np2def::TRL_BYTES;
        const uint8_t hdr[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        for (uint32_t i = 0; i < 16; ++i) slot[i] = hdr[i];
        slot[16] = (uint8_t)((bsize - 1u) & 255u), slot[17] = (uint8_t)((bsize - 1u) >> 8);
        uint8_t *t = slot + np2def::HDR_BYTES + k;
        const uint32_t c = crc[b];
        for (uint32_t i = 0; i < 4; ++i) t[i] = (uint8_t)(c >> (8 * i)), t[4 + i] = (uint8_t)(n >> (8 * i));
        sizes[b] = bsize;
    }
}

__global__ void k_deflate_pieces(InfBlock *__restrict__ tb, uint32_t n_blk, uint32_t block_bytes, uint64_t total) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blk) return;
    const uint64_t off = (uint64_t)b * block_bytes;
    const uint64_t left = off < total ? total - off : 0;
    tb[b] = InfBlock{0, off, 0, (uint32_t)(left < block_bytes ? left : block_bytes)};
}

__global__ __launch_bounds__(BS_THREADS) void k_deflate_offsets(const uint32_t *__restrict__ sizes, uint32_t n_blk, uint32_t *__restrict__ offs,
                                                                 uint32_t *__restrict__ total_host) {
    __shared__ uint32_t sh[16];
    const uint32_t total = block_scan_array<OpAdd>(n_blk, sh, [&](uint32_t i) { return sizes[i]; }, [&](uint32_t i, uint32_t pre, uint32_t) { offs[i] = pre; });
    if (threadIdx.x == 0) {
        offs[n_blk] = total;
        if (total_host) *total_host = total;
    }
}
static constexpr uint32_t PACK_THREADS = 256;
__global__ __launch_bounds__(PACK_THREADS) void k_deflate_pack(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                               const uint32_t *__restrict__ offs, uint32_t n_blk, uint8_t *__restrict__ packed) {
    const uint32_t b = blockIdx.x;
    if (b >= n_blk) return;
    const uint32_t n = sizes[b] <= np2def::SLOT_BYTES ? sizes[b] : 0u; // (a size no slot holds: nothing is read)
    const uint8_t *src = slots + (size_t)b * np2def::SLOT_BYTES;
    uint8_t *dst = packed + offs[b];
    for (uint32_t i = threadIdx.x * 16u; i < n; i += PACK_THREADS * 16u) {
        if (i + 16u <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i); // (slots are 64 KiB apart)
            __builtin_memcpy(dst + i, &v, 16);
        } else {
            for (uint32_t j = i; j < n; ++j) dst[j] = src[j];
        }
    }
}

void launch_deflate_pieces(hipStream_t s, InfBlock *tb, uint32_t n_blk, uint32_t block_bytes, uint64_t total) {
    if (n_blk) hipLaunchKernelGGL(k_deflate_pieces, dim3((n_blk + 255) / 256), dim3(256), 0, s, tb, n_blk, block_bytes, total);
}
void launch_bgzf_deflate(hipStream_t s, const uint8_t *in, uint64_t total, uint32_t block_bytes, uint32_t n_blk, const uint32_t *crc, uint8_t *slots,
                         uint32_t *tok, uint32_t *sizes) {
    if (!n_blk) return;
    if (!block_bytes || block_bytes > np2def::MAX_BLOCK || (uint64_t)n_blk * block_bytes < total || (uint64_t)(n_blk - 1) * block_bytes >= total)
        throw np2h::Np2Error(NP2_E_ARG, "launch_bgzf_deflate: the blocks do not tile the input");
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(n_blk), dim3(64), 0, s, in, total, block_bytes, n_blk, crc, slots, tok, sizes);
}
void launch_deflate_pack(hipStream_t s, const uint8_t *slots, const uint32_t *sizes, uint32_t n_blk, uint32_t *offs, uint8_t *packed, uint32_t *total_host) {
    if (!n_blk) return;
    hipLaunchKernelGGL(k_deflate_offsets, dim3(1), dim3(BS_THREADS), 0, s, sizes, n_blk, offs, total_host);
    hipLaunchKernelGGL(k_deflate_pack, dim3(n_blk), dim3(PACK_THREADS), 0, s, slots, sizes, offs, n_blk, packed);
}

} // namespace np2
