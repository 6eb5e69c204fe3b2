// CRC-32 of the inflated BGZF blocks on the GPU (gfx950, wave64): every BGZF block ends in CRC32 | ISIZE, DEFLATE has no
// checksum of its own, and a damaged block that still inflates to ISIZE bytes would be polished into a different FASTA
// without a word.  htslib checks the word for every block it inflates (the reference dies on the error, main.rs:1751-1752).
//
// k_bgzf_crc32 — one wavefront per block over the INFLATED stream, launched on the same stream right behind
//   k_bgzf_inflate, four blocks per workgroup sharing one 4 KB copy of the slice-by-4 tables in LDS.  The arithmetic is
//   np2_crc32_core.hpp's: the block lies right-aligned in a frame of 64 KiB, lane l sums frame bytes [1024 l, 1024 (l + 1))
//   — the lane that holds the block's first byte takes its up to 15 odd bytes one at a time, the rest is 16-byte chunks —,
//   and six steps of mulmod(left, x^(8 * 1024 * 2^s)) ^ right join the 64 registers in lane 63.
//   The bytes come through LDS in tiles of 128 B a lane: eight lanes load one lane's 128 contiguous bytes (16 B each,
//   unaligned: a block starts at any byte of the stream), the rows lie 144 bytes apart in LDS (a lane's ds_read_b128 of its
//   own row: 36 dwords of stride, no two lanes of a group of sixteen on one bank), and the next tile's loads are in flight
//   while this one goes through the tables.  (Each lane loading its own 16 bytes — 64 cache lines per wave-wide load, each
//   read seven more times by its lane — took 0.16 / 2.37 ms where this takes 0.09 / 0.62 for 210 MB / 2.7 GB of stream and
//   fetched 1.8 / 4.3 times the bytes: the lines did not stay in the CU's cache, profiles/bgzf_crc32_cost.txt.)
//   A mismatch writes ST_CRC_MISMATCH into the block's status word and bumps n_bad — the words the host already waits for
//   behind the inflate.  A block whose inflate failed keeps its status (its output is partial and is not read).  No load
//   leaves the block's [out_off, out_off + isize).
#include <hip/hip_runtime.h>
#include "np2_crc32_core.hpp"
#include "np2_inflate_core.hpp"
#include "np2_inflate.hpp"

namespace np2 {

static constexpr uint32_t CRC_WAVES = 4; // blocks per workgroup
static constexpr uint32_t CRC_ROW = 128, CRC_ROW_STRIDE = 144, CRC_TILES = np2crc::PIECE / CRC_ROW;
static_assert(CRC_ROW == 8 * 16 && CRC_ROW_STRIDE % 16 == 0, "eight lanes of 16 bytes load a row; rows stay 16-byte aligned");

__device__ __forceinline__ void crc_sync() { // LDS written by this wavefront is read by this wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * CRC_WAVES) void k_bgzf_crc32(const InfBlock *__restrict__ blk, uint32_t n_blk, const uint32_t *__restrict__ want,
                                                                const uint8_t *__restrict__ data, uint32_t *__restrict__ status,
                                                                uint32_t *__restrict__ n_bad, uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t T[1024];
    __shared__ __attribute__((aligned(16))) uint8_t stage[CRC_WAVES][64 * CRC_ROW_STRIDE];
    for (uint32_t i = threadIdx.x; i < 1024u; i += 64u * CRC_WAVES) T[i] = np2crc::table_word(i >> 8, i & 255u);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * CRC_WAVES + wave;
    if (b >= n_blk) return;
    if (status && status[b] != np2inf::ST_OK) return; // (not inflated: nothing to check, and the inflate's verdict stands)
    const InfBlock B = blk[b];
    uint32_t crc = 0; // (of the empty block)
    const bool ok = B.isize <= np2crc::FRAME;
    if (ok && B.isize) {
        const uint8_t *__restrict__ d = data + B.out_off;
        const uint32_t n = B.isize;
        // Row r of tile t = the block's bytes [hi(r) - 1024 + 128 t, + 128), as far as they lie at or behind the row's first
        // 16-byte chunk (block offsets, signed: in front of a short first piece they are negative and never loaded).
        auto chunks_from = [&](uint32_t r) { // first byte of row r's 16-byte chunks; beyond every offset for a lane without bytes
            const np2crc::LanePiece p = np2crc::lane_piece(n, r);
            return p.lo == p.hi ? (int32_t)np2crc::FRAME : (int32_t)(p.lo + np2crc::piece_head(p));
        };
        auto tile_at = [&](uint32_t r, uint32_t t) { return (int32_t)np2crc::lane_piece(n, r).hi - (int32_t)np2crc::PIECE + (int32_t)(CRC_ROW * t); };
        const np2crc::LanePiece mine = np2crc::lane_piece(n, lane);
        uint32_t r = mine.first ? 0xFFFFFFFFu : 0u;
        if (mine.first)
            for (uint32_t k = 0; k < np2crc::piece_head(mine); ++k) r = np2crc::step1(T, r, d[k]);
        const int32_t my_from = chunks_from(lane);
        // the first tile that holds a chunk: all of them once a second lane has a piece (the same in every lane)
        uint32_t t0 = 0;
        if (n <= np2crc::PIECE) t0 = (np2crc::PIECE - (n & ~15u)) / CRC_ROW; // (CRC_TILES: fewer than 16 bytes, no chunk at all)
        uint4 v[8];
        auto load_tile = [&](uint32_t t) {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t rr = 8u * j + (lane >> 3);
                const int32_t o = tile_at(rr, t) + 16 * (int32_t)(lane & 7u);
                v[j] = make_uint4(0, 0, 0, 0);
                if (o >= chunks_from(rr)) __builtin_memcpy(&v[j], d + o, 16); // (o + 16 <= hi(rr) <= n)
            }
        };
        uint8_t *S = stage[wave];
        if (t0 < CRC_TILES) load_tile(t0);
        for (uint32_t t = t0; t < CRC_TILES; ++t) {
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) *reinterpret_cast<uint4 *>(S + (8u * j + (lane >> 3)) * CRC_ROW_STRIDE + 16u * (lane & 7u)) = v[j];
            crc_sync();
            if (t + 1 < CRC_TILES) load_tile(t + 1);
            const int32_t o0 = tile_at(lane, t);
#pragma unroll
            for (uint32_t c = 0; c < 8; ++c) {
                const uint4 w = *reinterpret_cast<const uint4 *>(S + lane * CRC_ROW_STRIDE + 16u * c);
                if (o0 + 16 * (int32_t)c >= my_from) {
                    r = np2crc::step4(T, r, w.x);
                    r = np2crc::step4(T, r, w.y);
                    r = np2crc::step4(T, r, w.z);
                    r = np2crc::step4(T, r, w.w);
                }
            }
            crc_sync(); // (the next tile overwrites the rows)
        }
#pragma unroll
        for (uint32_t s = 0; s < 6u; ++s) r = np2crc::fold_step(s, lane, r, (uint32_t)__shfl_up((int)r, 1u << s, 64));
        crc = ~(uint32_t)__builtin_amdgcn_readlane((int)r, 63);
    }
    if (lane == 0) {
        if (crc_out) crc_out[b] = crc;
        if (want && (!ok || crc != want[b])) {
            status[b] = np2inf::ST_CRC_MISMATCH;
            atomicAdd(n_bad, 1u);
        }
    }
}

void launch_bgzf_crc32(hipStream_t s, const InfBlock *blk, uint32_t n_blk, const uint32_t *want, const uint8_t *data, uint32_t *status, uint32_t *n_bad,
                       uint32_t *crc_out) {
    if (n_blk) hipLaunchKernelGGL(k_bgzf_crc32, dim3((n_blk + CRC_WAVES - 1) / CRC_WAVES), dim3(64 * CRC_WAVES), 0, s, blk, n_blk, want, data, status, n_bad, crc_out);
}

} // namespace np2
