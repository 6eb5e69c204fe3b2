// Mapping depth of a contig from its alignment records, and the runs of sufficient depth (include/np2_io.h: np2_depth_*).
//
//   k_depth_events  a wavefront per record: the lanes stride over its CIGAR words, the three sums of np2_depth_core.hpp are
//                   reduced across the wavefront, lane 0 applies the admission rule and adds +1 at diff[pos] and -1 at
//                   diff[min(pos + span, L)].  uint32 words that wrap: every prefix sum is a count of open records.  Integer
//                   atomics: the result does not depend on the order of the records.
//   k_depth_scan    inclusive sums of diff in place = depth; 8192 positions a block, blocks chained by the decoupled
//                   look-back (np2_lookback.hpp).  The same pass reduces sum_depth, max_depth and bases_ok.
//                   4 bytes read and 4 written per base.
//   k_depth_runs    position i starts a run iff it is ok and i - 1 is not, ends one iff it is ok and i + 1 is not.  A block
//                   counts its starts, the look-back gives the number of runs before it, and the r-th start and the r-th end
//                   go to starts[r] and ends[r]: runs do not overlap, so the end met after r + 1 starts closes run r.
//                   4 bytes read per base.
//   k_depth_keep    the same compaction over the runs: those of at least min_len positions, in order.
#include "np2_depth.hpp"
#include "np2_blockscan.hpp"

namespace np2 {

namespace {

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void k_depth_events(const np2_bamrec_t *__restrict__ recs, const uint32_t *__restrict__ cigar, uint32_t n_recs,
                                                      uint32_t L, DepthRule rule, uint32_t *__restrict__ diff, DepthDev *__restrict__ ctr) {
    __shared__ uint32_t sh_counted;
    if (threadIdx.x == 0) sh_counted = 0;
    __syncthreads();
    const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (r < n_recs) { // (uniform across the wavefront)
        const np2_bamrec_t rec = recs[r];
        np2depth::Measure m;
        for (uint32_t k = lane; k < rec.n_cigar; k += 64) np2depth::add_op(m, cigar[rec.cigar_off + k]);
        m.span = wave_sum64(m.span), m.aligned = wave_sum64(m.aligned), m.read_len = wave_sum64(m.read_len);
        uint32_t lo, hi;
        if (lane == 0 && np2depth::counted(rec.flag, rec.mapq, rec.n_cigar, m, rule.exclude_flags, rule.min_mapq, rule.min_aligned_fra) &&
            np2depth::cover(rec.pos, m.span, L, lo, hi)) { // lo < L, hi <= L: inside the L + 1 words
            atomicAdd(&diff[lo], 1u);
            atomicAdd(&diff[hi], 0xFFFFFFFFu);
            atomicAdd(&sh_counted, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t first = blockIdx.x * (blockDim.x >> 6);
        atomicAdd(&ctr->n_seen, min(n_recs - first, blockDim.x >> 6));
        if (sh_counted) atomicAdd(&ctr->n_counted, sh_counted);
    }
}

// v[k] = in[i0 + k], 0 from n on; 16-byte loads for whole octets (in is 16-byte aligned: the start of an allocation)
__device__ __forceinline__ void load8(const uint32_t *__restrict__ in, uint32_t i0, uint32_t n, uint32_t (&v)[DEPTH_ITEMS]) {
    if (i0 < n && n - i0 >= DEPTH_ITEMS) {
        const uint4 a = *reinterpret_cast<const uint4 *>(in + i0), b = *reinterpret_cast<const uint4 *>(in + i0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) v[k] = i0 < n && k < n - i0 ? in[i0 + k] : 0u;
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_scan(Lookback lb, uint32_t *__restrict__ depth, uint32_t L, uint32_t min_depth,
                                                              DepthDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    __shared__ uint64_t sh_sum[16];
    __shared__ uint32_t sh_max[16], sh_ok[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    uint32_t v[DEPTH_ITEMS], sum = 0;
    load8(depth, i0, L, v);
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) sum += v[k];
    uint32_t total, pre, unused;
    uint32_t run = block_excl_scan<OpAdd, 16>(sum, sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    run += pre;
    uint64_t dsum = 0;
    uint32_t dmax = 0, n_ok = 0;
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
        run += v[k];
        v[k] = run;
        const bool live = i0 < L && k < L - i0;
        dsum += live ? run : 0u;
        dmax = max(dmax, live ? run : 0u);
        n_ok += live && np2depth::depth_ok(run, min_depth) ? 1u : 0u;
    }
    if (i0 < L && L - i0 >= DEPTH_ITEMS) {
        *reinterpret_cast<uint4 *>(depth + i0) = make_uint4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<uint4 *>(depth + i0 + 4) = make_uint4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < DEPTH_ITEMS; ++k)
            if (i0 < L && k < L - i0) depth[i0 + k] = v[k];
    }
    // the block's three reductions: one atomic each
    dsum = wave_sum64(dsum), dmax = wave_max32(dmax), n_ok = (uint32_t)wave_sum64(n_ok);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh_sum[w] = dsum, sh_max[w] = dmax, sh_ok[w] = n_ok;
    __syncthreads();
    if (threadIdx.x < 64) {
        dsum = lane < 16 ? sh_sum[lane] : 0, dmax = lane < 16 ? sh_max[lane] : 0, n_ok = lane < 16 ? sh_ok[lane] : 0;
        dsum = wave_sum64(dsum), dmax = wave_max32(dmax), n_ok = (uint32_t)wave_sum64(n_ok);
        if (lane == 0) {
            if (dsum) atomicAdd(&ctr->sum_depth, (unsigned long long)dsum);
            if (dmax) atomicMax(&ctr->max_depth, dmax);
            if (n_ok) atomicAdd(&ctr->bases_ok, n_ok);
        }
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_runs(Lookback lb, const uint32_t *__restrict__ depth, uint32_t L, uint32_t min_depth,
                                                              uint32_t *__restrict__ starts, uint32_t *__restrict__ ends, DepthDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    uint32_t v[DEPTH_ITEMS];
    load8(depth, i0, L, v);
    // ok of the positions i0 - 1 .. i0 + 8 in bits 0 .. 9 (outside [0, L): not ok)
    uint32_t okm = 0;
    if (i0 > 0 && i0 - 1 < L && np2depth::depth_ok(depth[i0 - 1], min_depth)) okm |= 1u;
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k)
        if (i0 < L && k < L - i0 && np2depth::depth_ok(v[k], min_depth)) okm |= 2u << k;
    if (i0 < L && L - i0 > DEPTH_ITEMS && np2depth::depth_ok(depth[i0 + DEPTH_ITEMS], min_depth)) okm |= 2u << DEPTH_ITEMS;
    const uint32_t is_start = (okm >> 1) & ~okm & 0xFFu, is_end = (okm >> 1) & ~(okm >> 2) & 0xFFu;
    uint32_t total, pre, unused;
    uint32_t rank = block_excl_scan<OpAdd, 16>((uint32_t)__builtin_popcount(is_start), sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    rank += pre; // runs that start before i0
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
        if ((is_start >> k) & 1u) starts[rank++] = i0 + k;
        if ((is_end >> k) & 1u) ends[rank - 1] = i0 + k; // (an ok position follows a start: rank >= 1)
    }
    if (bid == lb.n_blocks - 1 && threadIdx.x == 0) ctr->n_runs = pre + total;
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_keep(Lookback lb, const uint32_t *__restrict__ starts, const uint32_t *__restrict__ ends,
                                                              uint32_t max_runs, uint32_t min_len, uint32_t *__restrict__ kept_s,
                                                              uint32_t *__restrict__ kept_e, DepthDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    __shared__ uint64_t sh_sum[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t n = min(ctr->n_runs, max_runs); // (written by the launch before this one)
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    uint32_t s[DEPTH_ITEMS], e[DEPTH_ITEMS], keep = 0;
    load8(starts, i0, n, s);
    load8(ends, i0, n, e);
    uint64_t bases = 0;
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k)
        if (i0 < n && k < n - i0 && e[k] >= s[k] && np2depth::run_kept(s[k], e[k], min_len)) keep |= 1u << k, bases += (uint64_t)e[k] - s[k] + 1;
    uint32_t total, pre, unused;
    uint32_t rank = block_excl_scan<OpAdd, 16>((uint32_t)__builtin_popcount(keep), sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    rank += pre;
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k)
        if ((keep >> k) & 1u) kept_s[rank] = s[k], kept_e[rank] = e[k], ++rank; // rank < n <= max_runs
    bases = wave_sum64(bases);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh_sum[w] = bases;
    __syncthreads();
    if (threadIdx.x < 64) {
        bases = wave_sum64(lane < 16 ? sh_sum[lane] : 0);
        if (lane == 0 && bases) atomicAdd(&ctr->bases_kept, (unsigned long long)bases);
    }
    if (bid == lb.n_blocks - 1 && threadIdx.x == 0) ctr->n_kept = pre + total;
}

} // namespace

void launch_depth_events(hipStream_t s, const np2_bamrec_t *recs, const uint32_t *cigar, uint32_t n_recs, uint32_t L, DepthRule rule,
                         uint32_t *diff, DepthDev *ctr) {
    if (n_recs) hipLaunchKernelGGL(k_depth_events, dim3((uint32_t)(((uint64_t)n_recs * 64 + 255) / 256)), dim3(256), 0, s, recs, cigar, n_recs, L, rule, diff, ctr);
}
void launch_depth_scan(hipStream_t s, const Lookback &lb, uint32_t *depth, uint32_t L, uint32_t min_depth, DepthDev *ctr) {
    if (L) hipLaunchKernelGGL(k_depth_scan, dim3(depth_blocks(L)), dim3(DEPTH_THREADS), 0, s, lb, depth, L, min_depth, ctr);
}
void launch_depth_runs(hipStream_t s, const Lookback &lb, const uint32_t *depth, uint32_t L, uint32_t min_depth, uint32_t *starts,
                       uint32_t *ends, DepthDev *ctr) {
    if (L) hipLaunchKernelGGL(k_depth_runs, dim3(depth_blocks(L)), dim3(DEPTH_THREADS), 0, s, lb, depth, L, min_depth, starts, ends, ctr);
}
void launch_depth_keep(hipStream_t s, const Lookback &lb, const uint32_t *starts, const uint32_t *ends, uint32_t max_runs, uint32_t min_len,
                       uint32_t *kept_s, uint32_t *kept_e, DepthDev *ctr) {
    if (max_runs) hipLaunchKernelGGL(k_depth_keep, dim3(depth_blocks(max_runs)), dim3(DEPTH_THREADS), 0, s, lb, starts, ends, max_runs, min_len, kept_s, kept_e, ctr);
}

} // namespace np2
