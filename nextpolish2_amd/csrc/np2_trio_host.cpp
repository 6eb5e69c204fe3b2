// Host driver of the trio scan (np2_trio.hip): np2_trio_strings streams host sequences through a staging buffer of fixed
// size (the QV driver's pieces: np2_qv_host.cpp), np2_trio_device scans one sequence where a polish left it.  The class of
// the last marker of a sequence that goes on in the next piece stays on the device (TrioScan::carry).
#include "np2_ctx.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_trio.hpp"

using namespace np2qv;
using namespace np2trio;
using np2kc::HALO;

namespace {

// tiles of the staging buffer (32 MiB of sequence per piece); NP2_TRIO_TEST_STAGE_TILES: a test's smaller pieces
uint32_t stage_tiles() { return (uint32_t)test_hook("NP2_TRIO_TEST_STAGE_TILES", 1, 1 << 16, 4096); }

// the grid: what the device holds at once (4 blocks per CU, as the QV scan), blocks striding over the tiles;
// NP2_TRIO_TEST_BLOCKS: a test's grid
uint32_t trio_blocks(int device) { return grid_blocks(device, 4, "NP2_TRIO_TEST_BLOCKS"); }

struct TrioBufs { // released after the call's device work has completed: cached blocks (DevCache)
    DevBuf<uint8_t> stage;
    DevBuf<uint32_t> desc, tiles, pat_bits, mat_bits, carry;
    DevBuf<uint64_t> stats;
    TrioBufs() { stage.cached = desc.cached = tiles.cached = pat_bits.cached = mat_bits.cached = carry.cached = stats.cached = true; }
};

np2_trio_t trio_of(const uint64_t *st) { return np2_trio_t{st[0], st[1], st[2], {st[3], st[4], st[5], st[6]}}; }

void add_to(np2_trio_t &o, const uint64_t *st) {
    o.n_kmers += st[0];
    o.n_pat += st[1];
    o.n_mat += st[2];
    for (int i = 0; i < 4; ++i) o.pairs[i] += st[3 + i];
}

// one scan and its join on the context's stream: `in` is the staged piece or the resident sequence
void run_scan(np2_ctx_t *cx, int pat_idx, int mat_idx, const np2::ScanStream &in, uint16_t min_count, uint16_t mid_count, const TrioBufs &d,
              bool pat_bits, bool mat_bits, KernelTimer &timer) {
    TrioScan q{};
    q.in = in;
    q.min_count = min_count;
    q.mid_count = mid_count;
    q.stats = reinterpret_cast<unsigned long long *>(d.stats.p);
    q.tiles = d.tiles.p;
    q.pat_bits = pat_bits ? d.pat_bits.p : nullptr;
    q.mat_bits = mat_bits ? d.mat_bits.p : nullptr;
    q.carry = d.carry.p;
    timer.start(cx->stream);
    launch_trio_scan(cx->stream, cx->yaks[pat_idx].dev(), cx->yaks[mat_idx].dev(), q, trio_blocks(cx->device));
    launch_trio_join(cx->stream, q);
    timer.stop(cx->stream);
    HIPCHK(hipGetLastError());
}

} // namespace

// everything about the tables and the thresholds, before anything is launched
void np2::trio_check_tables(np2_ctx *cx, int pat_idx, int mat_idx, uint16_t min_count, uint16_t mid_count, const std::string &who) {
    check_table(cx, pat_idx, who, "pat_idx");
    check_table(cx, mat_idx, who, "mat_idx");
    if (pat_idx == mat_idx) throw Np2Error(NP2_E_ARG, who + ": pat_idx == mat_idx: the parents need a table each");
    if (cx->yaks[pat_idx].k != cx->yaks[mat_idx].k)
        throw Np2Error(NP2_E_ARG, who + ": the parental tables have different k (" + std::to_string(cx->yaks[pat_idx].k) + " and " +
                                      std::to_string(cx->yaks[mat_idx].k) + ")");
    if (!thresholds_ok(min_count, mid_count))
        throw Np2Error(NP2_E_ARG, who + ": thresholds need 1 <= min_count <= mid_count <= 1023 (got " + std::to_string(min_count) + ", " +
                                      std::to_string(mid_count) + ")");
}

extern "C" {

int np2_trio_strings(np2_ctx_t *cx, int pat_idx, int mat_idx, const uint8_t *strs, const uint64_t *off, uint64_t n,
                     uint16_t min_count, uint16_t mid_count, np2_trio_t *out, uint8_t *pat_bits, uint8_t *mat_bits, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        np2::trio_check_tables(cx, pat_idx, mat_idx, min_count, mid_count, "np2_trio_strings");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_trio_strings: out is NULL");
        check_string_set("np2_trio_strings", strs, off, n);
        if (kernel_ms) *kernel_ms = 0.f;
        for (uint64_t i = 0; i < n; ++i) out[i] = np2_trio_t{};
        if (n == 0 || off[n] == off[0]) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        uint64_t all_tiles = 0;
        for (uint64_t i = 0; i < n; ++i) all_tiles += tiles_of(off[i + 1] - off[i]);
        const uint32_t cap = (uint32_t)std::min<uint64_t>(stage_tiles(), all_tiles);
        TrioBufs d;
        d.stage.ensure(HALO + (size_t)cap * QV_TILE);
        d.desc.ensure(cap);
        d.tiles.ensure(cap);
        d.stats.ensure(TRIO_STATS * (size_t)cap);
        d.carry.ensure(1);
        if (pat_bits) d.pat_bits.ensure((size_t)cap * QV_BLOCK);
        if (mat_bits) d.mat_bits.ensure((size_t)cap * QV_BLOCK);
        HIPCHK(hipMemsetAsync(d.carry.p, 0, 4, cx->stream));
        std::vector<uint8_t> hbp(pat_bits ? (size_t)cap * QV_TILE_BITS : 0), hbm(mat_bits ? (size_t)cap * QV_TILE_BITS : 0);
        std::vector<uint64_t> hst(TRIO_STATS * (size_t)cap);
        KernelTimer timer(kernel_ms != nullptr);
        StringPieces sp(strs, off, n, cap, QV_TILE, HALO, QV_PAD, QV_FIRST, QV_TILE_BITS); // (the QV driver's pieces)
        while (sp.next()) {
            const uint32_t nt = sp.nt;
            const auto &spans = sp.spans;
            const uint64_t n_rel = spans.size(); // (<= nt: every span has a tile)
            HIPCHK(hipMemcpyAsync(d.stage.p, sp.hs.data(), HALO + (size_t)nt * QV_TILE, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemcpyAsync(d.desc.p, sp.hd.data(), (size_t)nt * 4, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemsetAsync(d.stats.p, 0, n_rel * TRIO_STATS * 8, cx->stream));
            run_scan(cx, pat_idx, mat_idx, {d.stage.p + HALO, -(int64_t)HALO, (int64_t)nt * QV_TILE, d.desc.p, nt}, min_count, mid_count, d,
                     pat_bits != nullptr, mat_bits != nullptr, timer);
            HIPCHK(hipMemcpyAsync(hst.data(), d.stats.p, n_rel * TRIO_STATS * 8, hipMemcpyDeviceToHost, cx->stream));
            if (pat_bits) HIPCHK(hipMemcpyAsync(hbp.data(), d.pat_bits.p, (size_t)nt * QV_TILE_BITS, hipMemcpyDeviceToHost, cx->stream));
            if (mat_bits) HIPCHK(hipMemcpyAsync(hbm.data(), d.mat_bits.p, (size_t)nt * QV_TILE_BITS, hipMemcpyDeviceToHost, cx->stream));
            HIPCHK(hipStreamSynchronize(cx->stream)); // (the staging buffers are filled again for the next piece)
            timer.collect();
            for (uint64_t r = 0; r < n_rel; ++r) add_to(out[spans[r].seq], &hst[TRIO_STATS * r]);
            for (const auto &s : spans) {
                if (pat_bits) memcpy(pat_bits + s.bit_at, hbp.data() + (size_t)s.tile0 * QV_TILE_BITS, s.bit_bytes);
                if (mat_bits) memcpy(mat_bits + s.bit_at, hbm.data() + (size_t)s.tile0 * QV_TILE_BITS, s.bit_bytes);
            }
        }
        if (kernel_ms) *kernel_ms = timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_trio_device(np2_ctx_t *cx, int pat_idx, int mat_idx, const uint8_t *dev_seq, uint64_t len, uint16_t min_count,
                    uint16_t mid_count, np2_trio_t *out, uint8_t *pat_bits, uint8_t *mat_bits, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        np2::trio_check_tables(cx, pat_idx, mat_idx, min_count, mid_count, "np2_trio_device");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_trio_device: out is NULL");
        if (len && !dev_seq) throw Np2Error(NP2_E_ARG, "np2_trio_device: dev_seq is NULL with a non-zero length");
        if (tiles_of(len) >= QV_FIRST) throw Np2Error(NP2_E_ARG, "np2_trio_device: the sequence is too long");
        if (kernel_ms) *kernel_ms = 0.f;
        *out = np2_trio_t{};
        if (len == 0) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        const uint32_t nt = (uint32_t)tiles_of(len);
        TrioBufs d;
        d.stats.ensure(TRIO_STATS);
        d.tiles.ensure(nt);
        d.carry.ensure(1);
        HIPCHK(hipMemsetAsync(d.stats.p, 0, TRIO_STATS * 8, cx->stream));
        HIPCHK(hipMemsetAsync(d.carry.p, 0, 4, cx->stream));
        if (pat_bits) d.pat_bits.ensure((size_t)nt * QV_BLOCK);
        if (mat_bits) d.mat_bits.ensure((size_t)nt * QV_BLOCK);
        KernelTimer timer(kernel_ms != nullptr);
        // any alignment, nothing readable promised around it: the kernel masks its first and last loads
        run_scan(cx, pat_idx, mat_idx, {dev_seq, 0, (int64_t)len, nullptr, nt}, min_count, mid_count, d, pat_bits != nullptr,
                 mat_bits != nullptr, timer);
        uint64_t st[TRIO_STATS] = {};
        HIPCHK(hipMemcpyAsync(st, d.stats.p, TRIO_STATS * 8, hipMemcpyDeviceToHost, cx->stream));
        if (pat_bits) HIPCHK(hipMemcpyAsync(pat_bits, d.pat_bits.p, bits_bytes(len), hipMemcpyDeviceToHost, cx->stream));
        if (mat_bits) HIPCHK(hipMemcpyAsync(mat_bits, d.mat_bits.p, bits_bytes(len), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        timer.collect();
        *out = trio_of(st);
        if (kernel_ms) *kernel_ms = timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

} // extern "C"
