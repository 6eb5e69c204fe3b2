// Host driver of the k-mer QV scan (np2_qv.hip): np2_qv_strings streams host sequences through a staging buffer of fixed
// size, np2_qv_device scans one sequence where a polish left it.  (np2_qv.cpp would share the kernel file's object name.)
#include "np2_ctx.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_qv.hpp"

using namespace np2qv;
using np2kc::HALO;

namespace {

// tiles of the staging buffer (32 MiB of sequence per piece); NP2_QV_TEST_STAGE_TILES: a test's smaller pieces
uint32_t stage_tiles() { return (uint32_t)test_hook("NP2_QV_TEST_STAGE_TILES", 1, 1 << 16, 4096); }

// the grid: what the device holds at once (the kernel's registers admit 4 wavefronts per SIMD: 4 blocks per CU), blocks
// striding over the tiles
uint32_t qv_blocks(int device) { return grid_blocks(device, 4); }

struct QvBufs { // released after the call's device work has completed: cached blocks (DevCache)
    DevBuf<uint8_t> stage;
    DevBuf<uint32_t> desc, bits;
    DevBuf<uint64_t> stats, hist;
    QvBufs() { stage.cached = desc.cached = bits.cached = stats.cached = hist.cached = true; }
};

// one scan on the context's stream: `in` is the staged piece or the resident sequence
void run_scan(np2_ctx_t *cx, int yak_idx, const np2::ScanStream &in, uint16_t min_count, const QvBufs &d, bool hist, bool bits,
              KernelTimer &timer) {
    QvScan q{};
    q.in = in;
    q.min_count = min_count;
    q.stats = reinterpret_cast<unsigned long long *>(d.stats.p);
    q.hist = hist ? reinterpret_cast<unsigned long long *>(d.hist.p) : nullptr;
    q.bits = bits ? d.bits.p : nullptr;
    timer.start(cx->stream);
    launch_qv_scan(cx->stream, cx->yaks[yak_idx].dev(), q, qv_blocks(cx->device));
    timer.stop(cx->stream);
    HIPCHK(hipGetLastError());
}

} // namespace

extern "C" {

int np2_qv_strings(np2_ctx_t *cx, int yak_idx, const uint8_t *strs, const uint64_t *off, uint64_t n, uint16_t min_count,
                   np2_qv_t *out, uint64_t *hist, uint8_t *absent_bits, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        check_table(cx, yak_idx, "np2_qv_strings", "yak_idx");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_qv_strings: out is NULL");
        check_string_set("np2_qv_strings", strs, off, n);
        if (kernel_ms) *kernel_ms = 0.f;
        if (hist) memset(hist, 0, QV_HIST_BINS * sizeof(uint64_t));
        for (uint64_t i = 0; i < n; ++i) out[i] = np2_qv_t{0, 0};
        if (n == 0 || off[n] == off[0]) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        // the staging buffers, host and device: what the call needs, up to the fixed piece size
        uint64_t all_tiles = 0;
        for (uint64_t i = 0; i < n; ++i) all_tiles += tiles_of(off[i + 1] - off[i]);
        const uint32_t cap = (uint32_t)std::min<uint64_t>(stage_tiles(), all_tiles);
        QvBufs d;
        d.stage.ensure(HALO + (size_t)cap * QV_TILE);
        d.desc.ensure(cap);
        d.stats.ensure(2 * (size_t)cap);
        if (absent_bits) d.bits.ensure((size_t)cap * QV_BLOCK);
        if (hist) {
            d.hist.ensure(QV_HIST_BINS);
            HIPCHK(hipMemsetAsync(d.hist.p, 0, QV_HIST_BINS * 8, cx->stream));
        }
        std::vector<uint8_t> hb(absent_bits ? (size_t)cap * QV_TILE_BITS : 0);
        std::vector<uint64_t> hst(2 * (size_t)cap);
        KernelTimer timer(kernel_ms != nullptr);
        StringPieces sp(strs, off, n, cap, QV_TILE, HALO, QV_PAD, QV_FIRST, QV_TILE_BITS);
        while (sp.next()) {
            const uint32_t nt = sp.nt;
            const auto &spans = sp.spans;
            const uint64_t n_rel = spans.size(); // (<= nt: every span has a tile)
            HIPCHK(hipMemcpyAsync(d.stage.p, sp.hs.data(), HALO + (size_t)nt * QV_TILE, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemcpyAsync(d.desc.p, sp.hd.data(), (size_t)nt * 4, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemsetAsync(d.stats.p, 0, n_rel * 16, cx->stream));
            run_scan(cx, yak_idx, {d.stage.p + HALO, -(int64_t)HALO, (int64_t)nt * QV_TILE, d.desc.p, nt}, min_count, d, hist != nullptr,
                     absent_bits != nullptr, timer);
            HIPCHK(hipMemcpyAsync(hst.data(), d.stats.p, n_rel * 16, hipMemcpyDeviceToHost, cx->stream));
            if (absent_bits) HIPCHK(hipMemcpyAsync(hb.data(), d.bits.p, (size_t)nt * QV_TILE_BITS, hipMemcpyDeviceToHost, cx->stream));
            HIPCHK(hipStreamSynchronize(cx->stream)); // (the staging buffers are filled again for the next piece)
            timer.collect();
            for (uint64_t r = 0; r < n_rel; ++r) {
                out[spans[r].seq].n_kmers += hst[2 * r];
                out[spans[r].seq].n_absent += hst[2 * r + 1];
            }
            if (absent_bits)
                for (const auto &s : spans) memcpy(absent_bits + s.bit_at, hb.data() + (size_t)s.tile0 * QV_TILE_BITS, s.bit_bytes);
        }
        if (hist) {
            HIPCHK(hipMemcpyAsync(hist, d.hist.p, QV_HIST_BINS * 8, hipMemcpyDeviceToHost, cx->stream));
            HIPCHK(hipStreamSynchronize(cx->stream));
        }
        if (kernel_ms) *kernel_ms = timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_qv_device(np2_ctx_t *cx, int yak_idx, const uint8_t *dev_seq, uint64_t len, uint16_t min_count, np2_qv_t *out,
                  uint64_t *hist, uint8_t *absent_bits, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        check_table(cx, yak_idx, "np2_qv_device", "yak_idx");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_qv_device: out is NULL");
        if (len && !dev_seq) throw Np2Error(NP2_E_ARG, "np2_qv_device: dev_seq is NULL with a non-zero length");
        if (tiles_of(len) >= QV_FIRST) throw Np2Error(NP2_E_ARG, "np2_qv_device: the sequence is too long");
        if (kernel_ms) *kernel_ms = 0.f;
        if (hist) memset(hist, 0, QV_HIST_BINS * sizeof(uint64_t));
        *out = np2_qv_t{0, 0};
        if (len == 0) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        const uint32_t nt = (uint32_t)tiles_of(len);
        QvBufs d;
        d.stats.ensure(2);
        HIPCHK(hipMemsetAsync(d.stats.p, 0, 16, cx->stream));
        if (hist) {
            d.hist.ensure(QV_HIST_BINS);
            HIPCHK(hipMemsetAsync(d.hist.p, 0, QV_HIST_BINS * 8, cx->stream));
        }
        if (absent_bits) d.bits.ensure((size_t)nt * QV_BLOCK);
        KernelTimer timer(kernel_ms != nullptr);
        // any alignment, nothing readable promised around it: the kernel masks its first and last loads
        run_scan(cx, yak_idx, {dev_seq, 0, (int64_t)len, nullptr, nt}, min_count, d, hist != nullptr, absent_bits != nullptr, timer);
        uint64_t st[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(st, d.stats.p, 16, hipMemcpyDeviceToHost, cx->stream));
        if (hist) HIPCHK(hipMemcpyAsync(hist, d.hist.p, QV_HIST_BINS * 8, hipMemcpyDeviceToHost, cx->stream));
        if (absent_bits) HIPCHK(hipMemcpyAsync(absent_bits, d.bits.p, bits_bytes(len), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        timer.collect();
        *out = np2_qv_t{st[0], st[1]};
        if (kernel_ms) *kernel_ms = timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

} // extern "C"
