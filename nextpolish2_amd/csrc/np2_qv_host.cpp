// Host driver of the k-mer QV scan (np2_qv.hip): np2_qv_strings streams host sequences through a staging buffer of fixed
// size, np2_qv_device scans one sequence where a polish left it.  (np2_qv.cpp would share the kernel file's object name.)
#include "np2_ctx.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_qv.hpp"

using namespace np2qv;
using np2kc::HALO;

namespace {

// tiles of the staging buffer (32 MiB of sequence per piece); NP2_QV_TEST_STAGE_TILES: a test's smaller pieces
uint32_t stage_tiles() {
    if (const char *e = getenv("NP2_QV_TEST_STAGE_TILES")) return (uint32_t)std::min<long>(1 << 16, std::max<long>(1, atol(e)));
    return 4096;
}

// the grid: what the device holds at once (the kernel's registers admit 4 wavefronts per SIMD: 4 blocks per CU), blocks
// striding over the tiles
uint32_t qv_blocks(int device) {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    return (uint32_t)std::max(1, cus) * 4u;
}

struct QvBufs { // released after the call's device work has completed: cached blocks (DevCache)
    DevBuf<uint8_t> stage;
    DevBuf<uint32_t> desc, bits;
    DevBuf<uint64_t> stats, hist;
    QvBufs() { stage.cached = desc.cached = bits.cached = stats.cached = hist.cached = true; }
};

void check_table(np2_ctx *cx, int yak_idx, const char *who) {
    if (yak_idx < 0 || (size_t)yak_idx >= cx->yaks.size())
        throw Np2Error(NP2_E_ARG, std::string(who) + ": yak_idx " + std::to_string(yak_idx) + " out of range (the context has " +
                                      std::to_string(cx->yaks.size()) + " tables)");
}

} // namespace

extern "C" {

int np2_qv_strings(np2_ctx_t *cx, int yak_idx, const uint8_t *strs, const uint64_t *off, uint64_t n, uint16_t min_count,
                   np2_qv_t *out, uint64_t *hist, uint8_t *absent_bits, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        check_table(cx, yak_idx, "np2_qv_strings");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_qv_strings: out is NULL");
        if (n && !off) throw Np2Error(NP2_E_ARG, "np2_qv_strings: off is NULL with n > 0");
        for (uint64_t i = 0; i < n; ++i)
            if (off[i + 1] < off[i]) throw Np2Error(NP2_E_ARG, "np2_qv_strings: off is descending at sequence " + std::to_string(i));
        if (n && off[n] > off[0] && !strs) throw Np2Error(NP2_E_ARG, "np2_qv_strings: strs is NULL with a non-zero length");
        if (kernel_ms) *kernel_ms = 0.f;
        if (hist) memset(hist, 0, QV_HIST_BINS * sizeof(uint64_t));
        for (uint64_t i = 0; i < n; ++i) out[i] = np2_qv_t{0, 0};
        if (n == 0 || off[n] == off[0]) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        const YakDev y = cx->yaks[yak_idx].dev();
        // the staging buffers, host and device: what the call needs, up to the fixed piece size
        uint64_t all_tiles = 0;
        for (uint64_t i = 0; i < n; ++i) all_tiles += tiles_of(off[i + 1] - off[i]);
        const uint32_t cap = (uint32_t)std::min<uint64_t>(stage_tiles(), all_tiles), blocks = qv_blocks(cx->device);
        QvBufs d;
        d.stage.ensure(HALO + (size_t)cap * QV_TILE);
        d.desc.ensure(cap);
        d.stats.ensure(2 * (size_t)cap);
        if (absent_bits) d.bits.ensure((size_t)cap * QV_BLOCK);
        if (hist) {
            d.hist.ensure(QV_HIST_BINS);
            HIPCHK(hipMemsetAsync(d.hist.p, 0, QV_HIST_BINS * 8, cx->stream));
        }
        std::vector<uint8_t> hs(HALO + (size_t)cap * QV_TILE), hb(absent_bits ? (size_t)cap * QV_TILE_BITS : 0);
        std::vector<uint32_t> hd(cap);
        std::vector<uint64_t> hst(2 * (size_t)cap);
        KernelTimer timer(kernel_ms != nullptr);

        struct Span { // a sequence's tiles in the piece, from tile0 on: the piece's counters `index in spans` are its own
            uint64_t seq, bit_at, bit_bytes;
            uint32_t tile0;
        };
        std::vector<Span> spans;
        uint64_t i = 0, p = 0, bit_base = 0; // sequence, bytes of it already scanned, its first bitmap byte
        while (i < n) {
            // a piece: whole tiles of consecutive sequences, each starting at a tile boundary; a sequence longer than what
            // is left of the piece goes on in the next one, whose halo then holds the 32 bytes before it
            uint32_t nt = 0;
            spans.clear();
            if (p && p < off[i + 1] - off[i])
                memcpy(hs.data(), strs + off[i] + p - HALO, HALO);
            else
                memset(hs.data(), QV_PAD, HALO);
            while (i < n && nt < cap) {
                const uint64_t len = off[i + 1] - off[i];
                if (p >= len) {
                    bit_base += bits_bytes(len);
                    ++i;
                    p = 0;
                    continue;
                }
                const uint32_t take = (uint32_t)std::min<uint64_t>(tiles_of(len - p), cap - nt);
                const uint64_t bytes = std::min<uint64_t>(len - p, (uint64_t)take * QV_TILE);
                uint8_t *dst = hs.data() + HALO + (size_t)nt * QV_TILE;
                memcpy(dst, strs + off[i] + p, bytes);
                memset(dst + bytes, QV_PAD, (size_t)take * QV_TILE - bytes);
                for (uint32_t x = 0; x < take; ++x) hd[nt + x] = (uint32_t)spans.size() | (p == 0 && x == 0 ? QV_FIRST : 0u);
                spans.push_back({i, bit_base + p / 8, std::min<uint64_t>(bits_bytes(len) - p / 8, (uint64_t)take * QV_TILE_BITS), nt});
                nt += take;
                p += (uint64_t)take * QV_TILE;
            }
            if (nt == 0) break;
            const uint64_t n_rel = spans.size(); // (<= nt: every span has a tile)
            HIPCHK(hipMemcpyAsync(d.stage.p, hs.data(), HALO + (size_t)nt * QV_TILE, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemcpyAsync(d.desc.p, hd.data(), (size_t)nt * 4, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemsetAsync(d.stats.p, 0, n_rel * 16, cx->stream));
            QvScan q{};
            q.src = d.stage.p + HALO;
            q.lo = -(int64_t)HALO;
            q.hi = (int64_t)nt * QV_TILE;
            q.desc = d.desc.p;
            q.n_tiles = nt;
            q.min_count = min_count;
            q.stats = reinterpret_cast<unsigned long long *>(d.stats.p);
            q.hist = hist ? reinterpret_cast<unsigned long long *>(d.hist.p) : nullptr;
            q.bits = absent_bits ? d.bits.p : nullptr;
            timer.start(cx->stream);
            launch_qv_scan(cx->stream, y, q, blocks);
            timer.stop(cx->stream);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hst.data(), d.stats.p, n_rel * 16, hipMemcpyDeviceToHost, cx->stream));
            if (absent_bits) HIPCHK(hipMemcpyAsync(hb.data(), d.bits.p, (size_t)nt * QV_TILE_BITS, hipMemcpyDeviceToHost, cx->stream));
            HIPCHK(hipStreamSynchronize(cx->stream)); // (the staging buffers are filled again for the next piece)
            timer.collect();
            for (uint64_t r = 0; r < n_rel; ++r) {
                out[spans[r].seq].n_kmers += hst[2 * r];
                out[spans[r].seq].n_absent += hst[2 * r + 1];
            }
            if (absent_bits)
                for (const Span &s : spans) memcpy(absent_bits + s.bit_at, hb.data() + (size_t)s.tile0 * QV_TILE_BITS, s.bit_bytes);
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
        check_table(cx, yak_idx, "np2_qv_device");
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
        QvScan q{};
        q.src = dev_seq; // any alignment, nothing readable promised around it: the kernel masks its first and last loads
        q.lo = 0;
        q.hi = (int64_t)len;
        q.desc = nullptr;
        q.n_tiles = nt;
        q.min_count = min_count;
        q.stats = reinterpret_cast<unsigned long long *>(d.stats.p);
        q.hist = hist ? reinterpret_cast<unsigned long long *>(d.hist.p) : nullptr;
        q.bits = absent_bits ? d.bits.p : nullptr;
        timer.start(cx->stream);
        launch_qv_scan(cx->stream, cx->yaks[yak_idx].dev(), q, qv_blocks(cx->device));
        timer.stop(cx->stream);
        HIPCHK(hipGetLastError());
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
