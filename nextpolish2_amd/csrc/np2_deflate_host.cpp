// BGZF output: the batches that drive np2_deflate.hip, the writer handle on top of them (np2_bgzf_writer_*, and through
// np2h::OutFile every native writer whose path ends in .gz or .bgz), the one-call form np2_bgzf_deflate_device, and the
// host twin np2_bgzf_deflate_host, which runs the same core (np2_deflate_core.hpp) on the CPU, 64 lanes in turn, and is the
// statement of what the kernel must produce.
#include "np2_kernel_timer.hpp"
#include "np2_deflate_core.hpp"
#include "np2_deflate.hpp"
#include "np2_kcount.hpp"

#include <zlib.h>

namespace {

using np2h::Np2Error;

constexpr uint32_t BATCH_BLOCKS = 256, BATCH_BLOCKS_MAX = 4096; // (a batch's packed bytes are counted in 32 bits)
const uint8_t EOF_BLOCK[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

uint32_t checked_block_bytes(uint32_t block_bytes, const char *who) {
    if (block_bytes > np2def::MAX_BLOCK) throw Np2Error(NP2_E_ARG, std::string(who) + ": block_bytes is at most 65280");
    return block_bytes ? block_bytes : np2def::MAX_BLOCK;
}
// One batch of blocks: pinned input and output, and what the kernels need on the device.
struct DeflateBatch {
    uint32_t cap_blocks = 0;
    np2h::PinnedBuf pin_in, pin_out, pin_total;
    np2h::DevBuf<uint8_t> d_in, d_slots, d_packed;
    np2h::DevBuf<uint32_t> d_tok, d_sizes, d_offs, d_crc;
    np2h::DevBuf<np2::InfBlock> d_tb;
    np2h::DevEvent e0, e1, f0, f1, done;
    uint32_t n_blk = 0;
    bool pending = false, device_filled = false;
    void size(uint32_t blocks) {
        cap_blocks = blocks;
        pin_in.ensure((size_t)blocks * np2def::MAX_BLOCK);
        pin_out.ensure((size_t)blocks * np2def::SLOT_BYTES);
        pin_total.ensure(64);
        d_in.ensure((size_t)blocks * np2def::MAX_BLOCK + 64);
        d_slots.ensure((size_t)blocks * np2def::SLOT_BYTES);
        d_packed.ensure((size_t)blocks * np2def::SLOT_BYTES);
        d_tok.ensure((size_t)blocks * np2def::TOK_WORDS);
        d_sizes.ensure(blocks + 1), d_offs.ensure(blocks + 2), d_crc.ensure(blocks + 1), d_tb.ensure(blocks + 1);
        e0.make(), e1.make(), f0.make(), f1.make(), done.make();
    }
    uint8_t *in() { return (uint8_t *)pin_in.p; }
    const uint8_t *out() const { return (const uint8_t *)pin_out.p; }
    // the first n bytes of in(), in blocks of bb: upload, CRCs, deflate, pack; nothing is waited for.  from_device: the
    // bytes are in d_in already, written on s between f0 and f1.  sizes_dst: the blocks' sizes are copied there, on the device.
    void submit(hipStream_t s, size_t n, uint32_t bb, bool from_device = false, uint32_t *sizes_dst = nullptr) {
        n_blk = (uint32_t)((n + bb - 1) / bb);
        if (!n_blk || n_blk > cap_blocks) throw Np2Error(NP2_E_ARG, "BGZF batch out of range");
        device_filled = from_device;
        if (!from_device) HIPCHK(hipMemcpyAsync(d_in.p, pin_in.p, n, hipMemcpyHostToDevice, s));
        np2::launch_deflate_pieces(s, d_tb.p, n_blk, bb, n);
        np2::launch_bgzf_crc32(s, d_tb.p, n_blk, nullptr, d_in.p, nullptr, nullptr, d_crc.p);
        HIPCHK(hipEventRecord(e0.e, s));
        np2::launch_bgzf_deflate(s, d_in.p, n, bb, n_blk, d_crc.p, d_slots.p, d_tok.p, d_sizes.p);
        HIPCHK(hipEventRecord(e1.e, s));
        if (sizes_dst) HIPCHK(hipMemcpyAsync(sizes_dst, d_sizes.p, (size_t)n_blk * 4, hipMemcpyDeviceToDevice, s));
        np2::launch_deflate_pack(s, d_slots.p, d_sizes.p, n_blk, d_offs.p, d_packed.p, nullptr);
        HIPCHK(hipMemcpyAsync(pin_total.p, d_offs.p + n_blk, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(done.e, s));
        pending = true;
    }
    // the batch's packed bytes in out(): waits for its kernels, then for the one copy; returns their number
    size_t finish(hipStream_t s, float &kernel_ms, float *fill_ms = nullptr) {
        HIPCHK(hipEventSynchronize(done.e));
        pending = false;
        const size_t total = *(const uint32_t *)pin_total.p;
        if (total < (size_t)n_blk * (np2def::HDR_BYTES + 2 + np2def::TRL_BYTES) || total > (size_t)n_blk * np2def::SLOT_BYTES)
            throw Np2Error(NP2_E_DEVICE, "BGZF deflate: the packed size is out of range");
        HIPCHK(hipMemcpyAsync(pin_out.p, d_packed.p, total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        kernel_ms += np2h::elapsed(e0, e1);
        if (device_filled && fill_ms) *fill_ms += np2h::elapsed(f0, f1);
        return total;
    }
};

uint32_t batch_blocks() { return (uint32_t)np2h::test_hook("NP2_BGZF_TEST_BATCH", 1, BATCH_BLOCKS_MAX, BATCH_BLOCKS); }

} // namespace

namespace np2h {

struct BgzfWriter::Impl {
    int device = 0;
    std::string path;
    FILE *f = nullptr;
    hipStream_t s = nullptr;
    DeflateBatch b[2];
    int cur = 0;
    size_t fill = 0, cap = 0;
    uint64_t n_in = 0, n_out = 0;
    float ms = 0.f, fill_ms = 0.f;
    bool failed = false; // a write or a batch failed: the file never gets its EOF block
    ~Impl() {
        (void)hipSetDevice(device);
        // (abandoned: whatever is in flight ends before the buffers go; the file stays without its EOF block)
        if (s) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
        if (f) fclose(f);
    }
    void put(const void *p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) throw Np2Error(NP2_E_ARG, "cannot write " + path);
        n_out += n;
    }
    void drain(int k) { // batch k's bytes to the file
        if (!b[k].pending) return;
        const size_t n = b[k].finish(s, ms, &fill_ms);
        put(b[k].out(), n);
    }
    void flush() { // the bytes gathered so far become a batch; the other one, compressed meanwhile, goes to the file first
        drain(cur ^ 1);
        if (fill) b[cur].submit(s, fill, np2def::MAX_BLOCK);
        cur ^= 1, fill = 0;
    }
};

BgzfWriter::BgzfWriter(int device, const char *path) : im(new Impl()) {
    if (!path) throw Np2Error(NP2_E_ARG, "np2_bgzf_writer_open: NULL path");
    im->device = device, im->path = path;
    im->f = fopen(path, "wb");
    if (!im->f) throw Np2Error(NP2_E_ARG, "cannot open " + im->path + " for writing");
    setvbuf(im->f, nullptr, _IOFBF, 1 << 20);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&im->s, hipStreamNonBlocking));
    const uint32_t blocks = batch_blocks();
    im->b[0].size(blocks), im->b[1].size(blocks);
    im->cap = (size_t)blocks * np2def::MAX_BLOCK;
}
BgzfWriter::~BgzfWriter() = default;
void BgzfWriter::write(const void *p, size_t n) {
    if (!im->f) throw Np2Error(NP2_E_ARG, "write to a closed BGZF writer");
    if (!n) return;
    HIPCHK(hipSetDevice(im->device));
    const uint8_t *q = (const uint8_t *)p;
    im->n_in += n;
    try {
        if (im->failed) throw Np2Error(NP2_E_ARG, "cannot write " + im->path);
        while (n) {
            const size_t take = std::min(n, im->cap - im->fill);
            memcpy(im->b[im->cur].in() + im->fill, q, take);
            im->fill += take, q += take, n -= take;
            if (im->fill == im->cap) im->flush();
        }
    } catch (...) {
        im->failed = true;
        throw;
    }
}
void BgzfWriter::close() {
    if (!im->f) return;
    FILE *g = im->f;
    try {
        if (im->failed) throw Np2Error(NP2_E_ARG, "cannot write " + im->path);
        HIPCHK(hipSetDevice(im->device));
        im->flush();          // (the partial batch, its last block partial)
        im->drain(im->cur ^ 1);
        im->put(EOF_BLOCK, sizeof(EOF_BLOCK));
    } catch (...) {
        im->failed = true, im->f = nullptr;
        fclose(g);
        throw;
    }
    im->f = nullptr;
    if (fclose(g) != 0) throw Np2Error(NP2_E_ARG, "cannot write " + im->path);
}
hipStream_t BgzfWriter::stream() const { return im->s; }
size_t BgzfWriter::batch_bytes() const { return im->cap; }
uint8_t *BgzfWriter::device_in() {
    if (!im->f || im->failed) throw Np2Error(NP2_E_ARG, "cannot write " + im->path);
    if (im->fill) throw Np2Error(NP2_E_ARG, "BGZF writer: device input after a partial host batch");
    HIPCHK(hipSetDevice(im->device));
    HIPCHK(hipEventRecord(im->b[im->cur].f0.e, im->s));
    return im->b[im->cur].d_in.p;
}
void BgzfWriter::commit_device(size_t n, uint32_t *sizes_dst) {
    if (!n || n > im->cap) throw Np2Error(NP2_E_ARG, "BGZF batch out of range");
    try {
        HIPCHK(hipEventRecord(im->b[im->cur].f1.e, im->s));
        im->n_in += n;
        im->drain(im->cur ^ 1);
        im->b[im->cur].submit(im->s, n, np2def::MAX_BLOCK, true, sizes_dst);
        im->cur ^= 1;
    } catch (...) {
        im->failed = true;
        throw;
    }
}
float BgzfWriter::fill_ms() const { return im->fill_ms; }
uint64_t BgzfWriter::bytes_in() const { return im->n_in; }
uint64_t BgzfWriter::bytes_out() const { return im->n_out; }
float BgzfWriter::kernel_ms() const { return im->ms; }

} // namespace np2h

struct np2_bgzf_writer {
    np2h::BgzfWriter w;
    np2_bgzf_writer(int device, const char *path) : w(device, path) {}
};

extern "C" {

int np2_bgzf_deflate_host(const uint8_t *data, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    return np2h::abi_guard([&] {
        if ((!data && n) || !out_len || (!out && out_cap)) throw Np2Error(NP2_E_ARG, "np2_bgzf_deflate_host: NULL argument");
        const uint32_t bb = checked_block_bytes(block_bytes, "np2_bgzf_deflate_host");
        std::vector<uint32_t> slot(np2def::SLOT_BYTES / 4), tok(np2def::TOK_WORDS);
        std::unique_ptr<np2def::Shared> S(new np2def::Shared);
        np2def::HostMachine m;
        uint64_t at = 0;
        auto put = [&](const uint8_t *p, size_t k) {
            if (at + k <= out_cap) memcpy(out + at, p, k);
            at += k;
        };
        for (uint64_t off = 0; off < n; off += bb) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(bb, n - off);
            const uint32_t k = np2def::deflate_block(m, *S, data + off, len, slot.data(), np2def::HDR_BYTES * 8u, tok.data());
            uint8_t *b = (uint8_t *)slot.data();
            const uint32_t bsize = np2def::HDR_BYTES + k + np2def::TRL_BYTES;
            memcpy(b, EOF_BLOCK, 16);
            b[16] = (uint8_t)((bsize - 1) & 255u), b[17] = (uint8_t)((bsize - 1) >> 8);
            const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), data + off, len);
            for (uint32_t i = 0; i < 4; ++i) b[18 + k + i] = (uint8_t)(crc >> (8 * i)), b[22 + k + i] = (uint8_t)(len >> (8 * i));
            put(b, bsize);
        }
        put(EOF_BLOCK, sizeof(EOF_BLOCK));
        *out_len = at;
        if (at > out_cap)
            throw Np2Error(NP2_E_ARG, "np2_bgzf_deflate_host: the output buffer holds " + std::to_string(out_cap) + " bytes, the stream needs " + std::to_string(at));
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_bgzf_deflate_device(np2_ctx_t *cx, const uint8_t *data, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                            float *kernel_ms) {
    if (!cx) return np2h::io_set_error(NP2_E_ARG, "np2_bgzf_deflate_device: NULL context");
    return np2h::abi_guard([&] {
        if ((!data && n) || !out_len || (!out && out_cap)) throw Np2Error(NP2_E_ARG, "np2_bgzf_deflate_device: NULL argument");
        const uint32_t bb = checked_block_bytes(block_bytes, "np2_bgzf_deflate_device");
        uint64_t at = 0;
        float ms = 0.f;
        if (n) {
            HIPCHK(hipSetDevice(cx->device));
            const uint64_t blocks = (n + bb - 1) / bb;
            DeflateBatch b;
            b.size((uint32_t)std::min<uint64_t>(blocks, BATCH_BLOCKS));
            for (uint64_t off = 0; off < n;) {
                const size_t take = (size_t)std::min<uint64_t>(n - off, (uint64_t)b.cap_blocks * bb);
                memcpy(b.in(), data + off, take);
                b.submit(cx->stream, take, bb);
                const size_t k = b.finish(cx->stream, ms);
                if (at + k <= out_cap) memcpy(out + at, b.out(), k);
                at += k, off += take;
            }
        }
        if (at + sizeof(EOF_BLOCK) <= out_cap) memcpy(out + at, EOF_BLOCK, sizeof(EOF_BLOCK));
        at += sizeof(EOF_BLOCK);
        *out_len = at;
        if (kernel_ms) *kernel_ms = ms;
        if (at > out_cap)
            throw Np2Error(NP2_E_ARG, "np2_bgzf_deflate_device: the output buffer holds " + std::to_string(out_cap) + " bytes, the stream needs " + std::to_string(at));
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        (void)hipStreamSynchronize(cx->stream);
        np2h::io_set_error(code, msg);
    });
}

int np2_bgzf_writer_open(int device, const char *path, np2_bgzf_writer_t **out) {
    if (!out) return np2h::io_set_error(NP2_E_ARG, "np2_bgzf_writer_open: NULL argument");
    *out = nullptr;
    return np2h::abi_guard([&] {
        *out = new np2_bgzf_writer(device, path);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_bgzf_writer_write(np2_bgzf_writer_t *w, const void *p, uint64_t n) {
    if (!w || (!p && n)) return np2h::io_set_error(NP2_E_ARG, "np2_bgzf_writer_write: NULL argument");
    return np2h::abi_guard([&] {
        w->w.write(p, (size_t)n);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_bgzf_writer_close(np2_bgzf_writer_t *w, uint64_t *bytes_in, uint64_t *bytes_out, float *kernel_ms) {
    if (!w) return NP2_OK;
    std::unique_ptr<np2_bgzf_writer> own(w); // (released on every way out; after an error the file has no EOF block)
    return np2h::abi_guard([&] {
        w->w.close();
        if (bytes_in) *bytes_in = w->w.bytes_in();
        if (bytes_out) *bytes_out = w->w.bytes_out();
        if (kernel_ms) *kernel_ms = w->w.kernel_ms();
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"
