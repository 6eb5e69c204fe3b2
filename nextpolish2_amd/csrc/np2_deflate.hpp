// BGZF output on the device (np2_deflate.hip) and the writer built on it (np2_deflate_host.cpp): the mirror of
// np2_inflate.hpp.  Host bytes are cut into blocks of at most 65280 bytes, a wavefront deflates each into a 65536-byte slot
// as a complete BGZF block (k_bgzf_deflate; the CRC32 words come from k_bgzf_crc32 over the input pieces), a scan of the
// slots' sizes and a copy kernel pack them into one stream, and a batch leaves the device in one copy.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <hip/hip_runtime.h>
#include "np2_inflate.hpp"

namespace np2 {

// tb[b] = {0, b * block_bytes, 0, bytes of piece b}: the pieces of in[0, total) as launch_bgzf_crc32 takes them
void launch_deflate_pieces(hipStream_t s, InfBlock *tb, uint32_t n_blk, uint32_t block_bytes, uint64_t total);
// Piece b of in[0, total) (block_bytes <= 65280 each, the last one shorter) -> a whole BGZF block at slots + 65536 b:
// header with the BC subfield, DEFLATE bytes, crc[b], ISIZE; sizes[b] = its bytes.  tok: 65536 words of scratch per block.
// Nothing is assumed of slots, tok or sizes.
void launch_bgzf_deflate(hipStream_t s, const uint8_t *in, uint64_t total, uint32_t block_bytes, uint32_t n_blk, const uint32_t *crc, uint8_t *slots,
                         uint32_t *tok, uint32_t *sizes);
// offs[b] = sizes[0] + ... + sizes[b - 1], offs[n_blk] = the total (also to *total_host, if given: host-mapped memory);
// then slot b's sizes[b] bytes to packed + offs[b]
void launch_deflate_pack(hipStream_t s, const uint8_t *slots, const uint32_t *sizes, uint32_t n_blk, uint32_t *offs, uint8_t *packed, uint32_t *total_host);

} // namespace np2

namespace np2h {

// A BGZF file written through the device: blocks are cut every 65280 bytes whatever the sizes of the write() calls, a batch
// of blocks (256; NP2_BGZF_TEST_BATCH, read once per writer) is compressed on the writer's stream while the caller fills
// the next.  close() flushes the partial block, appends the 28-byte EOF block and reports a write error as NP2_E_ARG
// "cannot write <path>".  A writer destroyed without close() — abandoned on an error — leaves the file WITHOUT the EOF
// block: readers see a truncated file.
class BgzfWriter {
public:
    BgzfWriter(int device, const char *path);
    ~BgzfWriter();
    BgzfWriter(const BgzfWriter &) = delete;
    BgzfWriter &operator=(const BgzfWriter &) = delete;
    void write(const void *p, size_t n);
    void close();
    uint64_t bytes_in() const;
    uint64_t bytes_out() const;
    float kernel_ms() const; // the deflate kernel alone (HIP events), summed over the batches
    // The device-input door, for bytes that are made on the device: the caller fills the first n bytes of device_in()
    // (batch_bytes() bytes, 16-byte aligned) with work on stream(), then commit_device(n) compresses them as one batch while
    // the next is filled; every batch but the last holds batch_bytes().  sizes_dst (device, may be NULL) receives the size of
    // each of the batch's blocks.  Not to be mixed with write().
    hipStream_t stream() const;
    size_t batch_bytes() const;
    uint8_t *device_in();
    void commit_device(size_t n, uint32_t *sizes_dst);
    float fill_ms() const;   // what ran on stream() between device_in() and commit_device(), summed over the drained batches
private:
    struct Impl;
    std::unique_ptr<Impl> im;
};

// a path the native writers compress: it ends in .gz or .bgz
inline bool bgzf_path(const char *p) {
    const std::string s = p ? p : "";
    auto ends = [&](const char *e) { return s.size() >= strlen(e) && s.compare(s.size() - strlen(e), strlen(e), e) == 0; };
    return ends(".gz") || ends(".bgz");
}

} // namespace np2h
