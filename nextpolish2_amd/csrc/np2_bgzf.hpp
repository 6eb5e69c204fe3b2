// The BGZF block header, parsed in one place for every reader of a BAM (np2_bamfile.hpp, np2_fetch_gpu.cpp): the FILE* stream that reads a BAM's header,
// the mmap reader of the host pool and the pinned pieces of the device path.  Host-only: no HIP here, so that a plain C++
// compiler builds it (tests/tools/bgzf_test.cpp, under the address and undefined-behaviour sanitizers).
#pragma once
#include "np2_abi.hpp"

#include <cstddef>
#include <cstdint>

namespace np2h {

inline uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

struct BgzfBlock { // a BGZF block of a file
    uint64_t file_off; // of the block
    uint64_t out_off;  // of its first inflated byte, in the stream of the blocks read with it
    uint32_t hdr_len;  // 12 + XLEN: the raw DEFLATE payload starts there
    uint32_t clen, isize;
    uint32_t bsize;    // the whole block
    uint32_t crc;      // its CRC32 word (of the inflated bytes)
};
struct BgzfHeader {
    uint32_t need; // != 0: nothing parsed, come back with this many bytes (18, then 12 + XLEN)
    uint32_t hdr_len, bsize, clen;
};
// The header of the block at p.  avail: the bytes the caller holds at p; left: the bytes from p to the end of the file (or
// of the data), avail <= left.  Whether the block belongs to what the caller reads is the caller's business.
inline BgzfHeader bgzf_header(const uint8_t *p, size_t avail, uint64_t left) {
    if (left >= 18 && avail < 18) return {18, 0, 0, 0};
    if (left < 18 || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) throw Np2Error(NP2_E_ARG, "not a BGZF block");
    const uint32_t xlen = p[10] | (p[11] << 8);
    if (left < 12 + (uint64_t)xlen) throw Np2Error(NP2_E_ARG, "truncated BGZF header");
    if (avail < 12 + (size_t)xlen) return {12 + xlen, 0, 0, 0};
    const uint8_t *extra = p + 12;
    uint32_t bsize = 0; // (the BC subfield is normally the first and only one)
    for (size_t q = 0; q + 4 <= xlen;) {
        const uint32_t slen = extra[q + 2] | (extra[q + 3] << 8);
        if (extra[q] == 'B' && extra[q + 1] == 'C' && slen == 2 && q + 6 <= xlen) bsize = (extra[q + 4] | (extra[q + 5] << 8)) + 1;
        q += 4 + slen;
    }
    if (!bsize) throw Np2Error(NP2_E_ARG, "BGZF block without BC field");
    if (bsize < 12 + xlen + 8 || left < bsize) throw Np2Error(NP2_E_ARG, "truncated BGZF block");
    return {0, 12 + xlen, bsize, bsize - 12 - xlen - 8};
}
struct BgzfTrailer { // the 8 bytes behind a block's payload
    uint32_t crc, isize;
};
inline BgzfTrailer bgzf_trailer(const uint8_t *p) { return {le32(p), le32(p + 4)}; }

} // namespace np2h
