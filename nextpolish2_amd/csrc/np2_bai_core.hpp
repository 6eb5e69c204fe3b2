// The .bai of an indexed BAM, from its bytes to what the readers use of it: per reference the virtual offset of its first
// record and of the end of its last one (smallest chunk begin, largest chunk end over the bins other than the metadata
// pseudo-bin 37450) and the linear index.  No HIP type, no file access: np2_bam_open calls it on the bytes it read, and
// tests/tools/bai_core_test.cpp calls it stand-alone under the sanitizers.  Every read is bounded by the buffer's length;
// what does not fit is refused with a message, never read.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace np2h {

struct BaiIndex {
    std::vector<uint64_t> ref_start;        // virtual offset of the first record of each reference (~0 = none)
    std::vector<uint64_t> ref_end;          // ... and of the end of its last record, as far as the chunks say (0 = unknown)
    std::vector<std::vector<uint64_t>> lin; // linear index: smallest virtual offset of a record overlapping each 16 kb window (0 = none)
};

inline uint32_t bai_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t bai_le64(const uint8_t *p) { return (uint64_t)bai_le32(p) | ((uint64_t)bai_le32(p + 4) << 32); }

// n bytes at d -> out, for a BAM of n_ref references.  nullptr: parsed; otherwise why not (out is then not to be used).
// The index may describe fewer references than the header has (the rest count as without records), never more; behind the
// last reference nothing or the 8-byte count of unplaced reads (n_no_coor) may follow.
inline const char *bai_parse(const uint8_t *d, size_t n, uint32_t n_ref, BaiIndex &out) {
    out.ref_start.assign(n_ref, ~0ull);
    out.ref_end.assign(n_ref, 0);
    out.lin.assign(n_ref, {});
    if (n < 8 || memcmp(d, "BAI\1", 4) != 0) return "bad .bai magic";
    size_t p = 4;
    const uint32_t n_ref_i = bai_le32(d + p);
    p += 4;
    if (n_ref_i > n_ref) return "the .bai index names more references than the BAM header";
    for (uint32_t r = 0; r < n_ref_i; ++r) {
        if (n - p < 4) return "truncated .bai";
        const uint32_t n_bin = bai_le32(d + p);
        p += 4;
        uint64_t best = ~0ull, last = 0;
        for (uint32_t bi = 0; bi < n_bin; ++bi) {
            if (n - p < 8) return "truncated .bai";
            const uint32_t bin = bai_le32(d + p), n_chunk = bai_le32(d + p + 4);
            p += 8;
            if (n_chunk > (n - p) / 16) return "truncated .bai";
            if (bin != 37450) // 37450 = metadata pseudo-bin: its two "chunks" are a range and two counts
                for (uint32_t ci = 0; ci < n_chunk; ++ci) {
                    const uint64_t beg = bai_le64(d + p + (size_t)ci * 16), end = bai_le64(d + p + (size_t)ci * 16 + 8);
                    best = std::min(best, beg);
                    last = std::max(last, end);
                }
            p += (size_t)n_chunk * 16;
        }
        if (n - p < 4) return "truncated .bai";
        const uint32_t n_intv = bai_le32(d + p);
        p += 4;
        if (n_intv > (n - p) / 8) return "truncated .bai";
        out.lin[r].resize(n_intv);
        for (uint32_t w = 0; w < n_intv; ++w) out.lin[r][w] = bai_le64(d + p + (size_t)w * 8);
        p += (size_t)n_intv * 8;
        out.ref_start[r] = best;
        out.ref_end[r] = last;
    }
    if (n - p != 0 && n - p != 8) return "bytes behind the last reference of the .bai that are not its 8-byte count of unplaced reads";
    return nullptr;
}

// Where the records of a zone begin: at the reference's first record (`first`), or — zone_lo > 0 — at the smallest offset of
// a record overlapping the 16 kb window of zone_lo in the linear index (an empty window takes the next one's, like htslib).
// ~0: no record.
inline uint64_t bai_zone_start(const std::vector<uint64_t> &lin, uint64_t first, uint32_t zone_lo) {
    if (first == ~0ull || zone_lo == 0 || lin.empty()) return first;
    size_t w = std::min<size_t>(zone_lo >> 14, lin.size() - 1);
    while (w + 1 < lin.size() && lin[w] == 0) ++w;
    return lin[w] != 0 ? lin[w] : first;
}

} // namespace np2h
