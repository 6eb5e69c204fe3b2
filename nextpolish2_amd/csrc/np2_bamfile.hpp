// The indexed BAM on the host (np2_bamfile.cpp): the BGZF readers, the staging of bytes on their way to the device, the handle
// np2_bam_open makes and the host pool's record reader.
#pragma once
#include "../../include/np2_io.h"
#include "np2_bgzf.hpp"
#include "np2_ctx.hpp"
#include "np2_iopool.hpp"

#include <atomic>
#include <functional>
#include <memory>
#include <sched.h>
#include <unordered_map>

namespace np2h {

struct GpuFetch;    // np2_fetch_gpu.cpp
struct ResidentBam; // np2_fetch_gpu.cpp

// NP2_BGZF_CRC=0 (read once per process) switches the CRC-32 check of inflated blocks off on every path, host and device
bool bgzf_crc_on();
std::string crc_msg(uint64_t file_off);
const char *inflater_name(); // the host's raw-deflate decoder: "libdeflate" or "zlib"
int io_set_error(int code, const std::string &msg); // the entry points' message slot (np2_io.cpp); returns `code`

// The BGZF stream a BAM's header is read from, block by block
struct Bgzf {
    FILE *f = nullptr;
    std::vector<uint8_t> block, cdata;
    size_t bpos = 0;
    uint64_t block_off = 0, flen = 0; // file offset of the current block; length of the file
    // virtual offset of the next byte to be read
    uint64_t tell() {
        if (bpos >= block.size()) return (uint64_t)ftello(f) << 16;
        return (block_off << 16) | bpos;
    }
    bool read_block(); // returns false at EOF
    // read exactly n bytes; returns false on clean EOF before the first byte
    bool read(void *dst, size_t n) {
        uint8_t *d = (uint8_t *)dst;
        size_t got = 0;
        while (got < n) {
            if (bpos >= block.size()) {
                if (!read_block()) {
                    if (got == 0) return false;
                    throw np2h::Np2Error(NP2_E_ARG, "truncated BAM");
                }
                continue;
            }
            const size_t k = std::min(n - got, block.size() - bpos);
            memcpy(d + got, block.data() + bpos, k);
            got += k;
            bpos += k;
        }
        return true;
    }
};

// Reads BGZF blocks in batches and inflates each batch with several host threads (blocks are independent).
struct BgzfBatch {
    // the file mapped read-only: a block's deflate payload is inflated straight out of the page cache (reading 35 MB of
    // blocks with two freads each was 9 of the 19 ms the records of an E. coli-sized contig took to arrive); the pages
    // are first touched by the inflating threads, in parallel
    const uint8_t *map = nullptr;
    size_t map_len = 0, fpos = 0;
    // (buffer position of a block's first inflated byte, file offset of the block) for the blocks in `buf`: a record's
    // BGZF virtual offset = file offset << 16 | offset inside the block
    // (the front block may begin before the buffer once consumed bytes were dropped: signed positions)
    std::vector<std::pair<int64_t, uint64_t>> blk_index;
    uint64_t voffset_at(size_t p) const {
        size_t lo = 0, hi = blk_index.size();
        while (hi - lo > 1) {
            const size_t mid = (lo + hi) / 2;
            if (blk_index[mid].first <= (int64_t)p) lo = mid; else hi = mid;
        }
        return (blk_index[lo].second << 16) | (uint64_t)((int64_t)p - blk_index[lo].first);
    }
    RawBuf buf; // inflated bytes not yet consumed (+ the current batch)
    size_t pos = 0, skip = 0; // (skip: offset inside the first block after a seek, applied by the first fill)
    // A HINT for where the wanted records end in the file (the index's last chunk end of the reference): a refill reads
    // blocks up to it instead of a full batch — a 0.75 Mb contig's records are 250 blocks, a batch 2048 —, and once past
    // it only a few at a time (8, 16, ...: an index that understates the end costs time, never records).
    size_t hint_fpos = SIZE_MAX, past_hint = 8;
    // the batch being inflated: its blocks, a completion flag per block, the prefix of `buf` known to be inflated
    std::vector<BgzfBlock> cur_blks; // (out_off: from cur_base on)
    std::unique_ptr<std::atomic<uint8_t>[]> blk_done;
    size_t blk_done_cap = 0, cur_base = 0, ready_bi = 0, ready_end = 0;
    bool eof = false;
    double ms_read = 0, ms_inflate = 0, ms_drop = 0; // where the refills' time goes (NP2_IO_PROFILE)
    double ms_walk = 0, ms_size = 0, ms_copy = 0;   // ... and the record pass over each refill
    size_t batch_blocks = 2048; // 64 KiB blocks per refill: 128 MiB of inflated BAM, all inflated in parallel
    bool read_raw(BgzfBlock &b) { // (its payload: map + file_off + hdr_len)
        if (fpos >= map_len) return false;
        const np2h::BgzfHeader h = np2h::bgzf_header(map + fpos, map_len - fpos, map_len - fpos);
        const np2h::BgzfTrailer t = np2h::bgzf_trailer(map + fpos + h.hdr_len + h.clen);
        b = BgzfBlock{fpos, 0, h.hdr_len, h.clen, t.isize, h.bsize, t.crc};
        fpos += h.bsize;
        return true;
    }
    // start at a virtual offset
    void seek(uint64_t voffset, bool prefill = true) {
        fpos = (size_t)(voffset >> 16);
        buf.clear();
        blk_index.clear();
        pos = 0;
        eof = false;
        skip = voffset & 0xFFFF;
        hint_fpos = SIZE_MAX, past_hint = 8;
        if (prefill) fill(8);
    }
    // Bytes [0, end) of `buf` inflated?  Blocks until they are while a fill is in flight (called from the fill's `during`
    // on the filling thread: blocks are handed to the pool in buffer order, so waiting for them in order cannot starve);
    // false when `end` lies beyond what the buffer will hold.
    bool wait_ready(size_t end) {
        if (end > buf.size()) return false;
        while (ready_end < end) {
            if (ready_bi >= cur_blks.size()) {
                ready_end = buf.size();
                break;
            }
            for (unsigned spin = 0; !blk_done[ready_bi].load(std::memory_order_acquire); ++spin)
                if (spin > 64) sched_yield();
            ready_end = cur_base + cur_blks[ready_bi].out_off + cur_blks[ready_bi].isize;
            ++ready_bi;
        }
        return true;
    }
    // Appends up to n_blocks inflated blocks to `buf`.  `during` (optional) runs on this thread while the pool inflates:
    // it may read the buffer through wait_ready() as the blocks complete.
    void fill(size_t n_blocks, const std::function<void()> *during = nullptr);
    // pointer to n contiguous bytes (nullptr on clean EOF before the first byte)
    const uint8_t *take(size_t n) {
        while (buf.size() - pos < n) {
            if (eof) {
                if (buf.size() == pos) return nullptr;
                throw np2h::Np2Error(NP2_E_ARG, "truncated BAM");
            }
            fill(batch_blocks);
        }
        const uint8_t *p = buf.data() + pos;
        pos += n;
        return p;
    }
};

// File bytes [off, off + n) -> dst; false: the file ends before them.
bool pread_full(int fd, uint8_t *dst, size_t n, uint64_t off);
// n bytes -> dst (device) through two alternating pinned pieces of piece_bytes each (ev: their events).  fill(stage, offset,
// bytes) -> bool writes bytes [offset, offset + bytes) of the n to `stage`, 1 MiB a call on `threads` of the host pool (the page
// cache is copied from at ~10 GB/s per thread, the bus takes 50); after_piece(stage, o0, o1) looks at a whole piece, bytes
// [o0, o1), once its copy is under way.  false: a fill came up short.
template <class Fill, class After>
bool staged_upload(void *const *pin, const hipEvent_t *ev, size_t piece_bytes, unsigned threads, size_t n, uint8_t *dst, hipStream_t s, Fill fill, After after_piece) {
    size_t piece = 0;
    for (size_t o = 0; o < n; o += piece_bytes, ++piece) {
        const int sl = (int)(piece & 1);
        if (piece >= 2) HIPCHK(hipEventSynchronize(ev[sl])); // the copy that last used this staging piece
        const size_t want = std::min(piece_bytes, n - o);
        uint8_t *stage = (uint8_t *)pin[sl];
        const size_t SUB = (size_t)1 << 20;
        std::atomic<int> bad{0};
        IoPool::get().parallel_for((want + SUB - 1) / SUB, threads, [&](size_t k) {
            if (!fill(stage + k * SUB, o + k * SUB, std::min(SUB, want - k * SUB))) bad.store(1);
        });
        if (bad.load()) return false;
        HIPCHK(hipMemcpyAsync(dst + o, stage, want, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev[sl], s));
        after_piece(stage, o, o + want);
    }
    return true;
}
inline void no_look(const uint8_t *, size_t, size_t) {}

// reference bases a CIGAR of n operations covers (M, D, N, =, X); given as words or as a record's little-endian bytes
inline uint32_t cigar_word(const uint32_t *cigar, uint32_t k) { return cigar[k]; }
inline uint32_t cigar_word(const uint8_t *cigar, uint32_t k) { return le32(cigar + 4 * k); }
template <class T>
uint64_t ref_span(const T *cigar, uint32_t n) {
    uint64_t span = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t w = cigar_word(cigar, k), op = w & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += w >> 4;
    }
    return span;
}

// std::vector storage in pinned host memory: the SEQ bytes gathered from the BAM go to the GPU by DMA straight from
// here (a pageable source is staged through bounce buffers at a fraction of the bus rate)
// growable byte buffer in pinned host memory WITHOUT value-initialisation (std::vector::resize zero-fills what the
// record copies overwrite a moment later: 69 MB of SEQ per E. coli-sized contig)
struct PinnedBytes {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    PinnedBytes() = default;
    PinnedBytes(const PinnedBytes &) = delete;
    PinnedBytes &operator=(const PinnedBytes &) = delete;
    ~PinnedBytes() {
        if (p) np2h::pinned_pool().put(p);
    }
    size_t size() const { return n; }
    uint8_t *data() { return p; }
    void clear() { n = 0; }
    void reserve(size_t m) {
        if (m <= cap) return;
        const size_t want = std::max(m, cap + cap / 2 + (1u << 20));
        void *q = np2h::pinned_pool().get(want); // (blocks of the process-wide pool: pinning 69 MB costs 50 ms)
        if (!q) throw std::bad_alloc();
        if (n) memcpy(q, p, n);
        if (p) np2h::pinned_pool().put(p);
        p = (uint8_t *)q;
        cap = want;
    }
    void resize(size_t m) { // (new bytes are NOT initialised)
        reserve(m);
        n = m;
    }
    void resize(size_t m, uint8_t fill) {
        const size_t old = n;
        resize(m);
        if (m > old) memset(p + old, fill, m - old);
    }
    void append(const uint8_t *src, size_t k) {
        reserve(n + k);
        memcpy(p + n, src, k);
        n += k;
    }
    uint8_t &operator[](size_t i) { return p[i]; }
};

// a block of the pinned pool of at least `bytes` bytes at p (kept while it is large enough; a new one: a quarter more + slack)
inline void *pinned_block(void *&p, size_t &cap, size_t bytes, size_t slack) {
    if (cap < bytes) {
        if (p) pinned_pool().put(p);
        p = nullptr, cap = 0;
        const size_t want = bytes + bytes / 4 + slack;
        p = pinned_pool().get(want);
        if (!p) throw Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
        cap = want;
    }
    return p;
}
struct SecSeq { // SEQ of a primary alignment in read orientation (4-bit BAM codes, high nibble first)
    std::vector<uint8_t> seq4;
    uint32_t len = 0;
};
// The SEQ bytes of a contig's records on their way to the device: batch by batch (one refill of the inflater: <= 128 MiB
// of BAM, ~40 MB of SEQ) through two alternating pinned pieces, each uploaded as soon as its records are copied.  The
// whole contig's SEQ as ONE pinned array (round 3) is 3.7 GB for a 248 Mb chromosome at 30x: page-locking that much takes
// ~1 s per 4 GB, grown by reallocation it was 1.5 - 5 s — and the driver serialises it with every other allocation of
// the process (the k-mer tables' hipMalloc waited 4.8 s behind it: tools/alloc_probe.py, profiles/r04_e2e_chr1_*).
struct SeqStream {
    hipStream_t s = nullptr;
    np2h::DevBuf<uint8_t> dev; // the contig's SEQ bytes, contiguous (capacity kept from contig to contig)
    uint64_t n = 0;            // bytes uploaded
    void *pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int turn = 0;
    SeqStream() { dev.cached = true; }
    ~SeqStream() {
        if (s) (void)hipStreamSynchronize(s); // (the device block goes back to the cache: nothing of ours may be in flight)
        for (int i = 0; i < 2; ++i) {
            if (pin[i]) np2h::pinned_pool().put(pin[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
    void begin(hipStream_t stream, uint64_t expect_bytes) {
        s = stream;
        n = 0;
        if (dev.cap < expect_bytes + 64) {
            HIPCHK(hipStreamSynchronize(s));
            dev.ensure(expect_bytes + 64);
        }
    }
    uint8_t *piece(size_t bytes) { // staging for the next batch
        const int i = turn;
        if (busy[i]) {
            HIPCHK(hipEventSynchronize(ev[i]));
            busy[i] = false;
        }
        pinned_block(pin[i], pin_cap[i], bytes, (size_t)1 << 20);
        if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        return (uint8_t *)pin[i];
    }
    void push(size_t bytes) { // the piece handed out last holds `bytes` bytes that follow the n uploaded so far
        if (dev.cap < n + bytes + 64) { // the estimate fell short: a larger block, what is there copied over on the device
            np2h::DevBuf<uint8_t> bigger;
            bigger.cached = true;
            bigger.ensure((n + bytes) * 3 / 2 + 64);
            if (n) HIPCHK(hipMemcpyAsync(bigger.p, dev.p, n, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            std::swap(bigger.p, dev.p);
            std::swap(bigger.cap, dev.cap);
            std::swap(bigger.cache_bytes, dev.cache_bytes);
            std::swap(bigger.slab_bytes, dev.slab_bytes);
        }
        const int i = turn;
        if (bytes) {
            HIPCHK(hipMemcpyAsync(dev.p + n, pin[i], bytes, hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(ev[i], s));
            busy[i] = true;
        }
        n += bytes;
        turn ^= 1;
    }
    void finish() { // 16 readable zero bytes behind the last record's SEQ (the columnariser loads whole words)
        if (dev.cap < n + 64) push(0);
        HIPCHK(hipMemsetAsync(dev.p + n, 0, 16, s));
        n += 16;
    }
};

} // namespace np2h

struct np2_bam {
    np2h::Bgzf z;
    std::vector<std::string> ref_names;
    std::vector<uint32_t> ref_lens;
    std::vector<uint64_t> ref_start; // virtual offset of the first record of each reference (~0 = none)
    std::vector<uint64_t> ref_end;   // ... and of the end of its last record, as far as the index's chunks say (0 = unknown)
    std::vector<std::vector<uint64_t>> lin; // .bai linear index per reference: smallest virtual offset of a record
                                            // overlapping each 16 kb window (0 = none)
    uint64_t first_rec = 0;          // virtual offset of the first alignment record
    // -S: secondary alignments carry no SEQ; recovered from the primary record of the same read (secondary.rs:82-148)
    bool sec_loaded = false;
    std::unordered_map<std::string, np2h::SecSeq> sec;
    np2h::PinnedBytes seq4; // SEQ staging of the contig being read (-S, and callers without a context; capacity kept across contigs)
    np2h::SeqStream seqs;   // ... streamed to the device batch by batch (the usual path)
    np2h::BgzfBatch batch;  // batch inflater (its buffer is reused from contig to contig)
    std::unique_ptr<np2h::GpuFetch> gpu; // read extraction on the device (NP2_INFLATE=gpu / auto: fetch_records_gpu); made on first use
    std::shared_ptr<np2h::ResidentBam> resident; // ... from the WHOLE file inflated on the device once (a many-reference BAM of moderate size)
    bool resident_tried = false;
    np2_bam(); // (both in np2_fetch_gpu.cpp, which knows GpuFetch)
    ~np2_bam();
    const uint8_t *map = nullptr; // the whole file, mapped read-only (BgzfBatch inflates out of it)
    size_t map_len = 0;
};

namespace np2h {
// index of the reference called `name` in the BAM's header (the last one of that name)
int ref_id(const np2_bam *bam, const char *name);
// Where the records of a zone begin: at the reference's first record, or — zone_lo > 0 — at the smallest offset of a record
// overlapping the 16 kb window of zone_lo in the linear index (an empty window takes the next one's, like htslib).  ~0: no record.
uint64_t zone_start_offset(const np2_bam *bam, int tid, uint32_t zone_lo);
// The records of reference `tid` that overlap [zone_lo, zone_hi) (the whole contig: [0, L)), in file order, as
// np2_bamrec_t + CIGAR words + SEQ bytes (pinned staging of the handle); optionally their BGZF virtual offsets.
// With `up_stream` (and without -S) the SEQ bytes do not stay on the host: they go to bam->seqs.dev batch by batch
// (SeqStream), *seq_bytes is their total, bam->seq4 stays empty.
// (no_seq: the caller reads positions, flags and CIGARs only — the depth report —: no SEQ byte is copied)
void fetch_records(np2_bam *bam, int tid, uint32_t L, uint32_t zone_lo, uint32_t zone_hi, const np2_front_opts_t *opts,
                   std::vector<np2_bamrec_t> &recs, std::vector<uint32_t> &cigar, std::vector<uint64_t> *voffs,
                   hipStream_t up_stream = nullptr, uint64_t *seq_bytes = nullptr, bool no_seq = false);
} // namespace np2h
