// Read extraction on the device: a reference's BGZF blocks inflated there, its records found along the .bai linear index
// (GpuFetch, fetch_records_gpu); the whole file inflated once and kept (ResidentBam); the raw inflate and CRC-32 doors.
#include "np2_fetch_gpu.hpp"
#include "np2_inflate.hpp"
#include "np2_inflate_core.hpp"
#include "np2_kernel_timer.hpp"

#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <mutex>
#include <tuple>

namespace np2h {

// The whole file inflated on the device, once per process and device, for BAMs of many references and moderate size (an
// assembly's: yeast 96 MB -> 600 MB): ONE inflate launch over every block — a block's decode latency, 2 - 3 ms, is paid once
// instead of once per reference, and 10^4 blocks fill the device where a reference's few hundred leave it idle —, after which
// a reference's front end is the record walk over its stretch of the resident stream.  Shared by the handles a process
// opens on the file (the command line: one per front-end thread); released with the last of them.
struct ResidentBam {
    std::mutex mu;
    bool built = false, failed = false;
    std::vector<BgzfBlock> blks;   // every block from the first record's on, the end-of-file marker included
    np2h::DevBuf<uint8_t> d_inf;
    ResidentBam() { d_inf.cached = true; }
};
// ---- read extraction on the device ---------------------------------------------------------------------------------------
// The contig's BGZF blocks go to the device as they lie in the file, are inflated there (k_bgzf_inflate: one wavefront per
// block), and the records are found by walking the inflated stream along the .bai linear index (k_bam_chain_*).  The host
// parses the 18-byte block headers, converts the index's virtual offsets to stream offsets and reads back one
// np2_bamrec_t + the CIGAR words per record for the admission pass (front_begin) — no payload byte is touched here, and the
// SEQ bytes never leave the device: a record's seq_off points into the inflated stream, which the columnariser reads in place.
//
// When: NP2_INFLATE=gpu, or — unset — when this rank's share of the host is under twelve CPUs (the two paths tie for an
// E. coli-sized contig with sixteen: 8.4 - 9 ms either way; eight ranks of a node on a 16-CPU quota have two each, where
// the pool's path takes 85 ms and this one 12), or when the reference's records are 128 MB of BAM and more.
// -S (SEQ of secondary records from their primaries) stays on the host path (read_records, np2_bamread.cpp).

// The block table of an inflate launch as it goes to the device in one copy: n InfBlock, then the blocks' n CRC32 words
// (k_bgzf_crc32 reads them there: d_blk.p + n).
static size_t blk_table_bytes(size_t n) { return n * sizeof(np2::InfBlock) + n * 4; }
static size_t blk_table_slots(size_t n) { return (blk_table_bytes(n) + sizeof(np2::InfBlock) - 1) / sizeof(np2::InfBlock) + 1; }
// What an inflate launch needs (inflate_blocks), and the staged upload that feeds it: all the two raw doors at the end use.
struct InflateBufs {
    np2h::DevBuf<uint8_t> d_comp, d_inf;
    np2h::DevBuf<np2::InfBlock> d_blk;
    np2h::DevBuf<uint32_t> d_status;
    void *h_tab = nullptr; // pinned: a launch's block table (GpuFetch reads the CIGAR words back into it: free until then)
    size_t h_tab_cap = 0;
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    static constexpr size_t PIECE = (size_t)16 << 20;
    InflateBufs() { d_comp.cached = d_inf.cached = true; }
    ~InflateBufs() {
        (void)hipDeviceSynchronize();
        for (int i = 0; i < 2; ++i) {
            if (pin[i]) np2h::pinned_pool().put(pin[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
        if (h_tab) np2h::pinned_pool().put(h_tab);
    }
    void *table_block(size_t n_blk) { return pinned_block(h_tab, h_tab_cap, std::max<size_t>(blk_table_bytes(n_blk), 64), 4096); }
    // n bytes -> dst (device): staged_upload through these buffers' two pieces of 16 MiB
    template <class Fill, class After> void upload(size_t n, uint8_t *dst, hipStream_t s, Fill fill, After after_piece) {
        for (int i = 0; i < 2; ++i) {
            if (!pin[i]) {
                pin[i] = np2h::pinned_pool().get(PIECE);
                if (!pin[i]) throw np2h::Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
            }
            if (!ev[i]) HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        if (!staged_upload(pin, ev, PIECE, 16, n, dst, s, fill, after_piece)) throw np2h::Np2Error(NP2_E_ARG, "truncated BAM"); // (the file ends inside the range)
    }
    // memory [src, src + n) -> dst
    void upload(const uint8_t *src, size_t n, uint8_t *dst, hipStream_t s) {
        upload(n, dst, s, [&](uint8_t *stage, size_t o, size_t k) { return memcpy(stage, src + o, k) != nullptr; }, no_look);
    }
};
struct GpuFetch {
    InflateBufs ib;
    np2h::DevBuf<uint32_t> d_cigar;
    np2h::DevBuf<uint64_t> d_starts, d_cig_src;
    np2h::DevBuf<uint2> d_info, d_off;
    np2h::DevBuf<np2_bamrec_t> d_recs;
    // pinned blocks the caller reads the records from (until the next fetch): h_recs and, for the CIGAR words, ib.h_tab
    void *h_recs = nullptr;
    size_t h_recs_cap = 0;
    ~GpuFetch() {
        (void)hipDeviceSynchronize();
        if (h_recs) np2h::pinned_pool().put(h_recs);
    }
};

} // namespace np2h

np2_bam::np2_bam() = default;
np2_bam::~np2_bam() {
    gpu.reset(); // (first, as ever: it waits for the device)
    if (map) munmap(const_cast<uint8_t *>(map), map_len);
    if (z.f) fclose(z.f);
}

namespace np2h {

bool gpu_fetch_wanted(const np2_bam *bam, int tid) {
    if (const char *e = getenv("NP2_INFLATE")) return !strcmp(e, "gpu");
    static const bool few_cpus = np2h::usable_cpus() / std::max(1u, np2h::local_ranks()) < 12u;
    if (few_cpus) return true;
    // with the host's CPUs to itself the pool's path ties for a bacterial contig (8.4 - 9 ms either way) and loses from a
    // few hundred MB of BAM on (a 248 Mb chromosome's 2 GB: front end 0.86 - 0.9 s here, 1.1 - 1.5 s there)
    const uint64_t lo = bam->ref_start[tid], hi = bam->ref_end[tid];
    return lo != ~0ull && hi && (hi >> 16) > (lo >> 16) && (hi >> 16) - (lo >> 16) >= ((uint64_t)128 << 20);
}

namespace {
// status words of an inflate launch and the walk behind it: [0, n_blk) per block, then n_bad, walk flags, (pad), tail_at (64-bit, 8-byte aligned)
struct StatusWords {
    size_t bad, flags, tail;
    explicit StatusWords(size_t n_blk) : bad((n_blk + 1) & ~(size_t)1), flags(bad + 1), tail(bad + 2) {}
    size_t count() const { return tail + 2; }
};
uint64_t inflated_bytes(const std::vector<BgzfBlock> &blks) { return blks.empty() ? 0 : blks.back().out_off + blks.back().isize; }
// One inflate launch over blocks whose payloads lie in d_comp (the file from c_lo on), into d_out: their table filled in the pinned
// block and copied up, the status words and `pad` bytes behind the stream zeroed (the columnariser loads whole words behind the last
// SEQ), the inflate kernel and, behind it, every block's CRC-32 over what the inflate left — reported through the same status words,
// no wait of its own.  e0, e1 (optional): recorded around the inflate kernel alone, once all before it is done.  g.d_blk, g.d_status: roomy.
void inflate_blocks(InflateBufs &g, const std::vector<BgzfBlock> &blks, size_t c_lo, const uint8_t *d_comp, uint8_t *d_out, size_t pad, hipStream_t s,
                    unsigned long long *d_prof = nullptr, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    const size_t n_blk = blks.size();
    np2::InfBlock *h_tb = (np2::InfBlock *)g.table_block(n_blk);
    uint32_t *h_crc = (uint32_t *)(h_tb + n_blk); // (the blocks' CRC32 words travel behind the table, in the same copy)
    for (size_t i = 0; i < n_blk; ++i) {
        h_tb[i] = np2::InfBlock{blks[i].file_off + blks[i].hdr_len - c_lo, blks[i].out_off, blks[i].clen, blks[i].isize};
        h_crc[i] = blks[i].crc;
    }
    HIPCHK(hipMemcpyAsync(g.d_blk.p, h_tb, blk_table_bytes(n_blk), hipMemcpyHostToDevice, s));
    const StatusWords w(n_blk);
    HIPCHK(hipMemsetAsync(g.d_status.p, 0, w.count() * 4, s));
    if (pad) HIPCHK(hipMemsetAsync(d_out + inflated_bytes(blks), 0, pad, s));
    if (e0) {
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipEventRecord(e0, s));
    }
    np2::launch_bgzf_inflate(s, g.d_blk.p, (uint32_t)n_blk, d_comp, d_out, g.d_status.p, g.d_status.p + w.bad, d_prof);
    if (e1) HIPCHK(hipEventRecord(e1, s));
    if (bgzf_crc_on()) np2::launch_bgzf_crc32(s, g.d_blk.p, (uint32_t)n_blk, (const uint32_t *)(g.d_blk.p + n_blk), d_out, g.d_status.p, g.d_status.p + w.bad);
}
// File bytes [c_lo, read_end) -> pinned pieces (pread on the pool's threads: the page cache is copied from, no mapping of the
// file is faulted in — through the mmap the same 2 GB of a chromosome's BAM took 0.08 to 2.7 s) -> g.d_comp; the block headers
// are parsed out of each piece while it is there.  blks: the blocks that lie wholly inside the range, their inflated bytes one
// stream; eof: nothing (but the end-of-file marker) follows them in the file.
void read_blocks_to_device(InflateBufs &g, int fd, size_t file_len, size_t c_lo, size_t read_end, hipStream_t s, std::vector<BgzfBlock> &blks, bool &eof) {
    std::vector<uint8_t> sb;
    auto small_read = [&](uint64_t off, size_t n) { // a few bytes that straddle a piece
        sb.resize(n);
        if (off + n > file_len || pread(fd, sb.data(), n, (off_t)off) != (ssize_t)n) throw np2h::Np2Error(NP2_E_ARG, "truncated BGZF block");
        return (const uint8_t *)sb.data();
    };
    uint64_t hdr_at = c_lo; // file offset of the next block header
    bool range_done = false;
    g.upload(read_end - c_lo, g.d_comp.p, s, [&](uint8_t *stage, size_t o, size_t n) { return pread_full(fd, stage, n, c_lo + o); },
             [&](const uint8_t *stage, size_t o0, size_t o1) { // the headers that begin inside this piece
        const uint64_t p0 = c_lo + o0, p1 = c_lo + o1;
        while (!range_done && hdr_at < p1) {
            np2h::BgzfHeader h = np2h::bgzf_header(stage + (hdr_at - p0), (size_t)(p1 - hdr_at), file_len - hdr_at);
            while (h.need) h = np2h::bgzf_header(small_read(hdr_at, h.need), h.need, file_len - hdr_at);
            if (hdr_at + h.bsize > read_end) { // (the block continues beyond what this round reads: not part of it)
                range_done = true;
                break;
            }
            const uint64_t tail = hdr_at + h.bsize - 8;
            const np2h::BgzfTrailer t = np2h::bgzf_trailer(tail + 8 > p1 ? small_read(tail, 8) : stage + (tail - p0));
            blks.push_back(BgzfBlock{hdr_at, inflated_bytes(blks), h.hdr_len, h.clen, t.isize, h.bsize, t.crc});
            hdr_at += h.bsize;
        }
    });
    eof = false;
    if (hdr_at >= file_len) eof = true;
    else if (hdr_at + 28 == file_len) { // nothing but the end-of-file marker behind the range: the range IS the rest of the file
        const uint8_t *mk = small_read(hdr_at, 28);
        if (mk[0] == 31 && mk[1] == 139 && (mk[24] | mk[25] | mk[26] | mk[27]) == 0) eof = true;
    }
}

// The resident stream of this handle's file (ResidentBam), built by the first caller; nullptr: not this file (one reference,
// too large, switched off, no room on the device, a damaged block — the per-reference path then says what is wrong with it).
//   NP2_BAM_RESIDENT_MB: largest file taken (default 1024; 0 = never)
ResidentBam *resident_for(np2_bam *bam, InflateBufs &g, hipStream_t s) {
    if (bam->resident) return bam->resident->built ? bam->resident.get() : nullptr;
    if (bam->resident_tried) return nullptr;
    bam->resident_tried = true;
    static const size_t max_mb = getenv("NP2_BAM_RESIDENT_MB") ? (size_t)std::max(0L, atol(getenv("NP2_BAM_RESIDENT_MB"))) : (size_t)1024;
    const size_t file_len = bam->map_len, c_lo = (size_t)(bam->first_rec >> 16);
    if (bam->ref_names.size() < 2 || !max_mb || file_len <= c_lo || file_len - c_lo > (max_mb << 20)) return nullptr;
    if (getenv("NP2_TEST_FETCH_NO_ROOM")) return nullptr; // (tests/test_gpu_inflate.py: a device without room)
    struct stat st;
    const int fd = fileno(bam->z.f);
    if (fstat(fd, &st) != 0) return nullptr;
    int dev = 0;
    (void)hipGetDevice(&dev);
    static std::mutex reg_mu;
    static std::map<std::tuple<int, uint64_t, uint64_t, uint64_t, int64_t>, std::weak_ptr<ResidentBam>> reg;
    std::shared_ptr<ResidentBam> rb;
    {
        std::lock_guard<std::mutex> l(reg_mu);
        auto &w = reg[std::make_tuple(dev, (uint64_t)st.st_dev, (uint64_t)st.st_ino, (uint64_t)st.st_size, (int64_t)st.st_mtime)];
        rb = w.lock();
        if (!rb) {
            rb = std::make_shared<ResidentBam>();
            w = rb;
        }
    }
    bam->resident = rb;
    std::lock_guard<std::mutex> l(rb->mu);
    if (rb->built) return rb.get();
    if (rb->failed) return nullptr;
    const bool prof = getenv("NP2_IO_PROFILE") != nullptr;
    const double t0 = np2h::now_ms();
    rb->failed = true; // (until the stream stands)
    try {
        g.d_comp.ensure(file_len - c_lo + 64);
        bool eof = false;
        read_blocks_to_device(g, fd, file_len, c_lo, file_len, s, rb->blks, eof);
        const size_t n_blk = rb->blks.size();
        if (!n_blk || !eof) throw np2h::Np2Error(NP2_E_ARG, "BGZF blocks do not reach the end of the file");
        const uint64_t total = inflated_bytes(rb->blks);
        const double t1 = np2h::now_ms();
        rb->d_inf.ensure(total + 128);
        g.d_blk.ensure(blk_table_slots(n_blk));
        g.d_status.ensure(n_blk + 8);
        // (a CRC mismatch counts like a block that does not inflate: no resident stream, and the per-reference path names the block)
        inflate_blocks(g, rb->blks, c_lo, g.d_comp.p, rb->d_inf.p, 128, s);
        const uint32_t *n_bad = (const uint32_t *)g.table_block(n_blk);
        HIPCHK(hipMemcpyAsync((void *)n_bad, g.d_status.p + StatusWords(n_blk).bad, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (*n_bad) throw np2h::Np2Error(NP2_E_ARG, "BGZF inflate failed"); // (or its CRC: caught below either way)
        g.d_comp.release(); // (the file's bytes are not needed again)
        rb->built = true;
        rb->failed = false;
        if (prof)
            fprintf(stderr, "resident BAM: %zu blocks (%.1f MB -> %.1f MB) inflated on the device once: file -> device %.2f ms, inflate %.2f ms\n", n_blk,
                    (file_len - c_lo) / 1e6, total / 1e6, t1 - t0, np2h::now_ms() - t1);
    } catch (const np2h::Np2Error &) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        rb->blks.clear();
        rb->d_inf.release();
        return nullptr;
    }
    return rb.get();
}

// One call of fetch_records_gpu, as its steps share it: what is asked for, the round's blocks, what a round hands to the next.
struct FetchJob {
    np2_bam *bam;
    GpuFetch &g;
    int tid;
    uint32_t L, zone_lo, zone_hi;
    hipStream_t s;
    bool prof;
    double t0;
    uint64_t start_off;
    size_t c_lo, file_len;
    // the round's blocks and the stream their inflated bytes make
    std::vector<BgzfBlock> blks;
    const uint8_t *inf = nullptr;
    uint64_t total = 0;
    size_t c_bytes = 0;
    bool eof = false;
    double t1 = 0, t_up = 0, t_inf = 0, t2 = 0;
    size_t extra = 0; // bytes read beyond the index's end of the reference (an index that understates it costs a second round)
    // A block that does not inflate, or not to bytes of its CRC, may lie in what is read AHEAD of the reference's last record
    // (64 KiB and more: another reference's blocks, which htslib would never open for this one).  The first such block ends
    // the range instead: the round is repeated up to it, and the error is raised only if the walk then wants to go on.
    size_t cap_end = 0;
    std::string held_err;
};
enum FetchNext { FETCH_GO, FETCH_DONE, FETCH_HOST, FETCH_AGAIN }; // after a step: the next one | records out (or none) | the host's way | another round

// Step 1, the blocks of [c_lo, read_end): the reference's stretch of the resident stream, or file bytes read, uploaded and inflated.
FetchNext fetch_take_blocks(FetchJob &j, ResidentBam *res, size_t read_end) {
    InflateBufs &g = j.g.ib;
    hipStream_t s = j.s;
    j.blks.clear();
    j.c_bytes = read_end - j.c_lo;
    j.t1 = j.t0, j.t_up = 0, j.t_inf = 0;
    if (res) {
        // ---- the reference's stretch of the resident stream --------------------------------------------------------------
        const auto &all = res->blks;
        size_t first = (size_t)(std::lower_bound(all.begin(), all.end(), (uint64_t)j.c_lo, [](const BgzfBlock &x, uint64_t v) { return x.file_off < v; }) - all.begin());
        if (first == all.size() || all[first].file_off != j.c_lo) return FETCH_HOST; // the index does not point at a block of this file
        size_t last = first;
        while (last < all.size() && all[last].file_off + all[last].bsize <= read_end) ++last;
        j.blks.assign(all.begin() + (long)first, all.begin() + (long)last);
        j.eof = last == all.size() || (last + 1 == all.size() && all[last].isize == 0);
        const size_t n_blk = j.blks.size();
        if (!n_blk) return FETCH_DONE;
        const uint64_t base = all[first].out_off;
        for (BgzfBlock &b : j.blks) b.out_off -= base;
        j.total = inflated_bytes(j.blks);
        j.inf = res->d_inf.p + base;
        g.d_status.ensure(n_blk + 8);
        HIPCHK(hipMemsetAsync(g.d_status.p, 0, StatusWords(n_blk).count() * 4, s));
        j.t1 = j.t_up = j.t_inf = np2h::now_ms();
        return FETCH_GO;
    }
    // ---- file bytes -> pinned pieces -> device; the block headers parsed on the way ---------------------------------------
    // (file bytes + inflated stream: 13 GB for a human chromosome.  No room on the device next to what else lives there ->
    // the host pool streams the same records through 128 MiB of host memory)
    static const bool test_no_room = getenv("NP2_TEST_FETCH_NO_ROOM") != nullptr; // (tests/test_gpu_inflate.py)
    auto room = [&](auto &buf, size_t n) {
        if (test_no_room && (void *)&buf == (void *)&g.d_inf) return false;
        try {
            buf.ensure(n);
        } catch (const np2h::Np2Error &) {
            (void)hipGetLastError();
            return false;
        }
        return true;
    };
    if (!room(g.d_comp, j.c_bytes + 64)) return FETCH_HOST;
    read_blocks_to_device(g, fileno(j.bam->z.f), j.file_len, j.c_lo, read_end, s, j.blks, j.eof);
    if (j.blks.empty()) {
        HIPCHK(hipStreamSynchronize(s));
        return FETCH_DONE;
    }
    const size_t n_blk = j.blks.size();
    j.total = inflated_bytes(j.blks);
    j.t1 = np2h::now_ms();
    // ---- inflate --------------------------------------------------------------------------------------------------------
    if (!room(g.d_inf, j.total + 128)) {
        HIPCHK(hipStreamSynchronize(s)); // (the uploads into d_comp)
        return FETCH_HOST;
    }
    j.inf = g.d_inf.p;
    g.d_blk.ensure(blk_table_slots(n_blk));
    g.d_status.ensure(n_blk + 8);
    if (j.prof) {
        HIPCHK(hipStreamSynchronize(s));
        j.t_up = np2h::now_ms();
    }
    inflate_blocks(g, j.blks, j.c_lo, g.d_comp.p, g.d_inf.p, 64, s);
    if (j.prof) {
        HIPCHK(hipStreamSynchronize(s));
        j.t_inf = np2h::now_ms();
    }
    return FETCH_GO;
}

// Step 2, chain starts: the linear index's record starts inside the range, as stream offsets.  false: the index is not this file's.
bool fetch_chain_starts(const FetchJob &j, std::vector<uint64_t> &starts) {
    const size_t n_blk = j.blks.size();
    starts.push_back(j.blks[0].out_off + (j.start_off & 0xFFFF));
    size_t bi = 0;
    uint64_t prev = j.start_off;
    for (uint64_t v : j.bam->lin[j.tid]) {
        if (v <= prev) continue; // (0 = empty window; entries repeat while one record spans several windows)
        const uint64_t fo = v >> 16;
        while (bi < n_blk && j.blks[bi].file_off < fo) ++bi;
        if (bi == n_blk) break;                      // beyond the range read so far
        if (j.blks[bi].file_off != fo) return false; // not the start of a block
        const uint64_t so = j.blks[bi].out_off + (v & 0xFFFF);
        if ((v & 0xFFFF) >= j.blks[bi].isize) return false;
        starts.push_back(so);
        prev = v;
    }
    return true;
}

// Step 3: the chains' records counted, then ONE wait — block statuses' summary, the walk's flags, the chains' counts (info) — and
// what they say: a damaged block, a walk that failed or wants a longer range, or on to the records.
FetchNext fetch_count_and_judge(FetchJob &j, const std::vector<uint64_t> &starts, std::vector<uint2> &info) {
    GpuFetch &g = j.g;
    hipStream_t s = j.s;
    const size_t n_blk = j.blks.size();
    const uint32_t n_chains = (uint32_t)starts.size();
    const StatusWords w(n_blk);
    void *h_tb = g.ib.table_block(n_blk);
    HIPCHK(hipMemsetAsync(g.ib.d_status.p + w.tail, 0xFF, 8, s));
    g.d_starts.ensure(n_chains + 1);
    g.d_info.ensure(n_chains + 1);
    g.d_off.ensure(n_chains + 1);
    uint64_t *h_st = (uint64_t *)pinned_block(g.h_recs, g.h_recs_cap, (size_t)n_chains * 8 + 64, 4096);
    memcpy(h_st, starts.data(), (size_t)n_chains * 8);
    HIPCHK(hipMemcpyAsync(g.d_starts.p, h_st, (size_t)n_chains * 8, hipMemcpyHostToDevice, s));
    np2::launch_bam_chain_count(s, j.inf, g.d_starts.p, n_chains, j.total, j.tid, j.L, j.zone_lo, j.zone_hi, g.d_info.p, g.ib.d_status.p + w.flags,
                                (unsigned long long *)(g.ib.d_status.p + w.tail));
    info.resize(n_chains);
    HIPCHK(hipMemcpyAsync(h_st, g.d_info.p, (size_t)n_chains * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_tb, g.ib.d_status.p + w.bad, 16, hipMemcpyDeviceToHost, s)); // (stream order: after the table's upload has read it)
    HIPCHK(hipStreamSynchronize(s));
    memcpy(info.data(), h_st, (size_t)n_chains * 8);
    const uint32_t *tailw = (const uint32_t *)h_tb; // n_bad, the walk's flags
    j.t2 = np2h::now_ms();
    if (tailw[0]) { // which block, and why
        std::vector<uint32_t> stv(n_blk);
        HIPCHK(hipMemcpy(stv.data(), g.ib.d_status.p, n_blk * 4, hipMemcpyDeviceToHost));
        size_t i = 0;
        while (i < n_blk && !stv[i]) ++i;
        if (i < n_blk) {
            const std::string msg = stv[i] == np2inf::ST_CRC_MISMATCH ? crc_msg(j.blks[i].file_off)
                                                                       : "BGZF inflate failed (block at file offset " + std::to_string(j.blks[i].file_off) + ", status " + std::to_string(stv[i]) + ")";
            if (i == 0 || !j.held_err.empty()) throw np2h::Np2Error(NP2_E_ARG, msg);
            j.held_err = msg, j.cap_end = (size_t)j.blks[i].file_off; // (the blocks before it once more, by themselves)
            return FETCH_AGAIN;
        }
    }
    const uint32_t flags = tailw[1];
    // (first: a chain that starts inside a record reads payload bytes as a length and reports a bad or cut-off record of its own)
    if (flags & np2::WALK_MISALIGNED) return FETCH_HOST;
    if (flags & np2::WALK_BAD) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
    if ((flags & (np2::WALK_TAIL | np2::WALK_AT_END)) && !j.eof) { // the reference's records go on beyond the index's end: further
        if (!j.held_err.empty()) throw np2h::Np2Error(NP2_E_ARG, j.held_err); // (into the damaged block)
        j.extra = std::max<size_t>((size_t)1 << 20, j.extra * 2 + j.c_bytes / 4);
        return FETCH_AGAIN;
    }
    if (flags & np2::WALK_TAIL) throw np2h::Np2Error(NP2_E_ARG, "truncated BAM");
    return FETCH_GO;
}

// Step 4: offsets of the chains' records and CIGAR words, the records themselves written on the device and read back, with
// their virtual offsets where the caller wants them.
void fetch_write_back(FetchJob &j, const std::vector<uint2> &info, RecordSet &out, std::vector<uint64_t> *voffs, uint64_t &n_rec, uint64_t &n_cig) {
    GpuFetch &g = j.g;
    hipStream_t s = j.s;
    const uint32_t n_chains = (uint32_t)info.size();
    std::vector<uint2> off(n_chains);
    n_rec = n_cig = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        off[c] = make_uint2((uint32_t)n_rec, (uint32_t)n_cig);
        n_rec += info[c].x, n_cig += info[c].y;
    }
    if (n_rec > 0xFFFFFFF0ull || n_cig > 0xFFFFFFF0ull) throw np2h::Np2Error(NP2_E_NOMEM, "too many records for one contig");
    out.n_recs = (uint32_t)n_rec;
    out.device_seq(j.inf, j.total + 16); // (seq_off points into the inflated stream)
    if (!n_rec) return;
    g.d_recs.ensure(n_rec + 1);
    g.d_cig_src.ensure(n_rec + 1);
    g.d_cigar.ensure(n_cig + 1);
    uint64_t *h_st = (uint64_t *)g.h_recs; // (the chain starts' block: n_chains * 8 bytes and more)
    memcpy(h_st, off.data(), (size_t)n_chains * 8);
    HIPCHK(hipMemcpyAsync(g.d_off.p, h_st, (size_t)n_chains * 8, hipMemcpyHostToDevice, s));
    np2::launch_bam_chain_write(s, j.inf, g.d_starts.p, n_chains, j.total, j.tid, j.L, j.zone_lo, j.zone_hi, g.d_off.p, g.d_recs.p, g.d_cig_src.p);
    np2::launch_bam_cigars(s, j.inf, g.d_recs.p, g.d_cig_src.p, (uint32_t)n_rec, g.d_cigar.p);
    HIPCHK(hipStreamSynchronize(s)); // (h_st is about to be given up for a larger block)
    if (j.prof) fprintf(stderr, "  fetch_records_gpu: offsets + write + cigars %.2f ms\n", np2h::now_ms() - j.t2);
    np2_bamrec_t *hr = (np2_bamrec_t *)pinned_block(g.h_recs, g.h_recs_cap, n_rec * sizeof(np2_bamrec_t) + 64, 4096);
    uint32_t *hc = (uint32_t *)pinned_block(g.ib.h_tab, g.ib.h_tab_cap, n_cig * 4 + 64, 4096);
    HIPCHK(hipMemcpyAsync(hr, g.d_recs.p, n_rec * sizeof(np2_bamrec_t), hipMemcpyDeviceToHost, s));
    if (n_cig) HIPCHK(hipMemcpyAsync(hc, g.d_cigar.p, n_cig * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out.recs = hr, out.cigar = hc, out.d_recs = g.d_recs.p, out.d_cigar = g.d_cigar.p;
    if (voffs) { // stream offset of every record's start -> (file offset of its block << 16 | offset inside the block)
        std::vector<uint64_t> src(n_rec);
        HIPCHK(hipMemcpy(src.data(), g.d_cig_src.p, n_rec * 8, hipMemcpyDeviceToHost));
        voffs->resize(n_rec);
        IoPool::get().parallel_for((size_t)((n_rec + 4095) / 4096), 16, [&](size_t blk) {
            for (uint64_t i = blk * 4096; i < std::min<uint64_t>(n_rec, (blk + 1) * 4096); ++i) {
                const uint64_t at = src[i] - 36u - hr[i].pad; // (first byte of the record's block_size field)
                const BgzfBlock &b = *(std::upper_bound(j.blks.begin(), j.blks.end(), at, [](uint64_t v, const BgzfBlock &x) { return v < x.out_off; }) - 1);
                (*voffs)[i] = (b.file_off << 16) | (at - b.out_off);
            }
        });
    }
}
} // namespace

bool fetch_records_gpu(np2_bam *bam, int tid, uint32_t L, uint32_t zone_lo, uint32_t zone_hi, hipStream_t s, RecordSet &out, std::vector<uint64_t> *voffs) {
    const bool prof = getenv("NP2_IO_PROFILE") != nullptr;
    const double t0 = np2h::now_ms();
    if (bam->ref_start[tid] == ~0ull) return true; // no record of this reference
    if (bam->lin[tid].empty()) return false;
    // where to stop: records that start at or beyond zone_hi lie behind the first record overlapping the window AFTER zone_hi's
    const uint64_t start_off = zone_start_offset(bam, tid, zone_lo);
    uint64_t end_hint = bam->ref_end[tid];
    if (zone_hi < L) {
        const std::vector<uint64_t> &lin = bam->lin[tid];
        size_t w = (size_t)(zone_hi >> 14) + 1;
        while (w < lin.size() && lin[w] == 0) ++w;
        if (w < lin.size()) end_hint = lin[w];
    }
    if (!bam->gpu) bam->gpu.reset(new GpuFetch());
    FetchJob j{bam, *bam->gpu, tid, L, zone_lo, zone_hi, s, prof, t0, start_off, (size_t)(start_off >> 16), bam->map_len};
    j.cap_end = j.file_len;
    size_t c_hi = end_hint ? (size_t)(end_hint >> 16) : j.file_len; // file offset of the last block wanted
    if (getenv("NP2_TEST_FETCH_SHORT_HINT")) c_hi = j.c_lo; // test hook: an index that understates where the reference's records end
    ResidentBam *res = resident_for(bam, j.g.ib, s); // the whole file on the device already (or now), or nullptr
    for (int round = 0;; ++round) {
        if (round > 40) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
        FetchNext next = fetch_take_blocks(j, res, std::min(std::min(j.file_len, c_hi + 65536 + j.extra), j.cap_end));
        if (next != FETCH_GO) return next == FETCH_DONE;
        std::vector<uint64_t> starts;
        if (!fetch_chain_starts(j, starts)) return false;
        std::vector<uint2> info;
        next = fetch_count_and_judge(j, starts, info);
        if (next == FETCH_AGAIN) continue;
        if (next != FETCH_GO) return false;
        uint64_t n_rec = 0, n_cig = 0;
        fetch_write_back(j, info, out, voffs, n_rec, n_cig);
        if (prof)
            fprintf(stderr, "fetch_records_gpu: %zu blocks (%.1f MB -> %.1f MB), %u chains, %llu records, %llu CIGAR words: file -> pinned pieces (+ block headers) %.2f ms, "
                            "rest of the upload %.2f ms, inflate %.2f ms, index + count + wait %.2f ms, records back %.2f ms%s\n", j.blks.size(), j.c_bytes / 1e6, j.total / 1e6,
                    (unsigned)starts.size(), (unsigned long long)n_rec, (unsigned long long)n_cig, j.t1 - t0, j.t_up - j.t1, j.t_inf - j.t_up, j.t2 - j.t_inf, np2h::now_ms() - j.t2,
                    res ? (round ? " (stretch of the resident stream, after extending the range)" : " (stretch of the resident stream)") : (round ? " (after extending the range)" : ""));
        return true;
    }
}

} // namespace np2h

extern "C" {

int np2_bgzf_inflate_device(np2_ctx_t *cx, const uint8_t *bgzf, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                            float *kernel_ms) {
    if (!cx || (!bgzf && n) || !out_len || (!out && out_cap)) return NP2_E_ARG;
    np2h::DevEvent e0, e1;
    return np2h::abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        hipStream_t s = cx->stream;
        BgzfBatch hdr;
        hdr.map = bgzf, hdr.map_len = (size_t)n, hdr.fpos = 0;
        std::vector<BgzfBlock> blks;
        for (BgzfBlock b; hdr.read_raw(b); blks.push_back(b)) b.out_off = inflated_bytes(blks);
        const uint64_t total = inflated_bytes(blks);
        const size_t n_blk = blks.size();
        *out_len = total;
        if (total > out_cap) throw np2h::Np2Error(NP2_E_ARG, "output buffer too small");
        if (!n_blk) return NP2_OK;
        InflateBufs g;
        g.d_comp.ensure(n + 64);
        g.d_inf.ensure(total + 64);
        g.d_blk.ensure(blk_table_slots(n_blk));
        g.d_status.ensure(n_blk + 8);
        g.upload(bgzf, (size_t)n, g.d_comp.p, s);
        np2h::DevBuf<uint64_t> d_prof;
        const bool kprof = getenv("NP2_INF_PROF") != nullptr; // (phase clocks of the inflate kernel: a tool's switch)
        if (kprof) {
            d_prof.ensure(n_blk * 8 + 8);
            HIPCHK(hipMemsetAsync(d_prof.p, 0, n_blk * 64, s));
        }
        e0.make(), e1.make();
        // (kernel_ms is the inflate kernel alone: the CRC check goes behind it)
        inflate_blocks(g, blks, 0, g.d_comp.p, g.d_inf.p, 0, s, kprof ? (unsigned long long *)d_prof.p : nullptr, e0.e, e1.e);
        if (kprof) {
            std::vector<uint64_t> pr(n_blk * 8);
            HIPCHK(hipMemcpyAsync(pr.data(), d_prof.p, pr.size() * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            double sum[8] = {0};
            for (size_t i = 0; i < n_blk; ++i)
                for (int k = 0; k < 8; ++k) sum[k] += (double)pr[i * 8 + k];
            const double nb = (double)n_blk;
            fprintf(stderr, "[inf_prof] %zu blocks; mean clocks per block: total %.0f, wide decode %.0f, chain %.0f (of which match copies %.0f); tokens %.0f, matches %.0f; "
                            "table builds %.0f clocks over %.1f deflate blocks\n",
                    n_blk, sum[0] / nb, sum[1] / nb, sum[2] / nb, sum[3] / nb, sum[4] / nb, sum[5] / nb, sum[6] / nb, sum[7] / nb);
        }
        std::vector<uint32_t> st(n_blk);
        HIPCHK(hipMemcpyAsync(st.data(), g.d_status.p, n_blk * 4, hipMemcpyDeviceToHost, s));
        if (total) HIPCHK(hipMemcpyAsync(out, g.d_inf.p, total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (kernel_ms) *kernel_ms = np2h::elapsed(e0, e1);
        for (size_t i = 0; i < n_blk; ++i)
            if (st[i] == np2inf::ST_CRC_MISMATCH) throw np2h::Np2Error(NP2_E_ARG, "BGZF CRC32 mismatch (block " + std::to_string(i) + ")");
            else if (st[i]) throw np2h::Np2Error(NP2_E_ARG, "BGZF inflate failed (block " + std::to_string(i) + ", status " + std::to_string(st[i]) + ")");
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        (void)hipStreamSynchronize(cx->stream);
        np2h::io_set_error(code, msg);
    });
}

int np2_crc32_device(np2_ctx_t *cx, const uint8_t *data, uint64_t n, const uint64_t *off, uint32_t n_pieces, uint32_t *crc_out, float *kernel_ms) {
    if (!cx || (!data && n) || (n_pieces && (!off || !crc_out))) return NP2_E_ARG;
    np2h::DevEvent e0, e1;
    return np2h::abi_guard([&] {
        if (!n_pieces) {
            if (kernel_ms) *kernel_ms = 0.f;
            return NP2_OK;
        }
        std::vector<np2::InfBlock> tb(n_pieces);
        for (uint32_t i = 0; i < n_pieces; ++i) {
            if (off[i + 1] < off[i]) throw np2h::Np2Error(NP2_E_ARG, "np2_crc32_device: descending offsets");
            if (off[i + 1] - off[i] > 65536u) throw np2h::Np2Error(NP2_E_ARG, "np2_crc32_device: a piece longer than 65536 bytes");
            tb[i] = np2::InfBlock{0, off[i], 0, (uint32_t)(off[i + 1] - off[i])};
        }
        if (off[n_pieces] > n) throw np2h::Np2Error(NP2_E_ARG, "np2_crc32_device: offsets beyond the data");
        HIPCHK(hipSetDevice(cx->device));
        hipStream_t s = cx->stream;
        InflateBufs g;
        g.d_inf.ensure(n + 64);
        g.d_blk.ensure((size_t)n_pieces + 1);
        g.d_status.ensure((size_t)n_pieces + 8);
        if (n) g.upload(data, (size_t)n, g.d_inf.p, s);
        HIPCHK(hipMemcpyAsync(g.d_blk.p, tb.data(), tb.size() * sizeof(np2::InfBlock), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s)); // (tb is pageable: the copy must have read it before it goes)
        e0.make(), e1.make();
        HIPCHK(hipEventRecord(e0.e, s));
        np2::launch_bgzf_crc32(s, g.d_blk.p, n_pieces, nullptr, g.d_inf.p, nullptr, nullptr, g.d_status.p);
        HIPCHK(hipEventRecord(e1.e, s));
        HIPCHK(hipMemcpyAsync(crc_out, g.d_status.p, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (kernel_ms) *kernel_ms = np2h::elapsed(e0, e1);
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        (void)hipStreamSynchronize(cx->stream);
        np2h::io_set_error(code, msg);
    });
}
}
