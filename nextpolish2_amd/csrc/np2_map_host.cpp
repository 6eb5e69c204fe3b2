// Host driver of the mapper (include/np2_io.h: np2_map_*; kernels: np2_map.hip; the rule's arithmetic: np2_map_core.hpp).
//
// The index.  An assembly's separator stream is made resident once, sketched, and its minimizers (h, x) are sorted stably by h
// (rocPRIM, np2_prims.hip) from (sequence, position) order.  The two sorted arrays stay in device memory behind the handle, and
// so does the assembly's text for the aligner (one byte per base).  A lookup is two binary searches.
//
// Reads.  A BATCH is consecutive whole reads, MAP_BATCH_PIECES pieces of bytes at the most (one read when a read is longer).
// Its bytes go to the device PIECE by piece (8 MiB; NP2_MAP_TEST_PIECE) and each piece is sketched by launches of its own:
// the count pass once every piece has arrived, one scan over all the batch's tiles, the emit pass.  A piece boundary may fall
// anywhere in a read: a tile reads the MAP_FRONT bytes before it and the MAP_SIDE bytes after it from the resident batch,
// whichever piece brought them.
// Then per minimizer its run in the index, a scan of the runs' lengths, and per read its first minimizer and anchor offset,
// which come to the host: a batch whose anchors exceed the device budget (2^25; NP2_MAP_TEST_BUDGET) is worked off in GROUPS
// of whole reads.  Per group: anchors emitted in minimizer order, two stable pair sorts (by r << 32 | q, then by read, rel,
// tid), the chain kernel, the hits' read-back and, on request, the primary chains' export.
//
// Alignment (np2_map_align_*; the rule: np2_io.h; kernels: np2_align.hip).  The index keeps the assembly's bytes.  Inside a
// group, after k_map_chain and the chains' export, with the batch's reads still resident: pins and slots per read (count, scan,
// emit), one thread per slot classifies, a scan of the slots' cells gives each matrix its place in the traceback buffer, and the
// reads' cell sums come to the host: a group whose matrices exceed the traceback budget (2^30 bytes; NP2_ALIGN_TEST_BUDGET) is
// worked off in sub-groups of whole reads.  Per sub-group: the DP kernel over its slots, the ops' count, a scan, the ops' emit;
// records and CIGARs come back and are packed in read order.
//
// np2_map_files feeds batches from the reader threads np2_bin_files uses (np2_pieces.hpp, np2_seqreader.hpp): their pieces
// are cut at byte counts, the device thread joins them into batches at read boundaries and writes the PAF lines.
#include "../../include/np2_io.h"
#include "np2_align.hpp"
#include "np2_align_cpu.hpp"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_kernels.hpp"
#include "np2_map.hpp"
#include "np2_map_core.hpp"
#include "np2_map_cpu.hpp"
#include "np2_pieces.hpp"
#include "np2_seqreader.hpp"

#include <chrono>

namespace {
using np2h::DevBuf;
using np2h::DevEvent;
using np2h::elapsed;
using np2h::Np2Error;
using np2map::Hit;

static_assert(sizeof(np2_map_hit_t) == sizeof(Hit) && sizeof(Hit) == 52, "np2_map_hit_t is np2map::Hit");
static_assert(sizeof(np2_map_opts_t) == sizeof(np2map::Opts), "np2_map_opts_t is np2map::Opts");

constexpr uint32_t MAP_BATCH_PIECES = 8;
constexpr uint64_t MAP_MAX_STREAM = 0xFFFFFFFFull - 4096; // offsets in a resident stream are 32 bits wide
constexpr uint8_t SEP = '\n';

thread_local np2_map_stats_t tl_stats{};
thread_local np2_align_stats_t tl_astats{};
static_assert(sizeof(np2_align_opts_t) == sizeof(np2aln::Opts), "np2_align_opts_t is np2aln::Opts");
static_assert(sizeof(np2_align_rec_t) == sizeof(np2aln::Rec) && sizeof(np2aln::Rec) == 32, "np2_align_rec_t is np2aln::Rec");

np2aln::Opts checked_align(const np2_align_opts_t *o, const char *who) {
    if (!o) throw Np2Error(NP2_E_ARG, std::string(who) + ": align_opts is NULL");
    np2aln::Opts r{o->match, o->mismatch, o->gap_open, o->gap_ext, o->band, o->end_bonus, o->ext_max, o->max_cells};
    if (const char *bad = np2aln::check_opts(r)) throw Np2Error(NP2_E_ARG, std::string(who) + ": " + bad);
    return r;
}

void add_counts(np2_align_stats_t &st, const unsigned long long *c) {
    using namespace np2aln;
    st.pins += c[C_PINS], st.segments += c[C_SEGMENTS], st.equal += c[C_EQUAL], st.pure_gap += c[C_GAP], st.snv += c[C_SNV];
    st.cores += c[C_CORES], st.cells += c[C_CELLS], st.clipped_bases += c[C_CLIPPED], st.overflow += c[C_OVERFLOW];
}

np2map::Opts checked(const np2_map_opts_t *o, const char *who) {
    if (!o) throw Np2Error(NP2_E_ARG, std::string(who) + ": opts is NULL");
    np2map::Opts r{o->k, o->w, o->max_occ, o->lookback, o->max_gap, o->bandwidth, o->min_cnt, o->min_score};
    bool unsupported = false;
    if (const char *bad = np2map::check_opts(r, &unsupported))
        throw Np2Error(unsupported ? NP2_E_UNSUPPORTED : NP2_E_ARG, std::string(who) + ": " + bad + " (k = " + std::to_string(o->k) +
                                                                        ", w = " + std::to_string(o->w) + ", lookback = " + std::to_string(o->lookback) + ")");
    return r;
}

struct Hooks {
    size_t piece = (size_t)8 << 20;
    uint64_t budget = 1ull << 25;
    uint64_t align_budget = 1ull << 30; // traceback bytes of a sub-group
    uint32_t align_cells = 1u << 24;    // a cap on max_cells
    Hooks() { // read once per call, like the other NP2_* switches
        piece = (size_t)np2h::test_hook("NP2_MAP_TEST_PIECE", 64, (long long)1 << 30, (long long)piece);
        piece = (piece + 15) & ~(size_t)15; // (tiles are staged with aligned 16-byte loads)
        budget = (uint64_t)np2h::test_hook("NP2_MAP_TEST_BUDGET", 1, (long long)1 << 28, (long long)budget);
        align_budget = (uint64_t)np2h::test_hook("NP2_ALIGN_TEST_BUDGET", 1, (long long)1 << 34, (long long)align_budget);
        align_cells = (uint32_t)np2h::test_hook("NP2_ALIGN_TEST_CELLS", 1, (long long)1 << 24, (long long)align_cells);
    }
    size_t batch_bytes() const { return piece * MAP_BATCH_PIECES; }
};

// the separators of a stream in host memory, checked: it ends in one, and no sequence is longer than 2^31 - 1
std::vector<uint64_t> ends_of(const uint8_t *s, uint64_t n, const char *who, const char *what) {
    if (n && !s) throw Np2Error(NP2_E_ARG, std::string(who) + ": " + what + " is NULL with a length");
    std::vector<uint64_t> e;
    if (!np2map::stream_ends(s, n, e)) throw Np2Error(NP2_E_ARG, std::string(who) + ": " + what + " does not end in a newline");
    uint64_t from = 0;
    for (size_t i = 0; i < e.size(); ++i) {
        if (e[i] - from > np2map::MAX_SEQ)
            throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": sequence " + std::to_string(i) + " of " + what + " is longer than 2^31 - 1");
        from = e[i] + 1;
    }
    return e;
}

struct Stream { // the stream, the events and the scratch of one call
    hipStream_t st = nullptr;
    DevEvent e0, e1;
    DevBuf<uint8_t> tmp;
    np2h::PinnedBuf pin;
    explicit Stream(int device) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        e0.make(), e1.make();
        tmp.cached = true;
    }
    ~Stream() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
    void begin() { HIPCHK(hipEventRecord(e0.e, st)); }
    float end() { // (drains the stream)
        HIPCHK(hipEventRecord(e1.e, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return elapsed(e0, e1);
    }
};

// a stream of n bytes in host memory -> resident on the device, its minimizers (h, x) in (sequence, position) order
struct Sketcher {
    DevBuf<uint8_t> d_seq;
    DevBuf<uint32_t> d_ends, d_cnt, d_off;
    DevBuf<uint64_t> mz_h, mz_x;
    uint32_t n_mz = 0, pieces = 0;
    Sketcher() { d_seq.cached = d_ends.cached = d_cnt.cached = d_off.cached = mz_h.cached = mz_x.cached = true; }

    float run(Stream &s, const uint8_t *bytes, uint64_t n, const uint32_t *ends, uint32_t n_ends, size_t piece, uint32_t k, uint32_t w) {
        using namespace np2;
        hipStream_t st = s.st;
        d_seq.ensure(MAP_FRONT + n + 64);
        d_ends.ensure((size_t)n_ends + 1);
        uint8_t *seq = d_seq.p + MAP_FRONT;
        uint32_t n_tiles = 0;
        for (uint64_t base = 0; base < n; base += piece) n_tiles += map_tiles(std::min<uint64_t>(piece, n - base));
        d_cnt.ensure((size_t)n_tiles + 1), d_off.ensure((size_t)n_tiles + 1);
        const size_t tmp_bytes = prim_temp_bytes((size_t)n_tiles + 1);
        s.tmp.ensure(tmp_bytes);
        uint32_t *h_total = (uint32_t *)s.pin.ensure(64);
        HIPCHK(hipMemsetAsync(d_seq.p, SEP, MAP_FRONT, st));
        HIPCHK(hipMemsetAsync(d_cnt.p + n_tiles, 0, 4, st));
        if (n_ends) HIPCHK(hipMemcpyAsync(d_ends.p, ends, (size_t)n_ends * 4, hipMemcpyHostToDevice, st));
        for (uint64_t base = 0; base < n; base += piece, ++pieces) // (the stream is whole before the first tile reads past its piece)
            HIPCHK(hipMemcpyAsync(seq + base, bytes + base, std::min<uint64_t>(piece, n - base), hipMemcpyHostToDevice, st));
        s.begin();
        uint32_t tile0 = 0;
        for (uint64_t base = 0; base < n; base += piece) {
            const uint64_t len = std::min<uint64_t>(piece, n - base);
            launch_map_sketch_count(st, seq, n, base, len, k, w, tile0, d_cnt.p);
            tile0 += map_tiles(len);
        }
        if (prim_exclusive_sum_u32(st, s.tmp.p, tmp_bytes, d_cnt.p, d_off.p, (size_t)n_tiles + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipMemcpyAsync(h_total, d_off.p + n_tiles, 4, hipMemcpyDeviceToHost, st));
        float ms = s.end();
        n_mz = *h_total;
        mz_h.ensure((size_t)n_mz + 1), mz_x.ensure((size_t)n_mz + 1);
        s.begin();
        tile0 = 0;
        for (uint64_t base = 0; base < n; base += piece) {
            const uint64_t len = std::min<uint64_t>(piece, n - base);
            launch_map_sketch_emit(st, seq, n, base, len, k, w, tile0, d_off.p, d_ends.p, n_ends, mz_h.p, mz_x.p);
            tile0 += map_tiles(len);
        }
        ms += s.end();
        return ms;
    }
};

uint32_t bits_for(uint64_t n) { // key bits that tell 0 .. n - 1 apart
    uint32_t b = 1;
    while (b < 32 && (1ull << b) < n) ++b;
    return b;
}

} // namespace

struct np2_map_index {
    int device = 0;
    uint32_t k = 0, w = 0, n = 0;
    DevBuf<uint64_t> h, x; // sorted by h
    DevBuf<uint8_t> seq;   // the assembly's separator stream, for the aligner
    DevBuf<uint32_t> ends; // its separators
    std::vector<std::string> names;
    std::vector<uint64_t> lens;
    float build_ms = 0.f;
    np2_map_index() { h.cached = x.cached = seq.cached = ends.cached = true; }
};

namespace {

np2_map_index *build_index(int device, const uint8_t *stream, uint64_t n, std::vector<std::string> names, const np2map::Opts &o, const char *who) {
    const std::vector<uint64_t> e64 = ends_of(stream, n, who, "the assembly stream");
    if (n > MAP_MAX_STREAM) throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": an assembly of 2^32 bytes or more");
    if (e64.size() > np2map::MAX_TID) throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 sequences");
    if (!names.empty() && names.size() != e64.size())
        throw Np2Error(NP2_E_ARG, std::string(who) + ": " + std::to_string(names.size()) + " names for " + std::to_string(e64.size()) + " sequences");
    std::unique_ptr<np2_map_index> ix(new np2_map_index());
    ix->device = device, ix->k = o.k, ix->w = o.w;
    std::vector<uint32_t> ends(e64.begin(), e64.end());
    uint64_t from = 0;
    for (size_t i = 0; i < e64.size(); ++i) {
        ix->lens.push_back(e64[i] - from), from = e64[i] + 1;
        ix->names.push_back(names.empty() ? std::to_string(i + 1) : names[i]);
    }
    const Hooks hooks;
    Stream s(device);
    Sketcher sk;
    ix->build_ms = sk.run(s, stream, n, ends.data(), (uint32_t)ends.size(), hooks.piece, o.k, o.w);
    ix->n = sk.n_mz;
    ix->seq.ensure(n + 64), ix->ends.ensure(ends.size() + 1);
    // (the sketcher holds both on the device already; its buffers go with it)
    if (n) HIPCHK(hipMemcpyAsync(ix->seq.p, sk.d_seq.p + np2::MAP_FRONT, n, hipMemcpyDeviceToDevice, s.st));
    if (!ends.empty()) HIPCHK(hipMemcpyAsync(ix->ends.p, sk.d_ends.p, ends.size() * 4, hipMemcpyDeviceToDevice, s.st));
    ix->h.ensure((size_t)ix->n + 1), ix->x.ensure((size_t)ix->n + 1);
    const size_t tmp_bytes = np2::prim_pairs64_temp_bytes(ix->n);
    s.tmp.ensure(tmp_bytes);
    s.begin();
    if (np2::prim_sort_pairs_u64_u64(s.st, s.tmp.p, tmp_bytes, sk.mz_h.p, ix->h.p, sk.mz_x.p, ix->x.p, ix->n, 2 * o.k))
        throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
    ix->build_ms += s.end();
    return ix.release();
}

// batches of reads against one index
struct Mapper {
    const np2_map_index &ix;
    np2map::Opts o;
    Hooks hooks;
    Stream s;
    Sketcher sk;
    DevBuf<uint32_t> d_lo, d_cnt, d_first, d_coff, d_chain;
    DevBuf<uint64_t> d_off, d_aoff, khi_a, klo_a, khi_b, klo_b;
    DevBuf<unsigned long long> d_ctr;
    DevBuf<int32_t> d_f, d_p, d_base, d_end;
    DevBuf<uint8_t> d_mark;
    DevBuf<Hit> d_hits;
    std::vector<uint32_t> h_first, h_coff;
    std::vector<uint64_t> h_aoff;
    np2_map_stats_t &stats;
    // the aligner: off while ao is null
    const np2aln::Opts *ao = nullptr;
    np2aln::Opts ao_v{};
    np2_align_stats_t &astats;
    DevBuf<uint8_t> d_pin, d_tb;
    DevBuf<uint32_t> d_nslots, d_soff, d_slot_read, d_cells, d_nops, d_ooff, d_a, d_b;
    DevBuf<uint64_t> d_tboff, d_rcells;
    DevBuf<np2aln::Slot> d_slots;
    DevBuf<np2aln::Res> d_res;
    DevBuf<np2aln::Rec> d_recs;
    DevBuf<unsigned long long> d_actr;
    std::vector<uint64_t> h_rcells;
    std::vector<uint32_t> h_soff, h_ooff, h_b;
    std::vector<np2aln::Rec> h_recs;

    void align_with(const np2aln::Opts &a) {
        ao_v = a, ao = &ao_v;
        if (ao_v.max_cells > hooks.align_cells) ao_v.max_cells = hooks.align_cells;
        d_pin.cached = d_tb.cached = d_nslots.cached = d_soff.cached = d_slot_read.cached = d_cells.cached = d_nops.cached = true;
        d_ooff.cached = d_a.cached = d_b.cached = d_tboff.cached = d_rcells.cached = d_slots.cached = d_res.cached = true;
        d_recs.cached = d_actr.cached = true;
        astats = np2_align_stats_t{};
    }

    Mapper(const np2_map_index &ix_, const np2map::Opts &o_) : ix(ix_), o(o_), s(ix_.device), stats(tl_stats), astats(tl_astats) {
        d_lo.cached = d_cnt.cached = d_first.cached = d_coff.cached = d_chain.cached = d_off.cached = d_aoff.cached = true;
        khi_a.cached = klo_a.cached = khi_b.cached = klo_b.cached = d_ctr.cached = d_f.cached = d_p.cached = d_base.cached = true;
        d_end.cached = d_mark.cached = d_hits.cached = true;
        stats = np2_map_stats_t{};
        stats.index_minimizers = ix.n;
    }

    // reads as a stream of n bytes with n_reads separators at ends[]: hits[0 .. n_reads); with `chain`, the primary chains'
    // (r, q) pairs appended to it and chain_n[i] = pairs of read i
    // with the aligner on: recs[0 .. n_reads) and the reads' CIGAR words appended to `cigar` in read order
    void batch(const uint8_t *bytes, uint64_t n, const uint32_t *ends, uint32_t n_reads, Hit *hits, std::vector<uint32_t> *chain,
               np2aln::Rec *recs = nullptr, std::vector<uint32_t> *cigar = nullptr) {
        using namespace np2;
        if (n_reads == 0) return;
        hipStream_t st = s.st;
        stats.sketch_ms += sk.run(s, bytes, n, ends, n_reads, hooks.piece, o.k, o.w);
        const uint32_t n_mz = sk.n_mz;
        d_lo.ensure((size_t)n_mz + 1), d_cnt.ensure((size_t)n_mz + 1), d_off.ensure((size_t)n_mz + 1);
        d_first.ensure((size_t)n_reads + 1), d_aoff.ensure((size_t)n_reads + 1), d_ctr.ensure(1);
        d_hits.ensure(n_reads), d_end.ensure(n_reads);
        const size_t scan_tmp = prim_temp_bytes((size_t)n_mz + 1);
        s.tmp.ensure(scan_tmp);
        h_first.resize((size_t)n_reads + 1), h_aoff.resize((size_t)n_reads + 1);
        unsigned long long dropped = 0;
        HIPCHK(hipMemsetAsync(d_ctr.p, 0, 8, st));
        HIPCHK(hipMemsetAsync(d_cnt.p + n_mz, 0, 4, st));
        s.begin();
        launch_map_seed_count(st, sk.mz_h.p, n_mz, ix.h.p, ix.n, o.max_occ, d_lo.p, d_cnt.p, d_ctr.p);
        if (prim_exclusive_sum_u32_u64(st, s.tmp.p, scan_tmp, d_cnt.p, d_off.p, (size_t)n_mz + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        launch_map_read_ranges(st, sk.mz_x.p, n_mz, d_off.p, n_reads, d_first.p, d_aoff.p);
        HIPCHK(hipMemcpyAsync(h_first.data(), d_first.p, ((size_t)n_reads + 1) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_aoff.data(), d_aoff.p, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&dropped, d_ctr.p, 8, hipMemcpyDeviceToHost, st));
        stats.seed_ms += s.end();
        stats.minimizers += n_mz, stats.dropped_occ += dropped, stats.anchors += h_aoff[n_reads];
        stats.pieces += sk.pieces, sk.pieces = 0;

        for (uint32_t r0 = 0; r0 < n_reads;) { // groups of whole reads within the anchor budget
            uint32_t r1 = r0 + 1;
            if (h_aoff[r1] - h_aoff[r0] > hooks.budget)
                throw Np2Error(NP2_E_UNSUPPORTED, "a read with " + std::to_string(h_aoff[r1] - h_aoff[r0]) + " anchors: more than the device budget of " +
                                                      std::to_string(hooks.budget) + " (lower max_occ)");
            while (r1 < n_reads && h_aoff[r1 + 1] - h_aoff[r0] <= hooks.budget) ++r1;
            group(r0, r1, hits, chain, recs, cigar);
            ++stats.groups;
            r0 = r1;
        }
        for (uint32_t i = 0; i < n_reads; ++i) ++(hits[i].tid >= 0 ? stats.mapped : stats.unmapped);
        stats.reads += n_reads;
    }

    void group(uint32_t r0, uint32_t r1, Hit *hits, std::vector<uint32_t> *chain, np2aln::Rec *recs, std::vector<uint32_t> *cigar) {
        using namespace np2;
        hipStream_t st = s.st;
        const uint64_t n_an = h_aoff[r1] - h_aoff[r0];
        const uint32_t n_reads = r1 - r0;
        khi_a.ensure(n_an + 1), klo_a.ensure(n_an + 1), khi_b.ensure(n_an + 1), klo_b.ensure(n_an + 1);
        d_f.ensure(n_an + 1), d_p.ensure(n_an + 1), d_base.ensure(n_an + 1), d_mark.ensure(n_an + 1);
        const size_t tmp_bytes = prim_pairs64_temp_bytes(n_an);
        s.tmp.ensure(tmp_bytes);
        s.begin();
        launch_map_seed_emit(st, h_first[r0], h_first[r1], sk.mz_x.p, d_lo.p, d_cnt.p, d_off.p, r0, sk.d_ends.p, ix.x.p, o.k, khi_a.p, klo_a.p);
        stats.seed_ms += s.end();
        s.begin();
        if (prim_sort_pairs_u64_u64(st, s.tmp.p, tmp_bytes, klo_a.p, klo_b.p, khi_a.p, khi_b.p, n_an, 64) ||
            prim_sort_pairs_u64_u64(st, s.tmp.p, tmp_bytes, khi_b.p, khi_a.p, klo_b.p, klo_a.p, n_an, 32 + bits_for(n_reads)))
            throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
        stats.sort_ms += s.end();
        MapChain c{};
        c.khi = khi_a.p, c.klo = klo_a.p, c.aoff = d_aoff.p, c.ends = sk.d_ends.p;
        c.f = d_f.p, c.p = d_p.p, c.base = d_base.p, c.mark = d_mark.p;
        c.hits = d_hits.p, c.chain_end = d_end.p, c.r0 = r0, c.n_reads = n_reads, c.o = o;
        s.begin();
        launch_map_chain(st, c);
        HIPCHK(hipMemcpyAsync(hits + r0, d_hits.p + r0, (size_t)n_reads * sizeof(Hit), hipMemcpyDeviceToHost, st));
        stats.chain_ms += s.end();
        if (ao)
            for (uint32_t i = r0; i < r1; ++i) recs[i] = np2aln::unaligned_rec();
        if (!chain && !ao) return;
        h_coff.resize(n_reads);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n_reads; ++i) h_coff[i] = (uint32_t)total, total += hits[r0 + i].tid >= 0 ? hits[r0 + i].n : 0;
        if (total == 0) return;
        d_coff.ensure(n_reads), d_chain.ensure(2 * total);
        const size_t at = chain ? chain->size() : 0;
        if (chain) chain->resize(at + 2 * total);
        HIPCHK(hipMemcpyAsync(d_coff.p, h_coff.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
        s.begin();
        launch_map_chain_export(st, c, d_coff.p, d_chain.p);
        if (chain) HIPCHK(hipMemcpyAsync(chain->data() + at, d_chain.p, 2 * total * 4, hipMemcpyDeviceToHost, st));
        stats.chain_ms += s.end();
        if (ao) align_group(r0, n_reads, total, recs, cigar);
    }

    // the group's mapped reads, their chains in d_chain at d_coff: recs[r0 + i] and the CIGAR words in read order
    void align_group(uint32_t r0, uint32_t n_reads, uint64_t total_pairs, np2aln::Rec *recs, std::vector<uint32_t> *cigar) {
        using namespace np2;
        hipStream_t st = s.st;
        AlignJob c{};
        c.asm_seq = ix.seq.p, c.asm_ends = ix.ends.p, c.rd_seq = sk.d_seq.p + MAP_FRONT, c.rd_ends = sk.d_ends.p;
        c.hits = d_hits.p, c.coff = d_coff.p, c.chain = d_chain.p;
        c.r0 = r0, c.n_reads = n_reads, c.k = o.k, c.max_cells = ao->max_cells, c.o = *ao;
        d_pin.ensure(total_pairs + 1), d_nslots.ensure((size_t)n_reads + 2), d_soff.ensure((size_t)n_reads + 2);
        d_rcells.ensure((size_t)n_reads + 2), d_nops.ensure((size_t)n_reads + 2), d_ooff.ensure((size_t)n_reads + 2);
        d_recs.ensure((size_t)n_reads + 1), d_actr.ensure(np2aln::C_N);
        c.pin = d_pin.p, c.nslots = d_nslots.p, c.soff = d_soff.p, c.read_cells = d_rcells.p, c.nops = d_nops.p, c.ooff = d_ooff.p;
        c.recs = d_recs.p, c.ctr = d_actr.p;
        size_t scan_tmp = prim_temp_bytes((size_t)n_reads + 2); // (the reads' scans; grows for the slots', never shrinks)
        s.tmp.ensure(scan_tmp);
        h_soff.resize((size_t)n_reads + 1), h_rcells.resize((size_t)n_reads + 1), h_ooff.resize((size_t)n_reads + 1), h_recs.resize(n_reads);
        HIPCHK(hipMemsetAsync(d_actr.p, 0, np2aln::C_N * 8, st));
        s.begin();
        launch_align_pins(st, c);
        if (prim_exclusive_sum_u32(st, s.tmp.p, scan_tmp, d_nslots.p, d_soff.p, (size_t)n_reads + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipMemcpyAsync(h_soff.data(), d_soff.p, ((size_t)n_reads + 1) * 4, hipMemcpyDeviceToHost, st));
        astats.pins_ms += s.end();
        const uint32_t n_slots = h_soff[n_reads];
        d_slots.ensure((size_t)n_slots + 1), d_slot_read.ensure((size_t)n_slots + 1), d_cells.ensure((size_t)n_slots + 2);
        d_tboff.ensure((size_t)n_slots + 2), d_res.ensure((size_t)n_slots + 1);
        c.slots = d_slots.p, c.slot_read = d_slot_read.p, c.cells = d_cells.p, c.tb_off = d_tboff.p, c.res = d_res.p;
        scan_tmp = std::max(scan_tmp, prim_temp_bytes((size_t)n_slots + 2));
        s.tmp.ensure(scan_tmp);
        s.begin();
        launch_align_plan(st, c);
        astats.pins_ms += s.end();
        s.begin();
        launch_align_classify(st, c, n_slots);
        if (prim_exclusive_sum_u32_u64(st, s.tmp.p, scan_tmp, d_cells.p, d_tboff.p, (size_t)n_slots + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        launch_align_read_cells(st, c);
        HIPCHK(hipMemcpyAsync(h_rcells.data(), d_rcells.p, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
        astats.classify_ms += s.end();
        uint32_t n_sub = 0;
        for (uint32_t g0 = 0; g0 < n_reads; ++n_sub) { // sub-groups of whole reads within the traceback budget, one read at the least
            uint32_t g1 = g0 + 1;
            while (g1 < n_reads && h_rcells[g1 + 1] - h_rcells[g0] <= hooks.align_budget) ++g1;
            const uint64_t tb_base = h_rcells[g0], tb_bytes = h_rcells[g1] - tb_base;
            d_tb.ensure(tb_bytes + 64);
            c.tb = d_tb.p;
            s.begin();
            launch_align_dp(st, c, h_soff[g0], h_soff[g1], tb_base);
            astats.dp_ms += s.end();
            const uint32_t ng = g1 - g0;
            s.begin();
            launch_align_ops_count(st, c, g0, g1, tb_base);
            if (prim_exclusive_sum_u32(st, s.tmp.p, scan_tmp, d_nops.p + g0, d_ooff.p + g0, (size_t)ng + 1))
                throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
            HIPCHK(hipMemcpyAsync(h_ooff.data(), d_ooff.p + g0, ((size_t)ng + 1) * 4, hipMemcpyDeviceToHost, st));
            astats.assemble_ms += s.end();
            const size_t n_ops = h_ooff[ng], n_b = 2 * n_ops + 2 * (size_t)ng;
            d_a.ensure(n_ops + 1), d_b.ensure(n_b + 1);
            c.a = d_a.p, c.b = d_b.p;
            h_b.resize(n_b + 1);
            s.begin();
            launch_align_ops_emit(st, c, g0, g1, tb_base);
            HIPCHK(hipMemcpyAsync(h_recs.data() + g0, d_recs.p + g0, (size_t)ng * sizeof(np2aln::Rec), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_b.data(), d_b.p, n_b * 4, hipMemcpyDeviceToHost, st));
            astats.assemble_ms += s.end();
            for (uint32_t i = 0; i < ng; ++i) {
                const np2aln::Rec &rc = h_recs[g0 + i];
                recs[r0 + g0 + i] = rc;
                const uint32_t *w = h_b.data() + 2 * (size_t)h_ooff[i] + 2 * (size_t)i;
                if (cigar) cigar->insert(cigar->end(), w, w + rc.n_cigar);
            }
            g0 = g1;
        }
        if (n_sub > 1) stats.groups += n_sub - 1;
        unsigned long long ctr[np2aln::C_N];
        HIPCHK(hipMemcpyAsync(ctr, d_actr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        add_counts(astats, ctr);
    }
};

void check_index_opts(const np2_map_index *ix, const np2map::Opts &o, const char *who) {
    if (!ix) throw Np2Error(NP2_E_ARG, std::string(who) + ": the index is NULL");
    if (o.k != ix->k || o.w != ix->w)
        throw Np2Error(NP2_E_ARG, std::string(who) + ": the index was built with k = " + std::to_string(ix->k) + ", w = " + std::to_string(ix->w) +
                                      ", the options say k = " + std::to_string(o.k) + ", w = " + std::to_string(o.w));
}

// chain_off[r0 .. r0 + n] from the hits (chain_off[r0] is set)
void chain_offsets(const Hit *hits, uint64_t n, uint64_t *chain_off) {
    for (uint64_t i = 0; i < n; ++i) chain_off[i + 1] = chain_off[i] + (hits[i].tid >= 0 ? hits[i].n : 0);
}

uint32_t *chain_out(const std::vector<uint32_t> &chain) { // a malloc block for the caller (np2_free); never NULL
    uint32_t *p = (uint32_t *)malloc(std::max<size_t>(chain.size(), 1) * 4);
    if (!p) throw Np2Error(NP2_E_NOMEM, "out of memory for the chains");
    if (!chain.empty()) memcpy(p, chain.data(), chain.size() * 4);
    return p;
}

// ---- files -> pieces (the read binner's reader threads) -> batches ------------------------------------------------------------
struct MapPiece {
    uint8_t *buf = nullptr; // pinned: HALO bytes (not used here), then up to `cap` bytes
    size_t n = 0;
    std::vector<uint32_t> ends;
    std::string names; // of the reads that end in the piece, '\n' after each
    bool last = false; // the file ends with this piece
};
using MapQueue = np2h::PieceQueue<MapPiece>;

struct MapWriter {
    np2h::HaloWriter<MapPiece> w;
    np2seq::NameCollector names;
    uint64_t open_len = 0;
    MapWriter(MapQueue &q, size_t cap) : w(q, cap) {
        w.on_fresh = [](MapPiece &p) {
            p.last = false;
            p.ends.clear(), p.names.clear();
        };
    }
    void finish() { // (a file without a byte still ends: with an empty piece)
        if (!w.cur && !w.fresh()) return;
        w.cur->last = true;
        w.flush(true);
    }
    void put(const uint8_t *p, size_t n) {
        const bool sep = n == 1 && *p == SEP; // (a line's bytes hold no '\n')
        if (!sep && (open_len += n) > np2map::MAX_SEQ) throw Np2Error(NP2_E_UNSUPPORTED, "np2_map_files: a read longer than 2^31 - 1");
        if (sep) { // the read that is open ends in the piece that takes its separator
            if (w.dead || (!w.cur && !w.fresh())) return;
            w.cur->ends.push_back((uint32_t)w.cur->n);
            w.cur->names += names.close();
            w.cur->names.push_back('\n');
            open_len = 0;
        }
        w.put(p, n);
    }
};

// whole reads gathered from pieces; what follows the last separator waits for the next piece
struct BatchBuf {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> ends;
    std::string names;
    void add(const MapPiece &p) {
        const size_t at = bytes.size();
        if (at + p.n > MAP_MAX_STREAM) throw Np2Error(NP2_E_UNSUPPORTED, "np2_map_files: a batch of 2^32 bytes or more");
        bytes.insert(bytes.end(), p.buf + np2h::HALO, p.buf + np2h::HALO + p.n);
        for (uint32_t e : p.ends) ends.push_back((uint32_t)(at + e));
        names += p.names;
    }
    size_t closed() const { return ends.empty() ? 0 : (size_t)ends.back() + 1; }
    void drop_closed() {
        bytes.erase(bytes.begin(), bytes.begin() + (ptrdiff_t)closed());
        ends.clear(), names.clear();
    }
};

void write_paf(np2h::OutFile &out, const np2_map_index &ix, const BatchBuf &b, const std::vector<Hit> &hits, std::string &text) {
    text.clear();
    size_t name_at = 0;
    for (size_t i = 0; i < b.ends.size(); ++i) {
        const size_t name_end = b.names.find('\n', name_at);
        const Hit &h = hits[i];
        if (h.tid >= 0) np2map::paf_line(text, b.names.data() + name_at, name_end - name_at, h, ix.names[(size_t)h.tid], ix.lens[(size_t)h.tid]);
        name_at = name_end + 1;
    }
    out.put(text.data(), text.size());
}

void fill_stats(np2_map_stats_t *stats) {
    if (stats) *stats = tl_stats;
}

void write_sam(np2h::OutFile &out, const np2_map_index &ix, const BatchBuf &b, const std::vector<Hit> &hits, const std::vector<np2aln::Rec> &recs,
               const std::vector<uint32_t> &cigar, std::string &text) {
    text.clear();
    size_t name_at = 0, cig_at = 0, from = 0;
    for (size_t i = 0; i < b.ends.size(); ++i) {
        const size_t name_end = b.names.find('\n', name_at);
        const np2aln::Rec &rc = recs[i];
        np2aln::sam_line(text, b.names.data() + name_at, name_end - name_at, rc, hits[i], cigar.data() + cig_at, b.bytes.data() + from,
                         (uint32_t)(b.ends[i] - from), rc.tid >= 0 ? &ix.names[(size_t)rc.tid] : nullptr);
        cig_at += rc.n_cigar, name_at = name_end + 1, from = (size_t)b.ends[i] + 1;
    }
    out.put(text.data(), text.size());
}

// np2_map_files (aopts null: PAF) and np2_map_align_files (SAM)
int map_files_impl(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const np2_align_opts_t *aopts,
                   bool align, const char *out_path, np2_map_stats_t *stats, const std::string who) {
    return np2h::abi_guard([&] {
        const np2map::Opts o = checked(opts, who.c_str());
        np2aln::Opts ao{};
        if (align) ao = checked_align(aopts, who.c_str());
        check_index_opts(ix, o, who.c_str());
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no read file given");
        if (!out_path) throw Np2Error(NP2_E_ARG, who + ": out_path is NULL");
        std::vector<std::string> files;
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, who + ": a read file path is NULL");
            FILE *f = fopen(paths[i], "rb");
            if (!f) throw Np2Error(NP2_E_ARG, who + ": cannot open " + paths[i]);
            fclose(f);
            files.push_back(paths[i]);
        }
        Mapper m(*ix, o);
        if (align) m.align_with(ao);
        np2h::OutFile out;
        out.open(out_path, ix->device);
        const size_t cap = m.hooks.piece;
        const size_t n_threads = std::min<size_t>(files.size(), 16);
        std::vector<MapQueue> queues(n_threads);
        std::vector<MapPiece> pieces(2 * n_threads);
        np2h::PinnedBlocks pinned;
        for (size_t i = 0; i < pieces.size(); ++i) {
            pieces[i].buf = pinned.get(np2h::HALO + cap + 64);
            queues[i / 2].idle.push_back(&pieces[i]);
        }
        auto readers = np2h::run_readers(n_threads, queues, [&](size_t ti) {
            for (size_t fi = ti; fi < files.size(); fi += n_threads) {
                MapWriter w(queues[ti], cap);
                np2seq::parse_file(files[fi], [&](const uint8_t *p, size_t n) { w.put(p, n); }, [&] { return w.w.dead; },
                                   [&](const uint8_t *p, size_t n, bool begin) { w.names(p, n, begin); });
                w.finish();
                if (w.w.dead) break;
            }
        });
        BatchBuf b;
        std::vector<Hit> hits;
        std::string text;
        std::vector<np2aln::Rec> recs;
        std::vector<uint32_t> cigar;
        if (align) {
            np2aln::sam_header(text, ix->names, ix->lens);
            out.put(text.data(), text.size());
        }
        auto flush = [&] {
            if (b.ends.empty()) return;
            hits.resize(b.ends.size());
            if (align) recs.resize(b.ends.size()), cigar.clear();
            m.batch(b.bytes.data(), b.closed(), b.ends.data(), (uint32_t)b.ends.size(), hits.data(), nullptr, align ? recs.data() : nullptr,
                    align ? &cigar : nullptr);
            const auto t0 = std::chrono::steady_clock::now();
            if (align) write_sam(out, *ix, b, hits, recs, cigar, text);
            else write_paf(out, *ix, b, hits, text);
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            tl_stats.write_ms += ms;
            if (align) tl_astats.write_ms += ms;
            b.drop_closed();
        };
        for (size_t fi = 0; fi < files.size(); ++fi) {
            MapQueue &q = queues[fi % n_threads];
            for (bool last = false; !last;) {
                const auto t0 = std::chrono::steady_clock::now();
                MapPiece *p = q.take_full();
                tl_stats.read_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (!p) throw Np2Error(q.err_code != NP2_OK ? q.err_code : NP2_E_ARG, q.err_code != NP2_OK ? q.err : who + ": a reader stopped early");
                last = p->last;
                b.add(*p);
                q.give_idle(p);
                if (b.closed() >= m.hooks.batch_bytes() || last) flush(); // (a file's last read ends with its separator)
            }
        }
        out.close();
        fill_stats(stats);
        return NP2_OK;
    }, np2h::io_set_error);
}

} // namespace

extern "C" {

int np2_map_index_bytes(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts, np2_map_index_t **out) {
    return np2h::abi_guard([&] {
        // every argument is checked before the first device call
        if (!out) throw Np2Error(NP2_E_ARG, "np2_map_index_bytes: out is NULL");
        *out = nullptr;
        const np2map::Opts o = checked(opts, "np2_map_index_bytes");
        std::vector<std::string> nm;
        if (names)
            for (const char *p = names; *p;) {
                const char *e = strchr(p, '\n');
                if (!e) throw Np2Error(NP2_E_ARG, "np2_map_index_bytes: names does not end in a newline");
                nm.emplace_back(p, e), p = e + 1;
            }
        *out = build_index(device, stream, n, std::move(nm), o, "np2_map_index_bytes");
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_index_files(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, np2_map_index_t **out) {
    return np2h::abi_guard([&] {
        if (!out) throw Np2Error(NP2_E_ARG, "np2_map_index_files: out is NULL");
        *out = nullptr;
        const np2map::Opts o = checked(opts, "np2_map_index_files");
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "np2_map_index_files: no assembly file given");
        for (int i = 0; i < n_paths; ++i)
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "np2_map_index_files: an assembly file path is NULL");
        std::vector<uint8_t> stream;
        std::vector<std::string> names;
        for (int i = 0; i < n_paths; ++i) {
            np2seq::NameCollector nc;
            np2seq::parse_file(paths[i], [&](const uint8_t *p, size_t m) {
                if (m == 1 && *p == SEP) names.push_back(nc.close());
                if (stream.size() + m > MAP_MAX_STREAM) throw Np2Error(NP2_E_UNSUPPORTED, "np2_map_index_files: an assembly of 2^32 bytes or more");
                stream.insert(stream.end(), p, p + m);
            }, nullptr, [&](const uint8_t *p, size_t m, bool begin) { nc(p, m, begin); });
        }
        *out = build_index(device, stream.data(), stream.size(), std::move(names), o, "np2_map_index_files");
        return NP2_OK;
    }, np2h::io_set_error);
}

void np2_map_index_free(np2_map_index_t *ix) {
    if (!ix) return;
    (void)np2h::abi_guard([&] {
        HIPCHK(hipSetDevice(ix->device));
        delete ix;
        return NP2_OK;
    });
}

int np2_map_index_info(const np2_map_index_t *ix, uint32_t *k, uint32_t *w, uint64_t *n_seqs, uint64_t *n_minimizers, float *build_ms) {
    if (!ix) return np2h::io_set_error(NP2_E_ARG, "np2_map_index_info: the index is NULL");
    if (k) *k = ix->k;
    if (w) *w = ix->w;
    if (n_seqs) *n_seqs = ix->names.size();
    if (n_minimizers) *n_minimizers = ix->n;
    if (build_ms) *build_ms = ix->build_ms;
    return NP2_OK;
}

int np2_map_index_seq(const np2_map_index_t *ix, uint64_t i, const char **name, uint64_t *len) {
    if (!ix || i >= ix->names.size()) return np2h::io_set_error(NP2_E_ARG, "np2_map_index_seq: no such sequence");
    if (name) *name = ix->names[i].c_str();
    if (len) *len = ix->lens[i];
    return NP2_OK;
}

int np2_map_bytes(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                  np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off) {
    return np2h::abi_guard([&] {
        if (chain) *chain = nullptr;
        const np2map::Opts o = checked(opts, "np2_map_bytes");
        check_index_opts(ix, o, "np2_map_bytes");
        if (n_reads && !hits) throw Np2Error(NP2_E_ARG, "np2_map_bytes: hits is NULL");
        if ((chain == nullptr) != (chain_off == nullptr)) throw Np2Error(NP2_E_ARG, "np2_map_bytes: chain and chain_off go together");
        const std::vector<uint64_t> ends = ends_of(reads, n, "np2_map_bytes", "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_map_bytes: n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        Mapper m(*ix, o);
        std::vector<uint32_t> ch, local;
        Hit *out = reinterpret_cast<Hit *>(hits);
        for (uint64_t r0 = 0; r0 < n_reads;) { // batches: whole reads, batch_bytes() at the most, one read at the least
            const uint64_t from = r0 ? ends[r0 - 1] + 1 : 0;
            uint64_t r1 = r0 + 1;
            while (r1 < n_reads && ends[r1] + 1 - from <= m.hooks.batch_bytes()) ++r1;
            local.clear();
            for (uint64_t i = r0; i < r1; ++i) local.push_back((uint32_t)(ends[i] - from));
            m.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), out + r0, chain ? &ch : nullptr);
            r0 = r1;
        }
        if (chain) {
            chain_off[0] = 0;
            chain_offsets(out, n_reads, chain_off);
            *chain = chain_out(ch);
        }
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_files(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const char *out_path,
                  np2_map_stats_t *stats) {
    return map_files_impl(ix, paths, n_paths, opts, nullptr, false, out_path, stats, "np2_map_files");
}

int np2_map_align_files(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                        const np2_align_opts_t *align_opts, const char *out_path, np2_map_stats_t *stats) {
    return map_files_impl(ix, paths, n_paths, map_opts, align_opts, true, out_path, stats, "np2_map_align_files");
}

int np2_map_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                 np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off) {
    return np2h::abi_guard([&] {
        if (chain) *chain = nullptr;
        const np2map::Opts o = checked(opts, "np2_map_host");
        if (n_reads && !hits) throw Np2Error(NP2_E_ARG, "np2_map_host: hits is NULL");
        if ((chain == nullptr) != (chain_off == nullptr)) throw Np2Error(NP2_E_ARG, "np2_map_host: chain and chain_off go together");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, "np2_map_host", "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, "np2_map_host", "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_map_host: n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w);
        np2_map_stats_t &st = tl_stats;
        st = np2_map_stats_t{};
        st.index_minimizers = hx.mz.size();
        std::vector<uint32_t> ch;
        Hit *out = reinterpret_cast<Hit *>(hits);
        np2map::ReadCounts rc;
        uint64_t from = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            np2map::map_read(hx, reads + from, (uint32_t)(ends[i] - from), o, &out[i], chain ? &ch : nullptr, &rc);
            ++(out[i].tid >= 0 ? st.mapped : st.unmapped);
            from = ends[i] + 1;
        }
        st.reads = n_reads, st.minimizers = rc.minimizers, st.anchors = rc.anchors, st.dropped_occ = rc.dropped_occ;
        if (chain) {
            chain_off[0] = 0;
            chain_offsets(out, n_reads, chain_off);
            *chain = chain_out(ch);
        }
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_align_bytes(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *map_opts,
                        const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off) {
    return np2h::abi_guard([&] {
        if (cigar) *cigar = nullptr;
        const np2map::Opts o = checked(map_opts, "np2_map_align_bytes");
        const np2aln::Opts ao = checked_align(align_opts, "np2_map_align_bytes");
        check_index_opts(ix, o, "np2_map_align_bytes");
        if (n_reads && !recs) throw Np2Error(NP2_E_ARG, "np2_map_align_bytes: recs is NULL");
        if ((cigar == nullptr) != (cigar_off == nullptr)) throw Np2Error(NP2_E_ARG, "np2_map_align_bytes: cigar and cigar_off go together");
        const std::vector<uint64_t> ends = ends_of(reads, n, "np2_map_align_bytes", "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_map_align_bytes: n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        Mapper m(*ix, o);
        m.align_with(ao);
        std::vector<uint32_t> cg, local;
        std::vector<Hit> own;
        if (!hits) own.resize(n_reads);
        Hit *out = hits ? reinterpret_cast<Hit *>(hits) : own.data();
        np2aln::Rec *rout = reinterpret_cast<np2aln::Rec *>(recs);
        for (uint64_t r0 = 0; r0 < n_reads;) {
            const uint64_t from = r0 ? ends[r0 - 1] + 1 : 0;
            uint64_t r1 = r0 + 1;
            while (r1 < n_reads && ends[r1] + 1 - from <= m.hooks.batch_bytes()) ++r1;
            local.clear();
            for (uint64_t i = r0; i < r1; ++i) local.push_back((uint32_t)(ends[i] - from));
            m.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), out + r0, nullptr, rout + r0, &cg);
            r0 = r1;
        }
        if (cigar) {
            cigar_off[0] = 0;
            for (uint64_t i = 0; i < n_reads; ++i) cigar_off[i + 1] = cigar_off[i] + rout[i].n_cigar;
            *cigar = chain_out(cg);
        }
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_align_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                       const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs,
                       uint32_t **cigar, uint64_t *cigar_off) {
    return np2h::abi_guard([&] {
        if (cigar) *cigar = nullptr;
        const np2map::Opts o = checked(map_opts, "np2_map_align_host");
        np2aln::Opts ao = checked_align(align_opts, "np2_map_align_host");
        if (n_reads && !recs) throw Np2Error(NP2_E_ARG, "np2_map_align_host: recs is NULL");
        if ((cigar == nullptr) != (cigar_off == nullptr)) throw Np2Error(NP2_E_ARG, "np2_map_align_host: cigar and cigar_off go together");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, "np2_map_align_host", "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, "np2_map_align_host", "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_map_align_host: n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        const Hooks hooks;
        if (ao.max_cells > hooks.align_cells) ao.max_cells = hooks.align_cells;
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w);
        np2_map_stats_t &st = tl_stats;
        st = np2_map_stats_t{};
        st.index_minimizers = hx.mz.size();
        tl_astats = np2_align_stats_t{};
        std::vector<uint32_t> cg, ch;
        np2map::ReadCounts rc;
        np2aln::Scratch w;
        unsigned long long ctr[np2aln::C_N] = {};
        np2aln::Rec *rout = reinterpret_cast<np2aln::Rec *>(recs);
        uint64_t from = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            Hit h;
            ch.clear();
            np2map::map_read(hx, reads + from, (uint32_t)(ends[i] - from), o, &h, &ch, &rc);
            ++(h.tid >= 0 ? st.mapped : st.unmapped);
            if (hits) reinterpret_cast<Hit *>(hits)[i] = h;
            rout[i] = np2aln::unaligned_rec();
            if (h.tid >= 0) {
                const uint64_t t_at = h.tid ? a_ends[(size_t)h.tid - 1] + 1 : 0;
                uint64_t c64[np2aln::C_N] = {};
                rout[i] = np2aln::align_read(asm_stream + t_at, (uint32_t)(a_ends[(size_t)h.tid] - t_at), reads + from, h, ch.data(), o.k, ao,
                                             ao.max_cells, w, cg, c64);
                for (int f = 0; f < np2aln::C_N; ++f) ctr[f] += c64[f];
            }
            from = ends[i] + 1;
        }
        st.reads = n_reads, st.minimizers = rc.minimizers, st.anchors = rc.anchors, st.dropped_occ = rc.dropped_occ;
        add_counts(tl_astats, ctr);
        if (cigar) {
            cigar_off[0] = 0;
            for (uint64_t i = 0; i < n_reads; ++i) cigar_off[i + 1] = cigar_off[i] + rout[i].n_cigar;
            *cigar = chain_out(cg);
        }
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_align_last_stats(np2_align_stats_t *stats) {
    if (!stats) return np2h::io_set_error(NP2_E_ARG, "np2_map_align_last_stats: stats is NULL");
    *stats = tl_astats;
    return NP2_OK;
}

int np2_map_last_stats(np2_map_stats_t *stats) {
    if (!stats) return np2h::io_set_error(NP2_E_ARG, "np2_map_last_stats: stats is NULL");
    *stats = tl_stats;
    return NP2_OK;
}

} // extern "C"
