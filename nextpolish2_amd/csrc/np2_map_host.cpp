// Host driver of the mapper (include/np2_io.h: np2_map_*; kernels: np2_map.hip; the rule's arithmetic: np2_map_core.hpp).
//
// The index.  An assembly's separator stream is made resident once, sketched, and its minimizers (h, x) are sorted stably by h
// (rocPRIM, np2_prims.hip) from (sequence, position) order.  The two sorted arrays stay in device memory behind the handle, and
// so does the assembly's text for the aligner (one byte per base).  A lookup is two binary searches.
//
// Weights (np2_map_weights_*, the _w entries; the rule: np2_io.h, "Weights").  A weight set is host memory: the listed canonical
// indices, ascending and unique.  An index built with one owns a bitmap of 4^k bits and its coarse level on the device, zeroed and
// set on the build's stream before the assembly is sketched; the Sketcher of every later call against the index takes the two
// pointers, so reads are sketched under the same weights with no new argument.  Null pointers select the unweighted launches.
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
// More chains (np2_map_*_m; the rule: np2_io.h, "More chains").  Only with max_chains > 1, inside a group right behind
// k_map_chain: k_map_chain_more, a scan of the reads' unit counts, whose sums come to the host, k_map_units_pack, and the
// units' hits, classes and parents in read order (Mapper::more_group); on request the units' chains.  With the aligner on
// (np2_map_align_*_m) the group's units are its jobs: align_group runs on them through AlignJob::unit_read, each unit with its own
// hit and chain, the arrays per unit; a batch's units are then settled on the host (Units::settle) and a read's records are
// written together (write_sam_units), so SA:Z: sees all of them whatever groups and sub-groups the units fell into.
//
// Alignment (np2_map_align_*; the rule: np2_io.h; kernels: np2_align.hip).  The index keeps the assembly's bytes.  Inside a
// group, after k_map_chain and the chains' export, with the batch's reads still resident: pins and slots per read (count, scan,
// emit), one thread per slot classifies, a scan of the slots' cells gives each matrix its place in the traceback buffer, and the
// reads' cell sums come to the host: a group whose matrices exceed the traceback budget (2^30 bytes; NP2_ALIGN_TEST_BUDGET) is
// worked off in sub-groups of whole reads.  Per sub-group: the DP kernel over its slots, the ops' count, a scan, the ops' emit;
// records and CIGARs come back and are packed in read order.
//
// The resident SAM straight from reads (np2_sam_from_reads, np2_sam_from_read_bytes; the rule: np2_io.h; kernels:
// np2_alnpack.hip).  The same batches, groups and sub-groups, but records and CIGARs do not come back: per sub-group the sizes of
// what is kept are scanned behind the ops' emit, their totals ride with the wait that is there anyway, the host makes room in
// the handle's input-order arrays (np2_sam_accum.hpp) and the pack kernel follows on the mapper's stream; after the last batch
// the SAM door's own sort and gather run there too.
//
// np2_map_files feeds batches from the reader threads np2_bin_files uses (np2_pieces.hpp, np2_seqreader.hpp): their pieces
// are cut at byte counts, the device thread joins them into batches at read boundaries and writes the PAF lines.
#include "../../include/np2_io.h"
#include "np2_align.hpp"
#include "np2_align_cpu.hpp"
#include "np2_aligntags.hpp"
#include "np2_alnpack.hpp"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_kernels.hpp"
#include "np2_map.hpp"
#include "np2_map_core.hpp"
#include "np2_map_cpu.hpp"
#include "np2_map_units.hpp"
#include "np2_pieces.hpp"
#include "np2_sam_accum.hpp"
#include "np2_seqreader.hpp"

#include <algorithm>
#include <chrono>

namespace {
using np2h::DevBuf;
using np2h::DevEvent;
using np2h::elapsed;
using np2h::Np2Error;
using np2aln::TagTexts;
using np2aln::Units;
using np2map::Hit;

static_assert(sizeof(np2_map_hit_t) == sizeof(Hit) && sizeof(Hit) == 52, "np2_map_hit_t is np2map::Hit");
static_assert(sizeof(np2_map_opts_t) == sizeof(np2map::Opts), "np2_map_opts_t is np2map::Opts");

constexpr uint32_t MAP_BATCH_PIECES = 8;
constexpr uint64_t MAP_MAX_STREAM = 0xFFFFFFFFull - 4096; // offsets in a resident stream are 32 bits wide
constexpr uint8_t SEP = '\n';

thread_local np2_map_stats_t tl_stats{};
thread_local np2_align_stats_t tl_astats{};
thread_local np2_align_tag_stats_t tl_tstats{};
thread_local np2_map_multi_stats_t tl_mstats{};
static_assert(sizeof(np2_map_multi_opts_t) == sizeof(np2map::MultiOpts), "np2_map_multi_opts_t is np2map::MultiOpts");
static_assert(NP2_ALN_QUAL == np2aln::ALN_QUAL && NP2_ALN_MD == np2aln::ALN_MD && NP2_ALN_CS == np2aln::ALN_CS && NP2_ALN_EQX == np2aln::ALN_EQX,
              "NP2_ALN_* are np2aln::ALN_*");
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
    bool coarse = true;                 // an index built with weights keeps the bitmap's coarse level
    Hooks() { // read once per call, like the other NP2_* switches
        piece = (size_t)np2h::test_hook("NP2_MAP_TEST_PIECE", 64, (long long)1 << 30, (long long)piece);
        piece = (piece + 15) & ~(size_t)15; // (tiles are staged with aligned 16-byte loads)
        budget = (uint64_t)np2h::test_hook("NP2_MAP_TEST_BUDGET", 1, (long long)1 << 28, (long long)budget);
        align_budget = (uint64_t)np2h::test_hook("NP2_ALIGN_TEST_BUDGET", 1, (long long)1 << 34, (long long)align_budget);
        align_cells = (uint32_t)np2h::test_hook("NP2_ALIGN_TEST_CELLS", 1, (long long)1 << 24, (long long)align_cells);
        coarse = np2h::test_hook("NP2_MAP_TEST_COARSE", 0, 1, 1) != 0;
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
    const uint64_t *listed = nullptr, *coarse = nullptr; // the index's weight bitmap and its coarse level; null: the unweighted launches
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
            launch_map_sketch_count(st, seq, n, base, len, k, w, tile0, d_cnt.p, listed, coarse);
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
            launch_map_sketch_emit(st, seq, n, base, len, k, w, tile0, d_off.p, d_ends.p, n_ends, mz_h.p, mz_x.p, listed, coarse);
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

struct np2_map_weights { // host memory only
    np2map::WeightSet ws;
};

struct np2_map_index {
    int device = 0;
    uint32_t k = 0, w = 0, n = 0;
    DevBuf<uint64_t> h, x; // sorted by h
    DevBuf<uint8_t> seq;   // the assembly's separator stream, for the aligner
    DevBuf<uint32_t> ends; // its separators
    std::vector<std::string> names;
    std::vector<uint64_t> lens;
    float build_ms = 0.f;
    // the weights the index was built with (0, 0: none): one bit per canonical k-mer index, set for the listed ones; reads are
    // sketched under it too
    uint32_t weights_k = 0;
    uint64_t n_listed = 0;
    DevBuf<uint64_t> listed; // 4^k / 64 words, then (unless NP2_MAP_TEST_COARSE=0) the coarse level's 4^k / 4096
    bool has_coarse = false;
    np2_map_index() { h.cached = x.cached = seq.cached = ends.cached = listed.cached = true; }
    const uint64_t *bitmap() const { return n_listed ? listed.p : nullptr; }
    const uint64_t *coarse() const { return n_listed && has_coarse ? listed.p + np2::map_weight_words(weights_k) : nullptr; }
};

namespace {

// a non-empty weight set's k: the membership test is a direct-addressed bitmap of 4^k bits
void check_weights_k(uint32_t k, const char *who) {
    if (k < np2map::KW_MIN || k > np2map::KW_MAX)
        throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": weights are built for 11 <= k <= 15, the list has k = " + std::to_string(k) +
                                              " (16 <= k <= 28 would need more than a direct-addressed bitmap)");
}
uint64_t revcomp_index(uint64_t v, uint32_t k) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < k; ++i) r = r << 2 | (3u - ((v >> (2u * i)) & 3u));
    return r;
}
void seal_weights(np2map::WeightSet &ws, uint32_t k) { // ascending and unique
    std::sort(ws.idx.begin(), ws.idx.end());
    ws.idx.erase(std::unique(ws.idx.begin(), ws.idx.end()), ws.idx.end());
    ws.k = k;
}

// the weights of a _w call: null for none or an empty set; a set of another k than the options' is NP2_E_ARG
const np2map::WeightSet *checked_weights(const np2_map_weights_t *w, const np2map::Opts &o, const char *who) {
    if (!w || w->ws.empty()) return nullptr;
    if (w->ws.k != o.k)
        throw Np2Error(NP2_E_ARG, std::string(who) + ": the weights list k-mers of length " + std::to_string(w->ws.k) + ", the options say k = " +
                                      std::to_string(o.k) + " (an index built with weights needs k equal to the list's)");
    return &w->ws;
}

np2_map_index *build_index(int device, const uint8_t *stream, uint64_t n, std::vector<std::string> names, const np2map::Opts &o, const char *who,
                           const np2map::WeightSet *ws = nullptr) {
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
    DevBuf<uint32_t> d_idx;
    d_idx.cached = true;
    if (ws) { // the bitmap: zeroed here, never assumed zero, then one bit per listed index
        const size_t fine = np2::map_weight_words(o.k), words = fine + (hooks.coarse ? np2::map_weight_coarse_words(o.k) : 0);
        ix->listed.ensure(words), d_idx.ensure(ws->idx.size());
        ix->has_coarse = hooks.coarse;
        HIPCHK(hipMemcpyAsync(d_idx.p, ws->idx.data(), ws->idx.size() * 4, hipMemcpyHostToDevice, s.st));
        s.begin();
        HIPCHK(hipMemsetAsync(ix->listed.p, 0, words * 8, s.st));
        np2::launch_map_weights_set(s.st, d_idx.p, ws->idx.size(), ix->listed.p, hooks.coarse ? ix->listed.p + fine : nullptr);
        ix->build_ms = s.end();
        ix->weights_k = ws->k, ix->n_listed = ws->idx.size();
        sk.listed = ix->bitmap(), sk.coarse = ix->coarse();
    }
    ix->build_ms += sk.run(s, stream, n, ends.data(), (uint32_t)ends.size(), hooks.piece, o.k, o.w);
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

// np2_sam_from_reads: a sub-group's records, CIGAR words and read bytes go from where k_align_ops_emit left them into the
// input-order arrays of a resident SAM handle (np2_sam_accum.hpp), on the mapper's stream.  Only the totals come to the host.
struct PackSink {
    np2h::SamAccum acc;
    uint32_t tie;
    DevBuf<uint32_t> d_kept, d_ncig, d_nseq, d_nname, d_koff, d_coff, d_soff, d_nmoff, d_nbad, d_name_at;
    DevBuf<uint8_t> d_names_in;
    np2h::PinnedBuf pin_tot, pin_names;
    DevEvent p0, p1, p2, p3;
    np2::AlnPackJob job{};
    bool pending = false;       // p2, p3 bracket a launch whose time has not been read
    uint64_t reads_before = 0;  // reads of the batches before this one
    uint32_t batch_reads = 0;
    float pack_ms = 0.f;

    PackSink(np2_sam &sam, hipStream_t st, bool keep_names, uint32_t tie_by_strand) : acc(sam, st), tie(tie_by_strand) {
        acc.keep_names = keep_names;
        d_kept.cached = d_ncig.cached = d_nseq.cached = d_nname.cached = d_koff.cached = d_coff.cached = d_soff.cached = true;
        d_nmoff.cached = d_nbad.cached = d_name_at.cached = d_names_in.cached = true;
        p0.make(), p1.make(), p2.make(), p3.make();
    }
    // k_alnpack is launched without a wait: when an error unwinds the call, it may still read the scans' outputs, the names and the
    // mapper's buffers, which go back to the block cache right after this (the mapper is destroyed after its sink)
    ~PackSink() { (void)hipStreamSynchronize(acc.st); }
    // the batch's names ('\n' after each of its n_reads reads) go up once
    void begin_batch(const char *names, size_t names_n, uint32_t n_reads) {
        batch_reads = n_reads;
        if (!acc.keep_names) return;
        hipStream_t st = acc.st;
        uint32_t *at = (uint32_t *)pin_names.ensure(((size_t)n_reads + 1) * 4 + names_n + 64);
        uint8_t *bytes = (uint8_t *)(at + n_reads + 1);
        size_t from = 0;
        for (uint32_t i = 0; i < n_reads; ++i) {
            const char *e = from < names_n ? (const char *)memchr(names + from, '\n', names_n - from) : nullptr;
            if (!e) throw Np2Error(NP2_E_ARG, "np2_sam_from_reads: fewer names than reads");
            at[i] = (uint32_t)from, from = (size_t)(e - names) + 1;
        }
        at[n_reads] = (uint32_t)from;
        memcpy(bytes, names, from);
        d_name_at.ensure((size_t)n_reads + 1), d_names_in.ensure(from + 1), d_nbad.ensure(1);
        HIPCHK(hipMemcpyAsync(d_name_at.p, at, ((size_t)n_reads + 1) * 4, hipMemcpyHostToDevice, st));
        if (from) HIPCHK(hipMemcpyAsync(d_names_in.p, bytes, from, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_nbad.p, 0xFF, 4, st));
    }
    void end_batch() { reads_before += batch_reads, acc.n_records += batch_reads; }

    // after launch_align_ops_emit of reads [g0, g1): the sizes, their scans and the totals' copies.  `tmp` serves the scans.
    void sizes(const np2::AlignJob &c, uint32_t g0, uint32_t g1, void *tmp, size_t tmp_bytes) {
        hipStream_t st = acc.st;
        const uint32_t ng = g1 - g0;
        const size_t m = (size_t)ng + 1;
        d_kept.ensure(m), d_ncig.ensure(m), d_nseq.ensure(m), d_koff.ensure(m), d_coff.ensure(m), d_soff.ensure(m);
        if (acc.keep_names) d_nname.ensure(m), d_nmoff.ensure(m);
        job = np2::AlnPackJob{c.recs, c.rd_seq, c.rd_ends, c.b, c.ooff, c.r0, g0, g1, acc.keep_names ? d_name_at.p : nullptr, d_names_in.p,
                              d_kept.p, d_ncig.p, d_nseq.p, d_nname.p, d_koff.p, d_coff.p, d_soff.p, d_nmoff.p};
        uint32_t *h = (uint32_t *)pin_tot.ensure(64);
        h[3] = 0, h[4] = 0xFFFFFFFFu;
        HIPCHK(hipEventRecord(p0.e, st));
        np2::launch_alnpack_sizes(st, job, d_nbad.p);
        if (np2::prim_exclusive_sum_u32(st, tmp, tmp_bytes, d_kept.p, d_koff.p, m) || np2::prim_exclusive_sum_u32(st, tmp, tmp_bytes, d_ncig.p, d_coff.p, m) ||
            np2::prim_exclusive_sum_u32(st, tmp, tmp_bytes, d_nseq.p, d_soff.p, m) ||
            (acc.keep_names && np2::prim_exclusive_sum_u32(st, tmp, tmp_bytes, d_nname.p, d_nmoff.p, m)))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipEventRecord(p1.e, st));
        HIPCHK(hipMemcpyAsync(h + 0, d_koff.p + ng, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + 1, d_coff.p + ng, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h + 2, d_soff.p + ng, 4, hipMemcpyDeviceToHost, st));
        if (acc.keep_names) {
            HIPCHK(hipMemcpyAsync(h + 3, d_nmoff.p + ng, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h + 4, d_nbad.p, 4, hipMemcpyDeviceToHost, st));
        }
    }
    // ... and once the stream has been drained: room for the totals, then the pack kernel, which nobody waits for here.
    // Returns the HIP-event time of sizes().
    float pack() {
        hipStream_t st = acc.st;
        const float ms = elapsed(p0, p1);
        pack_ms += ms;
        const uint32_t *h = (const uint32_t *)pin_tot.p;
        const uint64_t kept = h[0], n_cig = h[1], n_seq = h[2], n_name = h[3];
        if (h[4] != 0xFFFFFFFFu)
            throw Np2Error(NP2_E_ARG, "np2_sam_from_reads: read " + std::to_string(reads_before + h[4] + 1) + ": QNAME is empty or longer than 254 bytes");
        if (kept > job.g1 - job.g0 || n_name > kept * 254u) throw Np2Error(NP2_E_DEVICE, "np2_sam_from_reads: record counters out of range");
        acc.check_room(kept, n_cig);
        if (kept) {
            acc.reserve(kept, n_cig, n_seq, n_name, 0);
            const np2::AlnPackOut o{acc.n_recs, acc.n_cigar, acc.seq_bytes, acc.name_bytes, tie, acc.recs_in.p, acc.tids_in.p, acc.keys_in.p,
                                    acc.cigar_in.p, acc.sam.seq4.p, acc.sam.names.p, acc.nref_in.p};
            HIPCHK(hipEventRecord(p2.e, st));
            np2::launch_alnpack(st, job, o);
            HIPCHK(hipEventRecord(p3.e, st));
            pending = true;
        }
        acc.advance(kept, n_cig, n_seq, n_name, 0);
        return ms;
    }
    void collect() { // (the stream has been drained since pack())
        if (pending) pack_ms += elapsed(p2, p3);
        pending = false;
    }
};

// The tag kernels around their scans, for the aligner's sub-groups and for np2_align_tags_device: sizes, three exclusive sums,
// the texts and the split CIGAR, which come to the host with their offsets.  Returns the HIP-event time, copies included.
struct TagRun {
    DevBuf<uint32_t> d_n_md, d_n_cs, d_n_eqx, d_eqx_off, d_eqx;
    DevBuf<uint64_t> d_md_off, d_cs_off;
    DevBuf<uint8_t> d_md, d_cs;
    std::vector<uint64_t> md_off, cs_off; // [n + 1]
    std::vector<uint32_t> eqx_off, eqx;
    std::vector<char> md, cs;
    TagRun() {
        d_n_md.cached = d_n_cs.cached = d_n_eqx.cached = d_eqx_off.cached = d_eqx.cached = d_md_off.cached = d_cs_off.cached = true;
        d_md.cached = d_cs.cached = true;
    }
    float run(Stream &s, np2::TagJob j) {
        using namespace np2;
        hipStream_t st = s.st;
        const size_t m = (size_t)j.n + 1;
        d_n_md.ensure(m), d_n_cs.ensure(m), d_n_eqx.ensure(m), d_md_off.ensure(m), d_cs_off.ensure(m), d_eqx_off.ensure(m);
        const size_t tmp_bytes = prim_temp_bytes(m);
        s.tmp.ensure(tmp_bytes);
        md_off.resize(m), cs_off.resize(m), eqx_off.resize(m);
        j.n_md = d_n_md.p, j.n_cs = d_n_cs.p, j.n_eqx = d_n_eqx.p;
        j.md_off = d_md_off.p, j.cs_off = d_cs_off.p, j.eqx_off = d_eqx_off.p;
        s.begin();
        launch_align_tags_size(st, j);
        if (prim_exclusive_sum_u32_u64(st, s.tmp.p, tmp_bytes, d_n_md.p, d_md_off.p, m) ||
            prim_exclusive_sum_u32_u64(st, s.tmp.p, tmp_bytes, d_n_cs.p, d_cs_off.p, m) ||
            prim_exclusive_sum_u32(st, s.tmp.p, tmp_bytes, d_n_eqx.p, d_eqx_off.p, m))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipMemcpyAsync(md_off.data(), d_md_off.p, m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(cs_off.data(), d_cs_off.p, m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(eqx_off.data(), d_eqx_off.p, m * 4, hipMemcpyDeviceToHost, st));
        float ms = s.end();
        const uint64_t n_md = md_off[j.n], n_cs = cs_off[j.n], n_eqx = eqx_off[j.n];
        d_md.ensure(n_md + 1), d_cs.ensure(n_cs + 1), d_eqx.ensure(n_eqx + 1);
        md.resize(n_md), cs.resize(n_cs), eqx.resize(n_eqx);
        j.md = (char *)d_md.p, j.cs = (char *)d_cs.p, j.eqx = d_eqx.p;
        s.begin();
        launch_align_tags_emit(st, j);
        if (n_md) HIPCHK(hipMemcpyAsync(md.data(), d_md.p, n_md, hipMemcpyDeviceToHost, st));
        if (n_cs) HIPCHK(hipMemcpyAsync(cs.data(), d_cs.p, n_cs, hipMemcpyDeviceToHost, st));
        if (n_eqx) HIPCHK(hipMemcpyAsync(eqx.data(), d_eqx.p, n_eqx * 4, hipMemcpyDeviceToHost, st));
        ms += s.end();
        return ms;
    }
};

// the host twin of the tag kernels for one record: its texts appended to tt (read i of the batch), its split CIGAR to `eqx`
void tags_of_record(const np2aln::TagIn &in, uint32_t flags, TagTexts &tt, size_t i, std::vector<uint32_t> *eqx) {
    np2aln::TagOut sz{};
    const auto one = [](bool b) { return (uint64_t)(b ? 1u : 0u); };
    np2aln::tag_walk(in, sz, 0, 1, one);
    np2aln::TagOut out{};
    const size_t md_at = tt.md.size(), cs_at = tt.cs.size(), x_at = eqx ? eqx->size() : 0;
    if (flags & NP2_ALN_MD) tt.md.resize(md_at + sz.n_md), tt.n_md[i] = sz.n_md, out.md = tt.md.data() + md_at;
    if (flags & NP2_ALN_CS) tt.cs.resize(cs_at + sz.n_cs), tt.n_cs[i] = sz.n_cs, out.cs = tt.cs.data() + cs_at;
    if (eqx && (flags & NP2_ALN_EQX)) eqx->resize(x_at + sz.n_eqx), out.eqx = eqx->data() + x_at;
    np2aln::tag_walk(in, out, 0, 1, one);
    if (out.n_md != sz.n_md || out.n_cs != sz.n_cs || out.n_eqx != sz.n_eqx) throw Np2Error(NP2_E_DEVICE, "the tag walk's two passes disagree");
}

uint32_t checked_out_flags(uint32_t flags, uint32_t allowed, const std::string &who) {
    if (flags & ~allowed) throw Np2Error(NP2_E_ARG, who + ": unknown flag bits in out_flags");
    return flags;
}

np2map::MultiOpts checked_multi(const np2_map_multi_opts_t *m, const std::string &who) {
    if (!m) throw Np2Error(NP2_E_ARG, who + ": multi is NULL");
    np2map::MultiOpts r{m->max_chains, m->supplementary, m->secondary_n, m->mask_pm, m->pri_pm};
    if (const char *bad = np2map::check_multi(r)) throw Np2Error(NP2_E_ARG, who + ": " + bad);
    return r;
}

void add_more_counts(np2_map_multi_stats_t &st, const unsigned long long *c) {
    st.selections += c[0], st.dropped_min_cnt += c[1], st.dropped_secondary += c[2], st.kept_supplementary += c[3], st.kept_secondary += c[4];
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
    PackSink *pk = nullptr; // np2_sam_from_reads: records and CIGAR words stay on the device (recs and cigar are null then)
    np2aln::Probe *probe = nullptr; // np2_align_chains_device: the slots, cells and traceback bytes come to the host as well
    // the opt-in outputs (NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX): off while tag_flags is 0; tt takes a batch's texts
    uint32_t tag_flags = 0;
    TagRun tg;
    TagTexts *tt = nullptr;
    // more chains: off while `units` is null (max_chains = 1 included: no further kernel is launched then)
    np2map::MultiOpts mo{};
    Units *units = nullptr;
    bool unit_chains = false;
    DevBuf<Hit> d_uh, d_phits;
    DevBuf<uint32_t> d_ucls, d_upar, d_ucnt, d_uoff, d_ppar, d_pread;
    DevBuf<int32_t> d_uend, d_pend;
    DevBuf<uint8_t> d_pcls;
    DevBuf<unsigned long long> d_mctr;
    std::vector<uint32_t> h_uoff;

    void more_with(const np2map::MultiOpts &m, Units *u, bool chains) {
        mo = m, units = u, unit_chains = chains;
        d_uh.cached = d_phits.cached = d_ucls.cached = d_upar.cached = d_ucnt.cached = d_uoff.cached = d_ppar.cached = d_pread.cached = true;
        d_uend.cached = d_pend.cached = d_pcls.cached = d_mctr.cached = true;
    }

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
        sk.listed = ix.bitmap(), sk.coarse = ix.coarse();
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

    // np2_align_chains_device: the caller's reads, hits and chains (checked: check_chains) take the places the sketcher, k_map_chain
    // and k_map_chain_export fill for align_group; one group
    void chains(const uint8_t *bytes, uint64_t n, const uint32_t *ends, uint32_t n_reads, const Hit *hits, const uint32_t *chain,
                const uint64_t *chain_off, np2aln::Rec *recs, std::vector<uint32_t> *cigar) {
        using namespace np2;
        hipStream_t st = s.st;
        for (uint32_t i = 0; i < n_reads; ++i) recs[i] = np2aln::unaligned_rec(), ++(hits[i].tid >= 0 ? stats.mapped : stats.unmapped);
        stats.reads += n_reads;
        const uint64_t total = n_reads ? chain_off[n_reads] : 0;
        if (total == 0) {
            if (probe) probe->slot_off.assign((size_t)n_reads + 1, 0);
            return;
        }
        sk.d_seq.ensure(MAP_FRONT + n + 64), sk.d_ends.ensure((size_t)n_reads + 1);
        d_hits.ensure(n_reads), d_coff.ensure(n_reads), d_chain.ensure(2 * total);
        h_coff.resize(n_reads);
        for (uint32_t i = 0; i < n_reads; ++i) h_coff[i] = (uint32_t)chain_off[i];
        HIPCHK(hipMemsetAsync(sk.d_seq.p, SEP, MAP_FRONT, st));
        HIPCHK(hipMemcpyAsync(sk.d_seq.p + MAP_FRONT, bytes, n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(sk.d_ends.p, ends, (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_hits.p, hits, (size_t)n_reads * sizeof(Hit), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_coff.p, h_coff.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_chain.p, chain, 2 * total * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        align_group(0, n_reads, total, recs, cigar, nullptr, nullptr, 0);
        ++stats.groups;
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
        if (units) {
            more_group(c);
            return;
        }
        if (ao && recs)
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
        if (ao) align_group(r0, n_reads, total, recs, cigar, nullptr, nullptr, r0);
    }

    // More chains of the group's reads, right behind k_map_chain: the selections, a scan of the reads' unit counts, the units
    // packed in read order; they come to the host and, when asked for, so do their chains.
    void more_group(const np2::MapChain &c) {
        using namespace np2;
        hipStream_t st = s.st;
        const uint32_t n_reads = c.n_reads;
        const size_t slots = (size_t)n_reads * (mo.max_chains - 1u) + 1;
        d_uh.ensure(slots), d_ucls.ensure(slots), d_upar.ensure(slots), d_uend.ensure(slots);
        d_ucnt.ensure((size_t)n_reads + 1), d_uoff.ensure((size_t)n_reads + 1), d_mctr.ensure(8);
        const size_t scan_tmp = prim_temp_bytes((size_t)n_reads + 1);
        s.tmp.ensure(scan_tmp);
        h_uoff.resize((size_t)n_reads + 1);
        MapMore mm{mo, d_uh.p, d_ucls.p, d_upar.p, d_uend.p, d_ucnt.p, d_mctr.p};
        HIPCHK(hipMemsetAsync(d_mctr.p, 0, 8 * 8, st));
        HIPCHK(hipMemsetAsync(d_ucnt.p + n_reads, 0, 4, st));
        s.begin();
        launch_map_chain_more(st, c, mm);
        if (prim_exclusive_sum_u32(st, s.tmp.p, scan_tmp, d_ucnt.p, d_uoff.p, (size_t)n_reads + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipMemcpyAsync(h_uoff.data(), d_uoff.p, ((size_t)n_reads + 1) * 4, hipMemcpyDeviceToHost, st));
        tl_mstats.more_ms += s.end();
        const uint32_t n_units = h_uoff[n_reads];
        if (n_units < n_reads || (uint64_t)n_units > (uint64_t)n_reads * mo.max_chains) throw Np2Error(NP2_E_DEVICE, "np2_map: unit counts out of range");
        d_phits.ensure((size_t)n_units + 1), d_pcls.ensure((size_t)n_units + 1), d_ppar.ensure((size_t)n_units + 1);
        d_pend.ensure((size_t)n_units + 1), d_pread.ensure((size_t)n_units + 1);
        const MapUnits u{d_uoff.p, d_phits.p, d_pcls.p, d_ppar.p, d_pread.p, d_pend.p};
        const size_t at = units->hits.size();
        units->hits.resize(at + n_units), units->cls.resize(at + n_units), units->parent.resize(at + n_units);
        unsigned long long ctr[8];
        s.begin();
        launch_map_units_pack(st, c, mm, u);
        HIPCHK(hipMemcpyAsync(units->hits.data() + at, d_phits.p, (size_t)n_units * sizeof(Hit), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(units->cls.data() + at, d_pcls.p, n_units, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(units->parent.data() + at, d_ppar.p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ctr, d_mctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
        tl_mstats.more_ms += s.end();
        add_more_counts(tl_mstats, ctr);
        for (uint32_t i = 0; i < n_reads; ++i) units->n_units.push_back(h_uoff[i + 1] - h_uoff[i]);
        if (ao) units->recs.resize(at + n_units, np2aln::unaligned_rec());
        if (ao && tag_flags) units->tt.n_md.resize(at + n_units, 0), units->tt.n_cs.resize(at + n_units, 0);
        if (!unit_chains && !ao) return;
        h_coff.resize(n_units);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n_units; ++i) {
            const Hit &h = units->hits[at + i];
            h_coff[i] = (uint32_t)total, total += h.tid >= 0 ? h.n : 0;
        }
        if (total == 0) return;
        d_coff.ensure(n_units), d_chain.ensure(2 * total);
        const size_t cat = units->chain.size();
        if (unit_chains) units->chain.resize(cat + 2 * total);
        HIPCHK(hipMemcpyAsync(d_coff.p, h_coff.data(), (size_t)n_units * 4, hipMemcpyHostToDevice, st));
        s.begin();
        launch_map_units_export(st, c, u, n_units, d_coff.p, d_chain.p);
        if (unit_chains) HIPCHK(hipMemcpyAsync(units->chain.data() + cat, d_chain.p, 2 * total * 4, hipMemcpyDeviceToHost, st));
        stats.chain_ms += s.end();
        // the aligner serves units as it serves reads: the jobs are the group's units, each with its own hit and chain
        if (ao) align_group(c.r0, n_units, total, units->recs.data(), &units->cigar, d_phits.p, d_pread.p, at);
    }

    // the group's mapped reads, their chains in d_chain at d_coff: recs[r0 + i] and the CIGAR words in read order
    // job_hits, unit_read (both or neither): the jobs are units (np2_align.hpp); out0: the first job's place in recs and the texts
    void align_group(uint32_t r0, uint32_t n_reads, uint64_t total_pairs, np2aln::Rec *recs, std::vector<uint32_t> *cigar, const Hit *job_hits,
                     const uint32_t *unit_read, size_t out0) {
        using namespace np2;
        hipStream_t st = s.st;
        AlignJob c{};
        c.asm_seq = ix.seq.p, c.asm_ends = ix.ends.p, c.rd_seq = sk.d_seq.p + MAP_FRONT, c.rd_ends = sk.d_ends.p;
        c.hits = job_hits ? job_hits : d_hits.p, c.unit_read = unit_read, c.coff = d_coff.p, c.chain = d_chain.p;
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
        std::vector<uint64_t> p_tboff;
        if (probe) { // the slots as k_align_classify left them, and where each matrix's bytes begin
            probe->slots.resize(n_slots), p_tboff.resize((size_t)n_slots + 1);
            if (n_slots) HIPCHK(hipMemcpyAsync(probe->slots.data(), d_slots.p, (size_t)n_slots * sizeof(np2aln::Slot), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(p_tboff.data(), d_tboff.p, ((size_t)n_slots + 1) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            probe->slot_off.assign(h_soff.begin(), h_soff.end()), probe->tb_off = p_tboff;
            if (probe->want_tb) probe->tb.resize(p_tboff[n_slots]);
        }
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
            if (pk) pk->collect();
            if (probe && probe->want_tb && tb_bytes) { // (the buffer is the next sub-group's too)
                HIPCHK(hipMemcpyAsync(probe->tb.data() + tb_base, d_tb.p, tb_bytes, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            }
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
            if (pk) { // the sub-group's records go on into the handle: the sizes now, the pack behind the one wait there is
                s.begin();
                launch_align_ops_emit(st, c, g0, g1, tb_base);
                pk->sizes(c, g0, g1, s.tmp.p, scan_tmp);
                astats.assemble_ms += s.end();
                astats.assemble_ms -= pk->pack();
                g0 = g1;
                continue;
            }
            h_b.resize(n_b + 1);
            s.begin();
            launch_align_ops_emit(st, c, g0, g1, tb_base);
            HIPCHK(hipMemcpyAsync(h_recs.data() + g0, d_recs.p + g0, (size_t)ng * sizeof(np2aln::Rec), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_b.data(), d_b.p, n_b * 4, hipMemcpyDeviceToHost, st));
            astats.assemble_ms += s.end();
            if (tag_flags) { // right behind k_align_ops_emit, whose records and words are still where it left them
                TagJob j{};
                j.c = c, j.g0 = g0, j.from_aligner = 1, j.n = ng, j.flags = tag_flags;
                tl_tstats.tags_ms += tg.run(s, j);
                tl_tstats.md_bytes += tg.md.size(), tl_tstats.cs_bytes += tg.cs.size(), tl_tstats.eqx_words += tg.eqx.size();
            }
            for (uint32_t i = 0; i < ng; ++i) {
                np2aln::Rec rc = h_recs[g0 + i];
                const uint32_t *w = h_b.data() + 2 * (size_t)h_ooff[i] + 2 * (size_t)i;
                if ((tag_flags & NP2_ALN_EQX) && rc.tid >= 0) w = tg.eqx.data() + tg.eqx_off[i], rc.n_cigar = tg.eqx_off[i + 1] - tg.eqx_off[i];
                recs[out0 + g0 + i] = rc;
                if (cigar) cigar->insert(cigar->end(), w, w + rc.n_cigar);
                if (tag_flags && tt) {
                    tt->n_md[out0 + g0 + i] = (uint32_t)(tg.md_off[i + 1] - tg.md_off[i]);
                    tt->n_cs[out0 + g0 + i] = (uint32_t)(tg.cs_off[i + 1] - tg.cs_off[i]);
                }
            }
            if (tag_flags && tt) tt->md.insert(tt->md.end(), tg.md.begin(), tg.md.end()), tt->cs.insert(tt->cs.end(), tg.cs.begin(), tg.cs.end());
            g0 = g1;
        }
        if (n_sub > 1) stats.groups += n_sub - 1;
        if (probe) { // a slot without a matrix has no cell: k_align_dp wrote none
            probe->res.resize(n_slots);
            if (n_slots) HIPCHK(hipMemcpyAsync(probe->res.data(), d_res.p, (size_t)n_slots * sizeof(np2aln::Res), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (uint32_t i = 0; i < n_slots; ++i)
                if (p_tboff[i + 1] == p_tboff[i]) probe->res[i] = np2aln::Res{};
        }
        unsigned long long ctr[np2aln::C_N];
        HIPCHK(hipMemcpyAsync(ctr, d_actr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (pk) pk->collect();
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
    std::vector<uint8_t> qual; // NP2_ALN_QUAL: n bytes beside the piece's, '\n' where it has one; 0xFF for a read without qualities
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
            p.ends.clear(), p.names.clear(), p.qual.clear();
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
    // NP2_ALN_QUAL: n bytes and the n quality bytes beside them (ql null: 0xFF, a read without qualities), cut at the same
    // places; a separator is its own call with one beside it
    void put_pair(const uint8_t *p, const uint8_t *ql, size_t n) {
        while (n && !w.dead) {
            if (!w.cur && !w.fresh()) return;
            const size_t take_n = std::min(n, w.cap - w.cur->n);
            if (ql) w.cur->qual.insert(w.cur->qual.end(), ql, ql + take_n), ql += take_n;
            else w.cur->qual.insert(w.cur->qual.end(), take_n, (uint8_t)0xFF);
            put(p, take_n); // (fills the piece at the most: one piece takes it)
            p += take_n, n -= take_n;
        }
    }
};

// One file's records with NP2_ALN_QUAL.  A FASTQ record's sequence waits for its quality line, which is checked (as long as
// the sequence, every byte in '!' .. '~'; NP2_E_ARG names the file and the 1-based record), and the two go into the pieces
// together; a FASTA or one-sequence-per-line file's reads have no qualities.
void parse_with_qual(const std::string &path, MapWriter &w) {
    np2seq::SeqParser ps;
    np2seq::RecordCheck chk;
    chk.file_begin(path);
    std::vector<uint8_t> seq, ql;
    const auto put = [&](const uint8_t *p, size_t n) {
        if (ps.fmt != np2seq::SeqParser::FASTQ) {
            const bool sep = n == 1 && *p == SEP;
            w.put_pair(p, sep ? &SEP : nullptr, n);
        } else if (n == 1 && *p == SEP) {
            chk.seq_end();
        } else {
            if (seq.size() + n > np2map::MAX_SEQ) throw Np2Error(NP2_E_UNSUPPORTED, "np2_map_align_files_x: a read longer than 2^31 - 1");
            chk.seq_bytes(n), seq.insert(seq.end(), p, p + n);
        }
    };
    const auto qual = [&](const uint8_t *p, size_t n) {
        if (n == 1 && *p == SEP) {
            chk.qual_end();
            if (!seq.empty()) w.put_pair(seq.data(), ql.data(), seq.size());
            w.put_pair(&SEP, &SEP, 1);
            seq.clear(), ql.clear();
            return;
        }
        chk.qual_bytes(n);
        for (size_t i = 0; i < n; ++i)
            if (p[i] < '!' || p[i] > '~')
                throw Np2Error(NP2_E_ARG, path + ": record " + std::to_string(chk.record + 1) + ": the quality line holds a byte outside '!' .. '~'");
        ql.insert(ql.end(), p, p + n);
    };
    const auto hdr = [&](const uint8_t *p, size_t n, bool begin) { w.names(p, n, begin); };
    if (np2seq::read_chunks(path, [&] { return w.w.dead; }, [&](const uint8_t *p, size_t n) { ps.feed(p, n, put, hdr, qual); })) {
        ps.finish(put, qual);
        chk.file_end();
    }
}

// whole reads gathered from pieces; what follows the last separator waits for the next piece
struct BatchBuf {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> ends;
    std::string names;
    std::vector<uint8_t> quals; // NP2_ALN_QUAL: beside bytes
    bool with_qual = false;
    void add(const MapPiece &p) {
        const size_t at = bytes.size();
        if (at + p.n > MAP_MAX_STREAM) throw Np2Error(NP2_E_UNSUPPORTED, "np2_map_files: a batch of 2^32 bytes or more");
        bytes.insert(bytes.end(), p.buf + np2h::HALO, p.buf + np2h::HALO + p.n);
        for (uint32_t e : p.ends) ends.push_back((uint32_t)(at + e));
        names += p.names;
        if (with_qual) {
            if (p.qual.size() != p.n) throw Np2Error(NP2_E_DEVICE, "np2_map_align_files_x: a piece's quality bytes do not line up with its bases");
            quals.insert(quals.end(), p.qual.begin(), p.qual.end());
        }
    }
    size_t closed() const { return ends.empty() ? 0 : (size_t)ends.back() + 1; }
    void drop_closed() {
        if (with_qual) quals.erase(quals.begin(), quals.begin() + (ptrdiff_t)closed());
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

// tt (may be null): the batch's MD and cs texts; b.quals, when the batch has them, become QUAL
void write_sam(np2h::OutFile &out, const np2_map_index &ix, const BatchBuf &b, const std::vector<Hit> &hits, const std::vector<np2aln::Rec> &recs,
               const std::vector<uint32_t> &cigar, std::string &text, const TagTexts *tt = nullptr) {
    text.clear();
    size_t name_at = 0, cig_at = 0, from = 0, md_at = 0, cs_at = 0;
    for (size_t i = 0; i < b.ends.size(); ++i) {
        const size_t name_end = b.names.find('\n', name_at);
        const np2aln::Rec &rc = recs[i];
        const uint32_t qlen = (uint32_t)(b.ends[i] - from);
        if (!tt && !b.with_qual) {
            np2aln::sam_line(text, b.names.data() + name_at, name_end - name_at, rc, hits[i], cigar.data() + cig_at, b.bytes.data() + from, qlen,
                             rc.tid >= 0 ? &ix.names[(size_t)rc.tid] : nullptr);
        } else {
            np2aln::SamExtra x{};
            if (b.with_qual && qlen && b.quals[from] != 0xFF) x.qual = b.quals.data() + from, ++tl_tstats.qual_reads;
            if (tt) x.md = tt->md.data() + md_at, x.n_md = tt->n_md[i], x.cs = tt->cs.data() + cs_at, x.n_cs = tt->n_cs[i];
            np2aln::sam_line_x(text, b.names.data() + name_at, name_end - name_at, rc, hits[i], cigar.data() + cig_at, b.bytes.data() + from, qlen,
                               rc.tid >= 0 ? &ix.names[(size_t)rc.tid] : nullptr, x);
            md_at += x.n_md, cs_at += x.n_cs;
        }
        cig_at += rc.n_cigar, name_at = name_end + 1, from = (size_t)b.ends[i] + 1;
    }
    out.put(text.data(), text.size());
}

// the read files of a call, each opened once before the first device call
std::vector<std::string> checked_files(const char *const *paths, int n_paths, const std::string &who) {
    if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no read file given");
    std::vector<std::string> files;
    for (int i = 0; i < n_paths; ++i) {
        if (!paths[i]) throw Np2Error(NP2_E_ARG, who + ": a read file path is NULL");
        FILE *f = fopen(paths[i], "rb");
        if (!f) throw Np2Error(NP2_E_ARG, who + ": cannot open " + paths[i]);
        fclose(f);
        files.push_back(paths[i]);
    }
    return files;
}

// The files' reads in file order as batches of whole reads, hooks.batch_bytes() at the most (a file's last batch may be
// smaller): flush(b) works a batch off, its closed reads are dropped afterwards.  Reader threads parse ahead.
// with_qual (NP2_ALN_QUAL): the batches carry the reads' quality bytes beside their bases.
template <class Flush>
void read_batches(const std::vector<std::string> &files, const Hooks &hooks, const std::string &who, Flush &&flush, bool with_qual = false) {
    const size_t cap = hooks.piece;
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
            if (with_qual)
                parse_with_qual(files[fi], w);
            else
                np2seq::parse_file(files[fi], [&](const uint8_t *p, size_t n) { w.put(p, n); }, [&] { return w.w.dead; },
                                   [&](const uint8_t *p, size_t n, bool begin) { w.names(p, n, begin); });
            w.finish();
            if (w.w.dead) break;
        }
    });
    BatchBuf b;
    b.with_qual = with_qual;
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
            if ((b.closed() >= hooks.batch_bytes() || last) && !b.ends.empty()) { // (a file's last read ends with its separator)
                flush(b);
                b.drop_closed();
            }
        }
    }
}

// np2_map_files (aopts null: PAF) and np2_map_align_files (SAM)
int map_files_impl(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const np2_align_opts_t *aopts,
                   bool align, const char *out_path, np2_map_stats_t *stats, const std::string who, uint32_t out_flags = 0) {
    return np2h::abi_guard([&] {
        const np2map::Opts o = checked(opts, who.c_str());
        np2aln::Opts ao{};
        if (align) ao = checked_align(aopts, who.c_str());
        checked_out_flags(out_flags, NP2_ALN_QUAL | NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, who);
        tl_tstats = np2_align_tag_stats_t{};
        const uint32_t tag_flags = out_flags & ~(uint32_t)NP2_ALN_QUAL;
        const bool with_qual = (out_flags & NP2_ALN_QUAL) != 0;
        TagTexts tt;
        check_index_opts(ix, o, who.c_str());
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no read file given");
        if (!out_path) throw Np2Error(NP2_E_ARG, who + ": out_path is NULL");
        const std::vector<std::string> files = checked_files(paths, n_paths, who);
        Mapper m(*ix, o);
        if (align) m.align_with(ao);
        m.tag_flags = tag_flags;
        if (tag_flags) m.tt = &tt;
        np2h::OutFile out;
        out.open(out_path, ix->device);
        std::vector<Hit> hits;
        std::string text;
        std::vector<np2aln::Rec> recs;
        std::vector<uint32_t> cigar;
        if (align) {
            np2aln::sam_header(text, ix->names, ix->lens);
            out.put(text.data(), text.size());
        }
        read_batches(files, m.hooks, who, [&](const BatchBuf &b) {
            hits.resize(b.ends.size());
            if (align) recs.resize(b.ends.size()), cigar.clear();
            if (tag_flags) tt.begin(b.ends.size());
            m.batch(b.bytes.data(), b.closed(), b.ends.data(), (uint32_t)b.ends.size(), hits.data(), nullptr, align ? recs.data() : nullptr,
                    align ? &cigar : nullptr);
            const auto t0 = std::chrono::steady_clock::now();
            if (align) write_sam(out, *ix, b, hits, recs, cigar, text, tag_flags ? &tt : nullptr);
            else write_paf(out, *ix, b, hits, text);
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            tl_stats.write_ms += ms;
            if (align) tl_astats.write_ms += ms;
        }, with_qual);
        out.close();
        fill_stats(stats);
        return NP2_OK;
    }, np2h::io_set_error);
}

// ---- np2_sam_from_reads, np2_sam_from_read_bytes: the aligner's records into a resident SAM handle -----------------------------
// What both check before the first device call, in this order: the options as np2_map_align_* do, then the rest.
struct FromReads {
    np2map::Opts o;
    np2aln::Opts ao;
    uint32_t tie;
    bool keep_names;
    FromReads(np2_ctx *cx, const np2_map_index_t *ix, const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_sam_opts_t *sam_opts,
              uint32_t flags, np2_sam_t **out, const char *who) {
        o = checked(map_opts, who);
        ao = checked_align(align_opts, who);
        check_index_opts(ix, o, who);
        if (!cx || !out) throw Np2Error(NP2_E_ARG, std::string(who) + ": NULL argument");
        if (flags & ~(uint32_t)(NP2_SAM_KEEP_NAMES | NP2_SAM_KEEP_ALL)) throw Np2Error(NP2_E_ARG, std::string(who) + ": unknown flag bits");
        if (flags & NP2_SAM_KEEP_ALL)
            throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": NP2_SAM_KEEP_ALL needs the SAM text (its NM, AS, cm, s1 and s2 fields are not kept "
                                              "as binary tails here): write it with `map -a -o map.sam.gz`, then `samsort --full`");
        if (ix->device != cx->device) throw Np2Error(NP2_E_ARG, std::string(who) + ": the index is on another device than the context");
        std::vector<std::string> sorted_names(ix->names);
        std::sort(sorted_names.begin(), sorted_names.end());
        const auto twice = std::adjacent_find(sorted_names.begin(), sorted_names.end());
        if (twice != sorted_names.end()) throw Np2Error(NP2_E_ARG, std::string(who) + ": the @SQ name " + *twice + " is given twice");
        tie = sam_opts ? (sam_opts->tie_by_strand ? 1u : 0u) : 1u;
        keep_names = (flags & NP2_SAM_KEEP_NAMES) != 0;
    }
};

// the mapper, the sink and the handle of one call; batches go in through batch(), finish() sorts and hands the handle over
struct FromReadsRun {
    std::unique_ptr<np2_sam> sam;
    Mapper m;
    PackSink pk;
    std::vector<Hit> hits;
    FromReadsRun(np2_ctx *cx, const np2_map_index_t *ix, const FromReads &a) : sam(new np2_sam()), m(*ix, a.o), pk(*sam, m.s.st, a.keep_names, a.tie) {
        sam->device = cx->device;
        for (size_t i = 0; i < ix->names.size(); ++i) sam->refs.names.push_back(ix->names[i]), sam->refs.lens.push_back((uint32_t)ix->lens[i]);
        m.align_with(a.ao);
        m.pk = &pk;
    }
    void batch(const uint8_t *bytes, uint64_t n, const uint32_t *ends, uint32_t n_reads, const char *names, size_t names_n) {
        hits.resize(n_reads);
        pk.begin_batch(names, names_n, n_reads);
        m.batch(bytes, n, ends, n_reads, hits.data(), nullptr, nullptr, nullptr);
        pk.end_batch();
    }
    np2_sam_t *finish() {
        pk.acc.finish();
        np2_sam_stats_t &st = sam->stats;
        st.lines = st.records + sam->refs.names.size() + 2; // (as the text would have: @HD, the @SQ lines, @PG, a line a read)
        st.parse_ms = 0.f, st.pack_ms = pk.pack_ms, st.read_ms = tl_stats.read_ms;
        return sam.release();
    }
};

// ---- the opt-in outputs' doors -------------------------------------------------------------------------------------------------
char *text_out(const std::vector<char> &t) { // a malloc block for the caller (np2_free); never NULL
    char *p = (char *)malloc(std::max<size_t>(t.size(), 1));
    if (!p) throw Np2Error(NP2_E_NOMEM, "out of memory for the tag texts");
    if (!t.empty()) memcpy(p, t.data(), t.size());
    return p;
}

// md / md_off and cs / cs_off of an _x call: each pair both or neither, and there when its flag asks for it
void check_tag_pairs(uint32_t flags, char **md, uint64_t *md_off, char **cs, uint64_t *cs_off, const std::string &who) {
    if (md) *md = nullptr;
    if (cs) *cs = nullptr;
    if ((md == nullptr) != (md_off == nullptr)) throw Np2Error(NP2_E_ARG, who + ": md and md_off go together");
    if ((cs == nullptr) != (cs_off == nullptr)) throw Np2Error(NP2_E_ARG, who + ": cs and cs_off go together");
    if ((flags & NP2_ALN_MD) && !md) throw Np2Error(NP2_E_ARG, who + ": NP2_ALN_MD without md and md_off");
    if ((flags & NP2_ALN_CS) && !cs) throw Np2Error(NP2_E_ARG, who + ": NP2_ALN_CS without cs and cs_off");
}

void offsets_of(const std::vector<uint32_t> &n, uint64_t *off) { // off[0 .. n.size()]
    off[0] = 0;
    for (size_t i = 0; i < n.size(); ++i) off[i + 1] = off[i] + n[i];
}

// a quality stream beside a read stream: the same length and separators; a read has none (its first byte 0xFF) or every byte in
// '!' .. '~'.  Returns the reads that have qualities.
uint64_t check_quals(const uint8_t *quals, const std::vector<uint64_t> &ends, const std::string &who) {
    uint64_t from = 0, have = 0;
    for (size_t i = 0; i < ends.size(); ++i) {
        if (quals[ends[i]] != SEP) throw Np2Error(NP2_E_ARG, who + ": read " + std::to_string(i + 1) + ": the quality stream has no newline where the read ends");
        if (ends[i] > from && quals[from] != 0xFF) {
            for (uint64_t x = from; x < ends[i]; ++x)
                if (quals[x] < '!' || quals[x] > '~')
                    throw Np2Error(NP2_E_ARG, who + ": read " + std::to_string(i + 1) + ": a quality byte outside '!' .. '~'");
            ++have;
        }
        from = ends[i] + 1;
    }
    return have;
}

// np2_align_tags_host, np2_align_tags_device: what both check before any walk
struct TagDoor {
    uint32_t flags;
    uint64_t n_words = 0;
    TagDoor(const uint8_t *ref, uint64_t n_ref, const uint8_t *reads, uint64_t n_read_bytes, uint64_t n_recs, const uint64_t *t_off, const uint64_t *q_off,
            const uint32_t *cigar, const uint64_t *cigar_off, uint32_t out_flags, char **md, uint64_t *md_off, char **cs, uint64_t *cs_off, uint32_t **eqx,
            uint64_t *eqx_off, const std::string &who) {
        flags = checked_out_flags(out_flags, NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, who);
        check_tag_pairs(flags, md, md_off, cs, cs_off, who);
        if (eqx) *eqx = nullptr;
        if ((eqx == nullptr) != (eqx_off == nullptr)) throw Np2Error(NP2_E_ARG, who + ": eqx and eqx_off go together");
        if ((flags & NP2_ALN_EQX) && !eqx) throw Np2Error(NP2_E_ARG, who + ": NP2_ALN_EQX without eqx and eqx_off");
        if ((n_ref && !ref) || (n_read_bytes && !reads)) throw Np2Error(NP2_E_ARG, who + ": a buffer is NULL with a length");
        if (n_recs && (!t_off || !q_off)) throw Np2Error(NP2_E_ARG, who + ": t_off or q_off is NULL");
        if (!cigar_off) throw Np2Error(NP2_E_ARG, who + ": cigar_off is NULL");
        if (n_recs >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, who + ": 2^31 records or more");
        uint64_t eqx_bound = 0;
        for (uint64_t i = 0; i < n_recs; ++i) {
            const std::string rec = who + ": record " + std::to_string(i);
            if (cigar_off[i + 1] < cigar_off[i]) throw Np2Error(NP2_E_ARG, rec + ": cigar_off is descending");
            const uint64_t nw = cigar_off[i + 1] - cigar_off[i];
            if (nw && !cigar) throw Np2Error(NP2_E_ARG, who + ": cigar is NULL with words");
            uint64_t ts = 0, qs = 0;
            if (!np2aln::tag_cigar_spans(cigar + cigar_off[i], nw, &ts, &qs)) throw Np2Error(NP2_E_ARG, rec + ": a CIGAR word that is not M, I, D or S");
            if (nw >= (1ull << 28) || ts >= (1ull << 30) || qs >= (1ull << 30)) throw Np2Error(NP2_E_UNSUPPORTED, rec + ": 2^30 columns or more");
            if (t_off[i] > n_ref || ts > n_ref - t_off[i]) throw Np2Error(NP2_E_ARG, rec + ": its columns reach beyond the reference buffer");
            if (q_off[i] > n_read_bytes || qs > n_read_bytes - q_off[i]) throw Np2Error(NP2_E_ARG, rec + ": its columns reach beyond the read buffer");
            eqx_bound += nw + ts;
        }
        n_words = n_recs ? cigar_off[n_recs] - cigar_off[0] : 0;
        if (eqx_bound >= (1ull << 32)) throw Np2Error(NP2_E_UNSUPPORTED, who + ": 2^32 columns or more in one call");
    }
};

template <class Body> int from_reads_guard(np2_ctx *cx, bool &touched, Body &&body) {
    return np2h::abi_guard(body, [&](int code, const std::string &msg) {
        if (touched) cx->err = msg; // (the call's own stream was drained when its PackSink went: the context's was never used)
        np2h::io_set_error(code, msg);
    });
}

} // namespace

extern "C" {

int np2_map_weights_from_indices(uint32_t k, const uint32_t *index, uint64_t n, np2_map_weights_t **out) {
    return np2h::abi_guard([&] {
        const char *who = "np2_map_weights_from_indices";
        if (!out) throw Np2Error(NP2_E_ARG, std::string(who) + ": out is NULL");
        *out = nullptr;
        if (n && !index) throw Np2Error(NP2_E_ARG, std::string(who) + ": index is NULL with a length");
        if (n) check_weights_k(k, who);
        std::unique_ptr<np2_map_weights> w(new np2_map_weights());
        if (n) {
            const uint64_t mask = np2map::kmer_mask(k);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t v = index[i];
                if (v > mask) throw Np2Error(NP2_E_ARG, std::string(who) + ": index[" + std::to_string(i) + "] = " + std::to_string(v) + " is beyond 4^k - 1");
                if (revcomp_index(v, k) < v)
                    throw Np2Error(NP2_E_ARG, std::string(who) + ": index[" + std::to_string(i) + "] = " + std::to_string(v) +
                                                  " is not canonical (its reverse complement is smaller)");
            }
            w->ws.idx.assign(index, index + n);
            seal_weights(w->ws, k);
        }
        *out = w.release();
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_weights_from_file(const char *path, np2_map_weights_t **out) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_weights_from_file";
        if (!out) throw Np2Error(NP2_E_ARG, who + ": out is NULL");
        *out = nullptr;
        if (!path) throw Np2Error(NP2_E_ARG, who + ": path is NULL");
        std::unique_ptr<np2_map_weights> w(new np2_map_weights());
        // a line: KMER or KMER<TAB>anything, ended by \n or \r\n (a last line may go without)
        uint64_t line_no = 1, fw = 0, rv = 0;
        uint32_t len = 0, k = 0;
        bool in_kmer = true, any = false; // any: the line has a byte
        auto bad = [&](const std::string &what) { return Np2Error(NP2_E_ARG, who + ": " + path + ": line " + std::to_string(line_no) + ": " + what); };
        auto end_line = [&] {
            if (k == 0) {
                if (len < 1 || len > 31) throw bad("a k-mer of 1 .. 31 letters is expected");
                k = len;
                check_weights_k(k, who.c_str());
            } else if (len != k) {
                throw bad("a k-mer of " + std::to_string(len) + " letters, the lines before have " + std::to_string(k));
            }
            w->ws.idx.push_back((uint32_t)std::min(fw, rv >> (62u - 2u * len)));
            fw = rv = 0, len = 0, in_kmer = true, any = false, ++line_no;
        };
        np2seq::read_chunks(path, nullptr, [&](const uint8_t *p, size_t m) {
            for (size_t i = 0; i < m; ++i) {
                const uint8_t ch = p[i];
                if (ch == '\n') {
                    end_line();
                    continue;
                }
                any = true;
                if (!in_kmer) continue;
                if (ch == '\t') {
                    in_kmer = false;
                    continue;
                }
                if (ch == '\r' && (i + 1 < m ? p[i + 1] == '\n' : true)) { // (a lone \r at a chunk's end is taken for a line end too)
                    in_kmer = false;
                    continue;
                }
                const uint32_t c = np2map::code(ch == 'U' || ch == 'u' ? (uint8_t)'T' : ch);
                if (c >= 4u) throw bad("a letter that is not one of ACGTU");
                if (++len > 31) throw bad("a k-mer of more than 31 letters");
                fw = fw << 2 | c, rv = rv >> 2 | (uint64_t)(3u - c) << 60;
            }
        });
        if (any) end_line();
        if (!w->ws.idx.empty()) seal_weights(w->ws, k);
        *out = w.release();
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_weights_info(const np2_map_weights_t *w, uint32_t *k, uint64_t *n_listed) {
    if (!w) return np2h::io_set_error(NP2_E_ARG, "np2_map_weights_info: the weights are NULL");
    if (k) *k = w->ws.k;
    if (n_listed) *n_listed = w->ws.idx.size();
    return NP2_OK;
}

void np2_map_weights_free(np2_map_weights_t *w) { delete w; }

static int index_bytes_impl(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts, const np2_map_weights_t *w,
                            np2_map_index_t **out, const std::string who) {
    return np2h::abi_guard([&] {
        // every argument is checked before the first device call
        if (!out) throw Np2Error(NP2_E_ARG, who + ": out is NULL");
        *out = nullptr;
        const np2map::Opts o = checked(opts, who.c_str());
        const np2map::WeightSet *ws = checked_weights(w, o, who.c_str());
        std::vector<std::string> nm;
        if (names)
            for (const char *p = names; *p;) {
                const char *e = strchr(p, '\n');
                if (!e) throw Np2Error(NP2_E_ARG, who + ": names does not end in a newline");
                nm.emplace_back(p, e), p = e + 1;
            }
        *out = build_index(device, stream, n, std::move(nm), o, who.c_str(), ws);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_map_index_bytes(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts, np2_map_index_t **out) {
    return index_bytes_impl(device, stream, n, names, opts, nullptr, out, "np2_map_index_bytes");
}
int np2_map_index_bytes_w(int device, const uint8_t *stream, uint64_t n, const char *names, const np2_map_opts_t *opts, const np2_map_weights_t *w,
                          np2_map_index_t **out) {
    return index_bytes_impl(device, stream, n, names, opts, w, out, "np2_map_index_bytes_w");
}

static int index_files_impl(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const np2_map_weights_t *w,
                            np2_map_index_t **out, const std::string who) {
    return np2h::abi_guard([&] {
        if (!out) throw Np2Error(NP2_E_ARG, who + ": out is NULL");
        *out = nullptr;
        const np2map::Opts o = checked(opts, who.c_str());
        const np2map::WeightSet *ws = checked_weights(w, o, who.c_str());
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no assembly file given");
        for (int i = 0; i < n_paths; ++i)
            if (!paths[i]) throw Np2Error(NP2_E_ARG, who + ": an assembly file path is NULL");
        std::vector<uint8_t> stream;
        std::vector<std::string> names;
        for (int i = 0; i < n_paths; ++i) {
            np2seq::NameCollector nc;
            np2seq::parse_file(paths[i], [&](const uint8_t *p, size_t m) {
                if (m == 1 && *p == SEP) names.push_back(nc.close());
                if (stream.size() + m > MAP_MAX_STREAM) throw Np2Error(NP2_E_UNSUPPORTED, who + ": an assembly of 2^32 bytes or more");
                stream.insert(stream.end(), p, p + m);
            }, nullptr, [&](const uint8_t *p, size_t m, bool begin) { nc(p, m, begin); });
        }
        *out = build_index(device, stream.data(), stream.size(), std::move(names), o, who.c_str(), ws);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_map_index_files(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, np2_map_index_t **out) {
    return index_files_impl(device, paths, n_paths, opts, nullptr, out, "np2_map_index_files");
}
int np2_map_index_files_w(int device, const char *const *paths, int n_paths, const np2_map_opts_t *opts, const np2_map_weights_t *w,
                          np2_map_index_t **out) {
    return index_files_impl(device, paths, n_paths, opts, w, out, "np2_map_index_files_w");
}

int np2_map_index_weights(const np2_map_index_t *ix, uint32_t *k, uint64_t *n_listed) {
    if (!ix) return np2h::io_set_error(NP2_E_ARG, "np2_map_index_weights: the index is NULL");
    if (k) *k = ix->weights_k;
    if (n_listed) *n_listed = ix->n_listed;
    return NP2_OK;
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

static int map_host_impl(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                         const np2_map_weights_t *w, np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off, const std::string name) {
    return np2h::abi_guard([&] {
        const char *who = name.c_str();
        if (chain) *chain = nullptr;
        const np2map::Opts o = checked(opts, who);
        const np2map::WeightSet *ws = checked_weights(w, o, who);
        if (n_reads && !hits) throw Np2Error(NP2_E_ARG, name + ": hits is NULL");
        if ((chain == nullptr) != (chain_off == nullptr)) throw Np2Error(NP2_E_ARG, name + ": chain and chain_off go together");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, who, "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, who, "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, name + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w, ws);
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
int np2_map_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                 np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off) {
    return map_host_impl(asm_stream, n_asm, reads, n, n_reads, opts, nullptr, hits, chain, chain_off, "np2_map_host");
}
int np2_map_host_w(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                   const np2_map_weights_t *w, np2_map_hit_t *hits, uint32_t **chain, uint64_t *chain_off) {
    return map_host_impl(asm_stream, n_asm, reads, n, n_reads, opts, w, hits, chain, chain_off, "np2_map_host_w");
}

// ---- More chains: the _m doors ------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
struct Freed {
    void *p = nullptr;
    ~Freed() { free(p); }
    void *release() {
        void *r = p;
        p = nullptr;
        return r;
    }
};
template <class T> void malloc_copy(Freed &f, const T *src, size_t n) { // never NULL
    f.p = malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (!f.p) throw Np2Error(NP2_E_NOMEM, "out of memory for the units");
    if (n) memcpy(f.p, src, n * sizeof(T));
}

// unit_off[n_reads + 1] of the caller's from the units' per-read counts
void fill_unit_off(const Units &u, uint64_t n_reads, uint64_t *unit_off) {
    unit_off[0] = 0;
    for (uint64_t i = 0; i < n_reads; ++i) unit_off[i + 1] = unit_off[i] + u.n_units[i];
}

struct UnitDoor { // the outputs the _bytes_m and _host_m doors share, checked and nulled first
    uint64_t *unit_off;
    np2_map_hit_t **hits;
    uint8_t **cls;
    uint32_t **parent, **chain;
    uint64_t **chain_off;
    void null_all() const {
        for (void **p : {(void **)hits, (void **)cls, (void **)parent, (void **)chain, (void **)chain_off})
            if (p) *p = nullptr;
    }
    void check(const std::string &who) const {
        if (!unit_off || !hits || !cls || !parent) throw Np2Error(NP2_E_ARG, who + ": unit_off, hits, cls and parent are outputs: none may be NULL");
        if ((chain == nullptr) != (chain_off == nullptr)) throw Np2Error(NP2_E_ARG, who + ": chain and chain_off go together");
    }
    void give(const Units &u, uint64_t n_reads) const {
        if (u.n_units.size() != n_reads) throw Np2Error(NP2_E_DEVICE, "np2_map: the units do not cover the reads");
        const size_t n = u.hits.size();
        Freed fh, fc, fp, fch, fco;
        malloc_copy(fh, u.hits.data(), n), malloc_copy(fc, u.cls.data(), n), malloc_copy(fp, u.parent.data(), n);
        if (chain) {
            std::vector<uint64_t> off(n + 1, 0);
            for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (u.hits[i].tid >= 0 ? u.hits[i].n : 0);
            if (2 * off[n] != u.chain.size()) throw Np2Error(NP2_E_DEVICE, "np2_map: the units' chains do not add up");
            malloc_copy(fch, u.chain.data(), u.chain.size()), malloc_copy(fco, off.data(), n + 1);
        }
        fill_unit_off(u, n_reads, unit_off);
        *hits = (np2_map_hit_t *)fh.release(), *cls = (uint8_t *)fc.release(), *parent = (uint32_t *)fp.release();
        if (chain) *chain = (uint32_t *)fch.release(), *chain_off = (uint64_t *)fco.release();
        tl_mstats.units = n;
    }
};

// a batch's PAF lines per unit: a read's primary line is np2_map_files', the kept others follow it
void write_paf_units(np2h::OutFile &out, const np2_map_index &ix, const BatchBuf &b, const Units &u, std::string &text) {
    text.clear();
    size_t name_at = 0, at = 0;
    for (size_t i = 0; i < b.ends.size(); ++i) {
        const size_t name_end = b.names.find('\n', name_at);
        for (uint32_t t = 0; t < u.n_units[i]; ++t, ++at) {
            const Hit &h = u.hits[at];
            if (h.tid >= 0)
                np2map::paf_line(text, b.names.data() + name_at, name_end - name_at, h, ix.names[(size_t)h.tid], ix.lens[(size_t)h.tid],
                                 u.cls[at] == np2map::CLS_SEC ? 'S' : 'P');
        }
        name_at = name_end + 1;
    }
    out.put(text.data(), text.size());
}
} // namespace
} // extern "C++"

int np2_map_bytes_m(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                    const np2_map_multi_opts_t *multi, uint64_t *unit_off, np2_map_hit_t **hits, uint8_t **cls, uint32_t **parent,
                    uint32_t **chain, uint64_t **chain_off) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_bytes_m";
        const UnitDoor door{unit_off, hits, cls, parent, chain, chain_off};
        door.null_all();
        const np2map::Opts o = checked(opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        check_index_opts(ix, o, who.c_str());
        door.check(who);
        const std::vector<uint64_t> ends = ends_of(reads, n, who.c_str(), "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, who + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        tl_mstats = np2_map_multi_stats_t{};
        Mapper m(*ix, o);
        Units u;
        if (mo.max_chains > 1) m.more_with(mo, &u, chain != nullptr);
        std::vector<uint32_t> local;
        std::vector<Hit> prim(n_reads);
        for (uint64_t r0 = 0; r0 < n_reads;) { // np2_map_bytes' batches
            const uint64_t from = r0 ? ends[r0 - 1] + 1 : 0;
            uint64_t r1 = r0 + 1;
            while (r1 < n_reads && ends[r1] + 1 - from <= m.hooks.batch_bytes()) ++r1;
            local.clear();
            for (uint64_t i = r0; i < r1; ++i) local.push_back((uint32_t)(ends[i] - from));
            m.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), prim.data() + r0,
                    mo.max_chains == 1 && chain ? &u.chain : nullptr);
            r0 = r1;
        }
        if (mo.max_chains == 1) u.add_plain(prim.data(), n_reads);
        door.give(u, n_reads);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_files_m(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *opts,
                    const np2_map_multi_opts_t *multi, const char *out_path, np2_map_stats_t *stats) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_files_m";
        const np2map::Opts o = checked(opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        check_index_opts(ix, o, who.c_str());
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no read file given");
        if (!out_path) throw Np2Error(NP2_E_ARG, who + ": out_path is NULL");
        const std::vector<std::string> files = checked_files(paths, n_paths, who);
        tl_mstats = np2_map_multi_stats_t{};
        Mapper m(*ix, o);
        Units u;
        if (mo.max_chains > 1) m.more_with(mo, &u, false);
        np2h::OutFile out;
        out.open(out_path, ix->device);
        std::vector<Hit> hits;
        std::string text;
        read_batches(files, m.hooks, who, [&](const BatchBuf &b) {
            hits.resize(b.ends.size());
            u.clear();
            m.batch(b.bytes.data(), b.closed(), b.ends.data(), (uint32_t)b.ends.size(), hits.data(), nullptr);
            if (mo.max_chains == 1) u.add_plain(hits.data(), hits.size());
            tl_mstats.units += u.hits.size();
            const auto t0 = std::chrono::steady_clock::now();
            write_paf_units(out, *ix, b, u, text);
            tl_stats.write_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
        out.close();
        fill_stats(stats);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_host_m(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *opts,
                   const np2_map_multi_opts_t *multi, const np2_map_weights_t *w, uint64_t *unit_off, np2_map_hit_t **hits, uint8_t **cls,
                   uint32_t **parent, uint32_t **chain, uint64_t **chain_off) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_host_m";
        const UnitDoor door{unit_off, hits, cls, parent, chain, chain_off};
        door.null_all();
        const np2map::Opts o = checked(opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        const np2map::WeightSet *ws = checked_weights(w, o, who.c_str());
        door.check(who);
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, who.c_str(), "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, who.c_str(), "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, who + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w, ws);
        np2_map_stats_t &st = tl_stats;
        st = np2_map_stats_t{};
        st.index_minimizers = hx.mz.size();
        tl_mstats = np2_map_multi_stats_t{};
        Units u;
        np2map::ReadCounts rc;
        np2map::MoreCounts mc{};
        Hit uh[np2map::MAX_CHAINS];
        uint32_t ucls[np2map::MAX_CHAINS], upar[np2map::MAX_CHAINS];
        uint64_t from = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint32_t nu = np2map::map_read_m(hx, reads + from, (uint32_t)(ends[i] - from), o, mo, uh, ucls, upar, chain ? &u.chain : nullptr, &rc, &mc);
            ++(uh[0].tid >= 0 ? st.mapped : st.unmapped);
            u.n_units.push_back(nu);
            for (uint32_t t = 0; t < nu; ++t) u.hits.push_back(uh[t]), u.cls.push_back((uint8_t)ucls[t]), u.parent.push_back(upar[t]);
            from = ends[i] + 1;
        }
        st.reads = n_reads, st.minimizers = rc.minimizers, st.anchors = rc.anchors, st.dropped_occ = rc.dropped_occ;
        const unsigned long long c[5] = {mc.selections, mc.dropped_cnt, mc.dropped_pri, mc.kept_supp, mc.kept_sec};
        add_more_counts(tl_mstats, c);
        door.give(u, n_reads);
        return NP2_OK;
    }, np2h::io_set_error);
}

// ---- More chains, aligned: np2_map_align_*_m ---------------------------------------------------------------------------------
extern "C++" {
namespace {
// a batch's SAM lines per settled unit (np2aln::sam_units_of_read), a read after the other
void write_sam_units(np2h::OutFile &out, const np2_map_index &ix, const BatchBuf &b, const Units &u, std::string &text, bool tags) {
    text.clear();
    size_t name_at = 0, from = 0;
    np2aln::UnitAt at;
    for (size_t i = 0; i < b.ends.size(); ++i) {
        const size_t name_end = b.names.find('\n', name_at);
        const uint32_t qlen = (uint32_t)(b.ends[i] - from);
        const uint8_t *qual = nullptr;
        if (b.with_qual && qlen && b.quals[from] != 0xFF) qual = b.quals.data() + from, ++tl_tstats.qual_reads;
        np2aln::sam_units_of_read(text, b.names.data() + name_at, name_end - name_at, b.bytes.data() + from, qlen, qual, u, u.n_units[i], tags, ix.names, at);
        name_at = name_end + 1, from = (size_t)b.ends[i] + 1;
    }
    out.put(text.data(), text.size());
}

// with max_chains = 1 through an aligned _m door: the plain door's arrays as units
void plain_units(Units &u, const Hit *hits, const np2aln::Rec *recs, size_t n, const std::vector<uint32_t> &cigar, const TagTexts *tt) {
    u.add_plain(hits, n);
    u.recs.insert(u.recs.end(), recs, recs + n), u.cigar.insert(u.cigar.end(), cigar.begin(), cigar.end());
    if (tt) {
        u.tt.n_md.insert(u.tt.n_md.end(), tt->n_md.begin(), tt->n_md.end()), u.tt.n_cs.insert(u.tt.n_cs.end(), tt->n_cs.begin(), tt->n_cs.end());
        u.tt.md.insert(u.tt.md.end(), tt->md.begin(), tt->md.end()), u.tt.cs.insert(u.tt.cs.end(), tt->cs.begin(), tt->cs.end());
    }
}

void append_units(Units &all, const Units &u) {
    all.hits.insert(all.hits.end(), u.hits.begin(), u.hits.end()), all.cls.insert(all.cls.end(), u.cls.begin(), u.cls.end());
    all.parent.insert(all.parent.end(), u.parent.begin(), u.parent.end()), all.n_units.insert(all.n_units.end(), u.n_units.begin(), u.n_units.end());
    all.recs.insert(all.recs.end(), u.recs.begin(), u.recs.end()), all.cigar.insert(all.cigar.end(), u.cigar.begin(), u.cigar.end());
    all.tt.n_md.insert(all.tt.n_md.end(), u.tt.n_md.begin(), u.tt.n_md.end()), all.tt.n_cs.insert(all.tt.n_cs.end(), u.tt.n_cs.begin(), u.tt.n_cs.end());
    all.tt.md.insert(all.tt.md.end(), u.tt.md.begin(), u.tt.md.end()), all.tt.cs.insert(all.tt.cs.end(), u.tt.cs.begin(), u.tt.cs.end());
}

// the aligned units of a call -> the caller's unit_off and the np2_free-owned arrays of *out
void give_units(const Units &u, uint64_t n_reads, uint32_t out_flags, uint64_t *unit_off, np2_map_units_t *out) {
    if (u.n_units.size() != n_reads) throw Np2Error(NP2_E_DEVICE, "np2_map_align: the units do not cover the reads");
    const size_t n = u.hits.size();
    Freed f[10];
    std::vector<uint64_t> off(n + 1, 0), md_off(n + 1, 0), cs_off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + u.recs[i].n_cigar;
    if (off[n] != u.cigar.size()) throw Np2Error(NP2_E_DEVICE, "np2_map_align: the units' CIGARs do not add up");
    malloc_copy(f[0], u.hits.data(), n), malloc_copy(f[1], u.cls.data(), n), malloc_copy(f[2], u.parent.data(), n);
    malloc_copy(f[3], u.recs.data(), n), malloc_copy(f[4], u.cigar.data(), u.cigar.size()), malloc_copy(f[5], off.data(), n + 1);
    const bool md = (out_flags & NP2_ALN_MD) != 0, cs = (out_flags & NP2_ALN_CS) != 0;
    if (md || cs) {
        for (size_t i = 0; i < n; ++i) md_off[i + 1] = md_off[i] + u.tt.n_md[i], cs_off[i + 1] = cs_off[i] + u.tt.n_cs[i];
    }
    if (md) malloc_copy(f[6], u.tt.md.data(), u.tt.md.size()), malloc_copy(f[7], md_off.data(), n + 1);
    if (cs) malloc_copy(f[8], u.tt.cs.data(), u.tt.cs.size()), malloc_copy(f[9], cs_off.data(), n + 1);
    fill_unit_off(u, n_reads, unit_off);
    out->n_units = n;
    out->hits = (np2_map_hit_t *)f[0].release(), out->cls = (uint8_t *)f[1].release(), out->parent = (uint32_t *)f[2].release();
    out->recs = (np2_align_rec_t *)f[3].release(), out->cigar = (uint32_t *)f[4].release(), out->cigar_off = (uint64_t *)f[5].release();
    out->md = (char *)f[6].release(), out->md_off = (uint64_t *)f[7].release();
    out->cs = (char *)f[8].release(), out->cs_off = (uint64_t *)f[9].release();
    tl_mstats.units = n;
}
} // namespace
} // extern "C++"

int np2_map_align_bytes_m(const np2_map_index_t *ix, const uint8_t *reads, const uint8_t *quals, uint64_t n, uint64_t n_reads,
                          const np2_map_opts_t *map_opts, const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts, uint32_t out_flags,
                          uint64_t *unit_off, np2_map_units_t *out) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_align_bytes_m";
        if (out) *out = np2_map_units_t{};
        const np2map::Opts o = checked(map_opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        const np2aln::Opts ao = checked_align(align_opts, who.c_str());
        check_index_opts(ix, o, who.c_str());
        checked_out_flags(out_flags, NP2_ALN_QUAL | NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, who);
        if (!unit_off || !out) throw Np2Error(NP2_E_ARG, who + ": unit_off and out are outputs: neither may be NULL");
        const std::vector<uint64_t> ends = ends_of(reads, n, who.c_str(), "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, who + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        tl_tstats = np2_align_tag_stats_t{};
        tl_mstats = np2_map_multi_stats_t{};
        if ((out_flags & NP2_ALN_QUAL) && quals) tl_tstats.qual_reads = check_quals(quals, ends, who);
        const uint32_t tag_flags = out_flags & ~(uint32_t)NP2_ALN_QUAL;
        Mapper m(*ix, o);
        m.align_with(ao);
        m.tag_flags = tag_flags;
        Units u, all;
        TagTexts tt;
        if (mo.max_chains > 1) m.more_with(mo, &u, false);
        if (tag_flags) m.tt = mo.max_chains > 1 ? &u.tt : &tt;
        std::vector<uint32_t> local, cg;
        std::vector<Hit> prim(n_reads);
        std::vector<np2aln::Rec> recs(n_reads);
        for (uint64_t r0 = 0; r0 < n_reads;) { // np2_map_align_bytes' batches
            const uint64_t from = r0 ? ends[r0 - 1] + 1 : 0;
            uint64_t r1 = r0 + 1;
            while (r1 < n_reads && ends[r1] + 1 - from <= m.hooks.batch_bytes()) ++r1;
            local.clear();
            for (uint64_t i = r0; i < r1; ++i) local.push_back((uint32_t)(ends[i] - from));
            u.clear(), cg.clear();
            if (tag_flags) tt.begin(r1 - r0);
            m.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), prim.data() + r0, nullptr, recs.data() + r0, &cg);
            if (mo.max_chains == 1) plain_units(u, prim.data() + r0, recs.data() + r0, r1 - r0, cg, tag_flags ? &tt : nullptr);
            else tl_mstats.overflow_units += u.settle();
            append_units(all, u);
            r0 = r1;
        }
        give_units(all, n_reads, out_flags, unit_off, out);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_align_files_m(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                          const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts, uint32_t out_flags, const char *out_path,
                          np2_map_stats_t *stats) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_align_files_m";
        const np2map::Opts o = checked(map_opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        const np2aln::Opts ao = checked_align(align_opts, who.c_str());
        checked_out_flags(out_flags, NP2_ALN_QUAL | NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, who);
        tl_tstats = np2_align_tag_stats_t{};
        tl_mstats = np2_map_multi_stats_t{};
        const uint32_t tag_flags = out_flags & ~(uint32_t)NP2_ALN_QUAL;
        const bool with_qual = (out_flags & NP2_ALN_QUAL) != 0;
        check_index_opts(ix, o, who.c_str());
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, who + ": no read file given");
        if (!out_path) throw Np2Error(NP2_E_ARG, who + ": out_path is NULL");
        const std::vector<std::string> files = checked_files(paths, n_paths, who);
        Mapper m(*ix, o);
        m.align_with(ao);
        m.tag_flags = tag_flags;
        Units u;
        TagTexts tt;
        if (mo.max_chains > 1) m.more_with(mo, &u, false);
        if (tag_flags) m.tt = mo.max_chains > 1 ? &u.tt : &tt;
        np2h::OutFile out;
        out.open(out_path, ix->device);
        std::vector<Hit> hits;
        std::string text;
        std::vector<np2aln::Rec> recs;
        std::vector<uint32_t> cigar;
        np2aln::sam_header(text, ix->names, ix->lens);
        out.put(text.data(), text.size());
        read_batches(files, m.hooks, who, [&](const BatchBuf &b) {
            hits.resize(b.ends.size()), recs.resize(b.ends.size()), cigar.clear(), u.clear();
            if (tag_flags) tt.begin(b.ends.size());
            m.batch(b.bytes.data(), b.closed(), b.ends.data(), (uint32_t)b.ends.size(), hits.data(), nullptr, recs.data(), &cigar);
            const auto t0 = std::chrono::steady_clock::now();
            if (mo.max_chains == 1) { // the plain door's writer: the parent's bytes
                write_sam(out, *ix, b, hits, recs, cigar, text, tag_flags ? &tt : nullptr);
                tl_mstats.units += hits.size();
            } else {
                tl_mstats.overflow_units += u.settle();
                tl_mstats.units += u.hits.size();
                write_sam_units(out, *ix, b, u, text, tag_flags != 0);
            }
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            tl_stats.write_ms += ms, tl_astats.write_ms += ms;
        }, with_qual);
        out.close();
        fill_stats(stats);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_align_host_m(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_map_multi_opts_t *multi, const np2_align_opts_t *align_opts,
                         const np2_map_weights_t *wts, uint32_t out_flags, uint64_t *unit_off, np2_map_units_t *out) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_map_align_host_m";
        if (out) *out = np2_map_units_t{};
        const np2map::Opts o = checked(map_opts, who.c_str());
        const np2map::MultiOpts mo = checked_multi(multi, who);
        np2aln::Opts ao = checked_align(align_opts, who.c_str());
        const np2map::WeightSet *ws = checked_weights(wts, o, who.c_str());
        checked_out_flags(out_flags, NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, who);
        if (!unit_off || !out) throw Np2Error(NP2_E_ARG, who + ": unit_off and out are outputs: neither may be NULL");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, who.c_str(), "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, who.c_str(), "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, who + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        const Hooks hooks;
        if (ao.max_cells > hooks.align_cells) ao.max_cells = hooks.align_cells;
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w, ws);
        np2_map_stats_t &st = tl_stats;
        st = np2_map_stats_t{};
        st.index_minimizers = hx.mz.size();
        tl_astats = np2_align_stats_t{};
        tl_tstats = np2_align_tag_stats_t{};
        tl_mstats = np2_map_multi_stats_t{};
        Units u;
        np2map::ReadCounts rc;
        np2map::MoreCounts mc{};
        np2aln::Scratch w;
        unsigned long long ctr[np2aln::C_N] = {};
        Hit uh[np2map::MAX_CHAINS];
        uint32_t ucls[np2map::MAX_CHAINS], upar[np2map::MAX_CHAINS];
        std::vector<uint32_t> ch, split;
        uint64_t from = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            ch.clear();
            const uint32_t nu = np2map::map_read_m(hx, reads + from, (uint32_t)(ends[i] - from), o, mo, uh, ucls, upar, &ch, &rc, &mc);
            ++(uh[0].tid >= 0 ? st.mapped : st.unmapped);
            u.n_units.push_back(nu);
            size_t ch_at = 0;
            for (uint32_t t = 0; t < nu; ++t) {
                const Hit &h = uh[t];
                const size_t at = u.hits.size();
                u.hits.push_back(h), u.cls.push_back((uint8_t)ucls[t]), u.parent.push_back(upar[t]);
                u.recs.push_back(np2aln::unaligned_rec());
                if (out_flags) u.tt.n_md.push_back(0), u.tt.n_cs.push_back(0);
                if (h.tid < 0) continue;
                const uint64_t t_at = h.tid ? a_ends[(size_t)h.tid - 1] + 1 : 0;
                uint64_t c64[np2aln::C_N] = {};
                np2aln::Rec &r = u.recs[at];
                r = np2aln::align_read(asm_stream + t_at, (uint32_t)(a_ends[(size_t)h.tid] - t_at), reads + from, h, ch.data() + ch_at, o.k, ao, ao.max_cells, w,
                                       u.cigar, c64);
                ch_at += 2 * (size_t)h.n;
                for (int f = 0; f < np2aln::C_N; ++f) ctr[f] += c64[f];
                if (out_flags && r.tid >= 0) {
                    const size_t cg_at = u.cigar.size() - r.n_cigar;
                    const np2aln::TagIn in{asm_stream + t_at + r.pos, reads + from, h.qlen, h.rev, u.cigar.data() + cg_at, r.n_cigar};
                    split.clear();
                    tags_of_record(in, out_flags, u.tt, at, &split);
                    if (out_flags & NP2_ALN_EQX) {
                        u.cigar.resize(cg_at), u.cigar.insert(u.cigar.end(), split.begin(), split.end());
                        r.n_cigar = (uint32_t)split.size(), tl_tstats.eqx_words += split.size();
                    }
                }
            }
            from = ends[i] + 1;
        }
        st.reads = n_reads, st.minimizers = rc.minimizers, st.anchors = rc.anchors, st.dropped_occ = rc.dropped_occ;
        add_counts(tl_astats, ctr);
        const unsigned long long c5[5] = {mc.selections, mc.dropped_cnt, mc.dropped_pri, mc.kept_supp, mc.kept_sec};
        add_more_counts(tl_mstats, c5);
        tl_mstats.overflow_units = u.settle();
        tl_tstats.md_bytes = u.tt.md.size(), tl_tstats.cs_bytes = u.tt.cs.size();
        give_units(u, n_reads, out_flags, unit_off, out);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_map_last_multi_stats(np2_map_multi_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (!stats) throw Np2Error(NP2_E_ARG, "np2_map_last_multi_stats: stats is NULL");
        *stats = tl_mstats;
        return NP2_OK;
    }, np2h::io_set_error);
}

// np2_map_align_bytes (out_flags 0, no texts) and np2_map_align_bytes_x
static int map_align_bytes_impl(const np2_map_index_t *ix, const uint8_t *reads, const uint8_t *quals, uint64_t n, uint64_t n_reads,
                                const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, uint32_t out_flags, np2_map_hit_t *hits,
                                np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, char **md, uint64_t *md_off, char **cs, uint64_t *cs_off,
                                const std::string name) {
    return np2h::abi_guard([&] {
        const char *who = name.c_str();
        if (cigar) *cigar = nullptr;
        const np2map::Opts o = checked(map_opts, who);
        const np2aln::Opts ao = checked_align(align_opts, who);
        check_index_opts(ix, o, who);
        checked_out_flags(out_flags, NP2_ALN_QUAL | NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, name);
        check_tag_pairs(out_flags, md, md_off, cs, cs_off, name);
        if (n_reads && !recs) throw Np2Error(NP2_E_ARG, name + ": recs is NULL");
        if ((cigar == nullptr) != (cigar_off == nullptr)) throw Np2Error(NP2_E_ARG, name + ": cigar and cigar_off go together");
        const std::vector<uint64_t> ends = ends_of(reads, n, who, "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, name + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        tl_tstats = np2_align_tag_stats_t{};
        if ((out_flags & NP2_ALN_QUAL) && quals) tl_tstats.qual_reads = check_quals(quals, ends, name);
        const uint32_t tag_flags = out_flags & ~(uint32_t)NP2_ALN_QUAL;
        TagTexts tt, all;
        all.begin(n_reads);
        Mapper m(*ix, o);
        m.align_with(ao);
        m.tag_flags = tag_flags;
        if (tag_flags) m.tt = &tt;
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
            if (tag_flags) tt.begin(r1 - r0);
            m.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), out + r0, nullptr, rout + r0, &cg);
            if (tag_flags) {
                std::copy(tt.n_md.begin(), tt.n_md.end(), all.n_md.begin() + (ptrdiff_t)r0);
                std::copy(tt.n_cs.begin(), tt.n_cs.end(), all.n_cs.begin() + (ptrdiff_t)r0);
                all.md.insert(all.md.end(), tt.md.begin(), tt.md.end()), all.cs.insert(all.cs.end(), tt.cs.begin(), tt.cs.end());
            }
            r0 = r1;
        }
        if (cigar) {
            cigar_off[0] = 0;
            for (uint64_t i = 0; i < n_reads; ++i) cigar_off[i + 1] = cigar_off[i] + rout[i].n_cigar;
            *cigar = chain_out(cg);
        }
        if (md) offsets_of(all.n_md, md_off), *md = text_out(all.md);
        if (cs) offsets_of(all.n_cs, cs_off), *cs = text_out(all.cs);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_map_align_bytes(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const np2_map_opts_t *map_opts,
                        const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off) {
    return map_align_bytes_impl(ix, reads, nullptr, n, n_reads, map_opts, align_opts, 0, hits, recs, cigar, cigar_off, nullptr, nullptr, nullptr, nullptr,
                                "np2_map_align_bytes");
}
int np2_map_align_bytes_x(const np2_map_index_t *ix, const uint8_t *reads, const uint8_t *quals, uint64_t n, uint64_t n_reads,
                          const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, uint32_t out_flags, np2_map_hit_t *hits,
                          np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, char **md, uint64_t *md_off, char **cs, uint64_t *cs_off) {
    return map_align_bytes_impl(ix, reads, quals, n, n_reads, map_opts, align_opts, out_flags, hits, recs, cigar, cigar_off, md, md_off, cs, cs_off,
                                "np2_map_align_bytes_x");
}
int np2_map_align_files_x(const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                          const np2_align_opts_t *align_opts, uint32_t out_flags, const char *out_path, np2_map_stats_t *stats) {
    return map_files_impl(ix, paths, n_paths, map_opts, align_opts, true, out_path, stats, "np2_map_align_files_x", out_flags);
}

static int map_align_host_impl(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                               const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_map_weights_t *wts, np2_map_hit_t *hits,
                               np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, const std::string name, uint32_t out_flags = 0,
                               char **md = nullptr, uint64_t *md_off = nullptr, char **cs = nullptr, uint64_t *cs_off = nullptr) {
    return np2h::abi_guard([&] {
        const char *who = name.c_str();
        if (cigar) *cigar = nullptr;
        const np2map::Opts o = checked(map_opts, who);
        np2aln::Opts ao = checked_align(align_opts, who);
        const np2map::WeightSet *ws = checked_weights(wts, o, who);
        checked_out_flags(out_flags, NP2_ALN_MD | NP2_ALN_CS | NP2_ALN_EQX, name);
        check_tag_pairs(out_flags, md, md_off, cs, cs_off, name);
        tl_tstats = np2_align_tag_stats_t{};
        TagTexts tt;
        tt.begin(n_reads);
        std::vector<uint32_t> split;
        if (n_reads && !recs) throw Np2Error(NP2_E_ARG, name + ": recs is NULL");
        if ((cigar == nullptr) != (cigar_off == nullptr)) throw Np2Error(NP2_E_ARG, name + ": cigar and cigar_off go together");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, who, "the assembly stream");
        const std::vector<uint64_t> ends = ends_of(reads, n, who, "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, name + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        const Hooks hooks;
        if (ao.max_cells > hooks.align_cells) ao.max_cells = hooks.align_cells;
        np2map::HostIndex hx;
        hx.build(asm_stream, a_ends, o.k, o.w, ws);
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
                if (out_flags && rout[i].tid >= 0) { // the same walk as the tag kernels', one caller
                    const size_t cg_at = cg.size() - rout[i].n_cigar;
                    const np2aln::TagIn in{asm_stream + t_at + rout[i].pos, reads + from, h.qlen, h.rev, cg.data() + cg_at, rout[i].n_cigar};
                    split.clear();
                    tags_of_record(in, out_flags, tt, i, &split);
                    if (out_flags & NP2_ALN_EQX) {
                        cg.resize(cg_at), cg.insert(cg.end(), split.begin(), split.end());
                        rout[i].n_cigar = (uint32_t)split.size(), tl_tstats.eqx_words += split.size();
                    }
                }
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
        tl_tstats.md_bytes = tt.md.size(), tl_tstats.cs_bytes = tt.cs.size();
        if (md) offsets_of(tt.n_md, md_off), *md = text_out(tt.md);
        if (cs) offsets_of(tt.n_cs, cs_off), *cs = text_out(tt.cs);
        return NP2_OK;
    }, np2h::io_set_error);
}
int np2_map_align_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                       const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, np2_map_hit_t *hits, np2_align_rec_t *recs,
                       uint32_t **cigar, uint64_t *cigar_off) {
    return map_align_host_impl(asm_stream, n_asm, reads, n, n_reads, map_opts, align_opts, nullptr, hits, recs, cigar, cigar_off,
                               "np2_map_align_host");
}
int np2_map_align_host_w(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_map_weights_t *w, np2_map_hit_t *hits,
                         np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off) {
    return map_align_host_impl(asm_stream, n_asm, reads, n, n_reads, map_opts, align_opts, w, hits, recs, cigar, cigar_off,
                               "np2_map_align_host_w");
}

int np2_map_align_host_x(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads,
                         const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_map_weights_t *w, uint32_t out_flags,
                         np2_map_hit_t *hits, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, char **md, uint64_t *md_off, char **cs,
                         uint64_t *cs_off) {
    return map_align_host_impl(asm_stream, n_asm, reads, n, n_reads, map_opts, align_opts, w, hits, recs, cigar, cigar_off, "np2_map_align_host_x",
                               out_flags, md, md_off, cs, cs_off);
}

int np2_align_tags_host(const uint8_t *ref, uint64_t n_ref, const uint8_t *reads, uint64_t n_read_bytes, uint64_t n_recs, const uint64_t *t_off,
                        const uint64_t *q_off, const uint32_t *cigar, const uint64_t *cigar_off, uint32_t out_flags, char **md, uint64_t *md_off,
                        char **cs, uint64_t *cs_off, uint32_t **eqx, uint64_t *eqx_off) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_align_tags_host";
        const TagDoor d(ref, n_ref, reads, n_read_bytes, n_recs, t_off, q_off, cigar, cigar_off, out_flags, md, md_off, cs, cs_off, eqx, eqx_off, who);
        TagTexts tt;
        tt.begin(n_recs);
        std::vector<uint32_t> split;
        if (eqx) eqx_off[0] = 0;
        for (uint64_t i = 0; i < n_recs; ++i) {
            const np2aln::TagIn in{ref + t_off[i], reads + q_off[i], 0, 0, cigar + cigar_off[i], (uint32_t)(cigar_off[i + 1] - cigar_off[i])};
            tags_of_record(in, d.flags, tt, i, &split);
            if (eqx) eqx_off[i + 1] = split.size();
        }
        if (md) offsets_of(tt.n_md, md_off), *md = text_out(tt.md);
        if (cs) offsets_of(tt.n_cs, cs_off), *cs = text_out(tt.cs);
        if (eqx) *eqx = chain_out(split);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_align_tags_device(int device, const uint8_t *ref, uint64_t n_ref, const uint8_t *reads, uint64_t n_read_bytes, uint64_t n_recs,
                          const uint64_t *t_off, const uint64_t *q_off, const uint32_t *cigar, const uint64_t *cigar_off, uint32_t out_flags, char **md,
                          uint64_t *md_off, char **cs, uint64_t *cs_off, uint32_t **eqx, uint64_t *eqx_off) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_align_tags_device";
        // every argument is checked before the first device call: a record's columns lie inside the two buffers
        const TagDoor d(ref, n_ref, reads, n_read_bytes, n_recs, t_off, q_off, cigar, cigar_off, out_flags, md, md_off, cs, cs_off, eqx, eqx_off, who);
        tl_tstats = np2_align_tag_stats_t{};
        Stream s(device);
        DevBuf<uint8_t> d_ref, d_reads;
        DevBuf<uint64_t> d_t, d_q, d_co;
        DevBuf<uint32_t> d_cig;
        d_ref.cached = d_reads.cached = d_t.cached = d_q.cached = d_co.cached = d_cig.cached = true;
        d_ref.ensure(n_ref + 1), d_reads.ensure(n_read_bytes + 1), d_t.ensure(n_recs + 1), d_q.ensure(n_recs + 1), d_co.ensure(n_recs + 1);
        d_cig.ensure(d.n_words + 1);
        std::vector<uint64_t> co(n_recs + 1); // (relative to the first record's words)
        for (uint64_t i = 0; i <= n_recs; ++i) co[i] = cigar_off[i] - cigar_off[0];
        if (n_ref) HIPCHK(hipMemcpyAsync(d_ref.p, ref, n_ref, hipMemcpyHostToDevice, s.st));
        if (n_read_bytes) HIPCHK(hipMemcpyAsync(d_reads.p, reads, n_read_bytes, hipMemcpyHostToDevice, s.st));
        if (n_recs) HIPCHK(hipMemcpyAsync(d_t.p, t_off, n_recs * 8, hipMemcpyHostToDevice, s.st));
        if (n_recs) HIPCHK(hipMemcpyAsync(d_q.p, q_off, n_recs * 8, hipMemcpyHostToDevice, s.st));
        HIPCHK(hipMemcpyAsync(d_co.p, co.data(), (n_recs + 1) * 8, hipMemcpyHostToDevice, s.st));
        if (d.n_words) HIPCHK(hipMemcpyAsync(d_cig.p, cigar + cigar_off[0], d.n_words * 4, hipMemcpyHostToDevice, s.st));
        HIPCHK(hipStreamSynchronize(s.st)); // (co is this call's own memory)
        np2::TagJob j{};
        j.ref = d_ref.p, j.reads = d_reads.p, j.t_off = d_t.p, j.q_off = d_q.p, j.cig_off = d_co.p, j.cigar = d_cig.p;
        j.n = (uint32_t)n_recs, j.flags = d.flags;
        TagRun tg;
        tl_tstats.tags_ms = tg.run(s, j);
        tl_tstats.md_bytes = tg.md.size(), tl_tstats.cs_bytes = tg.cs.size(), tl_tstats.eqx_words = tg.eqx.size();
        if (md) std::copy(tg.md_off.begin(), tg.md_off.end(), md_off), *md = text_out(tg.md);
        if (cs) std::copy(tg.cs_off.begin(), tg.cs_off.end(), cs_off), *cs = text_out(tg.cs);
        if (eqx) std::copy(tg.eqx_off.begin(), tg.eqx_off.end(), eqx_off), *eqx = chain_out(tg.eqx);
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"

// ---- np2_align_chains_device, np2_align_chains_host: the aligner on the caller's hits and chains ---------------------------------
namespace {
static_assert(sizeof(np2_align_slot_t) == sizeof(np2aln::Slot) && sizeof(np2aln::Slot) == 40, "np2_align_slot_t is np2aln::Slot");
static_assert(sizeof(np2_align_res_t) == sizeof(np2aln::Res) && sizeof(np2aln::Res) == 12, "np2_align_res_t is np2aln::Res");

// What both doors check before any walk and before anything is uploaded (np2_io.h): after it no anchor of a chain can become an
// access outside its read or its contig.  Returns the reads' separators.
std::vector<uint64_t> check_chains(const std::vector<uint64_t> &lens, const uint8_t *reads, uint64_t n, uint64_t n_reads, uint32_t k, const np2_map_hit_t *hits,
                                   const uint32_t *chain, const uint64_t *chain_off, np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off,
                                   np2_align_probe_t *probe, const std::string &who) {
    if (n_reads && !recs) throw Np2Error(NP2_E_ARG, who + ": recs is NULL");
    if ((cigar == nullptr) != (cigar_off == nullptr)) throw Np2Error(NP2_E_ARG, who + ": cigar and cigar_off go together");
    if (probe && (probe->want & ~(uint32_t)(NP2_PROBE_SLOTS | NP2_PROBE_TB))) throw Np2Error(NP2_E_ARG, who + ": unknown bits in probe->want");
    if (n_reads && !hits) throw Np2Error(NP2_E_ARG, who + ": hits is NULL");
    if (!chain_off) throw Np2Error(NP2_E_ARG, who + ": chain_off is NULL");
    std::vector<uint64_t> ends = ends_of(reads, n, who.c_str(), "the read stream");
    if (ends.size() != n_reads)
        throw Np2Error(NP2_E_ARG, who + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
    if (n > MAP_MAX_STREAM || n_reads > np2map::MAX_SEQ) throw Np2Error(NP2_E_UNSUPPORTED, who + ": a read stream of 2^32 bytes or more");
    if (chain_off[0] != 0) throw Np2Error(NP2_E_ARG, who + ": chain_off[0] is not 0");
    uint64_t from = 0;
    for (uint64_t i = 0; i < n_reads; ++i) {
        const np2_map_hit_t &h = hits[i];
        const std::string rd = who + ": read " + std::to_string(i);
        if (chain_off[i + 1] < chain_off[i]) throw Np2Error(NP2_E_ARG, rd + ": chain_off descends");
        const uint64_t pairs = chain_off[i + 1] - chain_off[i], qlen = ends[i] - from;
        from = ends[i] + 1;
        if (h.tid < 0) {
            if (pairs) throw Np2Error(NP2_E_ARG, rd + " is unmapped, chain_off gives it " + std::to_string(pairs) + " anchors");
            continue;
        }
        if ((uint64_t)h.tid >= lens.size()) throw Np2Error(NP2_E_ARG, rd + ": tid " + std::to_string(h.tid) + " names no contig of " + std::to_string(lens.size()));
        if (h.qlen != qlen) throw Np2Error(NP2_E_ARG, rd + ": qlen is " + std::to_string(h.qlen) + ", the read has " + std::to_string(qlen) + " bases");
        if (h.rev > 1) throw Np2Error(NP2_E_ARG, rd + ": rev is neither 0 nor 1");
        if (h.n < 1) throw Np2Error(NP2_E_ARG, rd + ": a mapped read with n = 0 anchors");
        if (pairs != h.n) throw Np2Error(NP2_E_ARG, rd + ": n is " + std::to_string(h.n) + ", chain_off gives it " + std::to_string(pairs) + " anchors");
        if (chain_off[i + 1] > np2map::MAX_SEQ) throw Np2Error(NP2_E_UNSUPPORTED, who + ": more than 2^31 - 1 anchors in a call");
        if (!chain) throw Np2Error(NP2_E_ARG, who + ": chain is NULL");
        const uint64_t tlen = lens[(size_t)h.tid];
        for (uint64_t a = 0; a < pairs; ++a) {
            const uint64_t r = chain[2 * (chain_off[i] + a)], q = chain[2 * (chain_off[i] + a) + 1];
            if (r + 1 < k || r >= tlen)
                throw Np2Error(NP2_E_ARG, rd + ", anchor " + std::to_string(a) + ": r = " + std::to_string(r) + " is outside " + std::to_string(k - 1) +
                                              " .. " + std::to_string(tlen) + " - 1 of contig " + std::to_string(h.tid));
            if (q + 1 < k || q >= qlen)
                throw Np2Error(NP2_E_ARG, rd + ", anchor " + std::to_string(a) + ": q = " + std::to_string(q) + " is outside " + std::to_string(k - 1) +
                                              " .. " + std::to_string(qlen) + " - 1 of the read");
        }
    }
    return ends;
}

template <class T> T *array_out(const std::vector<T> &v) { // a malloc block for the caller (np2_free); never NULL
    T *p = (T *)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (!p) throw Np2Error(NP2_E_NOMEM, "out of memory for the probe");
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

void clear_probe(np2_align_probe_t *p) {
    if (p) p->n_slots = 0, p->slot_off = nullptr, p->slots = nullptr, p->res = nullptr, p->tb_off = nullptr, p->tb = nullptr;
}

void probe_out(const np2aln::Probe &pr, np2_align_probe_t *p) {
    if (!p) return;
    std::unique_ptr<void, decltype(&free)> f[5] = {{nullptr, free}, {nullptr, free}, {nullptr, free}, {nullptr, free}, {nullptr, free}};
    if (p->want & NP2_PROBE_SLOTS) {
        f[0].reset(array_out(pr.slot_off)), f[1].reset(array_out(pr.slots)), f[2].reset(array_out(pr.res));
    }
    if (p->want & NP2_PROBE_TB) f[3].reset(array_out(pr.tb_off)), f[4].reset(array_out(pr.tb));
    p->n_slots = pr.slots.size();
    p->slot_off = (uint64_t *)f[0].release(), p->slots = (np2_align_slot_t *)f[1].release(), p->res = (np2_align_res_t *)f[2].release();
    p->tb_off = (uint64_t *)f[3].release(), p->tb = (uint8_t *)f[4].release();
}

void cigars_out(const np2aln::Rec *rout, uint64_t n_reads, const std::vector<uint32_t> &cg, uint32_t **cigar, uint64_t *cigar_off) {
    if (!cigar) return;
    cigar_off[0] = 0;
    for (uint64_t i = 0; i < n_reads; ++i) cigar_off[i + 1] = cigar_off[i] + rout[i].n_cigar;
    *cigar = chain_out(cg);
}
} // namespace

extern "C" {
int np2_align_chains_device(const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, uint32_t k, const np2_map_hit_t *hits,
                            const uint32_t *chain, const uint64_t *chain_off, const np2_align_opts_t *align_opts, np2_align_rec_t *recs, uint32_t **cigar,
                            uint64_t *cigar_off, np2_align_probe_t *probe) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_align_chains_device";
        if (cigar) *cigar = nullptr;
        clear_probe(probe);
        const np2aln::Opts ao = checked_align(align_opts, who.c_str());
        if (!ix) throw Np2Error(NP2_E_ARG, who + ": the index is NULL");
        if (k != ix->k) throw Np2Error(NP2_E_ARG, who + ": the index was built with k = " + std::to_string(ix->k) + ", the call says k = " + std::to_string(k));
        const std::vector<uint64_t> ends = check_chains(ix->lens, reads, n, n_reads, k, hits, chain, chain_off, recs, cigar, cigar_off, probe, who);
        np2map::Opts o{};
        o.k = ix->k, o.w = ix->w;
        Mapper m(*ix, o);
        m.align_with(ao);
        np2aln::Probe pr;
        if (probe) pr.want_tb = (probe->want & NP2_PROBE_TB) != 0, m.probe = &pr;
        const std::vector<uint32_t> local(ends.begin(), ends.end());
        std::vector<uint32_t> cg;
        np2aln::Rec *rout = reinterpret_cast<np2aln::Rec *>(recs);
        m.chains(reads, n, local.data(), (uint32_t)n_reads, reinterpret_cast<const Hit *>(hits), chain, chain_off, rout, &cg);
        cigars_out(rout, n_reads, cg, cigar, cigar_off);
        probe_out(pr, probe);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_align_chains_host(const uint8_t *asm_stream, uint64_t n_asm, const uint8_t *reads, uint64_t n, uint64_t n_reads, uint32_t k,
                          const np2_map_hit_t *hits, const uint32_t *chain, const uint64_t *chain_off, const np2_align_opts_t *align_opts,
                          np2_align_rec_t *recs, uint32_t **cigar, uint64_t *cigar_off, np2_align_probe_t *probe) {
    return np2h::abi_guard([&] {
        const std::string who = "np2_align_chains_host";
        if (cigar) *cigar = nullptr;
        clear_probe(probe);
        np2aln::Opts ao = checked_align(align_opts, who.c_str());
        if (k < np2map::K_MIN || k > np2map::K_MAX) throw Np2Error(NP2_E_ARG, who + ": k = " + std::to_string(k) + " is outside 11 .. 28");
        const std::vector<uint64_t> a_ends = ends_of(asm_stream, n_asm, who.c_str(), "the assembly stream");
        std::vector<uint64_t> lens;
        for (size_t i = 0; i < a_ends.size(); ++i) lens.push_back(a_ends[i] - (i ? a_ends[i - 1] + 1 : 0));
        const std::vector<uint64_t> ends = check_chains(lens, reads, n, n_reads, k, hits, chain, chain_off, recs, cigar, cigar_off, probe, who);
        const Hooks hooks;
        if (ao.max_cells > hooks.align_cells) ao.max_cells = hooks.align_cells;
        np2_map_stats_t &st = tl_stats;
        st = np2_map_stats_t{};
        tl_astats = np2_align_stats_t{};
        np2aln::Probe pr;
        if (probe) pr.want_tb = (probe->want & NP2_PROBE_TB) != 0;
        np2aln::Scratch w;
        std::vector<uint32_t> cg;
        uint64_t ctr[np2aln::C_N] = {};
        np2aln::Rec *rout = reinterpret_cast<np2aln::Rec *>(recs);
        uint64_t from = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            const Hit &h = reinterpret_cast<const Hit *>(hits)[i];
            ++(h.tid >= 0 ? st.mapped : st.unmapped);
            rout[i] = np2aln::unaligned_rec();
            if (h.tid >= 0) {
                const uint64_t t_at = h.tid ? a_ends[(size_t)h.tid - 1] + 1 : 0;
                rout[i] = np2aln::align_read(asm_stream + t_at, (uint32_t)lens[(size_t)h.tid], reads + from, h, chain + 2 * chain_off[i], k, ao, ao.max_cells, w,
                                             cg, ctr, probe ? &pr : nullptr);
            } else {
                pr.unmapped();
            }
            from = ends[i] + 1;
        }
        st.reads = n_reads;
        unsigned long long c[np2aln::C_N];
        for (int f = 0; f < np2aln::C_N; ++f) c[f] = ctr[f];
        add_counts(tl_astats, c);
        cigars_out(rout, n_reads, cg, cigar, cigar_off);
        probe_out(pr, probe);
        return NP2_OK;
    }, np2h::io_set_error);
}
} // extern "C"

extern "C" {
int np2_map_align_last_tag_stats(np2_align_tag_stats_t *stats) {
    if (!stats) return np2h::io_set_error(NP2_E_ARG, "np2_map_align_last_tag_stats: stats is NULL");
    *stats = tl_tstats;
    return NP2_OK;
}

int np2_sam_from_reads(np2_ctx_t *cx, const np2_map_index_t *ix, const char *const *paths, int n_paths, const np2_map_opts_t *map_opts,
                       const np2_align_opts_t *align_opts, const np2_sam_opts_t *sam_opts, uint32_t flags, np2_sam_t **out) {
    if (out) *out = nullptr;
    bool touched = false;
    return from_reads_guard(cx, touched, [&] {
        const char *who = "np2_sam_from_reads";
        const FromReads a(cx, ix, map_opts, align_opts, sam_opts, flags, out, who);
        const std::vector<std::string> files = checked_files(paths, n_paths, who);
        touched = true;
        FromReadsRun run(cx, ix, a);
        read_batches(files, run.m.hooks, who, [&](const BatchBuf &b) {
            run.batch(b.bytes.data(), b.closed(), b.ends.data(), (uint32_t)b.ends.size(), b.names.data(), b.names.size());
        });
        *out = run.finish();
        return NP2_OK;
    });
}

int np2_sam_from_read_bytes(np2_ctx_t *cx, const np2_map_index_t *ix, const uint8_t *reads, uint64_t n, uint64_t n_reads, const char *names,
                            const np2_map_opts_t *map_opts, const np2_align_opts_t *align_opts, const np2_sam_opts_t *sam_opts, uint32_t flags,
                            np2_sam_t **out) {
    if (out) *out = nullptr;
    bool touched = false;
    return from_reads_guard(cx, touched, [&] {
        const char *who = "np2_sam_from_read_bytes";
        const FromReads a(cx, ix, map_opts, align_opts, sam_opts, flags, out, who);
        const std::vector<uint64_t> ends = ends_of(reads, n, who, "the read stream");
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, std::string(who) + ": n_reads is " + std::to_string(n_reads) + ", the stream holds " + std::to_string(ends.size()) + " newlines");
        std::vector<size_t> name_at; // where each read's name begins, and the end of the last
        if (names && a.keep_names) {
            const char *p = names;
            for (uint64_t i = 0; i < n_reads; ++i) {
                const char *e = strchr(p, '\n');
                if (!e) throw Np2Error(NP2_E_ARG, std::string(who) + ": names holds fewer than n_reads newline-terminated names");
                name_at.push_back((size_t)(p - names)), p = e + 1;
            }
            name_at.push_back((size_t)(p - names));
        }
        touched = true;
        FromReadsRun run(cx, ix, a);
        std::vector<uint32_t> local;
        std::string numbered;
        for (uint64_t r0 = 0; r0 < n_reads;) { // batches: whole reads, batch_bytes() at the most, one read at the least
            const uint64_t from = r0 ? ends[r0 - 1] + 1 : 0;
            uint64_t r1 = r0 + 1;
            while (r1 < n_reads && ends[r1] + 1 - from <= run.m.hooks.batch_bytes()) ++r1;
            local.clear();
            for (uint64_t i = r0; i < r1; ++i) local.push_back((uint32_t)(ends[i] - from));
            const char *nm = nullptr;
            size_t nm_n = 0;
            if (a.keep_names && names) {
                nm = names + name_at[r0], nm_n = name_at[r1] - name_at[r0];
            } else if (a.keep_names) { // numbered from 1
                numbered.clear();
                for (uint64_t i = r0; i < r1; ++i) numbered += std::to_string(i + 1) + "\n";
                nm = numbered.data(), nm_n = numbered.size();
            }
            run.batch(reads + from, ends[r1 - 1] + 1 - from, local.data(), (uint32_t)(r1 - r0), nm, nm_n);
            r0 = r1;
        }
        *out = run.finish();
        return NP2_OK;
    });
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
