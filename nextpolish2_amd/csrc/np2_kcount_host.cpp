// Host driver of the k-mer counter (include/np2_io.h: np2_kcount_*, np2_ctx_create_from_reads, np2_seqfile_stream):
// sequence files -> separator stream in pinned pieces -> count kernel (np2_kcount.hip) -> yak tables.
//
// Reader: one thread per input file (at most 16), each parsing FASTA / FASTQ / one-sequence-per-line text, plain or gzip
// (zlib's gzread: multi-member files work through it), into pieces of the separator stream.  Every piece carries the
// last 32 bytes of ITS OWN stream in front (the halo), so pieces are self-contained and are counted in whatever order they
// fill; a k-mer that straddles two pieces is counted once, with the piece that holds its last byte.  The input is parsed
// once per pass: a resident piece is counted for every k before its buffer goes back to its reader.
//
// Sizing: a table is 1024 (or a bucket range's share of them) sub-tables of one power-of-two capacity.  Before a piece of
// n bytes (at most n k-mers) is launched the host makes sure claimed + n <= slots / 2, doubling the table first otherwise
// (k_kcount_rehash).  One sub-table can still fill; its k-mers come back in the spill list, the table is doubled and the
// list replayed before the next piece.  `claimed` is the device counter, read back once per piece and k.
//
// Memory: mem_bytes bounds the tables of all k together, a growth's old and new table included (0: half of the device
// memory that is free when the call starts).  A growth that would exceed it restarts the run with twice as many passes
// over bucket ranges (inputs reopened / rescanned; every range is emitted before the next begins).
//
// Quality filter (the *_qc entry points with options): the reader threads fill pieces of BOTH streams that end at a read
// boundary (np2_srqc_host.hpp), and count_piece runs the filter kernel on the uploaded bases before the count kernels read
// them: failed reads and trimmed ends are 'N' by then, which ends a k-mer run as a separator does.  Without options
// nothing of this runs.
//
// Adapter trimming (the *_ad entry points with options): the same pieces, the trimming kernel (np2_sradapt.hip) in the filter
// kernel's place.  In pair mode the files are R1 R2 R1 R2 ..: a reader thread takes a pair of files, reads the two in step
// (a thread and a bounded queue per file, np2_sradapt_host.hpp) and closes a piece only after an even number of reads; at
// most 5 pairs are read at a time (15 threads beside the counting thread).
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kcount_core.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_seqreader.hpp"
#include "np2_sradapt_host.hpp"
#include "np2_srqc_host.hpp"

#include <sys/stat.h>
#include <zlib.h>

#include <functional>

namespace {
using np2h::Np2Error;
using namespace np2kc;
using np2seq::parse_file;

// ---------------------------------------------------------------------------------------------------------------
// pieces between the reader threads and the counting thread
// ---------------------------------------------------------------------------------------------------------------
struct Piece {
    uint8_t *buf = nullptr; // pinned: HALO bytes, then up to `cap` bytes, then room for the padding
    size_t n = 0;
    np2h::QcPiece qc; // with the quality filter: qc.seq == buf, the quality bytes and the separators beside it
};
using PieceQueue = np2h::PieceQueue<Piece>;
using PieceWriter = np2h::HaloWriter<Piece>; // what a reader thread writes its stream into

// ---------------------------------------------------------------------------------------------------------------
// the run
// ---------------------------------------------------------------------------------------------------------------
struct NeedPasses {}; // the next doubling would exceed the memory budget: the run starts over with more passes

struct Stats {
    uint64_t kmers = 0, distinct = 0, spilled = 0;
    uint32_t growths = 0, passes = 0;
    float kernel_ms = 0, read_ms = 0;
};
thread_local Stats g_stats;

struct Hooks {
    uint32_t cap_log2 = 10;
    size_t piece = (size_t)8 << 20;
    uint32_t passes = 0;
    Hooks() { // read once per call, like the other NP2_* switches
        cap_log2 = (uint32_t)np2h::test_hook("NP2_KCOUNT_TEST_CAP_LOG2", 4, 30, cap_log2);
        piece = (size_t)np2h::test_hook("NP2_KCOUNT_TEST_PIECE", 64, LLONG_MAX, (long long)piece);
        passes = (uint32_t)np2h::test_hook("NP2_KCOUNT_TEST_PASSES", 1, 1024, passes);
    }
};

struct Source { // files, or one separator stream in host memory
    std::vector<std::string> paths;
    const uint8_t *mem = nullptr;
    uint64_t mem_n = 0;
    bool rescannable() const {
        for (auto &p : paths) {
            struct stat st;
            if (stat(p.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
        }
        return true;
    }
};

struct KTable {
    uint32_t k = 0, cap_log2 = 0;
    std::shared_ptr<np2h::DevBuf<uint64_t>> tab;
    uint64_t claimed = 0, kmers = 0;
    size_t bytes(uint32_t n_sub) const { return ((size_t)n_sub << cap_log2) * 8; }
};

// what a finished bucket range of one k hands on: its sorted file words on the device and the buckets' sizes
struct RangeOut {
    int ki;
    uint32_t lo, hi;
    const uint64_t *d_words;
    uint64_t n;
    const uint32_t *sizes; // [hi - lo]
};

struct Counter {
    int device;
    hipStream_t st = nullptr;
    bool own_stream = false;
    Hooks hooks;
    uint32_t min_count = 1;
    size_t budget = 0;
    std::vector<KTable> tabs;
    uint32_t lo = 0, hi = N_BUCKETS;
    np2h::DevBuf<uint8_t> d_in;
    np2h::DevBuf<uint64_t> d_ctr, d_spill[2];
    np2h::PinnedBuf pin_ctr;
    np2h::DevEvent ev0, ev1;
    Stats stats;
    bool qc = false; // pieces of both streams: the quality filter, or the adapter trimmer, runs in front of the count kernel
    np2h::SrqcDev qcd;
    uint64_t qc_totals[np2srqc::N_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    bool ad = false; // ... the adapter trimmer
    np2h::AdDev add;
    uint64_t ad_totals[np2sradapt::N_TOTALS] = {};

    ~Counter() {
        if (st && own_stream) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
    void init(hipStream_t given, uint64_t mem_bytes) {
        HIPCHK(hipSetDevice(device));
        if (given) st = given;
        else {
            HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            own_stream = true;
        }
        ev0.make(), ev1.make();
        budget = mem_bytes;
        if (!budget) {
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            budget = fr / 2;
        }
        d_in.ensure(HALO + hooks.piece + 64);
        d_spill[0].ensure(hooks.piece);
        d_ctr.ensure((size_t)np2::KC_N_CTR * tabs.size());
        pin_ctr.ensure(np2::KC_N_CTR * 8);
        if (ad) add.init(st, hooks.piece);
        else if (qc) qcd.init(st, hooks.piece);
    }
    np2::KcTable kt(const KTable &t) const { return np2::KcTable{t.tab->p, t.cap_log2, lo, hi}; }
    uint64_t *ctr(size_t ki) { return d_ctr.p + ki * np2::KC_N_CTR; }
    size_t tables_bytes() const {
        size_t b = 0;
        for (auto &t : tabs) b += t.tab ? t.bytes(hi - lo) : 0;
        return b;
    }
    const uint64_t *read_ctr(size_t ki) { // (synchronises the stream)
        uint64_t *h = (uint64_t *)pin_ctr.p;
        HIPCHK(hipMemcpyAsync(h, ctr(ki), np2::KC_N_CTR * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return h;
    }
    void begin_range(uint32_t lo_, uint32_t hi_) {
        lo = lo_, hi = hi_;
        for (auto &t : tabs) {
            t.cap_log2 = hooks.cap_log2;
            t.claimed = 0;
            t.tab = std::make_shared<np2h::DevBuf<uint64_t>>();
            const size_t slots = (size_t)(hi - lo) << t.cap_log2;
            t.tab->ensure(slots);
            HIPCHK(hipMemsetAsync(t.tab->p, 0xFF, slots * 8, st));
        }
        HIPCHK(hipMemsetAsync(d_ctr.p, 0, np2::KC_N_CTR * 8 * tabs.size(), st));
        if (ad) add.zero(st); // (every pass filters again: the totals are one pass's)
        else if (qc) qcd.zero(st);
    }
    // the table of tabs[ki] with twice the capacity (or more, should a sub-table of the new one fill)
    void grow(size_t ki) {
        KTable &t = tabs[ki];
        for (uint32_t cl = t.cap_log2 + 1;; ++cl) {
            const size_t slots = (size_t)(hi - lo) << cl;
            if (cl > 40 || tables_bytes() + slots * 8 > budget) throw NeedPasses();
            auto nt = std::make_shared<np2h::DevBuf<uint64_t>>();
            nt->ensure(slots);
            HIPCHK(hipMemsetAsync(nt->p, 0xFF, slots * 8, st));
            HIPCHK(hipMemsetAsync(ctr(ki) + np2::KC_REHASH_FAIL, 0, 8, st));
            np2::launch_kcount_rehash(st, kt(t), np2::KcTable{nt->p, cl, lo, hi}, ctr(ki));
            const bool failed = read_ctr(ki)[np2::KC_REHASH_FAIL] != 0;
            if (failed) continue; // (nt is released; the old table is untouched)
            t.tab = nt;
            t.cap_log2 = cl;
            ++stats.growths;
            return;
        }
    }
    void count_piece(Piece &pc) {
        const size_t n = pc.n;
        HIPCHK(hipMemcpyAsync(d_in.p, pc.buf, np2h::pad_piece(pc.buf, n), hipMemcpyHostToDevice, st));
        if (ad) add.run(st, d_in.p, pc.qc, nullptr);
        else if (qc) qcd.run(st, d_in.p, pc.qc, nullptr);
        for (size_t ki = 0; ki < tabs.size(); ++ki) {
            KTable &t = tabs[ki];
            while (t.claimed + n > ((uint64_t)(hi - lo) << t.cap_log2) / 2) grow(ki);
            HIPCHK(hipMemsetAsync(ctr(ki) + np2::KC_SPILLED, 0, 8, st));
            HIPCHK(hipEventRecord(ev0.e, st));
            np2::launch_kcount(st, d_in.p, n, t.k, kt(t), ctr(ki), d_spill[0].p);
            HIPCHK(hipEventRecord(ev1.e, st));
            const uint64_t *c = read_ctr(ki);
            stats.kernel_ms += np2h::elapsed(ev0, ev1);
            t.claimed = c[np2::KC_CLAIMED];
            t.kmers = c[np2::KC_KMERS];
            uint64_t n_spill = c[np2::KC_SPILLED];
            stats.spilled += n_spill;
            int from = 0;
            while (n_spill) { // a sub-table filled: a larger table, then the list again through the same insert
                grow(ki);
                d_spill[from ^ 1].ensure(n_spill);
                HIPCHK(hipMemsetAsync(ctr(ki) + np2::KC_SPILLED, 0, 8, st));
                np2::launch_kcount_insert_hashes(st, d_spill[from].p, n_spill, kt(t), ctr(ki), d_spill[from ^ 1].p);
                c = read_ctr(ki);
                t.claimed = c[np2::KC_CLAIMED];
                n_spill = c[np2::KC_SPILLED];
                from ^= 1;
            }
        }
    }

    // one pass over the source for the current bucket range
    void stream_source(const Source &src) {
        PieceQueue q;
        const bool paired = ad && (add.o.flags & np2sradapt::PAIRED);
        const size_t n_threads = src.mem ? 1 : paired ? std::min<size_t>(src.paths.size() / 2, 5) : std::min<size_t>(src.paths.size(), 16);
        std::vector<Piece> pieces(2 * n_threads);
        np2h::PinnedBlocks pinned;
        for (auto &p : pieces) {
            p.buf = pinned.get(HALO + hooks.piece + 64);
            if (qc) {
                p.qc.seq = p.buf, p.qc.owner = &p;
                p.qc.qual = pinned.get(HALO + hooks.piece + 64);
            }
            q.idle.push_back(&p);
        }
        auto readers = np2h::run_readers(n_threads, q, [&](size_t ti) {
            if (qc) { // both streams, in pieces that end at a read boundary
                np2h::QcAssembler as(hooks.piece, false);
                as.take = [&]() -> np2h::QcPiece * {
                    Piece *p = q.take_idle();
                    return p ? &p->qc : nullptr;
                };
                as.full = [&](np2h::QcPiece *c) {
                    Piece *p = (Piece *)c->owner;
                    p->n = c->n;
                    q.give_full(p);
                };
                as.unused = [&](np2h::QcPiece *c) { q.give_idle((Piece *)c->owner); };
                if (paired)
                    for (size_t fi = ti; 2 * fi < src.paths.size() && !as.dead; fi += n_threads) np2h::pair_files(as, src.paths[2 * fi], src.paths[2 * fi + 1]);
                else
                    for (size_t fi = ti; fi < src.paths.size() && !as.dead; fi += n_threads) as.file(src.paths[fi]);
                as.flush();
            } else {
                PieceWriter w(q, hooks.piece);
                auto put = [&](const uint8_t *p, size_t n) { w.put(p, n); };
                if (src.mem) {
                    put(src.mem, src.mem_n);
                    static const uint8_t NL = '\n';
                    put(&NL, 1);
                } else {
                    for (size_t fi = ti; fi < src.paths.size() && !w.dead; fi += n_threads) {
                        parse_file(src.paths[fi], put, [&] { return w.dead; }); // (its stream ends with a separator)
                    }
                }
                w.flush();
            }
        });
        for (;;) { // read_ms: what the counting thread waits for its readers (the part of the pass the input bounds)
            const double t0 = np2h::now_ms();
            Piece *p = q.take_full();
            stats.read_ms += (float)(np2h::now_ms() - t0);
            if (!p) break;
            count_piece(*p);
            q.give_idle(p);
        }
        if (q.err_code != NP2_OK) throw Np2Error(q.err_code, q.err);
        if (ad) add.totals(st, ad_totals);
        else if (qc) qcd.totals(st, qc_totals);
    }

    // the current range of tabs[ki] as sorted file words on the device
    struct Emitted {
        np2h::DevBuf<uint64_t> keys_in, keys_out, d_off;
        np2h::DevBuf<uint32_t> cnt_in, cnt_out, d_sizes;
        np2h::DevBuf<uint8_t> tmp;
        std::vector<uint32_t> sizes;
        uint64_t n = 0, max_bucket = 0;
        const uint64_t *words() const { return keys_in.p; }
    };
    void bucket_sizes(size_t ki, uint32_t minc, Emitted &e) {
        const uint32_t n_sub = hi - lo;
        e.d_sizes.ensure(n_sub);
        e.sizes.resize(n_sub);
        np2::launch_kcount_bucket_sizes(st, kt(tabs[ki]), minc, e.d_sizes.p);
        HIPCHK(hipMemcpyAsync(e.sizes.data(), e.d_sizes.p, n_sub * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        e.n = 0, e.max_bucket = 0;
        for (uint32_t s : e.sizes) e.n += s, e.max_bucket = std::max<uint64_t>(e.max_bucket, s);
    }
    void emit(size_t ki, Emitted &e) {
        bucket_sizes(ki, min_count, e);
        if (e.n == 0) return;
        e.keys_in.ensure(e.n), e.keys_out.ensure(e.n), e.cnt_in.ensure(e.n), e.cnt_out.ensure(e.n);
        const size_t tmp_bytes = np2::prim_temp_bytes(e.n);
        e.tmp.ensure(tmp_bytes);
        std::vector<uint64_t> off(e.sizes.size() + 1, 0);
        for (size_t b = 0; b < e.sizes.size(); ++b) off[b + 1] = off[b] + e.sizes[b];
        e.d_off.ensure(off.size());
        HIPCHK(hipMemcpyAsync(e.d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // (`off` is pageable and leaves scope)
        np2::launch_kcount_emit(st, kt(tabs[ki]), min_count, e.d_off.p, e.keys_in.p, e.cnt_in.p);
        // ascending (bucket, slot key) = bucket-major, ascending word order inside every bucket
        if (np2::prim_sort_pairs_u64_u32(st, e.tmp.p, tmp_bytes, e.keys_in.p, e.keys_out.p, e.cnt_in.p, e.cnt_out.p, e.n, 62))
            throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
        np2::launch_kcount_words(st, e.keys_out.p, e.cnt_out.p, e.n, e.keys_in.p);
        HIPCHK(hipStreamSynchronize(st));
    }
};

// Counts `src` for every k; `on_range(RangeOut)` receives every finished bucket range (ascending ranges per k), `on_reset`
// is called when the run starts over with more passes.  With `resident` (single pass only) the tables stay in `c.tabs`.
void run_count(Counter &c, const Source &src, bool resident, const std::function<void(const RangeOut &)> &on_range,
               const std::function<void()> &on_reset) {
    uint32_t P = c.hooks.passes ? c.hooks.passes : 1;
    const char *no_pass_msg = "the k-mer tables of these reads do not fit the memory budget in one pass, and a polish context is built in one "
                              "pass only: count to dumps (np2_kcount_files_to_dumps) or raise mem_bytes";
    for (;;) {
        if (resident && P > 1) throw Np2Error(NP2_E_NOMEM, no_pass_msg);
        c.stats = Stats();
        c.stats.passes = P;
        try {
            for (uint32_t p = 0; p < P; ++p) {
                c.begin_range(N_BUCKETS * p / P, N_BUCKETS * (p + 1) / P);
                c.stream_source(src);
                for (auto &t : c.tabs) c.stats.kmers += t.kmers, c.stats.distinct += t.claimed;
                if (resident) return;
                for (size_t ki = 0; ki < c.tabs.size(); ++ki) {
                    Counter::Emitted e;
                    c.emit(ki, e);
                    on_range(RangeOut{(int)ki, c.lo, c.hi, e.words(), e.n, e.sizes.data()});
                    c.tabs[ki].tab.reset();
                }
            }
            return;
        } catch (const NeedPasses &) {
            for (auto &t : c.tabs) t.tab.reset();
            if (resident) throw Np2Error(NP2_E_NOMEM, no_pass_msg);
            if (P >= N_BUCKETS) throw Np2Error(NP2_E_NOMEM, "the k-mer table of one bucket does not fit the memory budget: raise mem_bytes");
            if (!src.mem && !src.rescannable())
                throw Np2Error(NP2_E_ARG, "the k-mer tables need several passes over the input within this memory budget, and an input "
                                          "that is not a regular file (a pipe?) cannot be read again: give files or raise mem_bytes");
            P = std::min<uint32_t>(P * 2, N_BUCKETS);
            on_reset();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// argument checks (before the first HIP call)
// ---------------------------------------------------------------------------------------------------------------
void check_ks(const uint32_t *ks, int n_k) {
    if (!ks || n_k < 1 || n_k > NP2_MAX_YAK) throw Np2Error(NP2_E_ARG, "the number of k values must be in [1, 15]");
    for (int i = 0; i < n_k; ++i)
        if (ks[i] >= 32 || ks[i] < 2)
            throw Np2Error(NP2_E_UNSUPPORTED, "k = " + std::to_string(ks[i]) + ", prefix bits = 10: only k < 32 with the default 10 prefix bits is supported");
}
void check_paths(const char *const *paths, int n_paths, Source &src) {
    if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "no sequence file given");
    for (int i = 0; i < n_paths; ++i) {
        if (!paths[i]) throw Np2Error(NP2_E_ARG, "a sequence file path is NULL");
        FILE *f = fopen(paths[i], "rb");
        if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + paths[i]);
        fclose(f);
        src.paths.push_back(paths[i]);
    }
}
uint32_t min_count_of(const np2_kcount_opts_t *o) {
    const uint32_t m = o ? o->min_count : 1;
    if (m > COUNT_MAX) throw Np2Error(NP2_E_ARG, "min_count must be at most 1023");
    return std::max(1u, m);
}

void setup(Counter &c, int device, const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts, hipStream_t st,
           const np2srqc::Opts *qc = nullptr, const np2sradapt::Opts *ad = nullptr) {
    c.device = device;
    c.qc = qc != nullptr || ad != nullptr;
    c.ad = ad != nullptr;
    if (ad) c.add.o = *ad, c.add.qc = qc ? *qc : np2h::sradapt_qc(nullptr);
    else if (qc) c.qcd.o = *qc;
    c.min_count = min_count_of(opts);
    c.tabs.resize(n_k);
    for (int i = 0; i < n_k; ++i) c.tabs[i].k = ks[i];
    c.init(st, opts ? opts->mem_bytes : 0);
}

// host arrays of one k, filled range by range
struct HostYak {
    std::vector<uint64_t> off = std::vector<uint64_t>(N_BUCKETS + 1, 0);
    uint64_t *words = nullptr;
    uint64_t n = 0, cap = 0;
    ~HostYak() { free(words); }
    void reset() { n = 0, std::fill(off.begin(), off.end(), 0); }
    void take(const RangeOut &r, hipStream_t st) {
        if (n + r.n > cap || !words) {
            cap = std::max<uint64_t>(n + r.n, cap * 2) + 1;
            uint64_t *w = (uint64_t *)realloc(words, cap * 8);
            if (!w) throw Np2Error(NP2_E_NOMEM, "out of memory for the k-mer table");
            words = w;
        }
        if (r.n) {
            HIPCHK(hipMemcpyAsync(words + n, r.d_words, r.n * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        for (uint32_t b = r.lo; b < r.hi; ++b) off[b + 1] = off[b] + r.sizes[b - r.lo];
        for (uint32_t b = r.hi; b < N_BUCKETS; ++b) off[b + 1] = off[r.hi];
        n += r.n;
    }
};

// the options of a *_qc call, checked; nullptr without them
const np2srqc::Opts *qc_of(const np2_srqc_opts_t *qc, np2srqc::Opts &store) {
    if (!qc) return nullptr;
    store = np2h::srqc_checked(qc);
    (void)np2h::srqc_piece_bytes();
    return &store;
}
// the options of a *_ad call, checked; nullptr without them.  Pair mode takes the paths two by two.
const np2sradapt::Opts *ad_of(const np2_sradapt_opts_t *ad, int n_paths, np2sradapt::Opts &store) {
    if (!ad) return nullptr;
    store = np2h::sradapt_checked(ad);
    (void)np2h::srqc_piece_bytes();
    if ((store.flags & np2sradapt::PAIRED) && n_paths % 2) throw Np2Error(NP2_E_ARG, "pair mode takes the files as R1 R2 R1 R2 ..: their number is odd");
    return &store;
}
void publish_qc(const Counter &c) {
    if (c.ad) np2h::sradapt_publish(c.ad_totals, c.add.kernel_ms);
    else if (c.qc) np2h::srqc_publish(c.qc_totals, c.qcd.kernel_ms);
}

int count_to_host(int device, const Source &src, const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts, np2_yak_t *out,
                  const np2srqc::Opts *qc = nullptr, const np2sradapt::Opts *ad = nullptr) {
    Counter c;
    setup(c, device, ks, n_k, opts, nullptr, qc, ad);
    std::vector<HostYak> hy(n_k);
    run_count(c, src, false, [&](const RangeOut &r) { hy[r.ki].take(r, c.st); }, [&] { for (auto &h : hy) h.reset(); });
    std::vector<uint64_t *> offs;
    for (int i = 0; i < n_k; ++i) {
        uint64_t *o = (uint64_t *)malloc((N_BUCKETS + 1) * 8);
        if (!o || (!hy[i].words && !(hy[i].words = (uint64_t *)malloc(8)))) {
            free(o);
            for (auto p : offs) free(p);
            throw Np2Error(NP2_E_NOMEM, "out of memory for the k-mer table");
        }
        memcpy(o, hy[i].off.data(), (N_BUCKETS + 1) * 8);
        offs.push_back(o);
    }
    for (int i = 0; i < n_k; ++i) {
        out[i].k = ks[i], out[i].pre = PRE, out[i].n_words = hy[i].n;
        out[i].words = hy[i].words, out[i].bucket_off = offs[i];
        hy[i].words = nullptr;
    }
    g_stats = c.stats;
    publish_qc(c);
    return NP2_OK;
}

struct DumpFile {
    std::string path;
    FILE *f = nullptr;
    ~DumpFile() {
        if (f) fclose(f);
    }
    void put(const void *p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) throw Np2Error(NP2_E_ARG, "cannot write " + path);
    }
    void start(uint32_t k) {
        if (f) fclose(f);
        f = fopen(path.c_str(), "wb");
        if (!f) throw Np2Error(NP2_E_ARG, "cannot open " + path + " for writing");
        const uint32_t hd[3] = {k, PRE, COUNT_BITS};
        put("YAK\2", 4);
        put(hd, 12);
    }
    // a range's buckets, the words brought over in pieces of 1 Mi words (no host copy of a whole table)
    void take(const RangeOut &r, hipStream_t st, std::vector<uint64_t> &stage) {
        const uint64_t CH = (uint64_t)1 << 20;
        stage.resize(CH);
        uint64_t have_lo = 0, have_hi = 0, at = 0; // stage holds words [have_lo, have_hi)
        for (uint32_t b = r.lo; b < r.hi; ++b) {
            const uint32_t hd[2] = {0u, r.sizes[b - r.lo]};
            put(hd, 8);
            uint64_t left = hd[1];
            while (left) {
                if (at >= have_hi) {
                    have_lo = at, have_hi = std::min(r.n, at + CH);
                    HIPCHK(hipMemcpyAsync(stage.data(), r.d_words + have_lo, (have_hi - have_lo) * 8, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                }
                const uint64_t take = std::min(left, have_hi - at);
                put(stage.data() + (at - have_lo), take * 8);
                at += take, left -= take;
            }
        }
    }
};

} // namespace

np2h::ResidentCount np2h::kcount_resident(int device, hipStream_t stream, const uint8_t *sep_stream, uint64_t n, uint32_t k) {
    check_ks(&k, 1);
    static const uint8_t none = '\n';
    Source src;
    src.mem = n ? sep_stream : &none, src.mem_n = n;
    Counter c;
    setup(c, device, &k, 1, nullptr, stream);
    run_count(c, src, true, [](const RangeOut &) {}, [] {});
    HIPCHK(hipStreamSynchronize(c.st));
    g_stats = c.stats;
    return ResidentCount{c.tabs[0].tab, c.tabs[0].cap_log2, c.tabs[0].claimed};
}

extern "C" {

int np2_seqfile_stream(const char *path, uint8_t **out, uint64_t *n) {
    if (!out || !n || !path) return np2h::io_set_error(NP2_E_ARG, "np2_seqfile_stream: NULL argument");
    *out = nullptr, *n = 0;
    return np2h::abi_guard([&] {
        std::vector<uint8_t> s;
        parse_file(path, [&](const uint8_t *p, size_t m) { s.insert(s.end(), p, p + m); }, nullptr);
        uint8_t *o = (uint8_t *)malloc(s.size() + 1);
        if (!o) throw Np2Error(NP2_E_NOMEM, "out of memory");
        memcpy(o, s.data(), s.size());
        *out = o, *n = s.size();
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_kcount_files(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                     const np2_kcount_opts_t *opts, np2_yak_t *out) {
    return np2_kcount_files_qc(device, paths, n_paths, ks, n_k, opts, nullptr, out);
}

int np2_kcount_files_qc(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                        const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, np2_yak_t *out) {
    return np2_kcount_files_ad(device, paths, n_paths, ks, n_k, opts, qc, nullptr, out);
}

int np2_kcount_files_ad(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts,
                        const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad, np2_yak_t *out) {
    return np2h::abi_guard([&] {
        if (!out) throw Np2Error(NP2_E_ARG, "np2_kcount_files: out is NULL");
        check_ks(ks, n_k);
        (void)min_count_of(opts);
        np2srqc::Opts qo;
        const np2srqc::Opts *q = qc_of(qc, qo);
        np2sradapt::Opts ao;
        const np2sradapt::Opts *a = ad_of(ad, n_paths, ao);
        Source src;
        check_paths(paths, n_paths, src);
        return count_to_host(device, src, ks, n_k, opts, out, q, a);
    }, np2h::io_set_error);
}

int np2_kcount_bytes(int device, const uint8_t *seq, uint64_t n, const uint32_t *ks, int n_k, const np2_kcount_opts_t *opts,
                     np2_yak_t *out) {
    return np2h::abi_guard([&] {
        if (!out || (n && !seq)) throw Np2Error(NP2_E_ARG, "np2_kcount_bytes: NULL argument");
        check_ks(ks, n_k);
        (void)min_count_of(opts);
        static const uint8_t none = '\n';
        Source src;
        src.mem = n ? seq : &none, src.mem_n = n;
        return count_to_host(device, src, ks, n_k, opts, out);
    }, np2h::io_set_error);
}

int np2_kcount_files_to_dumps(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                              const np2_kcount_opts_t *opts, const char *const *out_paths) {
    return np2_kcount_files_to_dumps_qc(device, paths, n_paths, ks, n_k, opts, nullptr, out_paths);
}

int np2_kcount_files_to_dumps_qc(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const char *const *out_paths) {
    return np2_kcount_files_to_dumps_ad(device, paths, n_paths, ks, n_k, opts, qc, nullptr, out_paths);
}

int np2_kcount_files_to_dumps_ad(int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad,
                                 const char *const *out_paths) {
    return np2h::abi_guard([&] {
        check_ks(ks, n_k);
        (void)min_count_of(opts);
        np2srqc::Opts qo;
        const np2srqc::Opts *q = qc_of(qc, qo);
        np2sradapt::Opts ao;
        const np2sradapt::Opts *a = ad_of(ad, n_paths, ao);
        if (!out_paths) throw Np2Error(NP2_E_ARG, "np2_kcount_files_to_dumps: out_paths is NULL");
        for (int i = 0; i < n_k; ++i)
            if (!out_paths[i]) throw Np2Error(NP2_E_ARG, "np2_kcount_files_to_dumps: an output path is NULL");
        Source src;
        check_paths(paths, n_paths, src);
        Counter c;
        setup(c, device, ks, n_k, opts, nullptr, q, a);
        std::vector<DumpFile> dumps(n_k);
        for (int i = 0; i < n_k; ++i) dumps[i].path = out_paths[i], dumps[i].start(ks[i]);
        std::vector<uint64_t> stage;
        run_count(c, src, false, [&](const RangeOut &r) { dumps[r.ki].take(r, c.st, stage); },
                  [&] { for (int i = 0; i < n_k; ++i) dumps[i].start(ks[i]); });
        for (auto &d : dumps) {
            if (fclose(d.f) != 0) {
                d.f = nullptr;
                throw Np2Error(NP2_E_ARG, "cannot write " + d.path);
            }
            d.f = nullptr;
        }
        g_stats = c.stats;
        publish_qc(c);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_ctx_create_from_reads(np2_ctx_t **out, int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                              const np2_kcount_opts_t *opts) {
    return np2_ctx_create_from_reads_qc(out, device, paths, n_paths, ks, n_k, opts, nullptr);
}

int np2_ctx_create_from_reads_qc(np2_ctx_t **out, int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc) {
    return np2_ctx_create_from_reads_ad(out, device, paths, n_paths, ks, n_k, opts, qc, nullptr);
}

int np2_ctx_create_from_reads_ad(np2_ctx_t **out, int device, const char *const *paths, int n_paths, const uint32_t *ks, int n_k,
                                 const np2_kcount_opts_t *opts, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad) {
    if (!out) return np2h::io_set_error(NP2_E_ARG, "np2_ctx_create_from_reads: out is NULL");
    *out = nullptr;
    return np2h::abi_guard([&] {
        check_ks(ks, n_k);
        (void)min_count_of(opts);
        np2srqc::Opts qo;
        const np2srqc::Opts *q = qc_of(qc, qo);
        np2sradapt::Opts ao;
        const np2sradapt::Opts *a = ad_of(ad, n_paths, ao);
        Source src;
        check_paths(paths, n_paths, src);
        std::vector<uint32_t> sk(ks, ks + n_k);
        std::sort(sk.begin(), sk.end()); // option.rs:238: tables ordered by k
        np2_ctx_t *made = nullptr;
        const int rc = np2_ctx_create(&made, device, nullptr, 0);
        if (rc != NP2_OK) return np2h::io_set_error(rc, "np2_ctx_create failed (see stderr)");
        std::unique_ptr<np2_ctx, void (*)(np2_ctx_t *)> cx(made, np2_ctx_destroy);
        {
            Counter c;
            setup(c, device, sk.data(), n_k, opts, cx->stream, q, a);
            run_count(c, src, true, [](const RangeOut &) {}, [] {});
            for (size_t ki = 0; ki < c.tabs.size(); ++ki) {
                KTable &t = c.tabs[ki];
                np2h::YakTable yt;
                yt.k = t.k;
                Counter::Emitted e;
                if (c.min_count <= 1) {
                    // the counting table IS the polisher's: the lookup probes until an EMPTY slot, so every sub-table keeps
                    // the free room np2_ctx_create gives it (capacity >= 2 * words + 2)
                    c.bucket_sizes(ki, 0, e);
                    try {
                        while (((uint64_t)1 << t.cap_log2) < e.max_bucket * 2 + 2) c.grow(ki);
                    } catch (const NeedPasses &) {
                        throw Np2Error(NP2_E_NOMEM, "the k-mer tables of these reads do not fit the memory budget: raise mem_bytes");
                    }
                    yt.cap_log2 = t.cap_log2;
                    yt.table = t.tab;
                } else {
                    // words below min_count dropped: the survivors re-inserted by the dump loader's kernel (boundary form);
                    // deleting from a linear-probing table is not attempted
                    c.emit(ki, e);
                    std::vector<uint64_t> off(N_BUCKETS + 1, 0);
                    for (uint32_t b = 0; b < N_BUCKETS; ++b) off[b + 1] = off[b] + e.sizes[b];
                    uint32_t cl = 4;
                    while ((1ull << cl) < e.max_bucket * 2 + 2) ++cl;
                    const size_t slots = (size_t)N_BUCKETS << cl;
                    t.tab.reset();
                    yt.cap_log2 = cl;
                    yt.table = std::make_shared<np2h::DevBuf<uint64_t>>();
                    yt.table->ensure(slots);
                    HIPCHK(hipMemsetAsync(yt.table->p, 0xFF, slots * 8, c.st));
                    np2h::DevBuf<uint64_t> d_off;
                    np2h::DevBuf<uint32_t> d_dup;
                    d_off.ensure(N_BUCKETS + 1), d_dup.ensure(1);
                    HIPCHK(hipMemsetAsync(d_dup.p, 0, 4, c.st));
                    HIPCHK(hipMemcpyAsync(d_off.p, off.data(), (N_BUCKETS + 1) * 8, hipMemcpyHostToDevice, c.st));
                    HIPCHK(hipStreamSynchronize(c.st));
                    if (e.n) np2::launch_yak_insert(c.st, e.words(), d_off.p, N_BUCKETS, e.max_bucket, yt.table->p, cl, d_dup.p, 0);
                    HIPCHK(hipStreamSynchronize(c.st));
                }
                t.tab.reset();
                cx->yaks.push_back(yt);
            }
            HIPCHK(hipStreamSynchronize(c.st));
            g_stats = c.stats;
            publish_qc(c);
        }
        *out = cx.release();
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_kcount_last_stats(uint64_t *kmers, uint64_t *distinct, uint64_t *spilled, uint32_t *growths, uint32_t *passes,
                          float *kernel_ms, float *read_ms) {
    if (kmers) *kmers = g_stats.kmers;
    if (distinct) *distinct = g_stats.distinct;
    if (spilled) *spilled = g_stats.spilled;
    if (growths) *growths = g_stats.growths;
    if (passes) *passes = g_stats.passes;
    if (kernel_ms) *kernel_ms = g_stats.kernel_ms;
    if (read_ms) *read_ms = g_stats.read_ms;
    return NP2_OK;
}

} // extern "C"
