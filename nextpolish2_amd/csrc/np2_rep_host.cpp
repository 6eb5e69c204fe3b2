// Host driver of the repetitive k-mer list (include/np2_io.h: np2_rep_bytes, np2_rep_files; kernels: np2_rep.hip).
//
// The separator stream goes to the device in pieces (8 MiB; NP2_REP_TEST_PIECE), each with the last 32 bytes of the stream
// before it in front (the halo), so an assembly is never resident as text and a k-mer that straddles two pieces is counted
// once, with the piece that holds its last byte.  The calling thread parses (np2_seqreader.hpp) into one of two pinned
// buffers while the stream copies and counts the other; there is one device buffer, so piece i + 1 is copied after piece i
// was counted.  Then one pass over the counters for the selection (a second one only when the threshold is 65 536 or more),
// the per-chunk sizes, their scan (rocPRIM, np2_prims.hip) and the ordered scatter.
//
// The table is the call's own hipMalloc block, released when the call returns: 4 GiB at k = 15 are not left in the device
// cache of a process that goes on to polish.
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_rep.hpp"
#include "np2_rep_core.hpp"
#include "np2_seqreader.hpp"

#include <sys/stat.h>

#include <cmath>

namespace {
using np2h::Np2Error;
using np2kc::HALO;

struct Opts {
    uint32_t k = np2rep::K_DEFAULT;
    bool use_min_count = false;
    uint32_t min_count = 0;
    double distinct = 0.9998;
};
Opts checked(const np2_rep_opts_t *o) {
    if (!o) throw Np2Error(NP2_E_ARG, "np2_rep: opts is NULL");
    if (o->k < np2rep::K_MIN || o->k > np2rep::K_MAX)
        throw Np2Error(NP2_E_UNSUPPORTED, "k = " + std::to_string(o->k) + ": the repetitive k-mer list is built for 2 <= k <= 16");
    Opts r;
    r.k = o->k, r.use_min_count = o->use_min_count != 0, r.min_count = o->min_count, r.distinct = o->distinct;
    if (!r.use_min_count && !(r.distinct >= 0.0 && r.distinct <= 1.0)) // (NaN fails both comparisons)
        throw Np2Error(NP2_E_ARG, "distinct must be a fraction in [0, 1]");
    return r;
}
void check_kmers(uint64_t stream_bytes, uint32_t k) {
    if (np2rep::max_kmers(stream_bytes, k) > np2rep::MAX_KMERS)
        throw Np2Error(NP2_E_UNSUPPORTED, "the input could hold more than 2^32 - 1 k-mers: a counter is 32 bits wide");
}

struct Hooks {
    size_t piece = (size_t)8 << 20;
    bool collapse = true;
    Hooks() { // read once per call, like the other NP2_* switches
        piece = (size_t)np2h::test_hook("NP2_REP_TEST_PIECE", 64, LLONG_MAX, (long long)piece);
        collapse = getenv("NP2_REP_NO_COLLAPSE") == nullptr; // (tools/rep_probe.py's A/B)
    }
};

using np2h::elapsed;

struct Run {
    int device = 0;
    Opts o;
    Hooks hooks;
    hipStream_t st = nullptr;
    uint32_t *table = nullptr;
    uint64_t table_n = 0;
    np2h::DevBuf<uint8_t> d_in;
    np2_rep_stats_t stats{};
    // the list, host arrays from malloc (np2_free)
    uint32_t *index = nullptr, *count = nullptr;
    uint64_t listed = 0;

    ~Run() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
        if (table) (void)hipFree(table);
        free(index), free(count);
    }

    void init() {
        HIPCHK(hipSetDevice(device));
        table_n = np2rep::table_size(o.k);
        const size_t chunks = (size_t)np2::rep_chunks(table_n) + 1;
        np2h::need_device_bytes(table_n * 4 + chunks * 8 + np2::prim_temp_bytes(chunks) + hooks.piece, (size_t)64 << 20, [&](size_t fr) {
            return "the counter table for k = " + std::to_string(o.k) + " takes " + std::to_string(table_n * 4) +
                   " bytes and does not fit the device's free memory (" + std::to_string(fr) + " bytes)";
        });
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if (hipMalloc((void **)&table, table_n * 4) != hipSuccess) {
            (void)hipGetLastError();
            table = nullptr;
            throw Np2Error(NP2_E_NOMEM, "the counter table for k = " + std::to_string(o.k) + " (" + std::to_string(table_n * 4) +
                                            " bytes) could not be allocated on the device");
        }
        np2h::poison_device(table, table_n * 4); // (a block of its own, not a pool's: the test hook sees it all the same)
        HIPCHK(hipMemsetAsync(table, 0, table_n * 4, st));
        d_in.cached = true; // (released after ~Run has drained the stream)
        d_in.ensure(HALO + hooks.piece + 64);
    }
};

// the stream, piece by piece, into the counters: the writer's two pieces are this thread's own, filled and counted in turn
struct Feeder {
    struct Piece {
        uint8_t *buf = nullptr;
        size_t n = 0;
    };
    Run &r;
    np2h::PinnedBuf pinned[2];
    Piece pc[2];
    np2h::DevEvent k0[2], k1[2];
    bool in_flight[2] = {false, false};
    int cur = 0;
    uint64_t stream_bytes = 0;
    np2h::HaloWriter<Piece> w;
    explicit Feeder(Run &r_) : r(r_), w(r_.hooks.piece) {
        for (int b = 0; b < 2; ++b) {
            pc[b].buf = (uint8_t *)pinned[b].ensure(HALO + r.hooks.piece + 64);
            k0[b].make(), k1[b].make();
        }
        w.take = [this] {
            retire(cur);
            return &pc[cur];
        };
        w.full = [this](Piece *p) { count(*p); };
        w.unused = [](Piece *) {};
    }
    ~Feeder() { (void)hipStreamSynchronize(r.st); } // (a copy out of a pinned buffer may be in flight when an exception unwinds)
    void retire(int b) { // the piece that last used buffer b has been copied and counted
        if (!in_flight[b]) return;
        HIPCHK(hipEventSynchronize(k1[b].e));
        r.stats.count_ms += elapsed(k0[b], k1[b]);
        in_flight[b] = false;
    }
    void count(Piece &p) { // (p is pc[cur])
        stream_bytes += p.n;
        check_kmers(stream_bytes, r.o.k);
        HIPCHK(hipMemcpyAsync(r.d_in.p, p.buf, np2h::pad_piece(p.buf, p.n), hipMemcpyHostToDevice, r.st));
        HIPCHK(hipEventRecord(k0[cur].e, r.st));
        np2::launch_rep_count(r.st, r.d_in.p, p.n, r.o.k, r.table, r.hooks.collapse);
        HIPCHK(hipEventRecord(k1[cur].e, r.st));
        in_flight[cur] = true;
        cur ^= 1;
    }
    void put(const uint8_t *p, size_t len) { w.put(p, len); }
    void finish() {
        w.flush();
        retire(0), retire(1);
        HIPCHK(hipGetLastError());
    }
};

// counters -> threshold -> the list on the host
void select_and_emit(Run &r) {
    hipStream_t st = r.st;
    const uint32_t blocks = np2h::grid_blocks(r.device, 8); // 16 KiB of LDS a block
    np2h::DevBuf<uint32_t> d_hist; // high halves, then low halves
    np2h::DevBuf<unsigned long long> d_ctr;
    np2h::DevBuf<uint32_t> d_sizes, d_off, d_index, d_count;
    np2h::DevBuf<uint8_t> tmp;
    // (every buffer here is released after the read-back of what its kernels wrote)
    d_hist.cached = d_ctr.cached = d_sizes.cached = d_off.cached = d_index.cached = d_count.cached = tmp.cached = true;
    d_hist.ensure(2 * np2::REP_HALF), d_ctr.ensure(np2::REP_N_CTR);
    np2h::PinnedBuf pin;
    uint32_t *h_hist = (uint32_t *)pin.ensure(2 * np2::REP_HALF * 4 + np2::REP_N_CTR * 8 + 8);
    unsigned long long *h_ctr = (unsigned long long *)(h_hist + 2 * np2::REP_HALF);
    np2h::DevEvent e0, e1;
    e0.make(), e1.make();

    HIPCHK(hipMemsetAsync(d_hist.p, 0, 2 * np2::REP_HALF * 4, st));
    HIPCHK(hipMemsetAsync(d_ctr.p, 0, np2::REP_N_CTR * 8, st));
    HIPCHK(hipEventRecord(e0.e, st));
    np2::launch_rep_hist(st, r.table, r.table_n, 0, true, d_hist.p, d_hist.p + np2::REP_HALF, d_ctr.p, blocks);
    HIPCHK(hipEventRecord(e1.e, st));
    HIPCHK(hipMemcpyAsync(h_hist, d_hist.p, 2 * np2::REP_HALF * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_ctr, d_ctr.p, np2::REP_N_CTR * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r.stats.select_ms = elapsed(e0, e1);
    r.stats.distinct = h_ctr[np2::REP_DISTINCT];
    r.stats.kmers = h_ctr[np2::REP_TOTAL];
    r.stats.max_count = (uint32_t)h_ctr[np2::REP_MAX];

    uint32_t threshold = 0;
    if (r.o.use_min_count) {
        threshold = r.o.min_count;
    } else if (r.stats.distinct) {
        const uint64_t target = np2rep::target_of(r.o.distinct, r.stats.distinct);
        std::vector<uint64_t> occ(np2::REP_HALF);
        for (uint32_t i = 0; i < np2::REP_HALF; ++i) occ[i] = h_hist[i];
        uint64_t before = 0, before_lo = 0;
        const uint64_t bin = np2rep::select_entry(occ.data(), np2::REP_HALF, target, &before);
        if (bin >= np2::REP_HALF) throw Np2Error(NP2_E_DEVICE, "np2_rep: the histogram of the counters does not add up");
        if (bin != 0) { // the low halves of another bin: one more pass
            HIPCHK(hipMemsetAsync(d_hist.p + np2::REP_HALF, 0, np2::REP_HALF * 4, st));
            HIPCHK(hipEventRecord(e0.e, st));
            np2::launch_rep_hist(st, r.table, r.table_n, (uint32_t)bin, false, d_hist.p, d_hist.p + np2::REP_HALF, d_ctr.p, blocks);
            HIPCHK(hipEventRecord(e1.e, st));
            HIPCHK(hipMemcpyAsync(h_hist + np2::REP_HALF, d_hist.p + np2::REP_HALF, np2::REP_HALF * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            r.stats.select_ms += elapsed(e0, e1);
        }
        for (uint32_t i = 0; i < np2::REP_HALF; ++i) occ[i] = h_hist[np2::REP_HALF + i];
        const uint64_t lo = np2rep::select_entry(occ.data(), np2::REP_HALF, target - before, &before_lo);
        if (lo >= np2::REP_HALF) throw Np2Error(NP2_E_DEVICE, "np2_rep: the histogram of the counters does not add up");
        threshold = (uint32_t)(bin << 16 | lo);
    }
    r.stats.threshold = threshold;
    if (r.stats.max_count <= threshold) return; // nothing is listed

    const size_t chunks = (size_t)np2::rep_chunks(r.table_n);
    d_sizes.ensure(chunks + 1), d_off.ensure(chunks + 1);
    const size_t tmp_bytes = np2::prim_temp_bytes(chunks + 1);
    tmp.ensure(tmp_bytes);
    uint32_t *h_total = (uint32_t *)(h_ctr + np2::REP_N_CTR);
    HIPCHK(hipMemsetAsync(d_sizes.p + chunks, 0, 4, st));
    HIPCHK(hipEventRecord(e0.e, st));
    np2::launch_rep_sizes(st, r.table, r.table_n, threshold, d_sizes.p);
    if (np2::prim_exclusive_sum_u32(st, tmp.p, tmp_bytes, d_sizes.p, d_off.p, chunks + 1))
        throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
    HIPCHK(hipEventRecord(e1.e, st));
    HIPCHK(hipMemcpyAsync(h_total, d_off.p + chunks, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r.stats.emit_ms = elapsed(e0, e1);
    const uint64_t listed = *h_total;
    if (listed == 0) return;
    r.index = (uint32_t *)malloc(listed * 4), r.count = (uint32_t *)malloc(listed * 4);
    if (!r.index || !r.count) throw Np2Error(NP2_E_NOMEM, "out of memory for the k-mer list");
    d_index.ensure(listed), d_count.ensure(listed);
    HIPCHK(hipEventRecord(e0.e, st));
    np2::launch_rep_emit(st, r.table, r.table_n, threshold, d_off.p, d_index.p, d_count.p);
    HIPCHK(hipEventRecord(e1.e, st));
    HIPCHK(hipMemcpyAsync(r.index, d_index.p, listed * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.count, d_count.p, listed * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    r.stats.emit_ms += elapsed(e0, e1);
    r.listed = listed;
    r.stats.listed = listed;
    for (uint64_t i = 0; i < listed; ++i) r.stats.listed_occurrences += r.count[i];
}

// what a plain (not gzip) file can add to the stream at most: its size, and a separator its last line may lack
uint64_t plain_bound(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + path);
    uint8_t magic[2] = {0, 0};
    const size_t got = fread(magic, 1, 2, f);
    fclose(f);
    struct stat sb;
    if (got == 2 && magic[0] == 0x1F && magic[1] == 0x8B) return 0; // gzip: known only as it is read
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return 0;
    return (uint64_t)sb.st_size + 1;
}

void write_list(const Run &r, const char *out_path, bool both) {
    FILE *f = fopen(out_path, "wb");
    if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + out_path + " for writing");
    std::unique_ptr<FILE, int (*)(FILE *)> guard(f, fclose);
    const uint32_t k = r.o.k;
    char line[np2rep::K_MAX + 16];
    bool ok = true;
    for (uint64_t i = 0; i < r.listed && ok; ++i) {
        const uint32_t v = r.index[i], rc = np2rep::revcomp(v, k);
        np2rep::index_text(v, k, line);
        const int m = snprintf(line + k, sizeof(line) - k, "\t%u\n", r.count[i]);
        ok = fwrite(line, 1, k + (size_t)m, f) == k + (size_t)m;
        if (both && rc != v && ok) {
            np2rep::index_text(rc, k, line);
            ok = fwrite(line, 1, k + (size_t)m, f) == k + (size_t)m;
        }
    }
    guard.release();
    if (fclose(f) != 0 || !ok) throw Np2Error(NP2_E_ARG, std::string("cannot write ") + out_path);
}

} // namespace

extern "C" {

int np2_rep_bytes(int device, const uint8_t *seq, uint64_t n, const np2_rep_opts_t *opts, uint32_t **index, uint32_t **count,
                  uint64_t *n_listed, np2_rep_stats_t *stats) {
    return np2h::abi_guard([&] {
        // every argument is checked before the first device call
        if (!index || !count || !n_listed || (n && !seq)) throw Np2Error(NP2_E_ARG, "np2_rep_bytes: NULL argument");
        *index = *count = nullptr, *n_listed = 0;
        Run r;
        r.device = device;
        r.o = checked(opts);
        check_kmers(n, r.o.k);
        r.init();
        {
            Feeder fd(r);
            fd.put(seq, n);
            fd.finish();
        }
        select_and_emit(r);
        *index = r.index, *count = r.count, *n_listed = r.listed;
        r.index = r.count = nullptr;
        if (stats) *stats = r.stats;
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_rep_files(int device, const char *const *paths, int n_paths, const np2_rep_opts_t *opts, const char *out_path,
                  int both_strands, np2_rep_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "np2_rep_files: no sequence file given");
        if (!out_path) throw Np2Error(NP2_E_ARG, "np2_rep_files: out_path is NULL");
        Run r;
        r.device = device;
        r.o = checked(opts);
        uint64_t bound = 0;
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "np2_rep_files: a sequence file path is NULL");
            bound += plain_bound(paths[i]);
        }
        check_kmers(bound, r.o.k); // (what gzip input holds shows as it is read: the same status then)
        r.init();
        {
            Feeder fd(r);
            auto put = [&](const uint8_t *p, size_t m) { fd.put(p, m); };
            for (int i = 0; i < n_paths; ++i) np2seq::parse_file(paths[i], put, nullptr); // (its stream ends with a separator)
            fd.finish();
        }
        select_and_emit(r);
        write_list(r, out_path, both_strands != 0);
        if (stats) *stats = r.stats;
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"
