// Host driver of the read binner (np2_bin.hip): np2_bin_stream walks a packed separator stream in host memory piece by
// piece, np2_bin_files feeds the same device path from reader threads (np2_seqreader.hpp: the counter's reader, with
// names and boundaries kept) and writes the report, the name lists and the two bins.  What a read that goes on in the
// next piece has gathered so far stays on the device: its tallies (BinScan::tally_in / tally_out, two buffers in turn)
// and the class of its last marker (BinScan::carry).
#include "../../include/np2_io.h"
#include "np2_bin.hpp"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_seqreader.hpp"
#include "np2_trio.hpp"

using namespace np2qv;
using namespace np2bin;
using np2kc::HALO;

namespace {

// tiles of a piece (32 MiB of reads); NP2_BIN_TEST_STAGE_TILES: a test's smaller pieces
uint32_t stage_tiles() { return (uint32_t)test_hook("NP2_BIN_TEST_STAGE_TILES", 1, 1 << 16, 4096); }

// the scan's grid: what the device holds at once (4 blocks per CU, as the QV scan); NP2_BIN_TEST_BLOCKS: a test's grid
uint32_t bin_blocks(int device) { return grid_blocks(device, 4, "NP2_BIN_TEST_BLOCKS"); }

np2_bin_opts_t opts_of(const np2_bin_opts_t *o) {
    return o ? *o : np2_bin_opts_t{2, 5, DEFAULT_MIN_SCORE, DEFAULT_MINOR_PERMILLE};
}

// everything about the tables and the options, before anything is launched
void check_common(np2_ctx *cx, int pat_idx, int mat_idx, const np2_bin_opts_t &o, const std::string &who) {
    np2::trio_check_tables(cx, pat_idx, mat_idx, o.min_count, o.mid_count, who);
    if (!opts_ok(o.minor_permille))
        throw Np2Error(NP2_E_ARG, who + ": minor_permille must be at most 1000 (got " + std::to_string(o.minor_permille) + ")");
}

// The device path: pieces of one stream in order.  One piece is in flight at a time (the call returns with its results).
struct BinRun {
    np2_ctx *cx;
    YakDev yp, ym;
    np2_bin_opts_t o;
    uint32_t blocks, n_pieces = 0;
    DevBuf<uint8_t> stage, cls;
    DevBuf<uint32_t> ends, owner, tiles, tallies, carry; // carry: the class word, then the two tally carries
    KernelTimer timer;

    BinRun(np2_ctx *cx_, int pat_idx, int mat_idx, const np2_bin_opts_t &o_, bool timed)
        : cx(cx_), yp(cx_->yaks[pat_idx].dev()), ym(cx_->yaks[mat_idx].dev()), o(o_), blocks(bin_blocks(cx_->device)), timer(timed) {
        stage.cached = cls.cached = ends.cached = owner.cached = tiles.cached = tallies.cached = carry.cached = true;
        carry.ensure(1 + 2 * BIN_STATS);
        HIPCHK(hipMemsetAsync(carry.p, 0, (1 + 2 * BIN_STATS) * 4, cx->stream));
    }
    // `halo`: the HALO bytes of the stream in front of the piece (nullptr: separators), `bytes`: its n bytes, `h_ends`: the
    // offsets of its n_ends separators.  cls_out: n_ends class bytes, stats_out (or nullptr): n_ends tallies.
    void piece(const uint8_t *halo, const uint8_t *bytes, uint32_t n, const uint32_t *h_ends, uint32_t n_ends, uint8_t *cls_out,
               np2_bin_t *stats_out) {
        if (n == 0) return;
        const uint32_t nt = (uint32_t)tiles_of(n);
        stage.ensure(HALO + (size_t)nt * QV_TILE);
        ends.ensure(n_ends + 1);
        owner.ensure(nt);
        tiles.ensure(nt);
        tallies.ensure(BIN_STATS * ((size_t)n_ends + 1));
        cls.ensure(n_ends + 1);
        if (halo) HIPCHK(hipMemcpyAsync(stage.p, halo, HALO, hipMemcpyHostToDevice, cx->stream));
        else HIPCHK(hipMemsetAsync(stage.p, SEP, HALO, cx->stream));
        HIPCHK(hipMemcpyAsync(stage.p + HALO, bytes, n, hipMemcpyHostToDevice, cx->stream));
        if (n_ends) HIPCHK(hipMemcpyAsync(ends.p, h_ends, (size_t)n_ends * 4, hipMemcpyHostToDevice, cx->stream));
        HIPCHK(hipMemsetAsync(tallies.p, 0, BIN_STATS * ((size_t)n_ends + 1) * 4, cx->stream));
        np2::BinScan q{};
        q.src = stage.p + HALO;
        q.n_bytes = n;
        q.n_tiles = nt;
        q.ends = ends.p;
        q.n_ends = n_ends;
        q.min_count = o.min_count, q.mid_count = o.mid_count, q.min_score = o.min_score, q.minor_permille = o.minor_permille;
        q.owner = owner.p;
        q.tiles = tiles.p;
        q.tallies = tallies.p;
        q.carry = carry.p;
        q.tally_in = carry.p + 1 + BIN_STATS * (n_pieces & 1u);
        q.tally_out = carry.p + 1 + BIN_STATS * ((n_pieces + 1) & 1u);
        q.cls = cls.p;
        timer.start(cx->stream);
        np2::launch_bin_piece(cx->stream, yp, ym, q, blocks);
        timer.stop(cx->stream);
        HIPCHK(hipGetLastError());
        if (n_ends) HIPCHK(hipMemcpyAsync(cls_out, cls.p, n_ends, hipMemcpyDeviceToHost, cx->stream));
        if (n_ends && stats_out) HIPCHK(hipMemcpyAsync(stats_out, tallies.p, (size_t)n_ends * sizeof(np2_bin_t), hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream)); // (the buffers are filled again for the next piece)
        timer.collect();
        ++n_pieces;
    }
};
static_assert(sizeof(np2_bin_t) == BIN_STATS * 4, "np2_bin_t is a read's seven counters");

// ---------------------------------------------------------------------------------------------------------------
// reader threads -> pieces with names and boundaries
// ---------------------------------------------------------------------------------------------------------------
struct BinPiece {
    uint8_t *buf = nullptr; // pinned: HALO bytes of the file's stream, then up to `cap` bytes
    size_t n = 0;
    std::vector<uint32_t> ends;
    std::string names; // of the reads that end in the piece, '\n' after each
    int file = 0;
    bool last = false; // the file ends with this piece
};
using BinQueue = PieceQueue<BinPiece>; // one per reader thread: its pieces come out in the order of its files

// one file's stream into pieces of `cap` bytes
struct BinWriter {
    HaloWriter<BinPiece> w;
    int file;
    np2seq::NameCollector names;
    uint64_t open_len = 0; // bytes of the read that is open
    BinWriter(BinQueue &q, size_t cap, int file_) : w(q, cap), file(file_) {
        w.on_fresh = [this](BinPiece &p) {
            p.file = file, p.last = false;
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
        if (!sep && (open_len += n) > MAX_READ) throw Np2Error(NP2_E_ARG, "np2_bin_files: a read of 2^32 - 1 bytes or more");
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

size_t class_slot(uint8_t c) { return c == 'p' ? 0 : c == 'm' ? 1 : c == 'a' ? 2 : 3; }

} // namespace

extern "C" {

int np2_bin_stream(np2_ctx_t *cx, int pat_idx, int mat_idx, const uint8_t *stream, uint64_t n_bytes, uint64_t n_reads,
                   const np2_bin_opts_t *opts, uint8_t *cls, np2_bin_t *stats, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        const np2_bin_opts_t o = opts_of(opts);
        check_common(cx, pat_idx, mat_idx, o, "np2_bin_stream");
        if (!cls) throw Np2Error(NP2_E_ARG, "np2_bin_stream: cls is NULL");
        if (n_bytes && !stream) throw Np2Error(NP2_E_ARG, "np2_bin_stream: stream is NULL with n_bytes > 0");
        if (n_bytes && stream[n_bytes - 1] != SEP) throw Np2Error(NP2_E_ARG, "np2_bin_stream: stream does not end in a newline");
        std::vector<uint64_t> all_ends;
        all_ends.reserve(n_reads);
        for (uint64_t at = 0; at < n_bytes;) {
            const uint8_t *e = (const uint8_t *)memchr(stream + at, SEP, n_bytes - at);
            if (!e) break;
            const uint64_t end = (uint64_t)(e - stream);
            if (end - at > MAX_READ) throw Np2Error(NP2_E_ARG, "np2_bin_stream: stream holds a read of 2^32 - 1 bytes or more (read " + std::to_string(all_ends.size()) + ")");
            if (all_ends.size() == n_reads) throw Np2Error(NP2_E_ARG, "np2_bin_stream: n_reads is " + std::to_string(n_reads) + ", stream holds more newlines");
            all_ends.push_back(end);
            at = end + 1;
        }
        if (all_ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_bin_stream: n_reads is " + std::to_string(n_reads) + ", stream holds " + std::to_string(all_ends.size()) + " newlines");
        if (kernel_ms) *kernel_ms = 0.f;
        if (n_reads == 0) return NP2_OK;

        HIPCHK(hipSetDevice(cx->device));
        BinRun run(cx, pat_idx, mat_idx, o, kernel_ms != nullptr);
        const uint64_t cap = (uint64_t)stage_tiles() * QV_TILE;
        std::vector<uint32_t> local;
        uint64_t r = 0; // reads closed so far
        for (uint64_t base = 0; base < n_bytes; base += cap) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(cap, n_bytes - base);
            local.clear();
            for (uint64_t i = r; i < n_reads && all_ends[i] < base + n; ++i) local.push_back((uint32_t)(all_ends[i] - base));
            run.piece(base ? stream + base - HALO : nullptr, stream + base, n, local.data(), (uint32_t)local.size(), cls + r, stats ? stats + r : nullptr);
            r += local.size();
        }
        if (kernel_ms) *kernel_ms = run.timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_bin_files(np2_ctx_t *cx, int pat_idx, int mat_idx, const char *const *paths, int n_paths, const np2_bin_opts_t *opts,
                  const np2_bin_out_t *out, uint64_t *counts, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        const np2_bin_opts_t o = opts_of(opts);
        check_common(cx, pat_idx, mat_idx, o, "np2_bin_files");
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "np2_bin_files: no read file given");
        std::vector<std::string> files;
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "np2_bin_files: a read file path is NULL");
            FILE *f = fopen(paths[i], "rb");
            if (!f) throw Np2Error(NP2_E_ARG, std::string("np2_bin_files: cannot open ") + paths[i]);
            fclose(f);
            files.push_back(paths[i]);
        }
        OutFile tsv, pat_list, mat_list, pat_fa, mat_fa;
        if (out) tsv.open(out->tsv, cx->device), pat_list.open(out->pat_list, cx->device), mat_list.open(out->mat_list, cx->device), pat_fa.open(out->pat_fa, cx->device), mat_fa.open(out->mat_fa, cx->device);
        const bool want_seq = pat_fa.is_open() || mat_fa.is_open();
        if (kernel_ms) *kernel_ms = 0.f;
        uint64_t n_class[4] = {0, 0, 0, 0};
        static const char HEAD[] = "read\tclass\ts_pat\ts_mat\tn_pat\tn_mat\tpm\tmp\tkmers\tlen\n";
        tsv.put(HEAD, sizeof(HEAD) - 1);

        HIPCHK(hipSetDevice(cx->device));
        BinRun run(cx, pat_idx, mat_idx, o, kernel_ms != nullptr);
        const size_t cap = (size_t)stage_tiles() * QV_TILE;
        const size_t n_threads = std::min<size_t>(files.size(), 16);
        std::vector<BinQueue> queues(n_threads);
        std::vector<BinPiece> pieces(2 * n_threads);
        PinnedBlocks pinned;
        for (size_t i = 0; i < pieces.size(); ++i) {
            pieces[i].buf = pinned.get(HALO + cap + 64);
            queues[i / 2].idle.push_back(&pieces[i]);
        }
        auto readers = run_readers(n_threads, queues, [&](size_t ti) {
            for (size_t fi = ti; fi < files.size(); fi += n_threads) {
                BinWriter w(queues[ti], cap, (int)fi);
                np2seq::parse_file(files[fi], [&](const uint8_t *p, size_t n) { w.put(p, n); }, [&] { return w.w.dead; },
                                   [&](const uint8_t *p, size_t n, bool begin) { w.names(p, n, begin); });
                w.finish();
                if (w.w.dead) break;
            }
        });

        std::vector<uint8_t> cls;
        std::vector<np2_bin_t> st;
        std::string open_seq, row; // the bytes of the read that goes on in the next piece (kept for the FASTA bins only)
        uint64_t open_len = 0;
        for (size_t fi = 0; fi < files.size(); ++fi) {
            BinQueue &q = queues[fi % n_threads];
            for (bool last = false; !last;) {
                BinPiece *p = q.take_full();
                if (!p) throw Np2Error(q.err_code != NP2_OK ? q.err_code : NP2_E_ARG, q.err_code != NP2_OK ? q.err : "np2_bin_files: a reader stopped early");
                last = p->last;
                const uint32_t n_ends = (uint32_t)p->ends.size();
                cls.resize(n_ends + 1), st.resize(n_ends + 1);
                run.piece(p->buf, p->buf + HALO, (uint32_t)p->n, p->ends.data(), n_ends, cls.data(), st.data());
                const uint8_t *bytes = p->buf + HALO;
                size_t from = 0, name_at = 0;
                for (uint32_t r = 0; r < n_ends; ++r) {
                    const size_t end = p->ends[r], name_end = p->names.find('\n', name_at);
                    const char *name = p->names.data() + name_at;
                    const size_t name_n = name_end - name_at;
                    const np2_bin_t &s = st[r];
                    const uint8_t c = cls[r];
                    ++n_class[class_slot(c)];
                    if (tsv.is_open()) {
                        row.assign(name, name_n);
                        char num[160];
                        snprintf(num, sizeof num, "\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%llu\n", (char)c, s.pairs[0], s.pairs[3], s.n_pat, s.n_mat, s.pairs[1],
                                 s.pairs[2], s.n_kmers, (unsigned long long)(open_len + (end - from)));
                        row += num;
                        tsv.put(row.data(), row.size());
                    }
                    for (int side = 0; side < 2; ++side) {
                        if (!(side == 0 ? keep_pat(c) : keep_mat(c))) continue;
                        OutFile &lst = side == 0 ? pat_list : mat_list, &fa = side == 0 ? pat_fa : mat_fa;
                        lst.put(name, name_n), lst.put("\n", 1);
                        if (fa.is_open()) fa.put(">", 1), fa.put(name, name_n), fa.put("\n", 1), fa.put(open_seq.data(), open_seq.size()), fa.put(bytes + from, end - from), fa.put("\n", 1);
                    }
                    open_seq.clear(), open_len = 0;
                    from = end + 1, name_at = name_end + 1;
                }
                open_len += p->n - from;
                if (want_seq) open_seq.append((const char *)bytes + from, p->n - from);
                q.give_idle(p);
            }
        }
        tsv.close(), pat_list.close(), mat_list.close(), pat_fa.close(), mat_fa.close();
        if (counts) memcpy(counts, n_class, sizeof n_class);
        if (kernel_ms) *kernel_ms = run.timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_seqfile_reads(const char *path, char **names, uint64_t *names_bytes, uint64_t **ends, uint64_t *n_reads) {
    if (!path || !names || !names_bytes || !ends || !n_reads) return np2h::io_set_error(NP2_E_ARG, "np2_seqfile_reads: NULL argument");
    *names = nullptr, *ends = nullptr, *names_bytes = 0, *n_reads = 0;
    return np2h::abi_guard([&] {
        np2seq::NameCollector nc;
        std::string blob;
        std::vector<uint64_t> e;
        uint64_t at = 0;
        np2seq::parse_file(path, [&](const uint8_t *p, size_t n) {
            if (n == 1 && *p == SEP) {
                e.push_back(at);
                blob += nc.close();
                blob.push_back('\n');
            }
            at += n;
        }, nullptr, [&](const uint8_t *p, size_t n, bool begin) { nc(p, n, begin); });
        char *nm = (char *)malloc(blob.size() + 1);
        uint64_t *en = (uint64_t *)malloc((e.size() + 1) * 8);
        if (!nm || !en) {
            free(nm), free(en);
            throw Np2Error(NP2_E_NOMEM, "out of memory");
        }
        memcpy(nm, blob.data(), blob.size());
        nm[blob.size()] = 0;
        if (!e.empty()) memcpy(en, e.data(), e.size() * 8);
        *names = nm, *names_bytes = blob.size(), *ends = en, *n_reads = e.size();
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"
