// Host driver of the short-read quality filter (include/np2_io.h: np2_srqc_*, np2_seqfile_stream_qual): a pair of streams
// in host memory, or FASTQ files, through the filter kernel (np2_srqc.hip) piece by piece.  The k-mer counter runs the
// same kernel in front of its own (np2_kcount_host.cpp: count_piece) on pieces its reader threads fill through the same
// assembler (np2_srqc_host.hpp).
//
// Pieces end at a read boundary: a read is judged by one wavefront that sees all of it, and the masked piece the counter
// reads then ends in a separator, so no k-mer run crosses into the next piece and the counter's halo is separators.
#include "np2_srqc_host.hpp"

#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"

namespace {
using np2h::Np2Error;
using np2h::QC_BACK;
using np2h::QC_FRONT;
using np2h::QcPiece;

struct Last {
    uint64_t totals[np2srqc::N_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    float kernel_ms = 0;
};
thread_local Last g_last;

// a stream of its own, one piece in pinned memory, the device buffers
struct Runner {
    hipStream_t st = nullptr;
    size_t piece;
    np2h::SrqcDev dev;
    np2h::DevBuf<uint8_t> d_seq;
    np2h::PinnedBuf pin_seq, pin_qual;
    QcPiece pc;
    std::vector<np2_srqc_read_t> reads;
    Runner(int device, const np2srqc::Opts &o) : piece(np2h::srqc_piece_bytes()) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        dev.o = o;
        dev.init(st, piece);
        d_seq.ensure(QC_FRONT + piece + QC_BACK);
        pc.seq = (uint8_t *)pin_seq.ensure(QC_FRONT + piece + QC_BACK);
        pc.qual = (uint8_t *)pin_qual.ensure(QC_FRONT + piece + QC_BACK);
    }
    ~Runner() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
    // the filter over `pc`; `reads` holds the results, pc.seq the masked bytes (with `masked`) when it returns
    void run(bool masked) {
        HIPCHK(hipMemcpyAsync(d_seq.p, pc.seq, np2h::pad_piece(pc.seq, pc.n), hipMemcpyHostToDevice, st));
        reads.resize(pc.ends.size());
        dev.run(st, d_seq.p, pc, reads.data());
        if (masked) HIPCHK(hipMemcpyAsync(pc.seq + QC_FRONT, d_seq.p + QC_FRONT, pc.n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
};

void add_totals(uint64_t *sum, const uint64_t *t) {
    for (uint32_t i = 0; i < np2srqc::N_TOTALS; ++i) sum[i] += t[i];
}

} // namespace

np2srqc::Opts np2h::srqc_checked(const np2_srqc_opts_t *opts) {
    np2srqc::Opts o = np2srqc::recipe();
    if (opts) memcpy(&o, opts, sizeof(o));
    if (const char *why = np2srqc::invalid(o)) throw Np2Error(NP2_E_ARG, std::string("quality filter options: ") + why);
    return o;
}
void np2h::srqc_publish(const uint64_t *totals, float kernel_ms) {
    memcpy(g_last.totals, totals, sizeof(g_last.totals));
    g_last.kernel_ms = kernel_ms;
}
size_t np2h::srqc_piece_bytes() {
    const size_t piece = (size_t)test_hook("NP2_KCOUNT_TEST_PIECE", 64, LLONG_MAX, 8 << 20);
    if (piece > ((size_t)1 << 31)) throw Np2Error(NP2_E_ARG, "NP2_KCOUNT_TEST_PIECE: at most 2147483648 with the quality filter");
    return piece;
}

extern "C" {

int np2_srqc_bytes(int device, const uint8_t *seq, const uint8_t *qual, uint64_t n, const np2_srqc_opts_t *opts, uint8_t *masked_out,
                   np2_srqc_read_t *reads_out, uint64_t n_reads, np2_srqc_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (n && (!seq || !qual)) throw Np2Error(NP2_E_ARG, "np2_srqc_bytes: NULL argument");
        const np2srqc::Opts o = np2h::srqc_checked(opts);
        const size_t piece = np2h::srqc_piece_bytes();
        if (n && seq[n - 1] != '\n') throw Np2Error(NP2_E_ARG, "np2_srqc_bytes: the streams must end with a separator");
        std::vector<uint64_t> ends;
        for (uint64_t at = 0; at < n;) {
            const uint8_t *e = (const uint8_t *)memchr(seq + at, '\n', n - at);
            const uint64_t sep = (uint64_t)(e - seq);
            if (qual[sep] != '\n' || memchr(qual + at, '\n', sep - at))
                throw Np2Error(NP2_E_ARG, "np2_srqc_bytes: read " + std::to_string(ends.size() + 1) + ": the two streams' separators differ");
            if (sep - at + 1 > piece)
                throw Np2Error(NP2_E_UNSUPPORTED, "read " + std::to_string(ends.size() + 1) + ": a read of " + std::to_string(sep - at) +
                                                      " bases does not fit a piece of " + std::to_string(piece) + " bytes");
            ends.push_back(sep);
            at = sep + 1;
        }
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_srqc_bytes: n_reads is " + std::to_string(n_reads) + ", the stream has " + std::to_string(ends.size()) + " separators");
        uint64_t total[np2srqc::N_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
        float ms = 0;
        if (n) {
            Runner r(device, o);
            for (size_t i = 0; i < ends.size();) { // reads i .. j - 1: as many as fit
                const uint64_t from = i ? ends[i - 1] + 1 : 0;
                size_t j = i;
                while (j < ends.size() && ends[j] + 1 - from <= piece) ++j;
                r.pc.n = (size_t)(ends[j - 1] + 1 - from);
                memset(r.pc.seq, '\n', QC_FRONT), memset(r.pc.qual, '\n', QC_FRONT);
                memcpy(r.pc.seq + QC_FRONT, seq + from, r.pc.n);
                memcpy(r.pc.qual + QC_FRONT, qual + from, r.pc.n);
                r.pc.ends.resize(j - i);
                for (size_t t = i; t < j; ++t) r.pc.ends[t - i] = (uint32_t)(ends[t] - from);
                r.run(masked_out != nullptr);
                if (masked_out) memcpy(masked_out + from, r.pc.seq + QC_FRONT, r.pc.n);
                if (reads_out) memcpy(reads_out + i, r.reads.data(), (j - i) * sizeof(np2_srqc_read_t));
                i = j;
            }
            r.dev.totals(r.st, total);
            ms = r.dev.kernel_ms;
        }
        if (stats) memcpy(stats, total, sizeof(total));
        np2h::srqc_publish(total, ms);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_srqc_files(int device, const char *const *paths, int n_paths, const np2_srqc_opts_t *opts, const char *const *out_paths,
                   np2_srqc_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "no sequence file given");
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "a sequence file path is NULL");
            FILE *f = fopen(paths[i], "rb");
            if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + paths[i]);
            fclose(f);
        }
        const np2srqc::Opts o = np2h::srqc_checked(opts);
        Runner r(device, o);
        uint64_t sum[np2srqc::N_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
        float ms = 0;
        for (int fi = 0; fi < n_paths; ++fi) {
            np2h::OutFile out;
            out.open(out_paths ? out_paths[fi] : nullptr, device);
            r.dev.zero(r.st);
            np2h::QcAssembler as(r.piece, out.is_open());
            as.take = [&] { return &r.pc; };
            as.unused = [](QcPiece *) {};
            as.full = [&](QcPiece *pc) {
                r.run(false);
                if (!out.is_open()) return;
                const char *h = pc->hdrs.data();
                for (size_t i = 0; i < pc->ends.size(); ++i) {
                    const char *he = (const char *)memchr(h, '\n', pc->hdrs.data() + pc->hdrs.size() - h);
                    const np2_srqc_read_t &rd = r.reads[i];
                    if (rd.cls == np2srqc::PASS) {
                        const size_t from = QC_FRONT + (i ? pc->ends[i - 1] + 1 : 0);
                        out.put(h, (size_t)(he - h) + 1);
                        out.put(pc->seq + from + rd.begin, rd.end - rd.begin);
                        out.put("\n+\n", 3);
                        out.put(pc->qual + from + rd.begin, rd.end - rd.begin);
                        out.put("\n", 1);
                    }
                    h = he + 1;
                }
            };
            as.file(paths[fi]);
            as.flush();
            out.close();
            uint64_t t[np2srqc::N_TOTALS];
            r.dev.totals(r.st, t);
            ms += r.dev.kernel_ms;
            if (stats) memcpy(stats + fi, t, sizeof(t));
            add_totals(sum, t);
        }
        if (stats) memcpy(stats + n_paths, sum, sizeof(sum));
        np2h::srqc_publish(sum, ms);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_srqc_last_stats(np2_srqc_stats_t *stats) {
    if (stats) memcpy(stats, g_last.totals, sizeof(g_last.totals));
    return NP2_OK;
}

int np2_srqc_last_kernel_ms(float *ms) {
    if (ms) *ms = g_last.kernel_ms;
    return NP2_OK;
}

int np2_seqfile_stream_qual(const char *path, uint8_t **seq, uint8_t **qual, uint64_t *n) {
    if (!path || !seq || !qual || !n) return np2h::io_set_error(NP2_E_ARG, "np2_seqfile_stream_qual: NULL argument");
    *seq = *qual = nullptr, *n = 0;
    return np2h::abi_guard([&] {
        std::vector<uint8_t> s, q;
        np2seq::RecordCheck chk;
        chk.file_begin(path);
        np2seq::parse_file_qual(
            path,
            [&](const uint8_t *p, size_t m) {
                if (m == 1 && *p == '\n') chk.seq_end();
                else chk.seq_bytes(m);
                s.insert(s.end(), p, p + m);
            },
            [&](const uint8_t *p, size_t m) {
                if (m == 1 && *p == '\n') chk.qual_end();
                else chk.qual_bytes(m);
                q.insert(q.end(), p, p + m);
            },
            nullptr, [](const uint8_t *, size_t, bool) {});
        chk.file_end();
        uint8_t *a = (uint8_t *)malloc(s.size() + 1), *b = (uint8_t *)malloc(s.size() + 1);
        if (!a || !b) {
            free(a), free(b);
            throw Np2Error(NP2_E_NOMEM, "out of memory");
        }
        memcpy(a, s.data(), s.size()), memcpy(b, q.data(), s.size());
        *seq = a, *qual = b, *n = s.size();
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"
