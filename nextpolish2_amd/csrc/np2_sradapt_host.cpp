// Host driver of the short-read adapter trimmer (include/np2_io.h: np2_sradapt_*): a pair of streams in host memory, or
// FASTQ files, through the trimming kernel (np2_sradapt.hip) piece by piece.  The k-mer counter runs the same kernel in front
// of its own (np2_kcount_host.cpp: count_piece) on pieces its reader threads fill through the same assembler.
//
// Pieces end at a read boundary and, in pair mode, after an even number of reads: a pair is judged by one wavefront that
// sees both mates.
#include "np2_sradapt_host.hpp"

#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"

namespace {
using np2h::Np2Error;
using np2h::QC_BACK;
using np2h::QC_FRONT;
using np2h::QcPiece;
using np2sradapt::N_TOTALS;

struct Last {
    uint64_t totals[N_TOTALS] = {};
    float kernel_ms = 0;
};
thread_local Last g_last;

// a stream of its own, one piece in pinned memory, the device buffers
struct Runner {
    hipStream_t st = nullptr;
    size_t piece;
    np2h::AdDev dev;
    np2h::DevBuf<uint8_t> d_seq;
    np2h::PinnedBuf pin_seq, pin_qual;
    QcPiece pc;
    std::vector<np2_sradapt_read_t> reads;
    Runner(int device, const np2srqc::Opts &qc, const np2sradapt::Opts &o) : piece(np2h::srqc_piece_bytes()) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        dev.qc = qc, dev.o = o;
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
    // the trimmer over `pc`; `reads` holds the results, pc.seq the masked bytes (with `masked`) when it returns
    void run(bool masked) {
        HIPCHK(hipMemcpyAsync(d_seq.p, pc.seq, np2h::pad_piece(pc.seq, pc.n), hipMemcpyHostToDevice, st));
        reads.resize(pc.ends.size());
        dev.run(st, d_seq.p, pc, reads.data());
        if (masked) HIPCHK(hipMemcpyAsync(pc.seq + QC_FRONT, d_seq.p + QC_FRONT, pc.n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
};

// read i of the piece as a FASTQ record: the header line as read, the kept bases, "+", the kept qualities
void put_record(np2h::OutFile &out, const QcPiece &pc, size_t i, const char *h, const char *he, const np2_sradapt_read_t &rd) {
    const size_t from = QC_FRONT + (i ? pc.ends[i - 1] + 1 : 0);
    out.put(h, (size_t)(he - h) + 1);
    out.put(pc.seq + from + rd.begin, rd.end - rd.begin);
    out.put("\n+\n", 3);
    out.put(pc.qual + from + rd.begin, rd.end - rd.begin);
    out.put("\n", 1);
}

} // namespace

np2srqc::Opts np2h::sradapt_qc(const np2_srqc_opts_t *qc) {
    if (qc) return srqc_checked(qc);
    return np2srqc::Opts{0, 0, 4, 20, 0xFFFFFFFFu, 0, 100, 0, 0};
}
np2sradapt::Opts np2h::sradapt_checked(const np2_sradapt_opts_t *ad) {
    np2sradapt::Opts o = np2sradapt::defaults();
    if (ad)
        if (const char *why = np2sradapt::make_opts(ad->flags, ad->overlap_min, ad->overlap_diff, ad->overlap_diff_percent, ad->adapter1,
                                                    ad->adapter2, o))
            throw Np2Error(NP2_E_ARG, std::string("adapter options: ") + why);
    return o;
}
void np2h::sradapt_publish(const uint64_t *totals, float kernel_ms) {
    memcpy(g_last.totals, totals, sizeof(g_last.totals));
    g_last.kernel_ms = kernel_ms;
}

extern "C" {

int np2_sradapt_bytes(int device, const uint8_t *seq, const uint8_t *qual, uint64_t n, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad,
                      uint8_t *masked_out, np2_sradapt_read_t *reads_out, uint64_t n_reads, np2_sradapt_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (n && (!seq || !qual)) throw Np2Error(NP2_E_ARG, "np2_sradapt_bytes: NULL argument");
        const np2srqc::Opts q = np2h::sradapt_qc(qc);
        const np2sradapt::Opts o = np2h::sradapt_checked(ad);
        const bool paired = (o.flags & np2sradapt::PAIRED) != 0;
        const size_t step = paired ? 2 : 1;
        const size_t piece = np2h::srqc_piece_bytes();
        if (paired && n_reads % 2) throw Np2Error(NP2_E_ARG, "np2_sradapt_bytes: n_reads is odd in pair mode");
        if (n && seq[n - 1] != '\n') throw Np2Error(NP2_E_ARG, "np2_sradapt_bytes: the streams must end with a separator");
        std::vector<uint64_t> ends;
        for (uint64_t at = 0; at < n;) {
            const uint8_t *e = (const uint8_t *)memchr(seq + at, '\n', n - at);
            const uint64_t sep = (uint64_t)(e - seq);
            if (qual[sep] != '\n' || memchr(qual + at, '\n', sep - at))
                throw Np2Error(NP2_E_ARG, "np2_sradapt_bytes: read " + std::to_string(ends.size() + 1) + ": the two streams' separators differ");
            ends.push_back(sep);
            at = sep + 1;
        }
        if (ends.size() != n_reads)
            throw Np2Error(NP2_E_ARG, "np2_sradapt_bytes: n_reads is " + std::to_string(n_reads) + ", the stream has " + std::to_string(ends.size()) + " separators");
        for (size_t i = 0; i < ends.size(); i += step) { // a unit: a read, or a pair
            const uint64_t from = i ? ends[i - 1] + 1 : 0, bytes = ends[i + step - 1] + 1 - from;
            if (bytes > piece)
                throw Np2Error(NP2_E_UNSUPPORTED, "read " + std::to_string(i + 1) + ": a " + (paired ? "pair" : "read") + " of " + std::to_string(bytes - step) +
                                                      " bases does not fit a piece of " + std::to_string(piece) + " bytes");
        }
        uint64_t total[N_TOTALS] = {};
        float ms = 0;
        if (n) {
            Runner r(device, q, o);
            for (size_t i = 0; i < ends.size();) { // units i .. j - 1: as many as fit
                const uint64_t from = i ? ends[i - 1] + 1 : 0;
                size_t j = i;
                while (j < ends.size() && ends[j + step - 1] + 1 - from <= piece) j += step;
                r.pc.n = (size_t)(ends[j - 1] + 1 - from);
                memset(r.pc.seq, '\n', QC_FRONT), memset(r.pc.qual, '\n', QC_FRONT);
                memcpy(r.pc.seq + QC_FRONT, seq + from, r.pc.n);
                memcpy(r.pc.qual + QC_FRONT, qual + from, r.pc.n);
                r.pc.ends.resize(j - i);
                for (size_t t = i; t < j; ++t) r.pc.ends[t - i] = (uint32_t)(ends[t] - from);
                r.run(masked_out != nullptr);
                if (masked_out) memcpy(masked_out + from, r.pc.seq + QC_FRONT, r.pc.n);
                if (reads_out) memcpy(reads_out + i, r.reads.data(), (j - i) * sizeof(np2_sradapt_read_t));
                i = j;
            }
            r.dev.totals(r.st, total);
            ms = r.dev.kernel_ms;
        }
        if (stats) memcpy(stats, total, sizeof(total));
        np2h::sradapt_publish(total, ms);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_sradapt_files(int device, const char *const *paths, int n_paths, const np2_srqc_opts_t *qc, const np2_sradapt_opts_t *ad,
                      const char *const *out_paths, np2_sradapt_stats_t *stats) {
    return np2h::abi_guard([&] {
        if (!paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "no sequence file given");
        const np2srqc::Opts q = np2h::sradapt_qc(qc);
        const np2sradapt::Opts o = np2h::sradapt_checked(ad);
        const bool paired = (o.flags & np2sradapt::PAIRED) != 0;
        const int step = paired ? 2 : 1;
        if (n_paths % step) throw Np2Error(NP2_E_ARG, "pair mode takes the files as R1 R2 R1 R2 ..: their number is odd");
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "a sequence file path is NULL");
            FILE *f = fopen(paths[i], "rb");
            if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + paths[i]);
            fclose(f);
        }
        Runner r(device, q, o);
        uint64_t sum[N_TOTALS] = {};
        float ms = 0;
        for (int fi = 0; fi < n_paths; fi += step) {
            np2h::OutFile out[2];
            for (int m = 0; m < step; ++m) out[m].open(out_paths ? out_paths[fi + m] : nullptr, device);
            const bool writes = out[0].is_open() || out[1].is_open();
            r.dev.zero(r.st);
            np2h::QcAssembler as(r.piece, writes);
            as.take = [&] { return &r.pc; };
            as.unused = [](QcPiece *) {};
            as.full = [&](QcPiece *pc) {
                r.run(false);
                if (!writes) return;
                const char *h = pc->hdrs.data(), *h_end = h + pc->hdrs.size();
                for (size_t i = 0; i < pc->ends.size(); i += step) {
                    bool pass = true;
                    for (int m = 0; m < step; ++m) pass = pass && r.reads[i + m].cls == np2srqc::PASS;
                    for (int m = 0; m < step; ++m) {
                        const char *he = (const char *)memchr(h, '\n', h_end - h);
                        if (pass) put_record(out[m], *pc, i + m, h, he, r.reads[i + m]);
                        h = he + 1;
                    }
                }
            };
            if (paired) np2h::pair_files(as, paths[fi], paths[fi + 1]);
            else as.file(paths[fi]);
            as.flush();
            for (int m = 0; m < step; ++m) out[m].close();
            uint64_t t[N_TOTALS];
            r.dev.totals(r.st, t);
            ms += r.dev.kernel_ms;
            if (stats) memcpy(stats + fi / step, t, sizeof(t));
            for (uint32_t i = 0; i < N_TOTALS; ++i) sum[i] += t[i];
        }
        if (stats) memcpy(stats + n_paths / step, sum, sizeof(sum));
        np2h::sradapt_publish(sum, ms);
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_sradapt_last_stats(np2_sradapt_stats_t *stats) {
    if (stats) memcpy(stats, g_last.totals, sizeof(g_last.totals));
    return NP2_OK;
}

int np2_sradapt_last_kernel_ms(float *ms) {
    if (ms) *ms = g_last.kernel_ms;
    return NP2_OK;
}

} // extern "C"
