// Host side of the short-read quality filter, shared by its own entry points (np2_srqc_host.cpp) and the k-mer counter
// (np2_kcount_host.cpp): pieces of the two streams that end at a read boundary, and the device buffers of one filter run.
#pragma once
#include "np2_ctx.hpp"
#include "np2_kcount_core.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"
#include "np2_seqreader.hpp"
#include "np2_srqc.hpp"

#include <functional>

namespace np2h {

// A piece of both streams.  Either buffer is pinned: QC_FRONT bytes of separators (the counter's halo: no k-mer straddles
// two pieces, a piece ends at a separator), then up to the piece size, then QC_BACK bytes of room.
static constexpr size_t QC_FRONT = np2kc::HALO, QC_BACK = 64;
struct QcPiece {
    uint8_t *seq = nullptr, *qual = nullptr;
    size_t n = 0;               // bytes of either stream; the last one is a separator
    std::vector<uint32_t> ends; // the separators' offsets
    std::string hdrs;           // (when asked for) the records' header lines without '\r', each followed by '\n'
    void *owner = nullptr;
};

// What a reader writes the two streams into.  A piece is closed at the last separator that fits: the bytes of the record
// that is open when a piece fills move to the next one.  A read that does not fit an empty piece is NP2_E_UNSUPPORTED.
struct QcAssembler {
    size_t cap;
    bool want_hdr;
    std::function<QcPiece *()> take;       // an empty piece; nullptr: the run was given up
    std::function<void(QcPiece *)> full;   // a closed piece
    std::function<void(QcPiece *)> unused; // a piece nothing was written to
    QcPiece *cur = nullptr;
    size_t rs = 0; // where the open record begins in `cur`
    np2seq::RecordCheck chk;
    bool over = false;     // the open record does not fit a piece: its bases are only counted from here on, for the message
    uint64_t over_len = 0;
    bool dead = false;
    std::string hdr;

    QcAssembler(size_t cap_, bool want_hdr_) : cap(cap_), want_hdr(want_hdr_) {}
    bool fresh() {
        cur = take();
        if (!cur) return !(dead = true);
        memset(cur->seq, '\n', QC_FRONT), memset(cur->qual, '\n', QC_FRONT);
        cur->n = 0, cur->ends.clear(), cur->hdrs.clear();
        rs = 0;
        return true;
    }
    // the open record's sequence grown to `sl` bytes, and its separator, fit `cur` (false: given up, or too long)
    bool room(size_t sl) {
        if (!cur && !fresh()) return false;
        if (rs + sl + 1 <= cap) return true;
        if (rs != 0) {
            QcPiece *old = cur;
            const std::vector<uint8_t> part(old->seq + QC_FRONT + rs, old->seq + QC_FRONT + rs + chk.sl);
            full(old);
            if (!fresh()) return false;
            if (!part.empty()) memcpy(cur->seq + QC_FRONT, part.data(), part.size());
            if (sl + 1 <= cap) return true;
        }
        over = true, over_len = chk.sl;
        return false;
    }
    void seq(const uint8_t *p, size_t n) {
        if (dead) return;
        if (n == 1 && *p == '\n') {
            if (!over) (void)room(chk.sl);
            if (over)
                throw Np2Error(NP2_E_UNSUPPORTED, chk.path + ": record " + std::to_string(chk.record + 1) + ": a read of " + std::to_string(over_len) +
                                                      " bases does not fit a piece of " + std::to_string(cap) + " bytes");
            if (dead) return;
            cur->seq[QC_FRONT + rs + chk.sl] = '\n';
            chk.seq_end();
            return;
        }
        if (!over && room(chk.sl + n)) {
            memcpy(cur->seq + QC_FRONT + rs + chk.sl, p, n);
            chk.seq_bytes(n);
        } else if (over) {
            over_len += n;
        }
    }
    void qual(const uint8_t *p, size_t n) {
        if (dead) return;
        if (n == 1 && *p == '\n') {
            if (!cur || !chk.seq_done || chk.ql != chk.sl) chk.mismatch();
            cur->qual[QC_FRONT + rs + chk.ql] = '\n';
            cur->ends.push_back((uint32_t)(rs + chk.sl));
            if (want_hdr) {
                while (!hdr.empty() && hdr.back() == '\r') hdr.pop_back();
                cur->hdrs += hdr, cur->hdrs += '\n';
            }
            rs += chk.sl + 1, cur->n = rs;
            chk.qual_end();
            return;
        }
        chk.qual_bytes(n);
        memcpy(cur->qual + QC_FRONT + rs + chk.ql - n, p, n);
    }
    void header(const uint8_t *p, size_t n, bool begin) {
        if (!want_hdr) return;
        if (begin) hdr.clear();
        else hdr.append((const char *)p, n);
    }
    void flush() { // what is complete goes on (the end of a file, or of the run)
        if (!cur) return;
        if (cur->n) full(cur);
        else unused(cur);
        cur = nullptr;
    }
    // one FASTQ file into the pieces
    void file(const std::string &path) {
        chk.file_begin(path);
        np2seq::parse_file_qual(
            path, [&](const uint8_t *p, size_t n) { seq(p, n); }, [&](const uint8_t *p, size_t n) { qual(p, n); }, [&] { return dead; },
            [&](const uint8_t *p, size_t n, bool b) { header(p, n, b); });
        if (!dead) chk.file_end();
    }
};

// Device side of one filter run: the quality bytes, the separators' offsets, the per-read results and the totals.
struct SrqcDev {
    np2srqc::Opts o{};
    DevBuf<uint8_t> d_qual;
    DevBuf<uint32_t> d_ends;
    DevBuf<np2_srqc_read_t> d_reads;
    DevBuf<uint64_t> d_tot;
    DevEvent ev0, ev1;
    bool timed = false;
    float kernel_ms = 0;
    void init(hipStream_t st, size_t piece) {
        d_qual.ensure(QC_FRONT + piece + QC_BACK);
        d_tot.ensure(np2srqc::N_TOTALS);
        ev0.make(), ev1.make();
        zero(st);
    }
    void zero(hipStream_t st) {
        HIPCHK(hipMemsetAsync(d_tot.p, 0, np2srqc::N_TOTALS * 8, st));
        kernel_ms = 0;
    }
    // `d_seq`: the piece's base bytes on the device, front included, already on their way on `st`.  reads (or nullptr):
    // host room for pc.ends.size() results.  `pc` must stay as it is until `st` has been synchronised.
    void run(hipStream_t st, uint8_t *d_seq, QcPiece &pc, np2_srqc_read_t *reads) {
        collect();
        const size_t n_reads = pc.ends.size();
        HIPCHK(hipMemcpyAsync(d_qual.p, pc.qual, pad_piece(pc.qual, pc.n), hipMemcpyHostToDevice, st));
        d_ends.ensure(n_reads + 1);
        HIPCHK(hipMemcpyAsync(d_ends.p, pc.ends.data(), n_reads * 4, hipMemcpyHostToDevice, st));
        if (reads) d_reads.ensure(n_reads + 1);
        HIPCHK(hipEventRecord(ev0.e, st));
        np2::launch_srqc(st, d_seq + QC_FRONT, d_qual.p + QC_FRONT, d_ends.p, (uint32_t)n_reads, o, reads ? d_reads.p : nullptr, d_tot.p);
        HIPCHK(hipEventRecord(ev1.e, st));
        timed = true;
        if (reads) HIPCHK(hipMemcpyAsync(reads, d_reads.p, n_reads * sizeof(np2_srqc_read_t), hipMemcpyDeviceToHost, st));
    }
    void collect() { // the last run's kernel time (its stream has been synchronised since)
        if (!timed) return;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0.e, ev1.e) == hipSuccess) kernel_ms += ms;
        timed = false;
    }
    void totals(hipStream_t st, uint64_t *out) { // (synchronises the stream)
        HIPCHK(hipMemcpyAsync(out, d_tot.p, np2srqc::N_TOTALS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        collect();
    }
};

// the options of a call, checked (NP2_E_ARG)
np2srqc::Opts srqc_checked(const np2_srqc_opts_t *opts);
// what np2_srqc_last_stats / np2_srqc_last_kernel_ms of this thread answer from now on
void srqc_publish(const uint64_t *totals, float kernel_ms);
// the piece size of this call (NP2_KCOUNT_TEST_PIECE), as the counter reads it
size_t srqc_piece_bytes();

} // namespace np2h
