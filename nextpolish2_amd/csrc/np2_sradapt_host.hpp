// Host side of the short-read adapter trimmer, shared by its own entry points (np2_sradapt_host.cpp) and the k-mer counter
// (np2_kcount_host.cpp): two FASTQ files read in step (np2_recordfeed.hpp) into pieces that hold whole pairs (on top of
// np2_srqc_host.hpp's assembler), and the device buffers of one trimming run.
#pragma once
#include "np2_recordfeed.hpp"
#include "np2_sradapt.hpp"
#include "np2_srqc_host.hpp"

namespace np2h {

// R1 and R2 in step into `as`: records interleaved, mate 1 then mate 2, a piece closed only after an even number of reads.
// Names are not compared.  The caller flushes.
inline void pair_files(QcAssembler &as, const std::string &p1, const std::string &p2) {
    RecordFeed f1, f2;
    f1.start(p1, as.want_hdr), f2.start(p2, as.want_hdr);
    as.chk.file_begin(p1 + " + " + p2);
    static const uint8_t NL = '\n';
    auto put = [&](const RecordFeed::Rec &r) {
        as.header(nullptr, 0, true);
        as.header(r.hdr, r.hdr_len, false);
        if (r.len) as.seq(r.seq, r.len);
        as.seq(&NL, 1);
        if (r.len) as.qual(r.qual, r.len);
        as.qual(&NL, 1);
    };
    while (!as.dead) {
        const RecordFeed::Rec *r1 = f1.next(), *r2 = f2.next();
        if (!r1 && !r2) return;
        if (!r1 || !r2) {
            const uint64_t k = (r1 ? f1.taken : f2.taken);
            throw Np2Error(NP2_E_ARG, p1 + " and " + p2 + " do not hold the same number of records: " + (r1 ? p2 : p1) + " ended at record " +
                                          std::to_string(k) + ", which " + (r1 ? p1 : p2) + " has");
        }
        const size_t need = r1->len + r2->len + 2;
        if (need > as.cap)
            throw Np2Error(NP2_E_UNSUPPORTED, p1 + ": record " + std::to_string(f1.taken) + ": a pair of " + std::to_string(r1->len) + " + " +
                                                  std::to_string(r2->len) + " bases does not fit a piece of " + std::to_string(as.cap) + " bytes");
        if (as.cur && as.rs && as.rs + need > as.cap) as.flush();
        put(*r1), put(*r2);
    }
}

// Device side of one trimming run: SrqcDev's buffers with the trimmer's results and totals.
struct AdDev {
    np2srqc::Opts qc{};
    np2sradapt::Opts o{};
    DevBuf<uint8_t> d_qual;
    DevBuf<uint32_t> d_ends;
    DevBuf<np2_sradapt_read_t> d_reads;
    DevBuf<uint64_t> d_tot;
    DevEvent ev0, ev1;
    bool timed = false;
    float kernel_ms = 0;
    void init(hipStream_t st, size_t piece) {
        d_qual.ensure(QC_FRONT + piece + QC_BACK);
        d_tot.ensure(np2sradapt::N_TOTALS);
        ev0.make(), ev1.make();
        zero(st);
    }
    void zero(hipStream_t st) {
        HIPCHK(hipMemsetAsync(d_tot.p, 0, np2sradapt::N_TOTALS * 8, st));
        kernel_ms = 0;
    }
    // as SrqcDev::run
    void run(hipStream_t st, uint8_t *d_seq, QcPiece &pc, np2_sradapt_read_t *reads) {
        collect();
        const size_t n_reads = pc.ends.size();
        HIPCHK(hipMemcpyAsync(d_qual.p, pc.qual, pad_piece(pc.qual, pc.n), hipMemcpyHostToDevice, st));
        d_ends.ensure(n_reads + 1);
        HIPCHK(hipMemcpyAsync(d_ends.p, pc.ends.data(), n_reads * 4, hipMemcpyHostToDevice, st));
        if (reads) d_reads.ensure(n_reads + 1);
        HIPCHK(hipEventRecord(ev0.e, st));
        np2::launch_sradapt(st, d_seq + QC_FRONT, d_qual.p + QC_FRONT, d_ends.p, (uint32_t)n_reads, qc, o, reads ? d_reads.p : nullptr, d_tot.p);
        HIPCHK(hipEventRecord(ev1.e, st));
        timed = true;
        if (reads) HIPCHK(hipMemcpyAsync(reads, d_reads.p, n_reads * sizeof(np2_sradapt_read_t), hipMemcpyDeviceToHost, st));
    }
    void collect() {
        if (!timed) return;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0.e, ev1.e) == hipSuccess) kernel_ms += ms;
        timed = false;
    }
    void totals(hipStream_t st, uint64_t *out) { // (synchronises the stream)
        HIPCHK(hipMemcpyAsync(out, d_tot.p, np2sradapt::N_TOTALS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        collect();
    }
};

// the quality options of a trimming call: checked, or every step off without them
np2srqc::Opts sradapt_qc(const np2_srqc_opts_t *qc);
// the options of a call, checked (NP2_E_ARG); nullptr: pair mode with the defaults
np2sradapt::Opts sradapt_checked(const np2_sradapt_opts_t *ad);
// what np2_sradapt_last_stats / np2_sradapt_last_kernel_ms of this thread answer from now on
void sradapt_publish(const uint64_t *totals, float kernel_ms);

} // namespace np2h
