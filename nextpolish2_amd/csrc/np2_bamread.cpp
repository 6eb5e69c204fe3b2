// The entry points that read a reference's records out of an indexed BAM — a contig, its depth, a reference-interval shard —
// over one record source: read_records, the only place that chooses between the device reader and the host pool.
#include "np2_bamfile.hpp"
#include "np2_depth.hpp"
#include "np2_fetch_gpu.hpp"
#include "np2_frontend.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_varcall.hpp"

namespace {

enum : unsigned { WANT_SEQ = 1, WANT_VOFFS = 2 }; // what a caller needs besides positions, flags and CIGARs
// The records of reference `tid` that overlap [zone_lo, zone_hi) (the whole contig: [0, L)), in file order.  Extracted on the
// device where that is wanted and possible — not for -S, whose SEQ of secondary records is a pass of the host's; a caller that
// wants no SEQ does not care —, by the host pool otherwise: its SEQ streamed to the device on `stream`, kept on the host for -S,
// not copied at all for a caller that wants none.
RecordSet read_records(np2_bam *bam, int tid, uint32_t L, uint32_t zone_lo, uint32_t zone_hi, const np2_front_opts_t *opts, hipStream_t stream,
                       unsigned want) {
    RecordSet rs;
    std::vector<uint64_t> *voffs = (want & WANT_VOFFS) ? &rs.voffs : nullptr;
    const bool with_seq = want & WANT_SEQ, from_primaries = with_seq && opts->use_secondary;
    // (fetch_records_gpu false: not this BAM / index, or no room on the device)
    rs.from_device = gpu_fetch_wanted(bam, tid) && !from_primaries && fetch_records_gpu(bam, tid, L, zone_lo, zone_hi, stream, rs, voffs);
    if (rs.from_device) return rs;
    rs.voffs.clear();
    fetch_records(bam, tid, L, zone_lo, zone_hi, opts, rs.own_recs, rs.own_cigar, voffs, with_seq ? stream : nullptr, &rs.seq_bytes, !with_seq);
    rs.recs = rs.own_recs.data(), rs.cigar = rs.own_cigar.data(), rs.n_recs = (uint32_t)rs.own_recs.size();
    if (with_seq && !from_primaries) rs.d_seq = bam->seqs.dev.p;
    else rs.seq4 = bam->seq4.data();
    return rs;
}

} // namespace

// ---- a reference-interval shard straight from the BAM -----------------------------------------------------------------
// Each rank reads only the records overlapping its zone (own interval +- halo; .bai linear index), admits and
// columnarises them on its GPU, and learns which of them are pushed (main.rs:1798-1813).  The contig-wide read numbers
// (the reference numbers pushed records in file order, main.rs:1813) come from one exchange: every rank publishes
// the BGZF virtual offsets of the pushed records that START in its own interval (it sees all of those); the lists,
// concatenated in rank order, are the contig's pushed records in file order, and a record's number is 1 + its place.
struct np2_shard_io {
    np2_ctx *cx = nullptr;
    FrontWork fw;
    np2_shard_plan_t plan{};
    std::vector<uint64_t> rec_voff;  // per fetched record
    std::vector<uint64_t> own_voff;  // pushed records starting in [own_lo, own_hi), file order
};

extern "C" {

int np2_contig_from_bam(np2_ctx_t *cx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L,
                        const np2_front_opts_t *opts, np2_contig_t **out) {
    if (!cx || !bam || !name || !ref || !opts || !out) return NP2_E_ARG;
    *out = nullptr;
    return np2h::abi_guard([&] {
        const int tid = ref_id(bam, name);
        const bool prof = getenv("NP2_IO_PROFILE") != nullptr;
        const double t_p0 = np2h::now_ms();
        bam->batch.ms_read = bam->batch.ms_inflate = bam->batch.ms_drop = bam->batch.ms_walk = bam->batch.ms_size = bam->batch.ms_copy = 0;
        HIPCHK(hipSetDevice(cx->device));
        const RecordSet rs = read_records(bam, tid, L, 0, L, opts, cx->stream, WANT_SEQ);
        const double t_p1 = np2h::now_ms();
        {
            FrontWork fw;
            front_begin(cx, ref, L, rs, opts, nullptr, fw);
            front_finish(cx, fw, out);
        }
        if (prof && rs.from_device)
            fprintf(stderr, "np2_contig_from_bam %s: device read extraction %.2f ms (%u records), records->pileup %.2f ms\n", name, t_p1 - t_p0, rs.n_recs, np2h::now_ms() - t_p1);
        else if (prof)
            fprintf(stderr, "np2_contig_from_bam %s: inflate+parse %.2f ms (block headers %.2f, inflate [%s] %.2f, buffer moves %.2f, record "
                            "walk %.2f, array sizing %.2f, record copies %.2f; %zu records, %zu SEQ bytes), records->pileup %.2f ms\n",
                    name, t_p1 - t_p0, bam->batch.ms_read, inflater_name(), bam->batch.ms_inflate, bam->batch.ms_drop,
                    bam->batch.ms_walk, bam->batch.ms_size, bam->batch.ms_copy, (size_t)rs.n_recs, (size_t)rs.seq_bytes, np2h::now_ms() - t_p1);
        np2h::flush_timings(cx);
        return NP2_OK;
    }, np2h::ctx_sink(cx, true));
}

// Mapping depth of contig `name` and its runs of sufficient depth (np2_depth.hip).  The records come from the reader
// np2_contig_from_bam would take: on the device path they and their CIGAR words are in HBM already (RecordSet::d_recs,
// d_cigar) and the kernels read them there; on the host path positions, flags and CIGAR words are uploaded, SEQ is not read.
int np2_depth_from_bam(np2_ctx_t *cx, np2_bam_t *bam, const char *name, uint32_t L, const np2_depth_opts_t *opts, uint32_t **starts,
                       uint32_t **ends, uint32_t *n_runs, uint32_t *depth, np2_depth_stats_t *stats) {
    if (!cx) return NP2_E_ARG;
    if (starts) *starts = nullptr;
    if (ends) *ends = nullptr;
    if (n_runs) *n_runs = 0;
    return np2h::abi_guard([&] {
        // every argument is checked before anything is launched
        const np2::DepthRule rule = np2h::depth_rule(opts);
        if (!bam || !name || !starts || !ends || !n_runs) throw np2h::Np2Error(NP2_E_ARG, "np2_depth_from_bam: bam, name, starts, ends or n_runs is NULL");
        const int tid = ref_id(bam, name);
        HIPCHK(hipSetDevice(cx->device));
        np2_front_opts_t fo;
        memset(&fo, 0, sizeof fo); // (read admission plays no part; -S off: no pass over the file for SEQ nobody reads)
        const RecordSet rs = read_records(bam, tid, L, 0, L, &fo, cx->stream, 0);
        np2h::DevBuf<np2_bamrec_t> d_recs;
        np2h::DevBuf<uint32_t> d_cigar;
        d_recs.cached = d_cigar.cached = true; // (released after depth_device has drained the stream)
        auto upload = [&](auto &buf, const auto &v) { // (the host reader's vectors: empty on the device path)
            if (v.empty()) return;
            buf.ensure(v.size());
            HIPCHK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice, cx->stream));
        };
        upload(d_recs, rs.own_recs), upload(d_cigar, rs.own_cigar);
        np2h::depth_device(cx, L, rs.from_device ? rs.d_recs : d_recs.p, rs.n_recs, rs.from_device ? rs.d_cigar : d_cigar.p, rule, starts, ends, n_runs,
                           depth, stats);
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}

// Read-supported variants of contig `name` (np2_varcall.hip).  The records come from the reader np2_contig_from_bam would
// take, SEQ included: on the device path records, CIGAR words and SEQ are in HBM already; on the host path the pool has
// streamed SEQ to the device, and positions, flags and CIGAR words are uploaded here.
int np2_varcall_from_bam(np2_ctx_t *cx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L, const np2_varcall_opts_t *opts,
                         np2_varcall_t **calls, uint32_t *n_calls, uint32_t *cov, uint32_t *alt, np2_varcall_stats_t *stats) {
    if (!cx) return NP2_E_ARG;
    if (calls) *calls = nullptr;
    if (n_calls) *n_calls = 0;
    return np2h::abi_guard([&] {
        // every argument is checked before anything is launched
        const np2vc::Rule rule = np2h::varcall_rule(opts);
        if (!bam || !name || !calls || !n_calls || (L && !ref)) throw np2h::Np2Error(NP2_E_ARG, "np2_varcall_from_bam: bam, name, ref, calls or n_calls is NULL");
        const int tid = ref_id(bam, name);
        HIPCHK(hipSetDevice(cx->device));
        np2_front_opts_t fo;
        memset(&fo, 0, sizeof fo); // (read admission plays no part; -S off: SEQ is every record's own)
        const RecordSet rs = read_records(bam, tid, L, 0, L, &fo, cx->stream, WANT_SEQ);
        uint64_t n_cig = rs.own_cigar.size();
        if (rs.from_device)
            for (uint32_t i = 0; i < rs.n_recs; ++i)
                if (rs.recs[i].n_cigar) n_cig = std::max<uint64_t>(n_cig, rs.recs[i].cigar_off + rs.recs[i].n_cigar);
        np2h::varcall_check_records(rs.recs, rs.n_recs, n_cig, rs.seq_bytes, "np2_varcall_from_bam");
        if (rs.seq_bytes && !rs.d_seq) throw np2h::Np2Error(NP2_E_DEVICE, "np2_varcall_from_bam: the reader left no SEQ on the device");
        np2h::DevBuf<np2_bamrec_t> d_recs;
        np2h::DevBuf<uint32_t> d_cigar;
        d_recs.cached = d_cigar.cached = true; // (released after varcall_device has drained the stream)
        auto upload = [&](auto &buf, const auto &v) { // (the host reader's vectors: empty on the device path)
            if (v.empty()) return;
            buf.ensure(v.size());
            HIPCHK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof v[0], hipMemcpyHostToDevice, cx->stream));
        };
        upload(d_recs, rs.own_recs), upload(d_cigar, rs.own_cigar);
        np2h::varcall_device(cx, ref, L, rs.from_device ? rs.d_recs : d_recs.p, rs.n_recs, rs.from_device ? rs.d_cigar : d_cigar.p, n_cig, rs.d_seq,
                             rs.seq_bytes, rule, calls, n_calls, cov, alt, stats);
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}

int np2_shard_bam_begin(np2_ctx_t *cx, np2_bam_t *bam, const char *name, const uint8_t *ref, uint32_t L, uint32_t own_lo,
                        uint32_t own_hi, uint32_t halo, const np2_front_opts_t *opts, np2_shard_io_t **out,
                        const uint64_t **own_voffsets, uint64_t *n_own) {
    if (!cx || !bam || !name || !ref || !opts || !out || !own_voffsets || !n_own || own_lo >= own_hi || own_hi > L)
        return NP2_E_ARG;
    *out = nullptr;
    std::unique_ptr<np2_shard_io> io; // (freed after the sink's sync)
    return np2h::abi_guard([&] {
        io.reset(new np2_shard_io());
        io->cx = cx;
        const int tid = ref_id(bam, name);
        np2_shard_plan_t &pl = io->plan;
        pl.own_lo = own_lo, pl.own_hi = own_hi;
        pl.zone_lo = own_lo > halo ? own_lo - halo : 0u;
        pl.zone_hi = (uint64_t)own_hi + halo < L ? own_hi + halo : L;
        HIPCHK(hipSetDevice(cx->device));
        // the interval's records: extracted on the device (a rank of eight has two of the node's CPUs) or by the host pool.  On the
        // device path they are read where they lie, in the handle's pinned blocks: good until the next fetch on the handle, and
        // nothing below keeps a pointer to them
        RecordSet rs = read_records(bam, tid, L, pl.zone_lo, pl.zone_hi, opts, cx->stream, WANT_SEQ | WANT_VOFFS);
        io->rec_voff = std::move(rs.voffs);
        // the sub-contig: from the first start to the last reference end among the fetched records
        uint32_t slo = pl.zone_lo, shi = pl.zone_hi;
        for (uint32_t i = 0; i < rs.n_recs; ++i) {
            const np2_bamrec_t &r = rs.recs[i];
            const uint64_t span = ref_span(rs.cigar + r.cigar_off, r.n_cigar);
            if (r.pos >= 0) slo = std::min<uint32_t>(slo, (uint32_t)r.pos);
            shi = (uint32_t)std::min<uint64_t>(L, std::max<uint64_t>(shi, (uint64_t)r.pos + span));
        }
        pl.sub_lo = own_lo == 0 ? 0u : (slo & ~63u);
        pl.sub_hi = own_hi == L ? L : shi;
        ShardSpec sp;
        sp.sub_lo = pl.sub_lo, sp.sub_hi = pl.sub_hi, sp.zone_lo = pl.zone_lo, sp.zone_hi = pl.zone_hi;
        front_begin(cx, ref, L, rs, opts, &sp, io->fw);
        for (size_t i = 1; i < io->fw.reads.size(); ++i) {
            const np2_bamrec_t &r = rs.recs[io->fw.rec_of[i]];
            if ((uint32_t)r.pos >= own_lo && (uint32_t)r.pos < own_hi) io->own_voff.push_back(io->rec_voff[io->fw.rec_of[i]]);
        }
        np2h::flush_timings(cx);
        *own_voffsets = io->own_voff.data();
        *n_own = io->own_voff.size();
        *out = io.release();
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}

void np2_shard_bam_abort(np2_shard_io_t *io) { delete io; }

int np2_shard_bam_finish(np2_shard_io_t *io, const uint64_t *all_voffsets, uint64_t n_all, np2_shard_plan_t *plan,
                         np2_contig_t **contig, uint32_t *n_reads_total) {
    if (!io || (n_all && !all_voffsets) || !plan || !contig || !n_reads_total) return NP2_E_ARG;
    std::unique_ptr<np2_shard_io> owned(io); // (freed after the sink's sync, whatever the outcome)
    np2_ctx *cx = io->cx;
    *contig = nullptr;
    return np2h::abi_guard([&] {
        FrontWork &fw = io->fw;
        // contig-wide number of every pushed record this shard fetched
        const size_t n = fw.reads.size();
        std::vector<uint32_t> gid(n, 0);
        for (size_t i = 1; i < n; ++i) {
            const uint64_t v = io->rec_voff[fw.rec_of[i]];
            const uint64_t *it = std::lower_bound(all_voffsets, all_voffsets + n_all, v);
            if (it == all_voffsets + n_all || *it != v)
                throw np2h::Np2Error(NP2_E_ARG, "shard: a pushed record is missing from the exchanged offsets (do the ranks' own intervals tile the contig?)");
            gid[i] = 1 + (uint32_t)(it - all_voffsets);
            if (i > 1 && gid[i] <= gid[i - 1]) throw np2h::Np2Error(NP2_E_ARG, "shard: exchanged offsets are not in file order");
        }
        np2_shard_plan_t &pl = io->plan;
        pl.read_lo = n > 1 ? gid[1] : 1u;
        pl.read_hi = n > 1 ? gid[n - 1] + 1 : 1u;
        // holes: reads of the contig inside [read_lo, read_hi) this shard does not hold keep their number
        std::vector<np2_read_t> reads(1 + (size_t)(pl.read_hi - pl.read_lo));
        std::vector<uint8_t> lable(reads.size(), 0);
        np2_read_t hole;
        memset(&hole, 0, sizeof hole);
        hole.flags = NP2_READ_DROPPED;
        hole.nib_off = 0; // (never decoded; slot 0 is a valid aligned offset)
        std::fill(reads.begin(), reads.end(), hole);
        reads[0] = fw.reads[0];
        for (size_t i = 1; i < n; ++i) {
            reads[gid[i] - pl.read_lo + 1] = fw.reads[i];
            lable[gid[i] - pl.read_lo + 1] = fw.lable[i];
        }
        fw.reads.swap(reads);
        fw.lable.swap(lable);
        np2_contig *c = nullptr;
        front_finish(cx, fw, &c);
        *contig = c;
        *plan = pl;
        *n_reads_total = 1 + (uint32_t)n_all;
        np2h::flush_timings(cx);
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}
}
