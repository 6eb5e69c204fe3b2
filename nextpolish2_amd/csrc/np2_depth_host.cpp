// Host driver of the mapping-depth kernels (np2_depth.hip): depth_device runs events -> scan -> runs -> keep over records
// that are on the device already and brings back the kept runs and the counters (the per-base array only on request);
// np2_depth_from_records uploads host records first.  np2_depth_from_bam (np2_bamread.cpp, over the record source of the readers) ends here too.
#include "np2_ctx.hpp"
#include "np2_depth.hpp"
#include "np2_kernel_timer.hpp"

namespace np2h {

np2::DepthRule depth_rule(const np2_depth_opts_t *o) {
    if (!o) throw Np2Error(NP2_E_ARG, "np2_depth: opts is NULL");
    if (!np2depth::fra_ok(o->min_aligned_fra))
        throw Np2Error(NP2_E_ARG, "np2_depth: min_aligned_fra must be a number in [0, 1], got " + std::to_string(o->min_aligned_fra));
    return np2::DepthRule{o->min_aligned_fra, o->min_depth, o->min_len, o->exclude_flags, o->min_mapq};
}

void depth_device(np2_ctx *cx, uint32_t L, const np2_bamrec_t *d_recs, uint32_t n_recs, const uint32_t *d_cigar, const np2::DepthRule &rule,
                  uint32_t **starts, uint32_t **ends, uint32_t *n_runs, uint32_t *depth_out, np2_depth_stats_t *stats) {
    if (L > np2::DEPTH_MAX_L) throw Np2Error(NP2_E_UNSUPPORTED, "np2_depth: contig of more than 4294901760 positions");
    *starts = *ends = nullptr;
    *n_runs = 0;
    np2_depth_stats_t st;
    memset(&st, 0, sizeof st);
    st.records_seen = n_recs;
    if (L == 0) { // no position, no run (and nothing to launch)
        if (stats) *stats = st;
        return;
    }
    hipStream_t s = cx->stream;
    const uint32_t max_runs = (uint32_t)(((uint64_t)L + 1) / 2);
    DevBuf<uint32_t> d_depth, d_s, d_e, d_ks, d_ke;
    DevBuf<np2::DepthDev> d_ctr;
    d_depth.cached = d_s.cached = d_e.cached = d_ks.cached = d_ke.cached = d_ctr.cached = true; // (released after the read-back below)
    d_depth.ensure((size_t)L + 1);
    d_s.ensure(max_runs), d_e.ensure(max_runs), d_ks.ensure(max_runs), d_ke.ensure(max_runs);
    d_ctr.ensure(1);
    HIPCHK(hipMemsetAsync(d_depth.p, 0, ((size_t)L + 1) * 4, s));
    HIPCHK(hipMemsetAsync(d_ctr.p, 0, sizeof(np2::DepthDev), s));
    // (descriptors first: the first one of a context fills its status words on the stream)
    Lookback lb_scan = next_lookback(cx, np2::depth_blocks(L)), lb_runs = next_lookback(cx, np2::depth_blocks(L)),
             lb_keep = next_lookback(cx, np2::depth_blocks(max_runs));
    lb_scan.err = lb_runs.err = lb_keep.err = &d_ctr.p->err;
    KernelTimer timer(true);
    try {
        timer.start(s);
        np2::launch_depth_events(s, d_recs, d_cigar, n_recs, L, rule, d_depth.p, d_ctr.p);
        np2::launch_depth_scan(s, lb_scan, d_depth.p, L, rule.min_depth, d_ctr.p);
        np2::launch_depth_runs(s, lb_runs, d_depth.p, L, rule.min_depth, d_s.p, d_e.p, d_ctr.p);
        np2::launch_depth_keep(s, lb_keep, d_s.p, d_e.p, max_runs, rule.min_len, d_ks.p, d_ke.p, d_ctr.p);
        timer.stop(s);
        HIPCHK(hipGetLastError());
    } catch (...) { // (tickets were issued for launches that may not have run: the next descriptor starts over)
        cx->lb_dirty = true;
        throw;
    }
    np2::DepthDev h;
    HIPCHK(hipMemcpyAsync(&h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    timer.collect();
    if (h.err) throw Np2Error(NP2_E_DEVICE, "np2_depth: a look-back wait gave up");
    if (h.n_runs > max_runs || h.n_kept > h.n_runs) throw Np2Error(NP2_E_DEVICE, "np2_depth: run counters out of range");
    if (h.n_kept) {
        uint32_t *hs = (uint32_t *)pinned_pool().get((size_t)h.n_kept * 4), *he = (uint32_t *)pinned_pool().get((size_t)h.n_kept * 4);
        if (!hs || !he) {
            if (hs) pinned_pool().put(hs);
            if (he) pinned_pool().put(he);
            throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
        }
        *starts = hs, *ends = he;
    }
    try {
        if (h.n_kept) {
            HIPCHK(hipMemcpyAsync(*starts, d_ks.p, (size_t)h.n_kept * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(*ends, d_ke.p, (size_t)h.n_kept * 4, hipMemcpyDeviceToHost, s));
        }
        if (depth_out) HIPCHK(hipMemcpyAsync(depth_out, d_depth.p, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } catch (...) { // (an error returns no array)
        if (*starts) pinned_pool().put(*starts);
        if (*ends) pinned_pool().put(*ends);
        *starts = *ends = nullptr;
        throw;
    }
    *n_runs = h.n_kept;
    st.records_counted = h.n_counted;
    st.sum_depth = h.sum_depth, st.max_depth = h.max_depth, st.bases_ok = h.bases_ok;
    st.runs = h.n_runs, st.runs_kept = h.n_kept, st.bases_kept = h.bases_kept;
    st.kernel_ms = timer.ms;
    if (stats) *stats = st;
}

} // namespace np2h

extern "C" {

int np2_depth_from_records(np2_ctx_t *cx, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                           const np2_depth_opts_t *opts, uint32_t **starts, uint32_t **ends, uint32_t *n_runs, uint32_t *depth,
                           np2_depth_stats_t *stats) {
    if (!cx) return NP2_E_ARG;
    if (starts) *starts = nullptr;
    if (ends) *ends = nullptr;
    if (n_runs) *n_runs = 0;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        const np2::DepthRule rule = depth_rule(opts);
        if (!starts || !ends || !n_runs) throw Np2Error(NP2_E_ARG, "np2_depth_from_records: starts, ends or n_runs is NULL");
        if (n_recs && !recs) throw Np2Error(NP2_E_ARG, "np2_depth_from_records: recs is NULL with n_recs > 0");
        uint64_t n_cig = 0;
        for (uint32_t i = 0; i < n_recs; ++i)
            if (recs[i].n_cigar) n_cig = std::max<uint64_t>(n_cig, recs[i].cigar_off + recs[i].n_cigar);
        if (n_cig && !cigar) throw Np2Error(NP2_E_ARG, "np2_depth_from_records: cigar is NULL with CIGAR words to read");
        HIPCHK(hipSetDevice(cx->device));
        DevBuf<np2_bamrec_t> d_recs;
        DevBuf<uint32_t> d_cigar;
        d_recs.cached = d_cigar.cached = true; // (released after depth_device has drained the stream)
        if (n_recs) {
            d_recs.ensure(n_recs);
            HIPCHK(hipMemcpyAsync(d_recs.p, recs, (size_t)n_recs * sizeof(np2_bamrec_t), hipMemcpyHostToDevice, cx->stream));
        }
        if (n_cig) {
            d_cigar.ensure(n_cig);
            HIPCHK(hipMemcpyAsync(d_cigar.p, cigar, n_cig * 4, hipMemcpyHostToDevice, cx->stream));
        }
        depth_device(cx, L, d_recs.p, n_recs, d_cigar.p, rule, starts, ends, n_runs, depth, stats);
        return NP2_OK;
    }, ctx_sink(cx));
}

} // extern "C"
