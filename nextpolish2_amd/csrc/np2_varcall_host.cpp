// Host driver of the variant caller's kernels (np2_varcall.hip).  varcall_device runs records -> key sorts -> alleles ->
// coverage scan -> calls (counted, then written) over records, CIGAR words and SEQ that are on the device already, and brings
// back the calls and the counters (cov and alt only on request); np2_varcall_from_records uploads host arrays first,
// np2_varcall_from_bam (np2_bamread.cpp, over the record source of the readers) ends here too.  np2_varcall_host is the rule
// on one CPU thread (np2vc::call_contig).
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_map.hpp"
#include "np2_varcall.hpp"

namespace np2h {

np2vc::Rule varcall_rule(const np2_varcall_opts_t *o) {
    if (!o) throw Np2Error(NP2_E_ARG, "np2_varcall: opts is NULL");
    const np2vc::Rule r{o->min_aligned_fra, o->exclude_flags, o->min_mapq, o->min_depth, o->min_alt, o->hom_pm, o->het_pm, o->max_indel};
    if (!np2depth::fra_ok(r.min_aligned_fra))
        throw Np2Error(NP2_E_ARG, "np2_varcall: min_aligned_fra must be a number in [0, 1], got " + std::to_string(o->min_aligned_fra));
    if (!np2vc::rule_ok(r))
        throw Np2Error(NP2_E_ARG, "np2_varcall: need het_pm <= hom_pm <= 1000, 1 <= max_indel <= 28 and min_alt >= 1, got het_pm " +
                                      std::to_string(r.het_pm) + ", hom_pm " + std::to_string(r.hom_pm) + ", max_indel " + std::to_string(r.max_indel) +
                                      ", min_alt " + std::to_string(r.min_alt));
    return r;
}

void varcall_check_records(const np2_bamrec_t *recs, uint32_t n_recs, uint64_t n_cig, uint64_t seq_bytes, const char *who) {
    for (uint32_t i = 0; i < n_recs; ++i) {
        const np2_bamrec_t &r = recs[i];
        if (r.n_cigar && (r.cigar_off > n_cig || r.n_cigar > n_cig - r.cigar_off))
            throw Np2Error(NP2_E_ARG, std::string(who) + ": CIGAR of record " + std::to_string(i) + " outside the buffer");
        const uint64_t nb = ((uint64_t)r.l_seq + 1) / 2;
        if (r.l_seq && (r.seq_off > seq_bytes || nb > seq_bytes - r.seq_off))
            throw Np2Error(NP2_E_ARG, std::string(who) + ": SEQ of record " + std::to_string(i) + " outside the buffer");
    }
}

static void fill_stats(np2_varcall_stats_t &st, const np2::VarDev &h) {
    st.records_counted = h.n_counted, st.records_no_seq = h.n_no_seq, st.records_skipped = h.n_skipped;
    st.events = h.n_events, st.alleles = h.n_alleles, st.callable = h.callable;
    for (int i = 0; i < 6; ++i) st.calls[i] = h.calls[i];
}

void varcall_device(np2_ctx *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *d_recs, uint32_t n_recs, const uint32_t *d_cigar,
                    uint64_t n_cig, const uint8_t *d_seq, uint64_t seq_bytes, const np2vc::Rule &rule, np2_varcall_t **calls, uint32_t *n_calls,
                    uint32_t *cov, uint32_t *alt, np2_varcall_stats_t *stats) {
    if (L > np2::DEPTH_MAX_L) throw Np2Error(NP2_E_UNSUPPORTED, "np2_varcall: contig of more than 4294901760 positions");
    if (n_cig > 0xFFFF0000ull) throw Np2Error(NP2_E_UNSUPPORTED, "np2_varcall: more than 4294901760 CIGAR words");
    *calls = nullptr;
    *n_calls = 0;
    np2_varcall_stats_t st;
    memset(&st, 0, sizeof st);
    st.records_seen = n_recs;
    if (L == 0) { // no position: no record is counted (and nothing to launch)
        if (stats) *stats = st;
        return;
    }
    hipStream_t s = cx->stream;
    const uint32_t ev_cap = (uint32_t)n_cig; // an event is a CIGAR word
    DevBuf<uint8_t> d_ref, d_tmp;
    DevBuf<uint32_t> d_cov, d_alt, d_best, d_bestc;
    DevBuf<uint64_t> d_hi, d_lo, d_hi2, d_lo2;
    DevBuf<np2_varcall_t> d_calls;
    DevBuf<np2::VarDev> d_ctr;
    DevBuf<np2::DepthDev> d_dctr;
    d_ref.cached = d_tmp.cached = d_cov.cached = d_alt.cached = d_best.cached = d_bestc.cached = d_hi.cached = d_lo.cached = d_hi2.cached =
        d_lo2.cached = d_calls.cached = d_ctr.cached = d_dctr.cached = true; // (released after the read-backs below)
    d_ref.ensure((size_t)L + 16);
    d_cov.ensure((size_t)L + 1), d_alt.ensure((size_t)4 * L), d_best.ensure((size_t)2 * L), d_bestc.ensure((size_t)2 * L);
    if (ev_cap) d_hi.ensure(ev_cap), d_lo.ensure(ev_cap);
    d_ctr.ensure(1), d_dctr.ensure(1);
    // every array a kernel adds into or reads without having written it is cleared on the stream; the key arrays are read up
    // to ctr->n_events only, which the record kernel wrote
    HIPCHK(hipMemcpyAsync(d_ref.p, ref, L, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_cov.p, 0, ((size_t)L + 1) * 4, s));
    HIPCHK(hipMemsetAsync(d_alt.p, 0, (size_t)L * 16, s));
    HIPCHK(hipMemsetAsync(d_best.p, 0, (size_t)L * 8, s));
    HIPCHK(hipMemsetAsync(d_bestc.p, 0, (size_t)L * 8, s));
    HIPCHK(hipMemsetAsync(d_ctr.p, 0, sizeof(np2::VarDev), s));
    HIPCHK(hipMemsetAsync(d_dctr.p, 0, sizeof(np2::DepthDev), s));
    Lookback lb_scan = next_lookback(cx, np2::depth_blocks(L)); // (the first one of a context fills its status words on the stream)
    lb_scan.err = &d_dctr.p->err;
    // HIP events around every stage: records, coverage scan, key sorts, alleles, calls counted, calls written
    KernelTimer t_rec(true), t_scan(true), t_sort(true), t_all(true), t_cnt(true), t_emit(true);
    std::vector<KernelTimer *> pending; // stopped, to be collected at the next synchronisation
    auto timed = [&](KernelTimer &t, auto &&launch) {
        t.start(s);
        launch();
        t.stop(s);
        pending.push_back(&t);
    };
    np2::VarDev h;
    const uint64_t *k_hi = nullptr, *k_lo = nullptr; // the sorted keys
    auto read_ctr = [&] {
        HIPCHK(hipMemcpyAsync(&h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (KernelTimer *t : pending) t->collect();
        pending.clear();
        if (h.err & np2::LB_ERR) throw Np2Error(NP2_E_DEVICE, "np2_varcall: a look-back wait gave up");
        if (h.err & np2::VC_ERR_SEQ) throw Np2Error(NP2_E_ARG, "np2_varcall: SEQ of a counted record outside the buffer");
        if (h.err || h.n_events > ev_cap) throw Np2Error(NP2_E_DEVICE, "np2_varcall: counters out of range");
    };
    try {
        timed(t_rec, [&] { np2::launch_varcall_records(s, d_recs, d_cigar, d_seq, seq_bytes, n_recs, d_ref.p, L, rule, d_cov.p, d_alt.p, d_hi.p, d_lo.p, ev_cap, d_ctr.p); });
        timed(t_scan, [&] { np2::launch_depth_scan(s, lb_scan, d_cov.p, L, rule.min_depth, d_dctr.p); });
        HIPCHK(hipGetLastError());
    } catch (...) { // (a ticket was issued for a launch that may not have run: the next descriptor starts over)
        cx->lb_dirty = true;
        throw;
    }
    read_ctr();
    const uint32_t n_ev = h.n_events;
    if (n_ev) {
        // stable pair sorts, least significant word first: by bases, then by (anchor, kind, n)
        d_hi2.ensure(n_ev), d_lo2.ensure(n_ev);
        const size_t tmp_bytes = np2::prim_pairs64_temp_bytes(n_ev);
        d_tmp.ensure(tmp_bytes);
        timed(t_sort, [&] {
            if (np2::prim_sort_pairs_u64_u64(s, d_tmp.p, tmp_bytes, d_lo.p, d_lo2.p, d_hi.p, d_hi2.p, n_ev, np2vc::KEY_LO_BITS) ||
                np2::prim_sort_pairs_u64_u64(s, d_tmp.p, tmp_bytes, d_hi2.p, d_hi.p, d_lo2.p, d_lo.p, n_ev, np2vc::KEY_HI_BITS))
                throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
        });
        k_hi = d_hi.p, k_lo = d_lo.p;
        timed(t_all, [&] { np2::launch_varcall_alleles(s, k_hi, k_lo, n_ev, L, d_best.p, d_bestc.p, d_ctr.p); });
    }
    timed(t_cnt, [&] { np2::launch_varcall_calls(s, lb_scan, d_ref.p, L, d_cov.p, d_alt.p, d_best.p, d_bestc.p, k_hi, k_lo, rule, nullptr, 0, d_ctr.p); });
    HIPCHK(hipGetLastError());
    read_ctr();
    {
        np2::DepthDev dh;
        HIPCHK(hipMemcpyAsync(&dh, d_dctr.p, sizeof dh, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (dh.err) throw Np2Error(NP2_E_DEVICE, "np2_varcall: a look-back wait gave up");
    }
    const uint32_t n = h.n_calls;
    if (n) {
        *calls = (np2_varcall_t *)pinned_pool().get((size_t)n * sizeof(np2_varcall_t));
        if (!*calls) throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
    }
    try {
        if (n) {
            d_calls.ensure(n);
            Lookback lb_calls = next_lookback(cx, np2::depth_blocks(L));
            lb_calls.err = &d_ctr.p->err;
            try {
                timed(t_emit, [&] { np2::launch_varcall_calls(s, lb_calls, d_ref.p, L, d_cov.p, d_alt.p, d_best.p, d_bestc.p, k_hi, k_lo, rule, d_calls.p, n, d_ctr.p); });
                HIPCHK(hipGetLastError());
            } catch (...) {
                cx->lb_dirty = true;
                throw;
            }
            HIPCHK(hipMemcpyAsync(*calls, d_calls.p, (size_t)n * sizeof(np2_varcall_t), hipMemcpyDeviceToHost, s));
        }
        if (cov) HIPCHK(hipMemcpyAsync(cov, d_cov.p, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        if (alt) HIPCHK(hipMemcpyAsync(alt, d_alt.p, (size_t)L * 16, hipMemcpyDeviceToHost, s));
        if (n) read_ctr(); // (the look-back's error word)
        else HIPCHK(hipStreamSynchronize(s));
    } catch (...) { // (an error returns no array)
        if (*calls) pinned_pool().put(*calls);
        *calls = nullptr;
        throw;
    }
    *n_calls = n;
    fill_stats(st, h);
    const KernelTimer *stages[6] = {&t_rec, &t_scan, &t_sort, &t_all, &t_cnt, &t_emit};
    for (int i = 0; i < 6; ++i) st.stage_ms[i] = stages[i]->ms, st.kernel_ms += stages[i]->ms;
    if (stats) *stats = st;
}

} // namespace np2h

extern "C" {

int np2_varcall_from_records(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                             const uint8_t *seq4, const np2_varcall_opts_t *opts, np2_varcall_t **calls, uint32_t *n_calls, uint32_t *cov,
                             uint32_t *alt, np2_varcall_stats_t *stats) {
    if (!cx) return NP2_E_ARG;
    if (calls) *calls = nullptr;
    if (n_calls) *n_calls = 0;
    return np2h::abi_guard([&] {
        using namespace np2h;
        // every argument is checked before anything is launched
        const np2vc::Rule rule = varcall_rule(opts);
        if (!calls || !n_calls) throw Np2Error(NP2_E_ARG, "np2_varcall_from_records: calls or n_calls is NULL");
        if (L && !ref) throw Np2Error(NP2_E_ARG, "np2_varcall_from_records: ref is NULL");
        if (n_recs && !recs) throw Np2Error(NP2_E_ARG, "np2_varcall_from_records: recs is NULL with n_recs > 0");
        uint64_t n_cig = 0, seq_bytes = 0;
        for (uint32_t i = 0; i < n_recs; ++i) {
            if (recs[i].n_cigar) n_cig = std::max<uint64_t>(n_cig, recs[i].cigar_off + recs[i].n_cigar);
            if (recs[i].l_seq) seq_bytes = std::max<uint64_t>(seq_bytes, recs[i].seq_off + ((uint64_t)recs[i].l_seq + 1) / 2);
        }
        if (n_cig && !cigar) throw Np2Error(NP2_E_ARG, "np2_varcall_from_records: cigar is NULL with CIGAR words to read");
        if (seq_bytes && !seq4) throw Np2Error(NP2_E_ARG, "np2_varcall_from_records: seq4 is NULL with SEQ to read");
        HIPCHK(hipSetDevice(cx->device));
        DevBuf<np2_bamrec_t> d_recs;
        DevBuf<uint32_t> d_cigar;
        DevBuf<uint8_t> d_seq;
        d_recs.cached = d_cigar.cached = d_seq.cached = true; // (released after varcall_device has drained the stream)
        auto upload = [&](auto &buf, const auto *p, size_t n) {
            if (!n) return;
            buf.ensure(n);
            HIPCHK(hipMemcpyAsync(buf.p, p, n * sizeof *p, hipMemcpyHostToDevice, cx->stream));
        };
        upload(d_recs, recs, n_recs), upload(d_cigar, cigar, n_cig), upload(d_seq, seq4, seq_bytes);
        varcall_device(cx, ref, L, d_recs.p, n_recs, d_cigar.p, n_cig, d_seq.p, seq_bytes, rule, calls, n_calls, cov, alt, stats);
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}

int np2_varcall_host(const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar, uint64_t n_cigar_words,
                     const uint8_t *seq4, uint64_t seq_bytes, const np2_varcall_opts_t *opts, np2_varcall_t **calls, uint32_t *n_calls,
                     uint32_t *cov, uint32_t *alt, np2_varcall_stats_t *stats) {
    if (calls) *calls = nullptr;
    if (n_calls) *n_calls = 0;
    return np2h::abi_guard([&] {
        using namespace np2h;
        const np2vc::Rule rule = varcall_rule(opts);
        if (!calls || !n_calls) throw Np2Error(NP2_E_ARG, "np2_varcall_host: calls or n_calls is NULL");
        if ((L && !ref) || (n_recs && !recs) || (n_cigar_words && !cigar) || (seq_bytes && !seq4))
            throw Np2Error(NP2_E_ARG, "np2_varcall_host: ref, recs, cigar or seq4 is NULL");
        if (L > np2::DEPTH_MAX_L) throw Np2Error(NP2_E_UNSUPPORTED, "np2_varcall: contig of more than 4294901760 positions");
        varcall_check_records(recs, n_recs, n_cigar_words, seq_bytes, "np2_varcall_host");
        np2vc::Contig c;
        if (!np2vc::call_contig(ref, L, recs, n_recs, cigar, seq4, seq_bytes, rule, c)) throw Np2Error(NP2_E_ARG, "np2_varcall_host: SEQ outside the buffer");
        if (!c.calls.empty()) {
            *calls = (np2_varcall_t *)malloc(c.calls.size() * sizeof(np2_varcall_t)); // (np2_free frees what is not the pool's)
            if (!*calls) throw Np2Error(NP2_E_NOMEM, "out of memory for the calls");
            memcpy(*calls, c.calls.data(), c.calls.size() * sizeof(np2_varcall_t));
        }
        *n_calls = (uint32_t)c.calls.size();
        if (cov && L) memcpy(cov, c.cov.data(), (size_t)L * 4);
        if (alt && L) memcpy(alt, c.alt.data(), (size_t)L * 16);
        if (stats) *stats = c.stats;
        return NP2_OK;
    }, [](int code, const std::string &msg) { np2h::io_set_error(code, msg); });
}

} // extern "C"
