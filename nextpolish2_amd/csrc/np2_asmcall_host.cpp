// Host driver of the assembly-to-reference caller's kernels (np2_asmcall.hip).  np2_asmcall checks every argument on the host
// (np2ac::check, which also decides admission: it has to walk every CIGAR anyway), uploads, and runs walk (counted) -> coverage
// scan -> cov == 1 counts -> event offsets -> runs -> walk (written) -> filter -> stable pair sort -> gather.  np2_asmcall_host
// is the rule on one CPU thread (np2ac::call_all).
#include <deque>

#include "np2_asmcall.hpp"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_map.hpp"

namespace np2h {

namespace {

struct AsmArgs {
    const uint8_t *refs;
    const uint64_t *ref_off;
    uint32_t n_refs;
    const uint8_t *query;
    uint64_t query_bytes;
    const np2_asmaln_t *alns;
    uint32_t n_alns;
    const uint32_t *cigar;
    uint64_t n_cigar_words;
    const np2_asmcall_opts_t *opts;
    np2_asmrun_t **runs;
    uint32_t *n_runs;
    np2_asmvar_t **vars;
    uint32_t *n_vars;
};

// every refusal of include/np2_io.h, before anything else; -> every alignment's admission outcome
std::vector<uint8_t> asmcall_check(const AsmArgs &a, const char *who) {
    const std::string w(who);
    if (!a.opts || !a.runs || !a.n_runs || !a.vars || !a.n_vars || !a.ref_off) throw Np2Error(NP2_E_ARG, w + ": opts, ref_off or an output is NULL");
    if ((a.ref_off[a.n_refs] && !a.refs) || (a.query_bytes && !a.query) || (a.n_alns && !a.alns) || (a.n_cigar_words && !a.cigar))
        throw Np2Error(NP2_E_ARG, w + ": refs, query, alns or cigar is NULL");
    std::vector<uint8_t> adm;
    bool unsupported;
    uint32_t bad;
    if (const char *msg = np2ac::check(a.ref_off, a.n_refs, a.query_bytes, a.alns, a.n_alns, a.cigar, a.n_cigar_words, a.opts->min_mapq, a.opts->min_aln,
                                       &adm, &unsupported, &bad))
        throw Np2Error(unsupported ? NP2_E_UNSUPPORTED : NP2_E_ARG, w + ": " + msg + (bad != 0xFFFFFFFFu ? " (alignment " + std::to_string(bad) + ")" : ""));
    return adm;
}

void count_admission(np2_asmcall_stats_t &st, const std::vector<uint8_t> &adm) {
    st.alns_seen = adm.size();
    for (uint8_t x : adm) {
        st.alns_admitted += x == np2ac::ALN_ADMITTED, st.alns_unaligned += x == np2ac::ALN_UNALIGNED, st.alns_low_mapq += x == np2ac::ALN_LOW_MAPQ;
        st.alns_skipped += x == np2ac::ALN_SKIPPED, st.alns_short += x == np2ac::ALN_SHORT;
    }
}

void asmcall_device(np2_ctx *cx, const AsmArgs &a, const std::vector<uint8_t> &adm, uint32_t *cov, np2_asmcall_stats_t *stats) {
    np2_asmcall_stats_t st;
    memset(&st, 0, sizeof st);
    count_admission(st, adm);
    const uint32_t G = (uint32_t)a.ref_off[a.n_refs];
    if (G == 0) { // no position: no column, no event, no run (and nothing to launch)
        if (stats) *stats = st;
        return;
    }
    std::vector<uint32_t> adm_idx;
    for (uint32_t i = 0; i < a.n_alns; ++i)
        if (adm[i] == np2ac::ALN_ADMITTED) adm_idx.push_back(i);
    const uint32_t n_adm = (uint32_t)adm_idx.size();
    const uint32_t max_runs = (uint32_t)std::min<uint64_t>(G, ((uint64_t)G + 1) / 2 + a.n_refs);
    hipStream_t s = cx->stream;
    DevBuf<uint8_t> d_refs, d_query, d_tmp;
    DevBuf<uint64_t> d_off, d_keys, d_kkeys, d_kidx, d_skeys, d_sidx;
    DevBuf<np2_asmaln_t> d_alns;
    DevBuf<uint32_t> d_cigar, d_adm, d_cov, d_ones, d_cnt;
    DevBuf<np2_asmrun_t> d_runs;
    DevBuf<np2_asmvar_t> d_raw, d_vars;
    DevBuf<np2::AsmDev> d_ctr;
    DevBuf<np2::DepthDev> d_dctr;
    d_refs.cached = d_query.cached = d_tmp.cached = d_off.cached = d_keys.cached = d_kkeys.cached = d_kidx.cached = d_skeys.cached = d_sidx.cached =
        d_alns.cached = d_cigar.cached = d_adm.cached = d_cov.cached = d_ones.cached = d_cnt.cached = d_runs.cached = d_raw.cached = d_vars.cached =
            d_ctr.cached = d_dctr.cached = true; // (released after the stream has been drained)
    auto upload = [&](auto &buf, const auto *p, size_t n) {
        buf.ensure(std::max<size_t>(n, 1));
        if (n) HIPCHK(hipMemcpyAsync(buf.p, p, n * sizeof *p, hipMemcpyHostToDevice, s));
    };
    upload(d_refs, a.refs, G), upload(d_off, a.ref_off, (size_t)a.n_refs + 1);
    if (n_adm) upload(d_query, a.query, a.query_bytes), upload(d_alns, a.alns, a.n_alns), upload(d_cigar, a.cigar, a.n_cigar_words), upload(d_adm, adm_idx.data(), n_adm);
    d_cov.ensure((size_t)G + 1), d_ones.ensure(G), d_runs.ensure(max_runs), d_ctr.ensure(1), d_dctr.ensure(3);
    if (n_adm) d_cnt.ensure(n_adm);
    // every array a kernel adds into is cleared on the stream; the others are written before they are read
    HIPCHK(hipMemsetAsync(d_cov.p, 0, ((size_t)G + 1) * 4, s));
    HIPCHK(hipMemsetAsync(d_ctr.p, 0, sizeof(np2::AsmDev), s));
    HIPCHK(hipMemsetAsync(d_dctr.p, 0, 3 * sizeof(np2::DepthDev), s));
    std::deque<KernelTimer> t; // HIP events around every stage
    for (int k = 0; k < 9; ++k) t.emplace_back(true);
    enum { T_COUNT, T_COV, T_ONES, T_OFFS, T_EMIT, T_RUNS, T_FILTER, T_SORT, T_GATHER };
    std::vector<KernelTimer *> pending; // stopped, to be collected at the next synchronisation
    auto timed = [&](int which, auto &&launch) {
        t[which].start(s);
        launch();
        t[which].stop(s);
        pending.push_back(&t[which]);
    };
    np2::AsmDev h;
    np2::DepthDev dh[3];
    auto read_ctr = [&] {
        HIPCHK(hipMemcpyAsync(&h, d_ctr.p, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(dh, d_dctr.p, sizeof dh, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (KernelTimer *x : pending) x->collect();
        pending.clear();
        if ((h.err | dh[0].err | dh[1].err | dh[2].err) & np2::LB_ERR) throw Np2Error(NP2_E_DEVICE, "np2_asmcall: a look-back wait gave up");
        if (h.err || dh[0].err || dh[1].err || dh[2].err) throw Np2Error(NP2_E_DEVICE, "np2_asmcall: counters out of range");
    };
    // a look-back descriptor is taken right before its launch: the tickets follow the order of the launches
    auto lookback = [&](uint32_t n, uint32_t *err) {
        Lookback lb = next_lookback(cx, np2::depth_blocks(n));
        lb.err = err;
        return lb;
    };
    try {
        uint32_t n_ev = 0, ones_last = 0;
        timed(T_COUNT, [&] { np2::launch_asmcall_walk(s, d_alns.p, d_adm.p, n_adm, d_cigar.p, d_query.p, d_refs.p, d_off.p, G, d_cov.p, d_cnt.p, nullptr, nullptr, 0, d_ctr.p); });
        timed(T_COV, [&] { np2::launch_depth_scan(s, lookback(G, &d_dctr.p[0].err), d_cov.p, G, 2, &d_dctr.p[0]); }); // (bases_ok: cov >= 2)
        timed(T_ONES, [&] {
            np2::launch_asmcall_ones(s, d_cov.p, G, d_ones.p);
            np2::launch_depth_scan(s, lookback(G, &d_dctr.p[1].err), d_ones.p, G, 1, &d_dctr.p[1]);
        });
        if (n_adm) timed(T_OFFS, [&] { np2::launch_depth_scan(s, lookback(n_adm, &d_dctr.p[2].err), d_cnt.p, n_adm, 1, &d_dctr.p[2]); });
        timed(T_RUNS, [&] { np2::launch_asmcall_runs(s, lookback(G, &d_ctr.p->err), d_cov.p, G, d_off.p, a.n_refs, d_runs.p, max_runs, d_ctr.p); });
        HIPCHK(hipGetLastError());
        if (n_adm) HIPCHK(hipMemcpyAsync(&n_ev, d_cnt.p + (n_adm - 1), 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&ones_last, d_ones.p + (G - 1), 4, hipMemcpyDeviceToHost, s));
        read_ctr();
        if (h.n_runs > max_runs || (uint64_t)n_ev > a.query_bytes + a.n_cigar_words) throw Np2Error(NP2_E_DEVICE, "np2_asmcall: counters out of range");
        st.runs = h.n_runs, st.r_bases = ones_last, st.cov2_bases = dh[0].bases_ok, st.cov0_bases = (uint64_t)G - ones_last - dh[0].bases_ok;
        uint32_t n_kept = 0;
        if (n_ev) {
            d_keys.ensure(n_ev), d_raw.ensure(n_ev), d_kkeys.ensure(n_ev), d_kidx.ensure(n_ev);
            timed(T_EMIT, [&] { np2::launch_asmcall_walk(s, d_alns.p, d_adm.p, n_adm, d_cigar.p, d_query.p, d_refs.p, d_off.p, G, d_cov.p, d_cnt.p, d_keys.p, d_raw.p, n_ev, d_ctr.p); });
            timed(T_FILTER, [&] { np2::launch_asmcall_filter(s, lookback(n_ev, &d_ctr.p->err), d_keys.p, d_raw.p, n_ev, d_cov.p, d_ones.p, d_off.p, d_kkeys.p, d_kidx.p, d_ctr.p); });
            HIPCHK(hipGetLastError());
            read_ctr();
            n_kept = h.n_kept;
            if (n_kept > n_ev) throw Np2Error(NP2_E_DEVICE, "np2_asmcall: counters out of range");
        }
        if (h.n_runs) {
            *a.runs = (np2_asmrun_t *)pinned_pool().get((size_t)h.n_runs * sizeof(np2_asmrun_t));
            if (!*a.runs) throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
            HIPCHK(hipMemcpyAsync(*a.runs, d_runs.p, (size_t)h.n_runs * sizeof(np2_asmrun_t), hipMemcpyDeviceToHost, s));
        }
        if (n_kept) {
            *a.vars = (np2_asmvar_t *)pinned_pool().get((size_t)n_kept * sizeof(np2_asmvar_t));
            if (!*a.vars) throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
            d_skeys.ensure(n_kept), d_sidx.ensure(n_kept), d_vars.ensure(n_kept);
            const size_t tmp_bytes = np2::prim_pairs64_temp_bytes(n_kept);
            d_tmp.ensure(tmp_bytes);
            timed(T_SORT, [&] { // stable: equal keys keep the order of (alignment, CIGAR)
                if (np2::prim_sort_pairs_u64_u64(s, d_tmp.p, tmp_bytes, d_kkeys.p, d_skeys.p, d_kidx.p, d_sidx.p, n_kept, np2ac::KEY_BITS))
                    throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
            });
            timed(T_GATHER, [&] { np2::launch_asmcall_gather(s, d_raw.p, d_sidx.p, n_kept, d_vars.p); });
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(*a.vars, d_vars.p, (size_t)n_kept * sizeof(np2_asmvar_t), hipMemcpyDeviceToHost, s));
        }
        if (cov) HIPCHK(hipMemcpyAsync(cov, d_cov.p, (size_t)G * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (KernelTimer *x : pending) x->collect();
        *a.n_runs = h.n_runs, *a.n_vars = n_kept;
    } catch (...) { // (an error returns no array; a ticket may have been issued for a launch that did not run)
        cx->lb_dirty = true;
        (void)hipStreamSynchronize(s);
        if (*a.runs) pinned_pool().put(*a.runs);
        if (*a.vars) pinned_pool().put(*a.vars);
        *a.runs = nullptr, *a.vars = nullptr;
        throw;
    }
    for (int k = 0; k < 3; ++k) st.found[k] = h.found[k], st.kept[k] = h.kept[k];
    st.ins_bases = h.ins_bases, st.del_bases = h.del_bases;
    for (int k = 0; k < 9; ++k) st.stage_ms[k] = t[k].ms, st.kernel_ms += t[k].ms;
    if (stats) *stats = st;
}

template <class T> T *copy_out(const std::vector<T> &v) {
    if (v.empty()) return nullptr;
    T *p = (T *)malloc(v.size() * sizeof(T)); // (np2_free frees what is not the pool's)
    if (!p) throw Np2Error(NP2_E_NOMEM, "out of memory for the results");
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

} // namespace

} // namespace np2h

extern "C" {

int np2_asmcall(np2_ctx_t *cx, const uint8_t *refs, const uint64_t *ref_off, uint32_t n_refs, const uint8_t *query, uint64_t query_bytes,
                const np2_asmaln_t *alns, uint32_t n_alns, const uint32_t *cigar, uint64_t n_cigar_words, const np2_asmcall_opts_t *opts,
                np2_asmrun_t **runs, uint32_t *n_runs, np2_asmvar_t **vars, uint32_t *n_vars, uint32_t *cov, np2_asmcall_stats_t *stats) {
    if (!cx) return NP2_E_ARG;
    if (runs) *runs = nullptr;
    if (vars) *vars = nullptr;
    if (n_runs) *n_runs = 0;
    if (n_vars) *n_vars = 0;
    return np2h::abi_guard([&] {
        using namespace np2h;
        const AsmArgs a{refs, ref_off, n_refs, query, query_bytes, alns, n_alns, cigar, n_cigar_words, opts, runs, n_runs, vars, n_vars};
        const std::vector<uint8_t> adm = asmcall_check(a, "np2_asmcall"); // every argument is checked before anything is launched
        HIPCHK(hipSetDevice(cx->device));
        asmcall_device(cx, a, adm, cov, stats);
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}

int np2_asmcall_host(const uint8_t *refs, const uint64_t *ref_off, uint32_t n_refs, const uint8_t *query, uint64_t query_bytes,
                     const np2_asmaln_t *alns, uint32_t n_alns, const uint32_t *cigar, uint64_t n_cigar_words, const np2_asmcall_opts_t *opts,
                     np2_asmrun_t **runs, uint32_t *n_runs, np2_asmvar_t **vars, uint32_t *n_vars, uint32_t *cov, np2_asmcall_stats_t *stats) {
    if (runs) *runs = nullptr;
    if (vars) *vars = nullptr;
    if (n_runs) *n_runs = 0;
    if (n_vars) *n_vars = 0;
    return np2h::abi_guard([&] {
        using namespace np2h;
        const AsmArgs a{refs, ref_off, n_refs, query, query_bytes, alns, n_alns, cigar, n_cigar_words, opts, runs, n_runs, vars, n_vars};
        const std::vector<uint8_t> adm = asmcall_check(a, "np2_asmcall_host");
        np2ac::Result r;
        np2ac::call_all(refs, ref_off, n_refs, query, alns, n_alns, cigar, adm, r);
        *runs = copy_out(r.runs);
        try {
            *vars = copy_out(r.vars);
        } catch (...) {
            free(*runs), *runs = nullptr;
            throw;
        }
        *n_runs = (uint32_t)r.runs.size(), *n_vars = (uint32_t)r.vars.size();
        if (cov && !r.cov.empty()) memcpy(cov, r.cov.data(), r.cov.size() * 4);
        if (stats) *stats = r.stats;
        return NP2_OK;
    }, [](int code, const std::string &msg) { np2h::io_set_error(code, msg); });
}

} // extern "C"
