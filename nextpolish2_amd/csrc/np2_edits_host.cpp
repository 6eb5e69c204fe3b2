// Host driver of the edit kernels (np2_edits.hip): edits_device runs heads -> flags -> runs -> trim -> shift -> emit ->
// support over a contig, its polished bases and their positions that are on the device already, and brings back the
// counters first and then exactly what they size.  np2_edits_buffers uploads host buffers first; np2_edits_last takes the
// consensus the last polish of the context left in HBM and unpacks the contig's codes next to it.
#include "np2_ctx.hpp"
#include "np2_edits.hpp"
#include "np2_kernel_timer.hpp"

namespace {

using np2::EditsDev;

struct Tables {
    np2::EditsTables dev{};
    uint32_t idx[NP2_EDITS_MAX_TABLES] = {0}, k[NP2_EDITS_MAX_TABLES] = {0};
};

Tables pick_tables(np2_ctx *cx, const np2_edits_opts_t *o, const char *who) {
    Tables t;
    const uint32_t have = (uint32_t)cx->yaks.size();
    const int32_t want = o ? o->tables : -1;
    t.dev.min_count = o ? o->min_count : 1;
    for (uint32_t i = 0; i < 32; ++i) {
        const bool on = want == -1 ? i < have : (((uint32_t)want >> i) & 1u) != 0;
        if (!on) continue;
        if (i >= have)
            throw Np2Error(NP2_E_ARG, std::string(who) + ": table " + std::to_string(i) + " asked for, the context has " + std::to_string(have));
        if (t.dev.n == NP2_EDITS_MAX_TABLES) throw Np2Error(NP2_E_UNSUPPORTED, std::string(who) + ": more than 8 tables");
        t.idx[t.dev.n] = i;
        t.dev.y[t.dev.n] = cx->yaks[i].dev();
        t.k[t.dev.n] = t.dev.y[t.dev.n].k;
        ++t.dev.n;
    }
    return t;
}

template <class T> T *host_block(size_t n) { // (np2_edits_free: free)
    T *p = (T *)calloc(n ? n : 1, sizeof(T));
    if (!p) throw Np2Error(NP2_E_NOMEM, "np2_edits: host result allocation failed");
    return p;
}

void edits_release(np2_edits_t *o) {
    free(o->edits), free(o->ref_off), free(o->alt_off), free(o->ref_pool), free(o->alt_pool), free(o->support);
    o->edits = nullptr, o->ref_off = o->alt_off = nullptr, o->ref_pool = o->alt_pool = nullptr, o->support = nullptr;
}

// ref[L], bases[n], pos[n] on the device; `who` names the entry point in messages
void edits_device(np2_ctx *cx, const uint8_t *d_ref, uint32_t L, const uint8_t *d_base, const uint32_t *d_pos, uint32_t n, const Tables &tb,
                  np2_edits_t *out, const char *who) {
    hipStream_t s = cx->stream;
    const uint32_t max_runs = (uint32_t)(((uint64_t)L + 1) / 2) + 1, n_words = (uint32_t)(((uint64_t)L + 31) / 32);
    const uint32_t blocks = grid_blocks(cx->device, 4); // what the device holds at once, wavefronts striding over their jobs
    DevBuf<uint32_t> gse, bits, offs, runs, list, scans, sup;
    DevBuf<np2edits::Edit> rec;
    DevBuf<uint8_t> pools;
    DevBuf<EditsDev> ctr;
    gse.cached = bits.cached = offs.cached = runs.cached = list.cached = scans.cached = sup.cached = rec.cached = pools.cached = ctr.cached = true;
    const size_t rs = ((size_t)max_runs + 8) & ~(size_t)3, ws = ((size_t)n_words + 8) & ~(size_t)3; // strides: 16-byte aligned pieces
    gse.ensure(2 * (size_t)L + 4);
    bits.ensure(2 * ws);
    offs.ensure(2 * ws);
    runs.ensure(8 * rs);
    list.ensure(5 * rs);
    scans.ensure(3 * rs);
    rec.ensure(max_runs);
    sup.ensure((size_t)max_runs * std::max(1u, tb.dev.n) * 4 + 4);
    const size_t pool_r = ((size_t)L + 15) & ~(size_t)15;
    pools.ensure(pool_r + n + 16);
    ctr.ensure(1);
    np2::EditsSeq q{d_ref, d_base, d_pos, L, n, gse.p, gse.p + L};
    np2::EditsRuns r{max_runs, runs.p, runs.p + rs, runs.p + 2 * rs, runs.p + 3 * rs, runs.p + 4 * rs, runs.p + 5 * rs, runs.p + 6 * rs, runs.p + 7 * rs};
    np2::EditsList e{list.p, list.p + rs, list.p + 2 * rs, list.p + 3 * rs, list.p + 4 * rs, rec.p};
    uint32_t *hbits = bits.p, *tbits = bits.p + ws, *hoff = offs.p, *toff = offs.p + ws;
    uint32_t *eidx = scans.p, *roff = scans.p + rs, *aoff = scans.p + 2 * rs;
    uint8_t *ref_pool = pools.p, *alt_pool = pools.p + pool_r;

    HIPCHK(hipMemsetAsync(ctr.p, 0, sizeof(EditsDev), s));
    if (L) {
        HIPCHK(hipMemsetAsync(q.gstart, 0xFF, (size_t)L * 4, s));
        HIPCHK(hipMemsetAsync(q.gend, 0, (size_t)L * 4, s));
    }
    HIPCHK(hipMemsetAsync(e.lr, 0, 2 * rs * 4, s)); // (lr and la: the size scans run over max_runs entries)
    // (descriptors first: the first one of a context fills its status words on the stream)
    Lookback lb[5];
    lb[0] = next_lookback(cx, np2::scan_lb_blocks((size_t)n_words + 1));
    lb[1] = next_lookback(cx, np2::scan_lb_blocks((size_t)n_words + 1));
    for (int i = 2; i < 5; ++i) lb[i] = next_lookback(cx, np2::scan_lb_blocks(max_runs));
    for (auto &l : lb) l.err = &ctr.p->err;
    std::vector<std::unique_ptr<KernelTimer>> tm;
    for (int i = 0; i < NP2_EDITS_STAGES; ++i) tm.emplace_back(new KernelTimer(true));
    try {
        tm[0]->start(s);
        np2::launch_edits_heads(s, q, ctr.p);
        np2::launch_edits_flags(s, q, ctr.p, hbits, tbits, n_words);
        tm[0]->stop(s);
        tm[1]->start(s);
        np2::launch_scan_lb_popc(s, lb[0], hbits, hoff, n_words, &ctr.p->err);
        np2::launch_scan_lb_popc(s, lb[1], tbits, toff, n_words, &ctr.p->err);
        np2::launch_edits_runs(s, hbits, tbits, hoff, toff, n_words, r, ctr.p);
        tm[1]->stop(s);
        tm[2]->start(s);
        np2::launch_edits_trim(s, q, r, ctr.p, blocks);
        np2::launch_scan_lb_excl(s, lb[2], r.real, eidx, max_runs, true, &ctr.p->err);
        tm[2]->stop(s);
        tm[3]->start(s);
        np2::launch_edits_compact(s, r, eidx, e, ctr.p);
        np2::launch_edits_shift(s, q, e, max_runs, ctr.p);
        tm[3]->stop(s);
        tm[4]->start(s);
        np2::launch_scan_lb_excl(s, lb[3], e.lr, roff, max_runs, true, &ctr.p->err);
        np2::launch_scan_lb_excl(s, lb[4], e.la, aoff, max_runs, true, &ctr.p->err);
        np2::launch_edits_emit(s, q, e, roff, aoff, max_runs, ref_pool, alt_pool, ctr.p, blocks);
        tm[4]->stop(s);
        tm[5]->start(s);
        np2::launch_edits_support(s, q, e, tb.dev, sup.p, max_runs, ctr.p, blocks);
        tm[5]->stop(s);
        HIPCHK(hipGetLastError());
    } catch (...) { // (tickets were issued for launches that may not have run: the next descriptor starts over)
        cx->lb_dirty = true;
        throw;
    }
    EditsDev h;
    HIPCHK(hipMemcpyAsync(&h, ctr.p, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < NP2_EDITS_STAGES; ++i) {
        tm[i]->collect();
        out->kernel_ms[i] = tm[i]->ms;
    }
    if (h.err & np2edits::E_POS_RANGE) throw Np2Error(NP2_E_ARG, std::string(who) + ": a position is not below the contig's length");
    if (h.err & np2edits::E_POS_ORDER) throw Np2Error(NP2_E_ARG, std::string(who) + ": the positions decrease somewhere");
    if (h.err & np2::LB_ERR) throw Np2Error(NP2_E_DEVICE, std::string(who) + ": a look-back wait gave up");
    if (h.err) throw Np2Error(NP2_E_DEVICE, std::string(who) + ": internal: a run outside its arrays");
    if (h.n_edits > h.n_raw || h.n_raw > max_runs || h.ref_bytes > L || h.alt_bytes > n)
        throw Np2Error(NP2_E_DEVICE, std::string(who) + ": counters out of range");

    const uint32_t ne = h.n_edits, nt = tb.dev.n;
    out->edits = host_block<np2_edit_t>(ne);
    out->ref_off = host_block<uint32_t>((size_t)ne + 1);
    out->alt_off = host_block<uint32_t>((size_t)ne + 1);
    out->ref_pool = host_block<uint8_t>(h.ref_bytes);
    out->alt_pool = host_block<uint8_t>(h.alt_bytes);
    out->support = host_block<np2_edit_support_t>((size_t)ne * nt);
    static_assert(sizeof(np2_edit_t) == sizeof(np2edits::Edit) && sizeof(np2_edit_support_t) == 16, "record layouts");
    if (ne) {
        HIPCHK(hipMemcpyAsync(out->edits, rec.p, (size_t)ne * sizeof(np2_edit_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->ref_off, roff, ((size_t)ne + 1) * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->alt_off, aoff, ((size_t)ne + 1) * 4, hipMemcpyDeviceToHost, s));
        if (h.ref_bytes) HIPCHK(hipMemcpyAsync(out->ref_pool, ref_pool, h.ref_bytes, hipMemcpyDeviceToHost, s));
        if (h.alt_bytes) HIPCHK(hipMemcpyAsync(out->alt_pool, alt_pool, h.alt_bytes, hipMemcpyDeviceToHost, s));
        if (nt) HIPCHK(hipMemcpyAsync(out->support, sup.p, (size_t)ne * nt * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    out->n_edits = ne;
    out->n_tables = nt;
    for (uint32_t i = 0; i < nt; ++i) out->table_idx[i] = tb.idx[i], out->table_k[i] = tb.k[i];
    out->has_span = h.has_span, out->first_pos = h.first, out->last_pos = h.last;
    out->raw_runs = h.n_raw, out->same_runs = h.same_runs;
    for (int i = 0; i < 5; ++i) out->n_kind[i] = h.n_kind[i];
    out->bases_inserted = h.bases_inserted, out->bases_deleted = h.bases_deleted, out->outside_span = h.outside;
}

} // namespace

extern "C" {

int np2_edits_buffers(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const uint8_t *bases, const uint32_t *pos, uint64_t n,
                      const np2_edits_opts_t *opts, np2_edits_t *out) {
    if (!cx) return NP2_E_ARG;
    if (out) memset(out, 0, sizeof *out);
    return abi_guard([&] {
        // every argument is checked before anything is launched (the positions themselves: on the device)
        if (!out) throw Np2Error(NP2_E_ARG, "np2_edits_buffers: out is NULL");
        if (L && !ref) throw Np2Error(NP2_E_ARG, "np2_edits_buffers: ref is NULL with L > 0");
        if (n && (!bases || !pos)) throw Np2Error(NP2_E_ARG, "np2_edits_buffers: bases or pos is NULL with n > 0");
        if (n >= 0xFFFF0000ull) throw Np2Error(NP2_E_UNSUPPORTED, "np2_edits_buffers: 2^32 - 65536 output bases or more");
        const Tables tb = pick_tables(cx, opts, "np2_edits_buffers");
        HIPCHK(hipSetDevice(cx->device));
        DevBuf<uint8_t> d_ref, d_base;
        DevBuf<uint32_t> d_pos;
        d_ref.cached = d_base.cached = d_pos.cached = true; // (released after edits_device has drained the stream)
        if (L) {
            d_ref.ensure(L);
            HIPCHK(hipMemcpyAsync(d_ref.p, ref, L, hipMemcpyHostToDevice, cx->stream));
        }
        if (n) {
            d_base.ensure(n), d_pos.ensure(n);
            HIPCHK(hipMemcpyAsync(d_base.p, bases, n, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemcpyAsync(d_pos.p, pos, n * 4, hipMemcpyHostToDevice, cx->stream));
        }
        try {
            edits_device(cx, d_ref.p, L, d_base.p, d_pos.p, (uint32_t)n, tb, out, "np2_edits_buffers");
        } catch (...) {
            edits_release(out);
            throw;
        }
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_edits_last(np2_ctx_t *cx, np2_contig_t *c, const np2_edits_opts_t *opts, np2_edits_t *out) {
    if (!cx) return NP2_E_ARG;
    if (out) memset(out, 0, sizeof *out);
    return abi_guard([&] {
        if (!out) throw Np2Error(NP2_E_ARG, "np2_edits_last: out is NULL");
        if (!c) throw Np2Error(NP2_E_ARG, "np2_edits_last: contig is NULL");
        if (!cx->last_dbase || !cx->last_dpos)
            throw Np2Error(NP2_E_ARG, "np2_edits_last: no polished sequence on this context (call np2_polish_resident first)");
        if (cx->last_len >= 0xFFFF0000ull) throw Np2Error(NP2_E_UNSUPPORTED, "np2_edits_last: 2^32 - 65536 output bases or more");
        const Tables tb = pick_tables(cx, opts, "np2_edits_last");
        HIPCHK(hipSetDevice(cx->device));
        DevBuf<uint8_t> d_ref;
        d_ref.cached = true;
        d_ref.ensure(c->L);
        np2::launch_edits_unpack_ref(cx->stream, c->refnib.p, c->L, d_ref.p);
        try {
            edits_device(cx, d_ref.p, c->L, cx->last_dbase, cx->last_dpos, (uint32_t)cx->last_len, tb, out, "np2_edits_last");
        } catch (...) {
            edits_release(out);
            throw;
        }
        return NP2_OK;
    }, ctx_sink(cx));
}

void np2_edits_free(np2_edits_t *out) {
    if (out) edits_release(out);
}

} // extern "C"
