// Life cycle of the np2 contexts and contigs and the small entry points around them: C ABI (include/np2.h) of np2_ctx_*,
// np2_contig_*, the pinned pool, the test hooks, traces and timings, string scoring and table lookups.  No CPU fallback:
// every entry point needs a HIP device.
#include "np2_ctx.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace np2;

namespace np2 {
Recorder *&tl_recorder() {
    static thread_local Recorder *r = nullptr;
    return r;
}
} // namespace np2

namespace {

void gpu_score_strings(np2_ctx *cx, int yak_idx, const std::vector<uint8_t> &blob, const std::vector<uint64_t> &off,
                       uint16_t min_kmer_count, std::vector<uint16_t> &scores) {
    const size_t n = off.size() - 1;
    scores.assign(n, 0);
    if (!n) return;
    cx->sstr.ensure(blob.size() + 16);
    cx->soff.ensure(off.size());
    cx->sscore.ensure(n);
    {
        op_sync(cx);
        uint8_t *pin = (uint8_t *)cx->pin_h2d.ensure(blob.size() + off.size() * 8 + 16);
        const size_t o2 = (blob.size() + 7) & ~(size_t)7;
        memcpy(pin, blob.data(), blob.size());
        memcpy(pin + o2, off.data(), off.size() * 8);
        op_h2d(cx, cx->sstr.p, pin, blob.size());
        op_h2d(cx, cx->soff.p, pin + o2, off.size() * 8);
        cx->h2d_inflight = true;
    }
    {
        EventTimer t(cx, "score_strings");
        launch_score_strings(cx->stream, cx->yaks[yak_idx].dev(), cx->sstr.p, cx->soff.p, n, min_kmer_count,
                             cx->sscore.p, false);
    }
    scores = d2h(cx, cx->sscore.p, n);
}

} // namespace

namespace np2h {
void finish_contig(np2_ctx *cx, np2_contig *c, const np2_read_t *reads, uint32_t n_reads, uint32_t L,
                   uint64_t nib_bytes) {
    if (reads[0].aln_t_s != 0 || reads[0].n_cols != L || reads[0].aln_t_e != L - 1 ||
        (reads[0].flags & NP2_READ_DROPPED))
        throw Np2Error(NP2_E_ARG, "reads[0] must be the contig aligned to itself (main.rs:1732-1739)");
    // what goes to the device is built in pinned blocks of the process-wide pool (pageable sources are staged by the
    // runtime at a fraction of the bus rate, synchronously: 4 MB of descriptors per E. coli-sized contig)
    struct PinnedTmp {
        void *p = nullptr;
        explicit PinnedTmp(size_t bytes) : p(pinned_pool().get(std::max<size_t>(bytes, 64))) {
            if (!p) throw Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
        }
        ~PinnedTmp() {
            if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize(); // (an upload out of it may still be in flight)
            pinned_pool().put(p);
        }
    };
    uint64_t total_chunks = 0;
    for (uint32_t r = 1; r < n_reads; ++r)
        if (!(reads[r].flags & NP2_READ_DROPPED)) total_chunks += ((uint64_t)reads[r].n_cols + DENSE_COLS - 1) / DENSE_COLS;
    if (total_chunks >= 0xFFFFFFF0ull) throw Np2Error(NP2_E_NOMEM, "too many pileup columns for one contig");
    PinnedTmp ck_pin((size_t)(n_reads + 1) * 8), descs_pin((size_t)(total_chunks + 1) * sizeof(ChunkDesc));
    uint64_t *ck = (uint64_t *)ck_pin.p;
    ChunkDesc *descs = (ChunkDesc *)descs_pin.p;
    uint32_t n_descs = 0;
    ck[0] = 0;
    uint64_t cols = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const np2_read_t &rd = reads[r];
        const bool dropped = rd.flags & NP2_READ_DROPPED;
        if (rd.nib_off & 15) throw Np2Error(NP2_E_ARG, "nib_off must be a multiple of 16");
        if (rd.nib_off >> 36) throw Np2Error(NP2_E_NOMEM, "a contig's nibble streams must stay below 64 GiB");
        if (!dropped && (rd.aln_t_e >= L || rd.aln_t_s > rd.aln_t_e))
            throw Np2Error(NP2_E_ARG, "read span outside the contig");
        if (rd.nib_off + ((uint64_t)(rd.n_cols + 1) >> 1) + 1 + 16 > nib_bytes)
            throw Np2Error(NP2_E_ARG, "nibble stream (plus 16 B tail padding) exceeds the buffer");
        uint32_t nck = 0, nch = 0;
        if (!dropped) {
            const uint32_t first = (rd.aln_t_s + CKPT - 1) >> CKPT_SHIFT, last = rd.aln_t_e >> CKPT_SHIFT;
            nck = last >= first ? last - first + 1 : 0;
            if (r != 0) nch = (uint32_t)(((uint64_t)rd.n_cols + DENSE_COLS - 1) / DENSE_COLS);
            cols += rd.n_cols;
        }
        ck[r + 1] = ck[r] + nck;
        const uint32_t first_chunk = n_descs;
        for (uint32_t k = 0; k < nch; ++k) {
            ChunkDesc &d = descs[n_descs++];
            memset(&d, 0, sizeof d);
            d.nib_off = rd.nib_off;
            d.ckbase = ck[r];
            d.read = r;
            d.ts = rd.aln_t_s;
            d.c0 = k * DENSE_COLS;
            d.ncols = rd.n_cols;
            d.first_chunk = first_chunk;
            d.aln_t_e = rd.aln_t_e;
            d.nck = nck;
        }
    }
    // reads overlapping each contig tile, ascending read index (candidate extraction looks reads up by position)
    const uint32_t n_tiles = (L + TILE - 1) >> TILE_SHIFT;
    PinnedTmp trd_off_pin(((size_t)n_tiles + 1) * 4);
    uint32_t *trd_off = (uint32_t *)trd_off_pin.p;
    memset(trd_off, 0, ((size_t)n_tiles + 1) * 4);
    for (uint32_t r = 0; r < n_reads; ++r)
        if (!(reads[r].flags & NP2_READ_DROPPED))
            for (uint32_t t = reads[r].aln_t_s >> TILE_SHIFT; t <= reads[r].aln_t_e >> TILE_SHIFT; ++t) ++trd_off[t + 1];
    for (uint32_t t = 0; t < n_tiles; ++t) trd_off[t + 1] += trd_off[t];
    const size_t n_trd = trd_off[n_tiles];
    PinnedTmp trd_pin((n_trd + 1) * 4);
    uint32_t *trd = (uint32_t *)trd_pin.p;
    {
        std::vector<uint32_t> cur(trd_off, trd_off + n_tiles);
        for (uint32_t r = 0; r < n_reads; ++r)
            if (!(reads[r].flags & NP2_READ_DROPPED))
                for (uint32_t t = reads[r].aln_t_s >> TILE_SHIFT; t <= reads[r].aln_t_e >> TILE_SHIFT; ++t) trd[cur[t]++] = r;
    }
    {
        uint32_t deepest = 0;
        for (uint32_t t = 0; t < n_tiles; ++t) deepest = std::max(deepest, trd_off[t + 1] - trd_off[t]);
        const uint64_t want = ((uint64_t)deepest * TILE / 24 + 255) & ~255ull; // ~4 % of the tile's columns
        c->tile_cap = (uint32_t)std::min<uint64_t>(TILE_CAP, std::max<uint64_t>(1024, want));
    }
    hipStream_t s = cx->stream;
    c->L = L;
    c->R = n_reads;
    c->n_tiles = n_tiles;
    c->tile_rd_off.ensure((size_t)n_tiles + 1);
    c->tile_rd.ensure(n_trd + 1);
    HIPCHK(hipMemcpyAsync(c->tile_rd_off.p, trd_off, ((size_t)n_tiles + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_trd) HIPCHK(hipMemcpyAsync(c->tile_rd.p, trd, n_trd * 4, hipMemcpyHostToDevice, s));
    c->nib_bytes = nib_bytes;
    c->n_cols = cols;
    c->n_ckpt = ck[n_reads];
    if (c->n_ckpt >> 32) throw Np2Error(NP2_E_NOMEM, "too many pileup columns for one contig (checkpoint offsets are 32-bit)");
    c->n_chunks = n_descs;
    c->reads.ensure(n_reads);
    const uint32_t refbytes = ((L + 1) >> 1) + 96; // padding so that 128-bit probes near the end stay in bounds
    c->ref_stride = (refbytes + 15) & ~15u; // (the dense pass's two copies follow the codes: launch_encode_ref)
    c->refnib.ensure(3 * (size_t)c->ref_stride);
    c->ck_off.ensure(n_reads + 1);
    c->ckpt.ensure(c->n_ckpt + 1);
    c->descs.ensure(c->n_chunks + 1);
    HIPCHK(hipMemcpyAsync(c->reads.p, reads, (size_t)n_reads * sizeof(np2_read_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->ck_off.p, ck, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    if (c->n_chunks)
        HIPCHK(hipMemcpyAsync(c->descs.p, descs, (size_t)c->n_chunks * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    cx->scal.ensure(SCAL_TOTAL);
    zero32(cx, cx->scal.p, 24);
    launch_encode_ref(s, c->nib.p + reads[0].nib_off, L, c->refnib.p, refbytes, c->ref_stride, cx->scal.p);
    auto sc = d2h(cx, cx->scal.p, 1); // also syncs: the pinned staging blocks above go back to the pool
    if (sc[0]) throw Np2Error(NP2_E_ARG, "reads[0] is not a plain self-alignment of the contig");
}
} // namespace np2h

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

// the context's streams, events and mailbox go back to the pool (synchronised), its result staging to the pinned pool
static void destroy_streams(np2_ctx *cx) {
    for (int i = 0; i < 2; ++i) {
        if (cx->out_host[i]) pinned_pool().put(cx->out_host[i]);
        cx->out_host[i] = nullptr;
        cx->out_host_cap[i] = 0;
    }
    if (cx->borrowed_state) { // (streams and mailbox are the batch driver's)
        if (cx->ev_out) (void)hipEventDestroy(cx->ev_out);
        cx->stream = cx->stream_out = nullptr;
        cx->ev_out = nullptr;
        cx->mbox_host = cx->mbox_dev = nullptr;
        return;
    }
    CtxDeviceState st;
    st.stream = cx->stream, st.stream_out = cx->stream_out;
    st.ev_out = cx->ev_out;
    st.mbox_host = cx->mbox_host, st.mbox_dev = cx->mbox_dev;
    cx->stream = cx->stream_out = nullptr;
    cx->ev_out = nullptr;
    cx->mbox_host = cx->mbox_dev = nullptr;
    const bool complete = st.stream && st.stream_out && st.ev_out && st.mbox_host;
    bool idle = complete;
    if (complete) // (nothing of this context may still be running on a set the next context takes over)
        idle = hipStreamSynchronize(st.stream) == hipSuccess && hipStreamSynchronize(st.stream_out) == hipSuccess;
    if (idle)
        ctx_state_pool().put(cx->device, st);
    else
        st.destroy();
}

// streams, events, mailbox: everything of a context but its k-mer tables
static void init_ctx_device(np2_ctx *cx, int device, hipStream_t borrow = nullptr, uint32_t *mbox_host = nullptr, uint32_t *mbox_dev = nullptr) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw Np2Error(NP2_E_DEVICE, "no HIP device available (the np2 hot path has no CPU fallback)");
    if (device < 0 || device >= ndev) throw Np2Error(NP2_E_ARG, "bad device index");
    cx->device = device;
    cx->hooks.read();
    HIPCHK(hipSetDevice(device));
    CtxDeviceState st;
    if (borrow) {
        cx->borrowed_state = true;
        cx->stream = cx->stream_out = borrow;
        cx->mbox_host = mbox_host, cx->mbox_dev = mbox_dev;
        HIPCHK(hipEventCreateWithFlags(&cx->ev_out, hipEventDisableTiming));
    } else if (ctx_state_pool().get(device, st)) {
        cx->stream = st.stream, cx->stream_out = st.stream_out;
        cx->ev_out = st.ev_out;
        cx->mbox_host = st.mbox_host, cx->mbox_dev = st.mbox_dev;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&cx->stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&cx->stream_out, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&cx->ev_out, hipEventDisableTiming));
        HIPCHK(hipHostMalloc((void **)&cx->mbox_host, 64 * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void **)&cx->mbox_dev, cx->mbox_host, 0));
    }
    cx->scal.ensure(SCAL_TOTAL);
    memset(cx->mbox_host, 0, 64 * sizeof(uint32_t));
    if (const char *e = getenv("NP2_TILE_CAP")) // test hook: smaller buckets force the spill / device-wide sort path
        cx->tile_cap = (uint32_t)std::min<long>(TILE_CAP, std::max<long>(1, atol(e)));
    if (const char *e = getenv("NP2_TEST_DEEP_COV")) // test hook: treat shallower pileups as too deep for the on-chip DP
        cx->deep_min = (uint32_t)std::min<long>(65536, std::max<long>(1, atol(e)));
}

// a context being made: released with its streams unless it is handed out
struct CtxDrop {
    void operator()(np2_ctx *cx) const {
        destroy_streams(cx);
        delete cx;
    }
};
using CtxPtr = std::unique_ptr<np2_ctx, CtxDrop>;

int np2_ctx_create(np2_ctx_t **out, int device, const np2_yak_t *yaks, int n_yak) {
    if (!out) return NP2_E_ARG;
    *out = nullptr;
    return abi_guard([&] {
        CtxPtr cx(new np2_ctx());
        const double t_c0 = now_ms();
        init_ctx_device(cx.get(), device);
        if (getenv("NP2_CTX_PROFILE")) fprintf(stderr, "np2_ctx_create: streams, events, mailbox %.2f ms\n", now_ms() - t_c0);
        // the final pass runs one splice round + one per yak table; their per-round device counters live in fixed slots
        if (n_yak < 0 || n_yak > NP2_MAX_YAK || (n_yak && !yaks))
            throw Np2Error(NP2_E_ARG, "n_yak must be in [0, 15]");
        cx->yaks.resize(n_yak);
        for (int i = 0; i < n_yak; ++i) {
            const np2_yak_t &y = yaks[i];
            if (y.k >= 32 || y.k < 2) throw Np2Error(NP2_E_UNSUPPORTED, "yak k must be in [2, 32) (main.rs:1433-1434)");
            if (y.pre != 10) throw Np2Error(NP2_E_UNSUPPORTED, "yak pre must be 10 (kmer.rs:52-54,123-125)");
            if (i && yaks[i - 1].k > y.k) throw Np2Error(NP2_E_ARG, "yak tables must be sorted by k (option.rs:238)");
            uint64_t mx = 0;
            for (uint32_t b = 0; b < 1024; ++b) mx = std::max(mx, y.bucket_off[b + 1] - y.bucket_off[b]);
            uint32_t cl = 4;
            while ((1ull << cl) < mx * 2 + 2) ++cl;
            YakTable &t = cx->yaks[i];
            t.k = y.k;
            t.cap_log2 = cl;
            const size_t slots = (size_t)1024 << cl;
            t.table = std::make_shared<DevBuf<uint64_t>>();
            t.table->ensure(slots);
            HIPCHK(hipMemsetAsync(t.table->p, 0xFF, slots * 8, cx->stream));
            HIPCHK(hipStreamSynchronize(cx->stream)); // large fill + pageable H2D below: do not rely on their ordering
            DevBuf<uint64_t> dw, doff;
            dw.ensure(y.n_words + 1);
            doff.ensure(1025);
            HIPCHK(hipMemcpyAsync(dw.p, y.words, y.n_words * 8, hipMemcpyHostToDevice, cx->stream));
            HIPCHK(hipMemcpyAsync(doff.p, y.bucket_off, 1025 * 8, hipMemcpyHostToDevice, cx->stream));
            zero32(cx.get(), cx->scal.p, S_COUNT);
            launch_yak_insert(cx->stream, dw.p, doff.p, 1024, mx, t.table->p, cl, cx->scal.p + S_DUP);
            auto sc = d2h(cx.get(), cx->scal.p, S_COUNT);
            if (sc[S_DUP]) { // a repeated key (yak writes none): a slot per word, the winner chosen at lookup (kmer.rs:148-167)
                t.ord = std::make_shared<DevBuf<uint32_t>>();
                t.ord->ensure(slots);
                HIPCHK(hipMemsetAsync(t.table->p, 0xFF, slots * 8, cx->stream));
                launch_yak_insert_dup(cx->stream, dw.p, doff.p, 1024, mx, t.table->p, cl, t.ord->p);
                HIPCHK(hipStreamSynchronize(cx->stream)); // (dw / doff are released at the end of this scope)
            }
        }
        *out = cx.release();
        return NP2_OK;
    }, [](int, const std::string &msg) { fprintf(stderr, "np2_ctx_create: %s\n", msg.c_str()); });
}

int np2_ctx_create_shared(np2_ctx_t **out, np2_ctx_t *parent) {
    if (!out || !parent) return NP2_E_ARG;
    *out = nullptr;
    return abi_guard([&] {
        CtxPtr cx(new np2_ctx());
        init_ctx_device(cx.get(), parent->device);
        cx->yaks = parent->yaks; // the HBM tables are reference-counted: freed with the last context using them
        cx->tile_cap = parent->tile_cap;
        *out = cx.release();
        return NP2_OK;
    }, [](int, const std::string &msg) { fprintf(stderr, "np2_ctx_create_shared: %s\n", msg.c_str()); });
}

} // extern "C"
// a batch driver's slot: the tables shared with `parent`, the stream and the mailbox the driver's (np2_batch.cpp)
np2_ctx *np2h::ctx_create_slot(np2_ctx *parent, hipStream_t s, uint32_t *mbox_host, uint32_t *mbox_dev) {
    CtxPtr cx(new np2_ctx());
    init_ctx_device(cx.get(), parent->device, s, mbox_host, mbox_dev);
    cx->yaks = parent->yaks;
    cx->tile_cap = parent->tile_cap;
    return cx.release();
}
void np2h::ctx_slot_set_stream(np2_ctx *cx, hipStream_t s) {
    if (cx->borrowed_state) cx->stream = cx->stream_out = s;
}
extern "C" {

void np2_ctx_destroy(np2_ctx_t *cx) {
    if (!cx) return;
    const bool prof = getenv("NP2_CTX_PROFILE") != nullptr;
    const double t0 = now_ms();
    (void)hipSetDevice(cx->device);
    if (cx->stream) (void)hipStreamSynchronize(cx->stream);
    if (cx->stream_out) (void)hipStreamSynchronize(cx->stream_out);
    const double t1 = now_ms();
    destroy_streams(cx);
    const double t2 = now_ms();
    {
        DevSyncScope idle; // the context's ~130 buffers go back to the slabs / the cache behind ONE device synchronisation
        delete cx;
    }
    if (prof)
        fprintf(stderr, "np2_ctx_destroy: stream syncs %.2f ms, streams/events/result staging %.2f ms, buffers %.2f ms\n", t1 - t0,
                t2 - t1, now_ms() - t2);
}
const char *np2_last_error(np2_ctx_t *cx) { return cx ? cx->err.c_str() : "null context"; }
void *np2_ctx_stream(np2_ctx_t *cx) { return cx ? (void *)cx->stream : nullptr; }
void np2_ctx_set_trace(np2_ctx_t *cx, int enable) {
    if (cx) cx->trace = enable != 0;
}
void np2_ctx_set_timing(np2_ctx_t *cx, int enable) {
    if (cx) cx->stage_timing = enable != 0;
}

int np2_contig_upload(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const np2_read_t *reads, uint32_t n_reads,
                      const uint8_t *nibbles, uint64_t nib_bytes, np2_contig_t **out) {
    if (!cx || !out) return NP2_E_ARG;
    *out = nullptr;
    std::unique_ptr<np2_contig> c; // (freed after the sink's sync: the nibble upload may still be in flight)
    return abi_guard([&] {
        (void)ref;
        HIPCHK(hipSetDevice(cx->device));
        if (L < 3 || n_reads < 1 || !reads || !nibbles) throw Np2Error(NP2_E_ARG, "bad contig arguments");
        c.reset(new np2_contig());
        c->nib.ensure(nib_bytes + 64);
        // (the caller's pageable buffer in one call: the runtime locks its pages and copies at the link's rate — 56 GB/s for
        // 32 MiB and more, tools/ubench_h2d.hip; a ring of pinned blocks filled by helper threads measured 38-51)
        HIPCHK(hipMemcpyAsync(c->nib.p, nibbles, nib_bytes, hipMemcpyHostToDevice, cx->stream));
        finish_contig(cx, c.get(), reads, n_reads, L, nib_bytes);
        *out = c.release();
        return NP2_OK;
    }, ctx_sink(cx));
}
void np2_contig_free(np2_ctx_t *cx, np2_contig_t *c) {
    if (cx) (void)hipSetDevice(cx->device);
    delete c;
}

void np2_free(void *p) {
    if (!p) return;
    if (!pinned_pool().put(p)) free(p);
}

int np2_score_strings(np2_ctx_t *cx, int yak_idx, const uint8_t *strs, const uint64_t *off, uint64_t n,
                      uint16_t min_kmer_count, uint16_t *scores) {
    if (!cx || yak_idx < 0 || (size_t)yak_idx >= cx->yaks.size()) return NP2_E_ARG;
    return abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        std::vector<uint8_t> blob(strs, strs + off[n]);
        blob.resize(blob.size() + 8, 0);
        std::vector<uint64_t> o(off, off + n + 1);
        std::vector<uint16_t> sc;
        gpu_score_strings(cx, yak_idx, blob, o, min_kmer_count, sc);
        memcpy(scores, sc.data(), n * 2);
        flush_timings(cx);
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_lookup_hashes(np2_ctx_t *cx, int yak_idx, const uint64_t *hashes, uint64_t n, uint16_t min_kmer_count,
                      uint16_t *counts) {
    if (!cx || yak_idx < 0 || (size_t)yak_idx >= cx->yaks.size()) return NP2_E_ARG;
    return abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        cx->soff.ensure(n + 1);
        cx->sscore.ensure(n + 1);
        HIPCHK(hipMemcpyAsync(cx->soff.p, hashes, n * 8, hipMemcpyHostToDevice, cx->stream));
        launch_lookup(cx->stream, cx->yaks[yak_idx].dev(), cx->soff.p, n, min_kmer_count, cx->sscore.p);
        HIPCHK(hipMemcpyAsync(counts, cx->sscore.p, n * 2, hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_trace_get(np2_ctx_t *cx, int pass, const char *name, const void **data, uint64_t *nbytes) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        auto it = cx->trace_items.find(std::to_string(pass) + ":" + name);
        if (it == cx->trace_items.end()) return NP2_E_ARG;
        *data = it->second.data();
        *nbytes = it->second.size();
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_last_timings(np2_ctx_t *cx, const char **names, const float **ms, int *n) {
    if (!cx) return NP2_E_ARG;
    *names = cx->timing.joined.c_str();
    *ms = cx->timing.ms.data();
    *n = (int)cx->timing.ms.size();
    return NP2_OK;
}

void *np2_alloc_pinned(uint64_t bytes) { return pinned_pool().get((size_t)bytes + 1); }
void np2_trim_device_cache(void) { dev_cache().trim(0); }

// test hook: the pools fill every block they hand out with this byte (np2_ctx.hpp: poison_device, poison_pinned)
int np2_debug_poison(int byte) { return poison().byte.exchange(byte < 0 ? -1 : (byte & 255), std::memory_order_relaxed); }
void np2_debug_poison_stats(uint64_t *device_bytes, uint64_t *pinned_bytes) {
    if (device_bytes) *device_bytes = poison().device_bytes.load(std::memory_order_relaxed);
    if (pinned_bytes) *pinned_bytes = poison().pinned_bytes.load(std::memory_order_relaxed);
}

} // extern "C"
