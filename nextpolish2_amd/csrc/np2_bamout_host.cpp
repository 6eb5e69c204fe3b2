// Host driver of the BAM writer (include/np2_io.h: np2_sam_write_bam, np2_sam_bam_stream, np2_bamout_host; kernels:
// np2_bamout.hip).
//
// np2_sam_write_bam: sizes and their scan on the context's stream, the refusals read back (nothing has been created yet), then
// the stream batch by batch on the BGZF writer's stream: the host-built header copied in by range, k_bam_emit for the records'
// part of the range, the writer's device-input door for the rest (CRCs, deflate, pack, one copy per batch).  Each block's
// compressed size stays on the device; after the last batch they are scanned into file offsets and the index kernels run.
// The runs of one (tid, bin) and the windows come back, and the host fills the holes and serialises the .bai.
// np2_bamout_host does all of it with the same per-record code (np2_bamout_core.hpp) in plain loops and no device.
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_bamout.hpp"
#include "np2_sam.hpp"
#include "np2_sam_handle.hpp"
#include "np2_samtail_core.hpp"

#include <algorithm>
#include <functional>

namespace {
using np2h::Np2Error;
using np2bam::Rec;

struct Run {
    uint64_t key, beg, end; // key: tid << 32 | bin
};

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i)));
}
void put64(std::vector<uint8_t> &v, uint64_t x) {
    for (int i = 0; i < 8; ++i) v.push_back((uint8_t)(x >> (8 * i)));
}

// the stream in front of the first record; text: the header text (the lean stream's: np2h::bam_header_text(refs, ""))
std::vector<uint8_t> bam_header(const np2sam::Refs &refs, const std::string &text) {
    std::vector<uint8_t> h = {'B', 'A', 'M', 1};
    put32(h, (uint32_t)text.size());
    h.insert(h.end(), text.begin(), text.end());
    put32(h, (uint32_t)refs.names.size());
    for (size_t i = 0; i < refs.names.size(); ++i) {
        put32(h, (uint32_t)refs.names[i].size() + 1u);
        h.insert(h.end(), refs.names[i].begin(), refs.names[i].end());
        h.push_back(0);
        put32(h, refs.lens[i]);
    }
    return h;
}

std::vector<uint8_t> bam_header(const np2_sam &sam) {
    return bam_header(sam.refs, sam.has_tails ? sam.header_text : np2h::bam_header_text(sam.refs, ""));
}

void check_refs(const np2sam::Refs &refs) {
    for (size_t i = 0; i < refs.names.size(); ++i)
        if (refs.lens[i] > np2bam::REF_MAX)
            throw Np2Error(NP2_E_UNSUPPORTED, "reference " + refs.names[i] + " has LN " + std::to_string(refs.lens[i]) +
                                                  ", more than 2^29: a .bai cannot index it (CSI is not written)");
}
void refuse(const np2bam::Refusals &r, const std::function<std::string(uint32_t)> &who) {
    // the smallest record speaks; of two refusals of one record, the order of k_bam_sizes
    const uint32_t first = std::min(r.big_cigar, std::min(r.neg_pos, r.far_end));
    if (first == np2bam::NONE) return;
    if (first == r.big_cigar)
        throw Np2Error(NP2_E_UNSUPPORTED, who(first) + " has more than 65535 CIGAR operations (no CG tag is written)");
    if (first == r.neg_pos) throw Np2Error(NP2_E_ARG, who(first) + " has POS 0: a mapped record without a position");
    throw Np2Error(NP2_E_UNSUPPORTED, who(first) + " ends behind base 2^29: a .bai cannot index it (CSI is not written)");
}

std::string bai_name(const char *bam_path, const char *bai_path) { return bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai"; }

// the .bai: runs ordered by key (runs of one key in file order), windows win[win_off[t] .. + n_intv[t]) with all ones where
// no record overlaps
void write_bai(const std::string &path, size_t n_refs, const std::vector<Run> &runs, const std::vector<uint32_t> &n_intv,
               const std::vector<uint32_t> &win_off, const std::vector<uint64_t> &win, np2_bamout_stats_t &st) {
    std::vector<uint8_t> out = {'B', 'A', 'I', 1};
    put32(out, (uint32_t)n_refs);
    size_t at = 0;
    for (size_t t = 0; t < n_refs; ++t) {
        size_t hi = at, n_bin = 0;
        while (hi < runs.size() && runs[hi].key >> 32 == t) {
            if (hi == at || runs[hi].key != runs[hi - 1].key) ++n_bin;
            ++hi;
        }
        put32(out, (uint32_t)n_bin);
        while (at < hi) {
            size_t e = at;
            while (e < hi && runs[e].key == runs[at].key) ++e;
            put32(out, (uint32_t)runs[at].key), put32(out, (uint32_t)(e - at));
            for (; at < e; ++at) put64(out, runs[at].beg), put64(out, runs[at].end);
        }
        st.bins += n_bin;
        put32(out, n_intv[t]);
        uint64_t prev = 0;
        for (uint32_t w = 0; w < n_intv[t]; ++w) {
            const uint64_t v = win[(size_t)win_off[t] + w];
            if (v != ~0ull) prev = v;
            put64(out, prev);
        }
    }
    st.chunks += runs.size();
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw Np2Error(NP2_E_ARG, "cannot open " + path + " for writing");
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    if (fclose(f) != 0 || !ok) throw Np2Error(NP2_E_ARG, "cannot write " + path);
}

std::vector<uint32_t> window_offsets(const std::vector<uint32_t> &n_intv) {
    std::vector<uint32_t> off(n_intv.size() + 1, 0u);
    for (size_t t = 0; t < n_intv.size(); ++t) off[t + 1] = off[t] + n_intv[t]; // (at most 2^15 a reference, below 2^31 references)
    return off;
}

// ---- the device ---------------------------------------------------------------------------------------------------------
template <class T> void upload(hipStream_t st, T *dst, const std::vector<T> &src) {
    if (src.empty()) return;
    HIPCHK(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (a pageable source that may go away)
}
template <class T> std::vector<T> download(hipStream_t st, const T *src, size_t n) {
    std::vector<T> v(n);
    if (n) {
        HIPCHK(hipMemcpyAsync(v.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return v;
}

// what k_bam_sizes and its scan leave, the refusals raised
struct Sized {
    DevBuf<uint32_t> sz, be, d_nintv;
    DevBuf<uint64_t> off;
    DevBuf<np2bam::Refusals> d_ref;
    DevBuf<uint8_t> tmp;
    size_t tmp_bytes = 0;
    std::vector<uint32_t> n_intv;
    uint64_t rec_total = 0;
    float ms = 0.f;
    Sized() { sz.cached = be.cached = d_nintv.cached = off.cached = d_ref.cached = tmp.cached = true; } // (released after a drained stream)
};

np2::BamSrc source(const np2_sam &sam) {
    return np2::BamSrc{sam.recs.p, sam.tids.p, sam.cigar.p, sam.seq4.p, sam.names.p, sam.name_ref.p, sam.has_tails ? sam.tails.p : nullptr,
                       sam.has_tails ? sam.tail_ref.p : nullptr, (uint32_t)sam.n_recs};
}

void sizes(np2_ctx *cx, const np2_sam &sam, size_t scan_items, Sized &z) {
    hipStream_t st = cx->stream;
    const uint32_t n = (uint32_t)sam.n_recs;
    const size_t n_refs = sam.refs.names.size();
    z.n_intv.assign(n_refs, 0u);
    z.tmp_bytes = np2::prim_temp_bytes(std::max(scan_items, (size_t)n + 1));
    z.tmp.ensure(z.tmp_bytes);
    if (!n) return;
    z.sz.ensure((size_t)n + 1), z.be.ensure(n), z.off.ensure((size_t)n + 1), z.d_nintv.ensure(n_refs), z.d_ref.ensure(1);
    np2h::DevEvent e0, e1;
    e0.make(), e1.make();
    HIPCHK(hipMemsetAsync(z.d_ref.p, 0xFF, sizeof(np2bam::Refusals), st));
    HIPCHK(hipMemsetAsync(z.d_nintv.p, 0, n_refs * 4, st));
    HIPCHK(hipEventRecord(e0.e, st));
    np2::launch_bam_sizes(st, source(sam), z.sz.p, z.be.p, z.d_ref.p, z.d_nintv.p);
    if (np2::prim_exclusive_sum_u32_u64(st, z.tmp.p, z.tmp_bytes, z.sz.p, z.off.p, (size_t)n + 1))
        throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
    HIPCHK(hipEventRecord(e1.e, st));
    HIPCHK(hipGetLastError());
    const np2bam::Refusals r = download(st, z.d_ref.p, 1)[0];
    z.n_intv = download(st, z.d_nintv.p, n_refs);
    z.rec_total = download(st, z.off.p + n, 1)[0];
    z.ms = np2h::elapsed(e0, e1);
    refuse(r, [&](uint32_t i) {
        if (i >= sam.keys.size()) throw Np2Error(NP2_E_DEVICE, "np2_bamout: refused record out of range");
        const uint64_t k = sam.keys[i];
        return "record " + std::to_string(i) + " of the sorted order (reference " + sam.refs.names[(size_t)(k >> 33)] + ", POS " +
               std::to_string((k >> 1) & 0xFFFFFFFFull) + ")";
    });
    for (uint32_t v : z.n_intv)
        if (v > (np2bam::REF_MAX >> np2bam::WIN_SHIFT)) throw Np2Error(NP2_E_DEVICE, "np2_bamout: window count out of range");
}

void common_checks(np2_ctx *cx, np2_sam *sam, const char *who) {
    if (!sam->has_names)
        throw Np2Error(NP2_E_ARG, std::string(who) + ": the SAM was opened without its names (np2_sam_open_ex with NP2_SAM_KEEP_NAMES)");
    if (cx->device != sam->device) throw Np2Error(NP2_E_ARG, std::string(who) + ": the context is on another device than the SAM");
    check_refs(sam->refs);
}

// created: set once the first file exists
void write_bam(np2_ctx *cx, np2_sam &sam, const std::string &bam_path, const std::string &bai_path, np2_bamout_stats_t &stats, bool &created) {
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t cs = cx->stream;
    const uint32_t n = (uint32_t)sam.n_recs;
    const size_t n_refs = sam.refs.names.size();
    const std::vector<uint8_t> hdr = bam_header(sam);
    const uint64_t H = hdr.size();
    Sized z;
    sizes(cx, sam, 0, z); // (throws the refusals: nothing has been created)
    const uint64_t total = H + z.rec_total, n_blk = (total + np2bam::BLOCK_BYTES - 1) / np2bam::BLOCK_BYTES;
    if (n_blk >= 0xFFFFFFF0ull) throw Np2Error(NP2_E_UNSUPPORTED, "a BAM stream of 2^32 blocks or more");
    z.tmp_bytes = np2::prim_temp_bytes(std::max<size_t>((size_t)n_blk + 1, (size_t)n + 1));
    z.tmp.ensure(z.tmp_bytes);
    stats.records = n, stats.stream_bytes = total, stats.blocks = n_blk, stats.sizes_ms = z.ms;
    const np2::BamSrc src = source(sam);
    DevBuf<uint32_t> blk_sizes;
    DevBuf<uint8_t> d_hdr;
    blk_sizes.cached = d_hdr.cached = true; // (released after drained streams)
    blk_sizes.ensure((size_t)n_blk + 1), d_hdr.ensure(H);
    {
        np2h::BgzfWriter w(cx->device, bam_path.c_str());
        created = true;
        hipStream_t ws = w.stream();
        upload(ws, d_hdr.p, hdr);
        const uint64_t cap = w.batch_bytes();
        const uint32_t grid = np2h::grid_blocks(cx->device, 8);
        for (uint64_t b0 = 0; b0 < total; b0 += cap) {
            const uint64_t b1 = std::min(total, b0 + cap);
            uint8_t *dst = w.device_in();
            if (b0 < H) HIPCHK(hipMemcpyAsync(dst, d_hdr.p + b0, std::min(H, b1) - b0, hipMemcpyDeviceToDevice, ws));
            if (b1 > H) {
                const uint64_t a = std::max(b0, H);
                np2::launch_bam_emit(ws, src, z.off.p, z.be.p, a - H, b1 - H, dst + (a - b0), grid);
                HIPCHK(hipGetLastError());
            }
            w.commit_device((size_t)(b1 - b0), blk_sizes.p + b0 / np2bam::BLOCK_BYTES);
        }
        w.close(); // (drains its stream)
        stats.file_bytes = w.bytes_out(), stats.emit_ms = w.fill_ms(), stats.deflate_ms = w.kernel_ms();
    }
    // the index
    std::vector<Run> runs;
    const std::vector<uint32_t> win_off = window_offsets(z.n_intv);
    std::vector<uint64_t> win;
    if (n) {
        np2h::DevEvent e0, e1, e2, e3;
        e0.make(), e1.make(), e2.make(), e3.make();
        DevBuf<uint64_t> C, beg, end, key, key_s, rbeg, rend;
        DevBuf<unsigned long long> d_win;
        DevBuf<uint32_t> head, run, val, val_s, d_woff;
        C.cached = beg.cached = end.cached = key.cached = key_s.cached = rbeg.cached = rend.cached = d_win.cached = true;
        head.cached = run.cached = val.cached = val_s.cached = d_woff.cached = true;
        C.ensure((size_t)n_blk + 1), beg.ensure(n), end.ensure(n), head.ensure((size_t)n + 1), run.ensure((size_t)n + 1);
        d_woff.ensure(win_off.size()), d_win.ensure((size_t)win_off.back() + 1);
        upload(cs, d_woff.p, win_off);
        HIPCHK(hipEventRecord(e0.e, cs));
        HIPCHK(hipMemsetAsync(blk_sizes.p + n_blk, 0, 4, cs));
        if (np2::prim_exclusive_sum_u32_u64(cs, z.tmp.p, z.tmp_bytes, blk_sizes.p, C.p, (size_t)n_blk + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        np2::launch_bai_voff(cs, src, z.off.p, z.be.p, H, C.p, beg.p, end.p, head.p);
        if (np2::prim_exclusive_sum_u32(cs, z.tmp.p, z.tmp_bytes, head.p, run.p, (size_t)n + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipEventRecord(e1.e, cs));
        HIPCHK(hipGetLastError());
        const uint32_t n_runs = download(cs, run.p + n, 1)[0];
        if (!n_runs || n_runs > n) throw Np2Error(NP2_E_DEVICE, "np2_bamout: run count out of range");
        key.ensure(n_runs), key_s.ensure(n_runs), rbeg.ensure(n_runs), rend.ensure(n_runs), val.ensure(n_runs), val_s.ensure(n_runs);
        HIPCHK(hipEventRecord(e2.e, cs));
        np2::launch_bai_chunks(cs, src, z.be.p, beg.p, end.p, head.p, run.p, key.p, rbeg.p, rend.p, val.p);
        if (np2::prim_sort_pairs_u64_u32(cs, z.tmp.p, z.tmp_bytes, key.p, key_s.p, val.p, val_s.p, n_runs, 64))
            throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
        HIPCHK(hipMemsetAsync(d_win.p, 0xFF, ((size_t)win_off.back() + 1) * 8, cs));
        np2::launch_bai_linear(cs, src, z.be.p, beg.p, d_woff.p, d_win.p);
        HIPCHK(hipEventRecord(e3.e, cs));
        HIPCHK(hipGetLastError());
        const std::vector<uint64_t> k = download(cs, key_s.p, n_runs), rb = download(cs, rbeg.p, n_runs), re = download(cs, rend.p, n_runs);
        const std::vector<uint32_t> v = download(cs, val_s.p, n_runs);
        const std::vector<unsigned long long> wv = download(cs, d_win.p, win_off.back());
        win.assign(wv.begin(), wv.end());
        stats.index_ms = np2h::elapsed(e0, e1) + np2h::elapsed(e2, e3);
        runs.resize(n_runs);
        for (uint32_t j = 0; j < n_runs; ++j) {
            if (v[j] >= n_runs || k[j] >> 32 >= n_refs) throw Np2Error(NP2_E_DEVICE, "np2_bamout: run out of range");
            runs[j] = Run{k[j], rb[v[j]], re[v[j]]};
        }
    }
    write_bai(bai_path, n_refs, runs, z.n_intv, win_off, win, stats);
}

// ---- the host twin ------------------------------------------------------------------------------------------------------
struct HostIn {
    const np2_bamrec_t *recs;
    const int32_t *tids;
    const uint32_t *cigar;
    const uint8_t *seq4;
    uint64_t n, n_cigar, seq_bytes;
    const uint8_t *names;
    uint64_t name_bytes;
    const uint64_t *name_ref;
    const uint8_t *tails = nullptr; // np2_bamout_host_full: the tails, tail_ref[i] = offset << 1 | has_qual, the header text
    uint64_t tail_bytes = 0;
    const uint64_t *tail_ref = nullptr;
    const char *header_text = nullptr;
    uint64_t header_bytes = 0;
};

Rec host_rec(const HostIn &in, uint64_t i, size_t n_refs) {
    const np2_bamrec_t &b = in.recs[i];
    const std::string who = "np2_bamout_host: record " + std::to_string(i);
    const uint64_t no = np2bam::name_off(in.name_ref[i]);
    const uint32_t nl = np2bam::name_len(in.name_ref[i]);
    if (in.tids[i] < 0 || (size_t)in.tids[i] >= n_refs) throw Np2Error(NP2_E_ARG, who + ": tid outside the reference list");
    if (nl == 0 || nl > np2bam::QNAME_MAX || no > in.name_bytes || nl > in.name_bytes - no) throw Np2Error(NP2_E_ARG, who + ": name outside the name bytes, empty or longer than 254 bytes");
    if (b.cigar_off > in.n_cigar || b.n_cigar > in.n_cigar - b.cigar_off) throw Np2Error(NP2_E_ARG, who + ": CIGAR words outside the array");
    if (b.seq_off > in.seq_bytes || ((uint64_t)b.l_seq + 1) / 2 > in.seq_bytes - b.seq_off) throw Np2Error(NP2_E_ARG, who + ": SEQ bytes outside the array");
    if (b.l_seq >= (1u << 31)) throw Np2Error(NP2_E_ARG, who + ": l_seq of 2^31 or more");
    Rec r;
    r.tid = in.tids[i], r.pos = b.pos, r.flag = b.flag, r.mapq = b.mapq, r.n_cigar = b.n_cigar, r.l_seq = b.l_seq, r.name_len = nl, r.bin = 0;
    r.name = in.names + no, r.cigar = in.cigar + b.cigar_off, r.seq = in.seq4 + b.seq_off;
    r.tail = nullptr, r.has_qual = 0u, r.aux_len = 0u;
    if (in.tail_ref) {
        const uint64_t to = np2tail::tail_off(in.tail_ref[i]);
        if (to % 4u || to > in.tail_bytes || in.tail_bytes - to < np2bam::TAIL_HEAD) throw Np2Error(NP2_E_ARG, who + ": tail outside the tail bytes or not at a word");
        r.tail = in.tails + to, r.has_qual = np2tail::tail_has_qual(in.tail_ref[i]) ? 1u : 0u, r.aux_len = np2bam::tail_word(r.tail, 3);
        if ((uint64_t)r.aux_len + (r.has_qual ? b.l_seq : 0u) > in.tail_bytes - to - np2bam::TAIL_HEAD)
            throw Np2Error(NP2_E_ARG, who + ": quality bytes or optional fields outside the tail bytes");
        if (r.aux_len >= (1u << 31)) throw Np2Error(NP2_E_ARG, who + ": aux_len of 2^31 or more");
    }
    return r;
}

void bamout_host(const HostIn &in, const np2sam::Refs &refs, const char *bam_path, const char *bai_path, uint8_t **S_out, uint64_t *n_S,
                 np2_bamout_stats_t &stats) {
    const size_t n_refs = refs.names.size();
    check_refs(refs);
    // k_bam_sizes and the scan
    std::vector<Rec> recs(in.n);
    std::vector<uint64_t> off(in.n + 1, 0);
    std::vector<uint32_t> last_win(in.n, 0), n_intv(n_refs, 0);
    np2bam::Refusals ref{np2bam::NONE, np2bam::NONE, np2bam::NONE};
    for (uint64_t i = 0; i < in.n; ++i) {
        if (i && (in.tids[i] < in.tids[i - 1] || (in.tids[i] == in.tids[i - 1] && in.recs[i].pos < in.recs[i - 1].pos)))
            throw Np2Error(NP2_E_ARG, "np2_bamout_host: record " + std::to_string(i) + " is not in coordinate order");
        Rec &r = recs[i] = host_rec(in, i, n_refs);
        uint64_t bytes = 0;
        const uint32_t ord = (uint32_t)std::min<uint64_t>(i, np2bam::NONE - 1u);
        if (r.n_cigar > np2bam::CIGAR_MAX) {
            ref.big_cigar = std::min(ref.big_cigar, ord);
        } else if (r.pos < 0) {
            ref.neg_pos = std::min(ref.neg_pos, ord);
        } else {
            const uint64_t span = np2bam::cigar_span(r.cigar, r.n_cigar), end = (uint64_t)r.pos + (span ? span : 1u);
            if (end > np2bam::REF_MAX) {
                ref.far_end = std::min(ref.far_end, ord);
            } else {
                last_win[i] = (uint32_t)(end - 1u) >> np2bam::WIN_SHIFT;
                bytes = np2bam::rec_bytes(r.name_len, r.n_cigar, r.l_seq, r.aux_len);
                r.bin = np2bam::reg2bin((uint32_t)r.pos, (uint32_t)end);
                n_intv[(size_t)r.tid] = std::max(n_intv[(size_t)r.tid], last_win[i] + 1u);
            }
        }
        off[i + 1] = off[i] + bytes;
    }
    refuse(ref, [&](uint32_t i) {
        return "record " + std::to_string(i) + " of the sorted order (reference " + refs.names[(size_t)in.tids[i]] + ", POS " +
               std::to_string((int64_t)in.recs[i].pos + 1) + ")";
    });
    // k_bam_emit, byte by byte
    const std::vector<uint8_t> hdr = bam_header(refs, in.header_text ? std::string(in.header_text, in.header_bytes) : np2h::bam_header_text(refs, ""));
    const uint64_t H = hdr.size(), total = H + off[in.n], n_blk = (total + np2bam::BLOCK_BYTES - 1) / np2bam::BLOCK_BYTES;
    std::unique_ptr<uint8_t, void (*)(void *)> S((uint8_t *)malloc(total), free);
    if (!S) throw Np2Error(NP2_E_NOMEM, "out of memory for the BAM stream");
    memcpy(S.get(), hdr.data(), H);
    for (uint64_t i = 0; i < in.n; ++i)
        for (uint64_t j = 0, m = off[i + 1] - off[i]; j < m; ++j) S.get()[H + off[i] + j] = np2bam::rec_byte(recs[i], j);
    stats.records = in.n, stats.stream_bytes = total, stats.blocks = n_blk;
    if (bam_path) {
        // the file, and the blocks' offsets from their sizes (what the device keeps of each block)
        std::vector<uint8_t> file((size_t)n_blk * 65536 + 28);
        uint64_t file_n = 0;
        if (np2_bgzf_deflate_host(S.get(), total, 0, file.data(), file.size(), &file_n) != NP2_OK) throw Np2Error(NP2_E_DEVICE, np2_io_last_error());
        std::vector<uint64_t> C((size_t)n_blk + 1, 0);
        for (uint64_t b = 0; b < n_blk; ++b) C[b + 1] = C[b] + ((uint64_t)file[C[b] + 16] | (uint64_t)file[C[b] + 17] << 8) + 1u;
        if (C[n_blk] + 28 != file_n) throw Np2Error(NP2_E_DEVICE, "np2_bamout_host: the blocks' sizes do not add up");
        stats.file_bytes = file_n;
        // k_bai_voff, k_bai_chunks, the sort by key (stable) and k_bai_linear
        const std::vector<uint32_t> win_off = window_offsets(n_intv);
        std::vector<uint64_t> win(win_off.back(), ~0ull);
        std::vector<Run> runs;
        for (uint64_t i = 0; i < in.n; ++i) {
            const uint64_t beg = np2bam::voff(C.data(), H + off[i]), end = np2bam::voff(C.data(), H + off[i + 1]);
            const uint64_t key = (uint64_t)(uint32_t)recs[i].tid << 32 | recs[i].bin;
            if (i == 0 || recs[i].tid != recs[i - 1].tid || recs[i].bin != recs[i - 1].bin) runs.push_back(Run{key, beg, end});
            else runs.back().end = end;
            for (uint32_t w = (uint32_t)recs[i].pos >> np2bam::WIN_SHIFT; w <= last_win[i]; ++w) {
                uint64_t &slot = win[(size_t)win_off[(size_t)recs[i].tid] + w];
                slot = std::min(slot, beg);
            }
        }
        std::stable_sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.key < b.key; });
        const std::string bai = bai_name(bam_path, bai_path);
        FILE *f = fopen(bam_path, "wb");
        if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + bam_path + " for writing");
        const bool ok = fwrite(file.data(), 1, file_n, f) == file_n;
        if (fclose(f) != 0 || !ok) {
            remove(bam_path);
            throw Np2Error(NP2_E_ARG, std::string("cannot write ") + bam_path);
        }
        try {
            write_bai(bai, n_refs, runs, n_intv, win_off, win, stats);
        } catch (...) {
            remove(bam_path), remove(bai.c_str());
            throw;
        }
    }
    if (S_out) *S_out = S.release(), *n_S = total;
}

} // namespace

namespace np2h {
std::string bam_header_text(const np2sam::Refs &refs, const std::string &extra) {
    std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
    for (size_t i = 0; i < refs.names.size(); ++i) text += "@SQ\tSN:" + refs.names[i] + "\tLN:" + std::to_string(refs.lens[i]) + "\n";
    return text + extra;
}
} // namespace np2h

extern "C" {

int np2_sam_write_bam(np2_ctx_t *cx, np2_sam_t *sam, const char *bam_path, const char *bai_path, np2_bamout_stats_t *stats) {
    bool touched = false, created = false;
    std::string bam, bai;
    return np2h::abi_guard([&] {
        // checked before anything of the context or the handle is looked at, and all of it before a file is created
        if (!cx || !sam || !bam_path) throw Np2Error(NP2_E_ARG, "np2_sam_write_bam: NULL argument");
        common_checks(cx, sam, "np2_sam_write_bam");
        bam = bam_path, bai = bai_name(bam_path, bai_path);
        touched = true;
        np2_bamout_stats_t st{};
        write_bam(cx, *sam, bam, bai, st, created);
        if (stats) *stats = st;
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            cx->err = msg;
        }
        if (created) remove(bam.c_str()), remove(bai.c_str()); // a failed call leaves no file; a refusal was raised before either existed
        np2h::io_set_error(code, msg);
    });
}

int np2_sam_bam_stream(np2_ctx_t *cx, np2_sam_t *sam, uint8_t **S, uint64_t *n_out) {
    bool touched = false;
    return np2h::abi_guard([&] {
        if (!cx || !sam || !S || !n_out) throw Np2Error(NP2_E_ARG, "np2_sam_bam_stream: NULL argument");
        *S = nullptr, *n_out = 0;
        common_checks(cx, sam, "np2_sam_bam_stream");
        touched = true;
        HIPCHK(hipSetDevice(cx->device));
        hipStream_t st = cx->stream;
        const std::vector<uint8_t> hdr = bam_header(*sam);
        Sized z;
        sizes(cx, *sam, 0, z);
        const uint64_t H = hdr.size(), total = H + z.rec_total;
        DevBuf<uint8_t> d_S;
        d_S.cached = true; // (released after the drained stream)
        d_S.ensure(total + 4);
        upload(st, d_S.p, hdr);
        np2::launch_bam_emit(st, source(*sam), z.off.p, z.be.p, 0, z.rec_total, d_S.p + H, np2h::grid_blocks(cx->device, 8));
        HIPCHK(hipGetLastError());
        std::unique_ptr<uint8_t, void (*)(void *)> h((uint8_t *)malloc(total), free);
        if (!h) throw Np2Error(NP2_E_NOMEM, "out of memory for the BAM stream");
        HIPCHK(hipMemcpyAsync(h.get(), d_S.p, total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *S = h.release(), *n_out = total;
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            cx->err = msg;
        }
        np2h::io_set_error(code, msg);
    });
}

int np2_sam_export_names(np2_ctx_t *cx, np2_sam_t *sam, uint8_t **names, uint64_t *name_bytes, uint64_t **name_ref, uint64_t *n_recs) {
    bool touched = false;
    return np2h::abi_guard([&] {
        if (!cx || !sam || !names || !name_bytes || !name_ref || !n_recs) throw Np2Error(NP2_E_ARG, "np2_sam_export_names: NULL argument");
        *names = nullptr, *name_ref = nullptr, *name_bytes = 0, *n_recs = 0;
        if (!sam->has_names) throw Np2Error(NP2_E_ARG, "np2_sam_export_names: the SAM was opened without its names (np2_sam_open_ex with NP2_SAM_KEEP_NAMES)");
        if (cx->device != sam->device) throw Np2Error(NP2_E_ARG, "np2_sam_export_names: the context is on another device than the SAM");
        touched = true;
        HIPCHK(hipSetDevice(cx->device));
        std::unique_ptr<uint8_t, void (*)(void *)> a((uint8_t *)malloc(sam->name_bytes + 1), free);
        std::unique_ptr<uint64_t, void (*)(void *)> b((uint64_t *)malloc((sam->n_recs + 1) * 8), free);
        if (!a || !b) throw Np2Error(NP2_E_NOMEM, "out of memory for the names");
        if (sam->name_bytes) HIPCHK(hipMemcpyAsync(a.get(), sam->names.p, sam->name_bytes, hipMemcpyDeviceToHost, cx->stream));
        if (sam->n_recs) HIPCHK(hipMemcpyAsync(b.get(), sam->name_ref.p, sam->n_recs * 8, hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        *name_bytes = sam->name_bytes, *n_recs = sam->n_recs;
        *names = a.release(), *name_ref = b.release();
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            cx->err = msg;
        }
        np2h::io_set_error(code, msg);
    });
}

int np2_bamout_host(const np2_bamrec_t *recs, const int32_t *tids, const uint32_t *cigar, const uint8_t *seq4, uint64_t n_recs,
                    uint64_t n_cigar_words, uint64_t seq_bytes, const uint8_t *names, uint64_t name_bytes, const uint64_t *name_ref,
                    const char *const *ref_names, const uint32_t *ref_lens, int n_refs, const char *bam_path, const char *bai_path,
                    uint8_t **S, uint64_t *n_S, np2_bamout_stats_t *stats) {
    return np2_bamout_host_full(recs, tids, cigar, seq4, n_recs, n_cigar_words, seq_bytes, names, name_bytes, name_ref, nullptr, 0, nullptr, nullptr,
                                0, ref_names, ref_lens, n_refs, bam_path, bai_path, S, n_S, stats);
}

int np2_bamout_host_full(const np2_bamrec_t *recs, const int32_t *tids, const uint32_t *cigar, const uint8_t *seq4, uint64_t n_recs,
                         uint64_t n_cigar_words, uint64_t seq_bytes, const uint8_t *names, uint64_t name_bytes, const uint64_t *name_ref,
                         const uint8_t *tails, uint64_t tail_bytes, const uint64_t *tail_ref, const char *header_text, uint64_t header_bytes,
                         const char *const *ref_names, const uint32_t *ref_lens, int n_refs, const char *bam_path, const char *bai_path,
                         uint8_t **S, uint64_t *n_S, np2_bamout_stats_t *stats) {
    return np2h::abi_guard([&] {
        if ((tail_ref && tail_bytes && !tails) || (!tail_ref && tails) || (header_bytes && !header_text))
            throw Np2Error(NP2_E_ARG, "np2_bamout_host: NULL argument");
        if (header_bytes >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "np2_bamout_host: a header text of 2 GiB or more");
        if (S) *S = nullptr;
        if (n_S) *n_S = 0;
        if (n_refs < 0 || (n_refs && (!ref_names || !ref_lens)) || (S && !n_S) || (n_recs && (!recs || !tids || !name_ref || !names)) ||
            (n_cigar_words && !cigar) || (seq_bytes && !seq4) || (!bam_path && bai_path))
            throw Np2Error(NP2_E_ARG, "np2_bamout_host: NULL argument");
        if (n_recs >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "np2_bamout_host: 2^31 records or more");
        np2sam::Refs refs;
        for (int i = 0; i < n_refs; ++i) {
            if (!ref_names[i] || !*ref_names[i]) throw Np2Error(NP2_E_ARG, "np2_bamout_host: a reference name is NULL or empty");
            refs.names.push_back(ref_names[i]), refs.lens.push_back(ref_lens[i]);
        }
        np2_bamout_stats_t st{};
        HostIn in{recs, tids, cigar, seq4, n_recs, n_cigar_words, seq_bytes, names, name_bytes, name_ref};
        in.tails = tails, in.tail_bytes = tail_bytes, in.tail_ref = n_recs ? tail_ref : nullptr, in.header_text = header_text, in.header_bytes = header_bytes;
        bamout_host(in, refs, bam_path, bai_path, S, n_S, st);
        if (stats) *stats = st;
        return NP2_OK;
    }, np2h::io_set_error);
}

} // extern "C"
