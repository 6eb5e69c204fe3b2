// The indexed BAM on the host: BGZF + BAI on zlib or libdeflate, the handle's entry points, the -S pass over the primaries' SEQ
// and the record reader of the host pool.
#include "np2_bamfile.hpp"
#include "np2_bai_core.hpp"

#include <zlib.h>
#include <dlfcn.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <unordered_set>

namespace np2h {
namespace {

// Raw-deflate decoder for BGZF blocks (each block is one complete deflate stream of known inflated size): libdeflate's
// whole-buffer decoder when the host has its runtime library (2-3 x zlib's rate on BAM payloads; htslib makes the same
// choice at build time), zlib otherwise or with NP2_INFLATE=zlib.  Resolved once, at run time: the image ships
// libdeflate.so.0 without headers, and a host without it must still work.
struct Inflater {
    typedef void *(*alloc_fn)(void);
    typedef int (*dec_fn)(void *, const void *, size_t, void *, size_t, size_t *);
    typedef void (*free_fn)(void *);
    typedef uint32_t (*crc_fn)(uint32_t, const void *, size_t);
    crc_fn crc_ld = nullptr; // libdeflate_crc32 (several bytes a clock; zlib's crc32 otherwise)
    alloc_fn alloc = nullptr;
    dec_fn dec = nullptr;
    free_fn fre = nullptr;
    Inflater() {
        const char *e = getenv("NP2_INFLATE");
        if (e && !strcmp(e, "zlib")) return;
        void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = (alloc_fn)dlsym(h, "libdeflate_alloc_decompressor");
        dec = (dec_fn)dlsym(h, "libdeflate_deflate_decompress");
        fre = (free_fn)dlsym(h, "libdeflate_free_decompressor");
        if (!alloc || !dec || !fre) alloc = nullptr, dec = nullptr, fre = nullptr;
        else crc_ld = (crc_fn)dlsym(h, "libdeflate_crc32");
    }
    static Inflater &get() {
        static Inflater *i = new Inflater();
        return *i;
    }
    const char *name() const { return dec ? "libdeflate" : "zlib"; }
    struct PerThread { // one decoder per thread, released with the thread
        void *d = nullptr;
        free_fn fre = nullptr;
        ~PerThread() {
            if (d && fre) fre(d);
        }
    };
    // inflates `clen` bytes at `in` into exactly `isize` bytes at `out`
    bool run(const uint8_t *in, size_t clen, uint8_t *out, size_t isize) const {
        if (dec) {
            static thread_local PerThread t;
            if (!t.d) t.d = alloc(), t.fre = fre;
            if (t.d) {
                size_t got = 0;
                return dec(t.d, in, clen, out, isize, &got) == 0 && got == isize;
            }
        }
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        zs.next_in = const_cast<Bytef *>(in);
        zs.avail_in = (uInt)clen;
        zs.next_out = out;
        zs.avail_out = (uInt)isize;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        return rc == Z_STREAM_END && zs.avail_out == 0;
    }
    // CRC-32 (gzip) of n bytes: what a BGZF block's CRC32 word must equal for its inflated bytes
    uint32_t crc(const uint8_t *d, size_t n) const {
        if (crc_ld) return crc_ld(0u, d, n);
        return (uint32_t)crc32(crc32(0L, Z_NULL, 0), d, (uInt)n);
    }
};

} // namespace

const char *inflater_name() { return Inflater::get().name(); }
// Every BGZF block a path inflates must carry the CRC-32 of its inflated bytes (htslib checks it; DEFLATE itself has no
// checksum, and most single-bit flips inside a payload still inflate to ISIZE bytes).  NP2_BGZF_CRC=0, read once per
// process, switches the check off on every path, host and device: it exists to time the check, not to read damaged files.
bool bgzf_crc_on() {
    static const bool on = !(getenv("NP2_BGZF_CRC") && !strcmp(getenv("NP2_BGZF_CRC"), "0"));
    return on;
}
std::string crc_msg(uint64_t file_off) { return "BGZF CRC32 mismatch (block at file offset " + std::to_string(file_off) + ")"; }

bool pread_full(int fd, uint8_t *dst, size_t n, uint64_t off) {
    for (size_t got = 0; got < n;) {
        const ssize_t r = pread(fd, dst + got, n - got, (off_t)(off + got));
        if (r <= 0) return false;
        got += (size_t)r;
    }
    return true;
}

bool Bgzf::read_block() {
    block.clear();
    bpos = 0;
    block_off = (uint64_t)ftello(f);
    if (block_off >= flen) return false;
    const uint64_t left = flen - block_off;
    size_t have = 0;
    auto get = [&](size_t upto) { // bytes [have, upto) of the block
        cdata.resize(upto);
        if (fread(cdata.data() + have, 1, upto - have, f) != upto - have) throw np2h::Np2Error(NP2_E_ARG, "truncated BGZF block");
        have = upto;
    };
    np2h::BgzfHeader h{(uint32_t)std::min<uint64_t>(18, left), 0, 0, 0};
    while (h.need) {
        get(h.need);
        h = np2h::bgzf_header(cdata.data(), have, left);
    }
    get(h.bsize);
    const uint8_t *payload = cdata.data() + h.hdr_len;
    const np2h::BgzfTrailer t = np2h::bgzf_trailer(payload + h.clen);
    block.resize(t.isize);
    if (t.isize && !Inflater::get().run(payload, h.clen, block.data(), t.isize)) throw np2h::Np2Error(NP2_E_ARG, "BGZF inflate failed");
    if (bgzf_crc_on() && Inflater::get().crc(block.data(), t.isize) != t.crc) throw np2h::Np2Error(NP2_E_ARG, crc_msg(block_off));
    return true;
}

void BgzfBatch::fill(size_t n_blocks, const std::function<void()> *during) {
    if (eof) {
        if (during) (*during)();
        return;
    }
    const double t_f0 = np2h::now_ms();
    if (pos) { // drop consumed bytes (blocks that lie entirely before the new front leave the index)
        size_t keep = 0;
        while (keep + 1 < blk_index.size() && blk_index[keep + 1].first <= (int64_t)pos) ++keep;
        blk_index.erase(blk_index.begin(), blk_index.begin() + (long)keep);
        for (auto &e : blk_index) e.first -= (int64_t)pos;
        buf.drop_front(pos);
        pos = 0;
    }
    const double t_f1 = np2h::now_ms();
    std::vector<BgzfBlock> &blks = cur_blks;
    blks.clear();
    size_t total = 0;
    const bool past = fpos > hint_fpos;
    if (past) n_blocks = std::min(n_blocks, past_hint), past_hint *= 2;
    for (size_t i = 0; i < n_blocks; ++i) {
        if (!past && fpos > hint_fpos) break;
        BgzfBlock b;
        if (!read_raw(b)) {
            eof = true;
            break;
        }
        b.out_off = total;
        total += b.isize;
        blks.push_back(b);
    }
    const size_t base = buf.size();
    buf.resize(base + total);
    for (auto &bk : blks) blk_index.emplace_back((int64_t)(base + bk.out_off), bk.file_off);
    if (blks.size() > blk_done_cap) {
        blk_done_cap = blks.size() + blks.size() / 2;
        blk_done.reset(new std::atomic<uint8_t>[blk_done_cap]);
    }
    for (size_t i = 0; i < blks.size(); ++i) blk_done[i].store(0, std::memory_order_relaxed);
    cur_base = base, ready_bi = 0, ready_end = base;
    if (skip) pos = std::min<size_t>(skip, buf.size()), skip = 0;
    const double t_f2 = np2h::now_ms();
    // 0: none; otherwise the first block (in file order) that failed: index + 1 in the low bits, bit 63 = its CRC (not its inflate)
    std::atomic<uint64_t> bad{0};
    const Inflater &inf = Inflater::get();
    const bool check_crc = bgzf_crc_on();
    auto one = [&](size_t i) {
        uint8_t *dst = buf.data() + base + blks[i].out_off;
        uint64_t why = 0;
        if (blks[i].isize && !inf.run(map + blks[i].file_off + blks[i].hdr_len, blks[i].clen, dst, blks[i].isize)) why = i + 1;
        else if (check_crc && inf.crc(dst, blks[i].isize) != blks[i].crc) why = (i + 1) | (1ull << 63);
        if (why) {
            uint64_t seen = bad.load();
            while ((!seen || (seen & ~(1ull << 63)) > i + 1) && !bad.compare_exchange_weak(seen, why)) {}
        }
        blk_done[i].store(1, std::memory_order_release); // (also after a failure: a reader must not wait forever)
    };
    auto throw_bad = [&]() {
        const uint64_t why = bad.load();
        if (why >> 63) throw np2h::Np2Error(NP2_E_ARG, crc_msg(blks[(size_t)(why & ~(1ull << 63)) - 1].file_off));
        throw np2h::Np2Error(NP2_E_ARG, "BGZF inflate failed");
    };
    const unsigned nt = (unsigned)std::max<size_t>(1, blks.size() / 2);
    try {
        if (during)
            IoPool::get().parallel_for_during(blks.size(), nt, one, *during);
        else
            IoPool::get().parallel_for(blks.size(), nt, one);
    } catch (...) {
        ready_end = buf.size();
        if (bad.load()) throw_bad(); // (what the reader tripped over)
        throw;
    }
    ready_bi = blks.size(), ready_end = buf.size();
    if (bad.load()) throw_bad();
    ms_drop += t_f1 - t_f0, ms_read += t_f2 - t_f1, ms_inflate += np2h::now_ms() - t_f2;
}

namespace {
// 4-bit SEQ nibble i (BAM: high nibble first)
inline uint8_t seq4_at(const uint8_t *s, uint32_t i) { return (i & 1) ? (s[i >> 1] & 15) : (s[i >> 1] >> 4); }
// reverse complement in the 4-bit domain: A(1)<->T(8), C(2)<->G(4), every other code unchanged
// (reverse_complement_seq_u8, secondary.rs:66-80, over the decoded letters "=ACMGRSVTWYHKDBN")
template <class V> void append_seq4(V &dst, const uint8_t *src, uint32_t len, bool revcomp) {
    const size_t base = dst.size();
    dst.resize(base + (len + 1) / 2, 0);
    for (uint32_t i = 0; i < len; ++i) {
        uint8_t c = seq4_at(src, revcomp ? len - 1 - i : i);
        if (revcomp) c = c == 1 ? 8 : (c == 8 ? 1 : (c == 2 ? 4 : (c == 4 ? 2 : c)));
        dst[base + (i >> 1)] |= (i & 1) ? c : (uint8_t)(c << 4);
    }
}

// retrieve_secondary_seq_from_bam (secondary.rs:8-148): pass 1 collects the names of all secondary records, pass 2
// the SEQ (read orientation) of the primary record (neither secondary nor supplementary) of each of those reads.
// Two sequential passes over the whole file, once per BAM handle.
void load_secondary_seqs(np2_bam *bam) {
    if (bam->sec_loaded) return;
    std::unordered_set<std::string> ids;
    for (int pass = 0; pass < 2; ++pass) {
        BgzfBatch z;
        z.map = bam->map, z.map_len = bam->map_len;
        z.seek(bam->first_rec);
        for (;;) {
            const uint8_t *h4 = z.take(4);
            if (!h4) break;
            const uint32_t bs = le32(h4);
            const uint8_t *rec = z.take(bs);
            if (!rec || bs < 32) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
            const uint32_t l_read_name = rec[8];
            const uint32_t n_cigar = rec[12] | (rec[13] << 8), flag = rec[14] | (rec[15] << 8);
            const uint32_t l_seq = le32(rec + 16);
            const uint8_t *ps = rec + 32 + l_read_name + (size_t)n_cigar * 4;
            if ((size_t)(ps - rec) + (l_seq + 1) / 2 > bs) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
            const std::string name((const char *)rec + 32, l_read_name ? l_read_name - 1 : 0); // qname without the NUL
            if (pass == 0) {
                if (flag & 0x100) ids.insert(name);
            } else if (!(flag & 0x900) && ids.count(name)) {
                SecSeq sq;
                sq.len = l_seq;
                append_seq4(sq.seq4, ps, l_seq, (flag & 0x10) != 0);
                if (!bam->sec.emplace(name, std::move(sq)).second) // assert!(seqs.insert(..).is_none()), secondary.rs:130
                    throw np2h::Np2Error(NP2_E_REFPANIC, "reference would panic: two primary records for one read name");
            }
        }
        if (ids.empty()) break;
    }
    bam->sec_loaded = true;
}
} // namespace

uint64_t zone_start_offset(const np2_bam *bam, int tid, uint32_t zone_lo) { return bai_zone_start(bam->lin[tid], bam->ref_start[tid], zone_lo); }

void fetch_records(np2_bam *bam, int tid, uint32_t L, uint32_t zone_lo, uint32_t zone_hi, const np2_front_opts_t *opts,
                   std::vector<np2_bamrec_t> &recs, std::vector<uint32_t> &cigar, std::vector<uint64_t> *voffs,
                   hipStream_t up_stream, uint64_t *seq_bytes, bool no_seq) {
        PinnedBytes &seq4 = bam->seq4;
        seq4.clear();
        const bool streamed = up_stream != nullptr && !opts->use_secondary;
        uint64_t seq_total = 0; // (streamed: the running SEQ offset that seq4.size() is otherwise)
        if (opts->use_secondary) load_secondary_seqs(bam);
        const uint64_t start_off = zone_start_offset(bam, tid, zone_lo);
        if (start_off != ~0ull) {
            BgzfBatch &z = bam->batch;
            z.map = bam->map, z.map_len = bam->map_len;
            z.seek(start_off, false);
            if (bam->ref_end[tid]) z.hint_fpos = (size_t)(bam->ref_end[tid] >> 16);
            if (streamed) {
                // SEQ is about a third of a record with qualities (half without), BAM deflates 3 - 6x: 2.5 bytes of SEQ per
                // compressed byte is rarely short (and a shortfall only costs one device-side copy)
                const uint64_t c_lo = start_off >> 16, c_hi = bam->ref_end[tid] ? (bam->ref_end[tid] >> 16) : (uint64_t)bam->map_len;
                double frac = 1.0;
                if (zone_lo > 0 || zone_hi < L) frac = std::min(1.0, ((double)zone_hi - zone_lo + 65536.0) / std::max<double>(1.0, L));
                bam->seqs.begin(up_stream, (uint64_t)((c_hi > c_lo ? (double)(c_hi - c_lo) : 0.0) * 2.5 * frac) + (32u << 20));
            }
            // Per refill (up to 128 MiB of inflated BAM, inflated in parallel): one light sequential walk over the record
            // length fields finds this contig's records — on this thread, WHILE the pool inflates, trailing the blocks as
            // they complete (10 k records = 10 k cache misses into lines other cores just wrote: 1.6 ms of an E. coli-sized
            // contig's 7.4 ms when it ran after the inflate) —, a prefix sum places their CIGAR words and SEQ bytes, and
            // the copies run in parallel (records are independent byte ranges).
            struct RecRef {
                size_t off; // first byte after the record's block_size field, inside z.buf
                uint32_t n_cigar, l_seq;
                uint64_t cigar_off, seq_off, voff;
            };
            std::vector<RecRef> rr;
            bool stop = false;
            while (!stop) {
                rr.clear();
                size_t p = 0;
                uint64_t co = cigar.size(), so = streamed ? seq_total : seq4.size();
                const uint64_t so0 = so;
                double t_walk = 0;
                const std::function<void()> walk = [&]() {
                const double t_w0 = np2h::now_ms();
                p = z.pos;
                while (z.wait_ready(p + 4)) {
                    const uint32_t bs = le32(z.buf.data() + p);
                    if (bs < 32) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
                    if (!z.wait_ready(p + 4 + (size_t)bs)) break; // the record continues in the next refill
                    const uint8_t *rec = z.buf.data() + p + 4;
                    const int32_t refID = (int32_t)le32(rec);
                    if (refID != tid) {
                        if (refID > tid || refID < 0) {
                            stop = true;
                            break;
                        }
                        p += 4 + (size_t)bs;
                        continue;
                    }
                    const int32_t pos = (int32_t)le32(rec + 4);
                    if (pos >= 0 && (uint32_t)pos >= zone_hi) { // coordinate-sorted: nothing further overlaps the zone
                        stop = true;
                        break;
                    }
                    bool take = (uint32_t)pos < L; // (fetch(tid, 0, len): records starting beyond the region are skipped)
                    if (take && zone_lo > 0) { // reference end from the CIGAR: the record must reach the zone
                        const uint32_t nc = rec[12] | (rec[13] << 8);
                        const uint8_t *pc0 = rec + 32 + rec[8];
                        if ((size_t)32 + rec[8] + (size_t)nc * 4 > bs) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
                        take = (uint64_t)pos + ref_span(pc0, nc) > zone_lo;
                    }
                    if (take) {
                        const uint32_t n_cigar = rec[12] | (rec[13] << 8), flag = rec[14] | (rec[15] << 8), l_seq = le32(rec + 16);
                        if ((size_t)32 + rec[8] + (size_t)n_cigar * 4 + ((size_t)l_seq + 1) / 2 > bs) throw np2h::Np2Error(NP2_E_ARG, "BAM/SAM parsing failed!");
                        rr.push_back(RecRef{p + 4, n_cigar, l_seq, co, so, z.voffset_at(p)});
                        co += n_cigar;
                        if (!no_seq && !(opts->use_secondary && (flag & 0x100))) so += ((uint64_t)l_seq + 1) / 2;
                    }
                    p += 4 + (size_t)bs;
                }
                t_walk = np2h::now_ms() - t_w0;
                };
                z.fill(z.batch_blocks, &walk);
                const double t_w1 = np2h::now_ms();
                const size_t r0 = recs.size();
                recs.resize(r0 + rr.size());
                if (voffs)
                    for (auto &q : rr) voffs->push_back(q.voff);
                cigar.resize(co);
                uint8_t *seq_dst = nullptr; // where SEQ byte offset so0 of this batch goes
                if (streamed) seq_dst = bam->seqs.piece((size_t)(so - so0));
                else if (!opts->use_secondary) {
                    seq4.resize(so);
                    seq_dst = seq4.data() + so0;
                }
                const double t_w2 = np2h::now_ms();
                z.ms_walk += t_walk, z.ms_size += t_w2 - t_w1;
                // record q but for its SEQ: the fixed fields, its CIGAR words to their place; -> its SEQ bytes in the buffer
                auto record = [&](const RecRef &q, np2_bamrec_t &r) {
                    const uint8_t *rec = z.buf.data() + q.off, *pc = rec + 32 + rec[8];
                    memset(&r, 0, sizeof r);
                    r.pos = (int32_t)le32(rec + 4);
                    r.flag = (uint16_t)(rec[14] | (rec[15] << 8));
                    r.mapq = rec[9];
                    r.n_cigar = q.n_cigar;
                    r.cigar_off = q.cigar_off;
                    r.l_seq = q.l_seq;
                    for (uint32_t k = 0; k < q.n_cigar; ++k) cigar[q.cigar_off + k] = le32(pc + 4 * k);
                    return pc + (size_t)q.n_cigar * 4;
                };
                if (!opts->use_secondary) {
                    IoPool::get().parallel_for(rr.size(), 64, [&](size_t i) {
                        const RecRef &q = rr[i];
                        const uint8_t *ps = record(q, recs[r0 + i]);
                        recs[r0 + i].seq_off = q.seq_off;
                        if (!no_seq) memcpy(seq_dst + (q.seq_off - so0), ps, ((size_t)q.l_seq + 1) / 2);
                    });
                    if (streamed) {
                        bam->seqs.push((size_t)(so - so0));
                        seq_total = so;
                    }
                } else {
                    for (size_t i = 0; i < rr.size(); ++i) { // -S: secondary records take their SEQ from the primary's
                        const RecRef &q = rr[i];
                        np2_bamrec_t &r = recs[r0 + i];
                        const uint8_t *ps = record(q, r), *rec = z.buf.data() + q.off;
                        r.seq_off = seq4.size();
                        if (r.flag & 0x100) {
                            // SEQ of the read's primary alignment, reverse-complemented again if this record is on the
                            // reverse strand (main.rs:1775-1784).  A missing name leaves l_seq = 0: the reference would only
                            // panic if the record passes the admission filters, and so do we (np2_contig_from_records).
                            const auto it = bam->sec.find(std::string((const char *)rec + 32, rec[8] ? rec[8] - 1 : 0));
                            r.l_seq = 0;
                            if (it != bam->sec.end()) {
                                r.l_seq = it->second.len;
                                append_seq4(seq4, it->second.seq4.data(), it->second.len, (r.flag & 0x10) != 0);
                            }
                        } else seq4.append(ps, ((size_t)q.l_seq + 1) / 2);
                    }
                }
                z.ms_copy += np2h::now_ms() - t_w2;
                z.pos = p;
                if (stop) break;
                if (z.eof) {
                    if (z.pos != z.buf.size()) throw np2h::Np2Error(NP2_E_ARG, "truncated BAM");
                    break;
                }
            }
        }
    if (streamed) {
        if (start_off == ~0ull) bam->seqs.begin(up_stream, 0);
        bam->seqs.finish();
        if (seq_bytes) *seq_bytes = bam->seqs.n;
    } else {
        seq4.resize(seq4.size() + 16, 0);
        if (seq_bytes) *seq_bytes = seq4.size();
    }
}

int ref_id(const np2_bam *bam, const char *name) {
    for (size_t i = bam->ref_names.size(); i-- > 0;)
        if (bam->ref_names[i] == name) return (int)i;
    throw np2h::Np2Error(NP2_E_ARG, std::string("Faield random access BAM/SAM! (contig not in the BAM header: ") + name + ")");
}

} // namespace np2h

extern "C" {

// ---- the handle ----------------------------------------------------------------------------------------
int np2_bam_open(const char *path, np2_bam_t **out) {
    return np2h::abi_guard([&] {
        std::unique_ptr<np2_bam> b(new np2_bam());
        b->z.f = fopen(path, "rb");
        if (!b->z.f) throw np2h::Np2Error(NP2_E_ARG, std::string("cannot open ") + path);
        struct stat st;
        if (fstat(fileno(b->z.f), &st) != 0) throw np2h::Np2Error(NP2_E_ARG, std::string("cannot stat ") + path);
        b->z.flen = b->map_len = (size_t)st.st_size;
        uint8_t h8[8];
        if (!b->z.read(h8, 8) || memcmp(h8, "BAM\1", 4) != 0) throw np2h::Np2Error(NP2_E_ARG, "not a BAM file");
        const uint32_t l_text = le32(h8 + 4);
        std::vector<uint8_t> text(l_text + 1);
        if (l_text) b->z.read(text.data(), l_text);
        uint8_t h4[4];
        b->z.read(h4, 4);
        const uint32_t n_ref = le32(h4);
        for (uint32_t i = 0; i < n_ref; ++i) {
            b->z.read(h4, 4);
            const uint32_t l_name = le32(h4);
            std::vector<char> nm(l_name + 1, 0);
            b->z.read(nm.data(), l_name);
            b->z.read(h4, 4);
            b->ref_names.emplace_back(nm.data());
            b->ref_lens.push_back(le32(h4));
        }
        b->ref_start.assign(n_ref, ~0ull);
        b->ref_end.assign(n_ref, 0);
        b->lin.assign(n_ref, {});
        b->first_rec = b->z.tell();
        void *m = b->map_len ? mmap(nullptr, b->map_len, PROT_READ, MAP_SHARED, fileno(b->z.f), 0) : nullptr;
        if (m == MAP_FAILED) throw np2h::Np2Error(NP2_E_NOMEM, std::string("cannot map ") + path);
        b->map = (const uint8_t *)m;
        // index: <path>.bai or <stem>.bai
        std::string p1 = std::string(path) + ".bai", p2 = path;
        if (p2.size() > 4 && p2.substr(p2.size() - 4) == ".bam") p2 = p2.substr(0, p2.size() - 4) + ".bai";
        std::unique_ptr<FILE, int (*)(FILE *)> fi(fopen(p1.c_str(), "rb"), fclose);
        if (!fi) fi.reset(fopen(p2.c_str(), "rb"));
        if (!fi) throw np2h::Np2Error(NP2_E_ARG, "Faield random access BAM/SAM! (no .bai index)");
        std::vector<uint8_t> idx;
        fseeko(fi.get(), 0, SEEK_END);
        idx.resize((size_t)ftello(fi.get()));
        fseeko(fi.get(), 0, SEEK_SET);
        if (fread(idx.data(), 1, idx.size(), fi.get()) != idx.size()) throw np2h::Np2Error(NP2_E_ARG, "cannot read the .bai index");
        fi.reset();
        np2h::BaiIndex bi;
        if (const char *why = np2h::bai_parse(idx.data(), idx.size(), n_ref, bi)) throw np2h::Np2Error(NP2_E_ARG, why);
        b->ref_start = std::move(bi.ref_start), b->ref_end = std::move(bi.ref_end), b->lin = std::move(bi.lin);
        *out = b.release();
        return NP2_OK;
    }, np2h::io_set_error);
}
void np2_bam_close(np2_bam_t *b) { delete b; }
int np2_bam_n_refs(np2_bam_t *b) { return b ? (int)b->ref_names.size() : 0; }
const char *np2_bam_ref_name(np2_bam_t *b, int tid, uint32_t *len) {
    if (!b || tid < 0 || (size_t)tid >= b->ref_names.size()) return nullptr;
    if (len) *len = b->ref_lens[tid];
    return b->ref_names[tid].c_str();
}
}
