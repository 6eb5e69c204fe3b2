// Host side of BAM input (include/np2_io.h: "BAM input"): telling a BAM from SAM text, reading a BAM's header with zlib, the
// host twin np2_bamin_host, which runs the one-lane text of the rule (np2_bamin_core.hpp: twin) and uses no device, and
// np2_sam_bamin_stats.  The device path is part of the SAM reader's driver (np2_sam_host.cpp); the kernels are np2_bamin.hip.
#include "../../include/np2_io.h"
#include "np2_bamfile.hpp"
#include "np2_bamin_core.hpp"
#include "np2_bgzf.hpp"
#include "np2_sam_handle.hpp"

#include <zlib.h>

namespace np2h {

bool is_bam_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> buf(65536);
    const size_t got = fread(buf.data(), 1, buf.size(), f);
    fclose(f);
    try {
        uint8_t out[4];
        size_t have = 0; // (the first blocks may hold fewer than four bytes, or none)
        for (size_t at = 0; have < 4 && at < got;) {
            const BgzfHeader h = bgzf_header(buf.data() + at, got - at, got - at);
            if (h.need || h.bsize > got - at) return false;
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) return false;
            zs.next_in = buf.data() + at + h.hdr_len, zs.avail_in = h.clen, zs.next_out = out + have, zs.avail_out = (uInt)(4 - have);
            (void)inflate(&zs, Z_SYNC_FLUSH);
            have = 4 - zs.avail_out;
            inflateEnd(&zs);
            at += h.bsize;
        }
        return have == 4 && memcmp(out, "BAM\1", 4) == 0;
    } catch (const Np2Error &) {
        return false;
    }
}

void bam_read_header(int fd, uint64_t file_len, const std::string &name, np2sam::Refs &refs, std::vector<std::string> &extra, uint64_t *first_block,
                     uint32_t *skip) {
    std::vector<uint8_t> inf, raw;
    std::vector<uint64_t> blk_off, blk_at; // of each block read: its file offset, and where its bytes begin in `inf`
    uint64_t off = 0;
    for (;;) {
        uint64_t end = 0;
        std::string bad;
        const int h = np2bamin::parse_header(inf.data(), inf.size(), &refs, &extra, &end, &bad);
        if (h == 0) {
            *first_block = off, *skip = 0; // (the header ends with its last block)
            for (size_t b = 0; b < blk_off.size(); ++b)
                if (end >= blk_at[b] && end < (b + 1 < blk_at.size() ? blk_at[b + 1] : inf.size())) *first_block = blk_off[b], *skip = (uint32_t)(end - blk_at[b]);
            return;
        }
        if (h != 1) throw Np2Error(NP2_E_ARG, name + ": the BAM header: " + bad);
        if (off >= file_len) throw Np2Error(NP2_E_ARG, name + ": truncated BAM: the file ends inside the header");
        try {
            raw.resize(18);
            if (file_len - off < 18 || !pread_full(fd, raw.data(), 18, off)) throw Np2Error(NP2_E_ARG, "truncated BGZF header");
            BgzfHeader bh = bgzf_header(raw.data(), 18, file_len - off);
            if (bh.need) {
                raw.resize(bh.need);
                if (!pread_full(fd, raw.data(), bh.need, off)) throw Np2Error(NP2_E_ARG, "truncated BGZF header");
                bh = bgzf_header(raw.data(), bh.need, file_len - off);
            }
            raw.resize(bh.bsize);
            if (!pread_full(fd, raw.data(), bh.bsize, off)) throw Np2Error(NP2_E_ARG, "truncated BGZF block");
            const BgzfTrailer t = bgzf_trailer(raw.data() + bh.bsize - 8);
            if (t.isize > 65536) throw Np2Error(NP2_E_ARG, "a BGZF block of more than 65536 bytes");
            const size_t at = inf.size();
            inf.resize(at + t.isize);
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) throw Np2Error(NP2_E_NOMEM, "zlib: inflateInit2 failed");
            zs.next_in = raw.data() + bh.hdr_len, zs.avail_in = bh.clen, zs.next_out = inf.data() + at, zs.avail_out = t.isize;
            const int rc = inflate(&zs, Z_FINISH);
            const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
            inflateEnd(&zs);
            if (!ok) throw Np2Error(NP2_E_ARG, "BGZF inflate failed (block at file offset " + std::to_string(off) + ")");
            if (bgzf_crc_on() && (uint32_t)crc32(crc32(0L, Z_NULL, 0), inf.data() + at, t.isize) != t.crc) throw Np2Error(NP2_E_ARG, crc_msg(off));
            blk_off.push_back(off), blk_at.push_back(at);
            off += bh.bsize;
        } catch (const Np2Error &e) {
            throw Np2Error(e.code, name + ": " + e.what());
        }
    }
}

} // namespace np2h

namespace {
using np2h::Np2Error;
template <class T> T *give(const std::vector<T> &v, std::vector<void *> &mine) { // a malloc'ed copy, NULL for none
    if (v.empty()) return nullptr;
    T *p = (T *)malloc(v.size() * sizeof(T));
    if (!p) throw Np2Error(NP2_E_NOMEM, "np2_bamin_host: out of memory");
    memcpy((void *)p, (const void *)v.data(), v.size() * sizeof(T));
    mine.push_back(p);
    return p;
}
} // namespace

extern "C" {

int np2_bamin_host(const uint8_t *stream, uint64_t n, uint32_t flags, const np2_sam_opts_t *opts, int32_t **status, uint32_t **where,
                   uint64_t *n_records, np2_bamrec_t **recs, int32_t **tids, uint32_t **cigar, uint64_t *n_cigar_words, uint8_t **seq4,
                   uint64_t *seq_bytes, uint8_t **names, uint64_t *name_bytes, uint64_t **name_ref, uint8_t **tails, uint64_t *tail_bytes,
                   uint64_t **tail_ref, uint64_t *n_kept) {
    std::vector<void *> mine;
    return np2h::abi_guard([&] {
        if (!status || !where || !n_records || !recs || !tids || !cigar || !n_cigar_words || !seq4 || !seq_bytes || !names || !name_bytes ||
            !name_ref || !tails || !tail_bytes || !tail_ref || !n_kept || (n && !stream))
            throw Np2Error(NP2_E_ARG, "np2_bamin_host: NULL argument");
        *status = nullptr, *where = nullptr, *recs = nullptr, *tids = nullptr, *cigar = nullptr, *seq4 = nullptr, *names = nullptr;
        *name_ref = nullptr, *tails = nullptr, *tail_ref = nullptr;
        *n_records = *n_cigar_words = *seq_bytes = *name_bytes = *tail_bytes = *n_kept = 0;
        if (flags & ~(uint32_t)(NP2_SAM_KEEP_NAMES | NP2_SAM_KEEP_ALL)) throw Np2Error(NP2_E_ARG, "np2_bamin_host: unknown flag bits");
        np2bamin::Twin t;
        std::string bad;
        static const uint8_t none = 0;
        if (np2bamin::twin(n ? stream : &none, n, flags, opts ? (opts->tie_by_strand ? 1u : 0u) : 1u, &t, &bad)) throw Np2Error(NP2_E_ARG, "the stream: " + bad);
        *status = give(t.status, mine), *where = give(t.where, mine), *recs = give(t.recs, mine), *tids = give(t.tids, mine);
        *cigar = give(t.cigar, mine), *seq4 = give(t.seq4, mine), *names = give(t.names, mine), *name_ref = give(t.name_ref, mine);
        *tails = give(t.tails, mine), *tail_ref = give(t.tail_ref, mine);
        *n_records = t.status.size(), *n_cigar_words = t.cigar.size(), *seq_bytes = t.seq4.size(), *name_bytes = t.names.size();
        *tail_bytes = t.tails.size(), *n_kept = t.recs.size();
        mine.clear();
        if (t.speaks >= 0) return np2h::io_set_error(t.status[t.speaks], "the stream: " + np2bamin::record_message((uint64_t)t.speaks, t.where[t.speaks]));
        return (int)NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (!mine.empty()) // (out of memory half way: nothing is handed out)
            *status = nullptr, *where = nullptr, *recs = nullptr, *tids = nullptr, *cigar = nullptr, *seq4 = nullptr, *names = nullptr, *name_ref = nullptr,
            *tails = nullptr, *tail_ref = nullptr;
        for (void *p : mine) free(p);
        np2h::io_set_error(code, msg);
    });
}

int np2_sam_bamin_stats(np2_sam_t *sam, np2_bamin_stats_t *stats) {
    if (!sam || !stats) return NP2_E_ARG;
    *stats = sam->bamin;
    return NP2_OK;
}

} // extern "C"
