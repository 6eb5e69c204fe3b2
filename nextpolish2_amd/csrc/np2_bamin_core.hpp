// Per-record rule of BAM input (include/np2_io.h: "BAM input"; kernels: np2_bamin.hip): what a record of an inflated BAM stream
// must look like, whether it is kept, and what it becomes in the resident arrays that the SAM text path fills.  Plain integer
// arithmetic without HIP types, as np2_samtail_core.hpp: the same text is the kernels' inner step and the host twin
// (np2_bamin_host), which walks the stream with one lane.  Host only, at the end: the binary header and the twin itself.
//
// A record at p: block_size u32, then refID i32 @4, pos i32 @8, l_read_name u8 @12, mapq u8 @13, bin u16 @14, n_cigar_op u16 @16,
// flag u16 @18, l_seq u32 @20, next_refID i32 @24, next_pos i32 @28, tlen i32 @32, the name with its NUL @36, the CIGAR words,
// (l_seq + 1) / 2 SEQ bytes, l_seq quality bytes, and the optional fields up to 4 + block_size.
#pragma once
#include <cstdint>

#include "np2_samtail_core.hpp"

namespace np2bamin {

static constexpr uint32_t FIXED = 32;      // bytes of the fixed fields behind block_size
static constexpr uint32_t KEEP_NAMES = 1u; // NP2_SAM_KEEP_NAMES
static constexpr uint32_t KEEP_ALL = 2u;   // NP2_SAM_KEEP_ALL

// what is wrong with a record: the `where` code.  Of several in one record the smallest speaks.  W_CG and W_PIECE are
// NP2_E_UNSUPPORTED, the others NP2_E_ARG.  Up to W_REFID the record's other fields cannot be looked at.
enum : uint32_t {
    W_OK = 0, W_SHORT, W_OVERRUN, W_REFID, W_POS, W_CIGAR, W_CG, W_NAME, W_NEXT_REFID, W_NEXT_POS, W_QUAL, W_AUX, W_TRUNC, W_GARBAGE, W_PIECE
};
inline const char *where_text(uint32_t w) {
    switch (w) {
    case W_SHORT: return "block_size is below 32: not a record";
    case W_OVERRUN: return "the name, CIGAR, SEQ and quality bytes overrun block_size";
    case W_REFID: return "refID is neither -1 nor the number of a reference";
    case W_POS: return "pos is below -1";
    case W_CIGAR: return "a CIGAR operation is not one of MIDNSHP=X";
    case W_CG: return "the CIGAR is the placeholder of a CG tag (l_seq S, then N): long CIGARs are not supported";
    case W_NAME: return "the read name is not 1..254 bytes with a NUL behind them";
    case W_NEXT_REFID: return "next_refID is neither -1 nor the number of a reference";
    case W_NEXT_POS: return "next_pos is below -1";
    case W_QUAL: return "a quality byte is above 93 (and not all of them are 0xFF)";
    case W_AUX: return "the optional fields do not end at the record's end";
    case W_TRUNC: return "truncated BAM: the stream ends inside the record";
    case W_GARBAGE: return "fewer than 4 bytes behind the last record: not a record";
    case W_PIECE: return "the record does not fit a piece";
    }
    return "ok";
}
NP2_SAM_HD bool where_unsupported(uint32_t w) { return w == W_CG || w == W_PIECE; }
NP2_SAM_HD bool structural(uint32_t w) { return w >= W_SHORT && w <= W_REFID; }
NP2_SAM_HD uint32_t first(uint32_t a, uint32_t b) { return a == W_OK ? b : b == W_OK ? a : a < b ? a : b; }

NP2_SAM_HD uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
NP2_SAM_HD uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }

// the fixed fields of a record, and where its parts lie (offsets from the block_size word)
struct Rec {
    uint32_t block_size, l_name, n_cigar, l_seq, flag, mapq;
    int32_t tid, pos, next_tid, next_pos, tlen;
    uint32_t cig_at, seq_at, qual_at, aux_at, aux_len;
    bool kept;
};
NP2_SAM_HD uint32_t seq_bytes(const Rec &r) { return (r.l_seq + 1u) / 2u; }
NP2_SAM_HD uint32_t tail_size(const Rec &r, bool has_qual) { return np2tail::HEAD_BYTES + (has_qual ? r.l_seq : 0u) + r.aux_len; }

// The record at p, whose 4 + block_size bytes are all there.  Returns the first of W_SHORT, W_OVERRUN, W_REFID (r->kept is then
// false and the rest of *r is not to be used), else the first of the checks of single fields that `flags` asks for; a record
// that is not kept is looked at no further (W_OK).  CIGAR operations, quality bytes and optional fields are the caller's
// (cigar_word_ok, qual_kind, aux_ok): a wavefront spreads them over its lanes.
NP2_SAM_HD uint32_t fixed(const uint8_t *p, uint32_t n_ref, uint32_t flags, Rec *r) {
    r->kept = false;
    r->block_size = rd32(p);
    if (r->block_size < FIXED) return W_SHORT;
    r->tid = (int32_t)rd32(p + 4), r->pos = (int32_t)rd32(p + 8), r->l_name = p[12], r->mapq = p[13], r->n_cigar = rd16(p + 16);
    r->flag = rd16(p + 18), r->l_seq = rd32(p + 20);
    r->next_tid = (int32_t)rd32(p + 24), r->next_pos = (int32_t)rd32(p + 28), r->tlen = (int32_t)rd32(p + 32);
    const uint64_t need = (uint64_t)FIXED + r->l_name + 4ull * r->n_cigar + ((uint64_t)r->l_seq + 1u) / 2u + r->l_seq;
    if (need > r->block_size) return W_OVERRUN;
    r->cig_at = 4u + FIXED + r->l_name, r->seq_at = r->cig_at + 4u * r->n_cigar, r->qual_at = r->seq_at + (r->l_seq + 1u) / 2u;
    r->aux_at = r->qual_at + r->l_seq, r->aux_len = r->block_size - (uint32_t)need;
    if (r->tid < -1 || (r->tid >= 0 && (uint32_t)r->tid >= n_ref)) return W_REFID;
    r->kept = r->tid >= 0 && !(r->flag & 4u);
    if (!r->kept) return W_OK;
    uint32_t w = W_OK;
    if (r->pos < -1) w = first(w, W_POS);
    if (r->n_cigar == 2u && rd32(p + r->cig_at) == (r->l_seq << 4 | 4u) && (rd32(p + r->cig_at + 4u) & 15u) == 3u) w = first(w, W_CG);
    if ((flags & (KEEP_NAMES | KEEP_ALL)) && (r->l_name < 2u || p[4u + FIXED + r->l_name - 1u] != 0)) w = first(w, W_NAME);
    if (flags & KEEP_ALL) {
        if (r->next_tid < -1 || (r->next_tid >= 0 && (uint32_t)r->next_tid >= n_ref)) w = first(w, W_NEXT_REFID);
        if (r->next_pos < -1) w = first(w, W_NEXT_POS);
    }
    return w;
}
NP2_SAM_HD bool cigar_word_ok(uint32_t w) { return (w & 15u) <= 8u; }
// the quality bytes: n_ff of the l_seq are 0xFF, n_high others are above 93.  *has_qual: they are carried
NP2_SAM_HD uint32_t qual_kind(uint32_t l_seq, uint32_t n_ff, uint32_t n_high, bool *has_qual) {
    *has_qual = false;
    if (l_seq == 0u || n_ff == l_seq) return W_OK;
    if (n_ff || n_high) return W_QUAL;
    *has_qual = true;
    return W_OK;
}
// the optional fields a[0, n), walked by one lane: do they end exactly at n?
NP2_SAM_HD bool aux_ok(const uint8_t *a, uint32_t n) {
    uint32_t i = 0;
    while (i < n) {
        if (n - i < 3u) return false;
        const uint8_t t = a[i + 2];
        i += 3u;
        uint32_t k = 0;
        switch (t) {
        case 'A': case 'c': case 'C': k = 1; break;
        case 's': case 'S': k = 2; break;
        case 'i': case 'I': case 'f': k = 4; break;
        case 'Z': case 'H':
            while (i < n && a[i]) ++i;
            if (i >= n) return false;
            ++i;
            continue;
        case 'B': {
            if (n - i < 5u) return false;
            const uint8_t sub = a[i];
            if (!(sub == 'c' || sub == 'C' || sub == 's' || sub == 'S' || sub == 'i' || sub == 'I' || sub == 'f')) return false;
            const uint64_t bytes = (uint64_t)rd32(a + i + 1) * np2tail::type_bytes(sub);
            i += 5u;
            if (bytes > n - i) return false;
            i += (uint32_t)bytes;
            continue;
        }
        default: return false;
        }
        if (n - i < k) return false;
        i += k;
    }
    return true;
}
// byte j of the record's packed SEQ as it is kept: the low nibble of an odd last byte is 0
NP2_SAM_HD uint8_t seq_byte(const uint8_t *p, const Rec &r, uint32_t j) {
    const uint8_t b = p[r.seq_at + j];
    return (r.l_seq & 1u) && j == r.l_seq / 2u ? (uint8_t)(b & 0xF0u) : b;
}
// the ten words of np2_bamrec_t, padding included
NP2_SAM_HD uint32_t rec_word(const Rec &r, uint64_t cigar_off, uint64_t seq_off, uint32_t j) {
    switch (j) {
    case 0: return (uint32_t)r.pos;
    case 1: return r.flag | r.mapq << 16;
    case 2: return r.n_cigar;
    case 4: return (uint32_t)cigar_off;
    case 5: return (uint32_t)(cigar_off >> 32);
    case 6: return r.l_seq;
    case 8: return (uint32_t)seq_off;
    case 9: return (uint32_t)(seq_off >> 32);
    }
    return 0u;
}

// One lane's judgement of the whole record at p (all of it is there): the `where` code, *r and *has_qual.
NP2_SAM_HD uint32_t judge(const uint8_t *p, uint32_t n_ref, uint32_t flags, Rec *r, bool *has_qual) {
    *has_qual = false;
    uint32_t w = fixed(p, n_ref, flags, r);
    if (structural(w) || !r->kept) return w;
    for (uint32_t j = 0; j < r->n_cigar; ++j)
        if (!cigar_word_ok(rd32(p + r->cig_at + 4u * j))) w = first(w, W_CIGAR);
    if (flags & KEEP_ALL) {
        uint32_t n_ff = 0, n_high = 0;
        for (uint32_t j = 0; j < r->l_seq; ++j) {
            const uint8_t q = p[r->qual_at + j];
            n_ff += q == 0xFFu ? 1u : 0u, n_high += q != 0xFFu && q > 93u ? 1u : 0u;
        }
        w = first(w, qual_kind(r->l_seq, n_ff, n_high, has_qual));
        if (!aux_ok(p + r->aux_at, r->aux_len)) w = first(w, W_AUX);
    }
    return w;
}

} // namespace np2bamin

// ---- host only: the binary header and the twin -----------------------------------------------------------------------------
#include <cstring>
#include <string>
#include <vector>

#include "../../include/np2_io.h"

namespace np2bamin {

// The header of the inflated stream s[0, n): "BAM\1", l_text, text, n_ref, then per reference l_name, name with NUL, l_ref.
// 0: it is complete: refs, the text's lines other than @HD and @SQ (as the SAM reader carries them) and *end, where the first
// record begins.  1: more bytes are needed.  Anything else: *bad says what is wrong.
inline int parse_header(const uint8_t *s, uint64_t n, np2sam::Refs *refs, std::vector<std::string> *extra, uint64_t *end, std::string *bad) {
    refs->names.clear(), refs->lens.clear(), extra->clear();
    if (n < 12) return 1;
    if (memcmp(s, "BAM\1", 4) != 0) return *bad = "no BAM magic", 2;
    const uint64_t l_text = rd32(s + 4);
    if (n < 12 + l_text) return 1;
    const uint32_t n_ref = rd32(s + 8 + l_text);
    if (n_ref >= (1u << 31)) return *bad = "a negative number of references", 2;
    uint64_t at = 12 + l_text;
    for (uint32_t i = 0; i < n_ref; ++i) {
        if (n < at + 4) return 1;
        const uint64_t l_name = rd32(s + at);
        if (l_name < 2 || l_name > (1u << 20)) return *bad = "reference " + std::to_string(i) + " has an empty or an overlong name", 2;
        if (n < at + 4 + l_name + 4) return 1;
        if (s[at + 4 + l_name - 1] != 0) return *bad = "the name of reference " + std::to_string(i) + " has no NUL", 2;
        std::string name((const char *)s + at + 4);
        if (name.size() != l_name - 1) return *bad = "the name of reference " + std::to_string(i) + " has a NUL inside", 2;
        for (const std::string &o : refs->names)
            if (o == name) return *bad = "the reference name " + name + " is given twice", 2;
        refs->names.push_back(name), refs->lens.push_back(rd32(s + at + 4 + l_name));
        at += 4 + l_name + 4;
    }
    for (uint64_t a = 8, te = 8 + l_text; a < te;) { // the text's lines, a trailing NUL padding left aside
        uint64_t nl = a;
        while (nl < te && s[nl] != '\n' && s[nl] != 0) ++nl;
        const uint64_t e = nl > a && s[nl - 1] == '\r' ? nl - 1 : nl;
        if (e > a && s[a] == '@' && np2sam::header_line_is_carried(s, a, e)) {
            std::string line((const char *)s + a, e - a);
            bool seen = false;
            for (const std::string &o : *extra) seen = seen || o == line;
            if (!seen) extra->push_back(std::move(line));
        }
        if (nl < te && s[nl] == 0) break;
        a = nl + 1;
    }
    *end = at;
    return 0;
}

// What the twin gives: per record of the stream, in input order, status (0 kept, 1 not kept, else NP2_E_ARG or
// NP2_E_UNSUPPORTED) and the `where` code; of the kept records the arrays of the resident handle, in input order.
struct Twin {
    np2sam::Refs refs;
    std::vector<std::string> extra;
    std::vector<int32_t> status;
    std::vector<uint32_t> where;
    std::vector<np2_bamrec_t> recs;
    std::vector<int32_t> tids;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> seq4, names, tails;
    std::vector<uint64_t> name_ref, tail_ref;
    int64_t speaks = -1; // the first refused record
};
inline int where_status(uint32_t w) { return where_unsupported(w) ? NP2_E_UNSUPPORTED : NP2_E_ARG; }

// The inflated stream s[0, n), header included, walked by one lane.  Returns 0, or what parse_header says of a bad or an
// unfinished header (*bad).  A stream that ends inside a record, or with fewer than 4 bytes behind the last one, gets a last
// entry with W_TRUNC or W_GARBAGE; so does a block_size below 32 (W_SHORT), behind which nothing can be found.
inline int twin(const uint8_t *s, uint64_t n, uint32_t flags, uint32_t tie_by_strand, Twin *t, std::string *bad) {
    uint64_t at = 0;
    const int h = parse_header(s, n, &t->refs, &t->extra, &at, bad);
    if (h == 1) *bad = "truncated BAM: the stream ends inside the header";
    if (h) return h;
    const uint32_t n_ref = (uint32_t)t->refs.names.size();
    auto refuse = [&](uint32_t w) {
        if (t->speaks < 0) t->speaks = (int64_t)t->status.size();
        t->status.push_back(where_status(w)), t->where.push_back(w);
    };
    while (at < n) {
        if (n - at < 4) {
            refuse(W_GARBAGE);
            break;
        }
        const uint32_t bs = rd32(s + at);
        if (bs < FIXED) {
            refuse(W_SHORT);
            break;
        }
        if (4ull + bs > n - at) {
            refuse(W_TRUNC);
            break;
        }
        const uint8_t *p = s + at;
        Rec r;
        bool hq = false;
        const uint32_t w = judge(p, n_ref, flags, &r, &hq);
        at += 4ull + bs;
        if (w != W_OK) {
            refuse(w);
            continue;
        }
        t->status.push_back(r.kept ? 0 : 1), t->where.push_back(W_OK);
        if (!r.kept) continue;
        np2_bamrec_t o;
        memset(&o, 0, sizeof o);
        o.pos = r.pos, o.flag = (uint16_t)r.flag, o.mapq = (uint8_t)r.mapq, o.n_cigar = r.n_cigar, o.cigar_off = t->cigar.size();
        o.l_seq = r.l_seq, o.seq_off = t->seq4.size();
        t->recs.push_back(o), t->tids.push_back(r.tid), t->keys.push_back(np2sam::sort_key(r.tid, r.pos, r.flag, tie_by_strand));
        for (uint32_t j = 0; j < r.n_cigar; ++j) t->cigar.push_back(rd32(p + r.cig_at + 4u * j));
        for (uint32_t j = 0; j < seq_bytes(r); ++j) t->seq4.push_back(seq_byte(p, r, j));
        if (flags & (KEEP_NAMES | KEEP_ALL)) {
            t->name_ref.push_back((uint64_t)t->names.size() << 8 | (r.l_name - 1u));
            t->names.insert(t->names.end(), p + 36, p + 36 + r.l_name - 1u);
        }
        if (flags & KEEP_ALL) {
            t->tail_ref.push_back(np2tail::tail_ref(t->tails.size(), hq));
            uint8_t head[np2tail::HEAD_BYTES];
            np2tail::put(head, (uint32_t)r.next_tid, 4u), np2tail::put(head + 4, (uint32_t)r.next_pos, 4u);
            np2tail::put(head + 8, (uint32_t)r.tlen, 4u), np2tail::put(head + 12, r.aux_len, 4u);
            t->tails.insert(t->tails.end(), head, head + np2tail::HEAD_BYTES);
            if (hq) t->tails.insert(t->tails.end(), p + r.qual_at, p + r.qual_at + r.l_seq);
            t->tails.insert(t->tails.end(), p + r.aux_at, p + r.aux_at + r.aux_len);
            while (t->tails.size() & 3u) t->tails.push_back(0);
        }
    }
    return 0;
}
// what a refused record's message says behind the file's name
inline std::string record_message(uint64_t record, uint32_t w) { return "record " + std::to_string(record) + ": " + where_text(w); }

} // namespace np2bamin
