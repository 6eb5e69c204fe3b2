// Per-lane logic of the SAM reader (np2_sam.hip; the rule is in include/np2_io.h): decimal runs, CIGAR letters and words, the
// SEQ base table, the @SQ name table and the sort key; and, host only, the header lines.  Plain integer arithmetic without
// HIP types: the same text is the kernels' inner step and a one-lane host program (tests/tools/sam_core_test.cpp), which
// walks a line with parse_line below the way a wavefront does with its 64 lanes.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NP2_SAM_HD __host__ __device__ __forceinline__
#else
#define NP2_SAM_HD inline
#endif

namespace np2sam {

// why a line is refused (all NP2_E_ARG); of several on one line the smallest speaks
enum : uint32_t { OK = 0, E_HEADER_LATE = 1, E_FIELDS = 2, E_FLAG = 3, E_RNAME = 4, E_POS = 5, E_MAPQ = 6, E_CIGAR = 7 };
static constexpr uint32_t N_TABS = 10;                // tabs in front of and behind the ten fields that are looked at
static constexpr uint32_t CIGAR_LEN_END = 1u << 28;   // an operation's length stays below it
static constexpr int32_t TID_NONE = -1, TID_UNKNOWN = -2, TID_EMPTY_LINE = -3;

inline const char *err_text(uint32_t e) {
    switch (e) {
    case E_HEADER_LATE: return "a header line (@) after the first alignment line";
    case E_FIELDS: return "fewer than 11 tab-separated fields";
    case E_FLAG: return "FLAG is not a decimal number in 0..65535";
    case E_RNAME: return "RNAME is not the name of an @SQ line";
    case E_POS: return "POS is not a decimal number in 0..2147483647";
    case E_MAPQ: return "MAPQ is not a decimal number in 0..255";
    case E_CIGAR: return "CIGAR is neither * nor a list of <length below 268435456><one of MIDNSHP=X>";
    }
    return "ok";
}

NP2_SAM_HD bool is_digit(uint8_t c) { return (uint8_t)(c - (uint8_t)'0') < 10u; }

// the decimal number text[a, b) -> *v.  false: no byte, a non-digit, or a value above max (max < 2^60)
NP2_SAM_HD bool parse_dec(const uint8_t *t, uint32_t a, uint32_t b, uint64_t max, uint64_t *v) {
    if (a >= b) return false;
    uint64_t x = 0;
    for (uint32_t i = a; i < b; ++i) {
        if (!is_digit(t[i])) return false;
        x = x * 10u + (uint64_t)(t[i] - (uint8_t)'0');
        if (x > max) return false;
    }
    *v = x;
    return true;
}

// BAM's operation number of a CIGAR letter, 16 for any other byte
NP2_SAM_HD uint32_t cigar_op(uint8_t c) {
    switch (c) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    }
    return 16;
}
// One byte of a CIGAR field text[a, b) that is not "*".  0: a digit with more of the field behind it; 1: an operation letter
// with its length in front, *w = len << 4 | op (the lane reads the digits back to the previous letter); 2: malformed (another
// byte, a letter without digits, a length of 2^28 or more, digits that end the field).
NP2_SAM_HD uint32_t cigar_byte(const uint8_t *t, uint32_t a, uint32_t b, uint32_t i, uint32_t *w) {
    if (is_digit(t[i])) return i + 1 == b ? 2u : 0u;
    const uint32_t op = cigar_op(t[i]);
    if (op == 16u) return 2u;
    uint32_t j = i;
    while (j > a && is_digit(t[j - 1])) --j;
    uint64_t len = 0;
    if (!parse_dec(t, j, i, CIGAR_LEN_END - 1u, &len)) return 2u;
    *w = (uint32_t)len << 4 | op;
    return 1u;
}

// BAM's 4-bit code of a SEQ byte: "=ACMGRSVTWYHKDBN" in either case, 15 for every other byte
NP2_SAM_HD uint32_t base_code(uint8_t c) {
    if (c == (uint8_t)'=') return 0u;
    const uint32_t u = (uint32_t)(c | 0x20u) - (uint32_t)'a';
    if (u >= 26u) return 15u; // (c | 0x20 is a lower-case letter only for the 52 letters)
    // letters a .. p and q .. z, one nibble each, a / q in the lowest
    return (uint32_t)((u < 16u ? 0xFFF3FCFFB4FFD2E1ull >> (4u * u) : 0xFAF97F865Full >> (4u * (u - 16u))) & 15u);
}

// (tid, pos + 1, strand) ascending; strand only under tie_by_strand.  tid >= 0, pos >= -1.
NP2_SAM_HD uint64_t sort_key(int32_t tid, int32_t pos, uint32_t flag, uint32_t tie_by_strand) {
    return (uint64_t)(uint32_t)tid << 33 | (uint64_t)(uint32_t)(pos + 1) << 1 | (tie_by_strand ? (flag >> 4) & 1u : 0u);
}

// ---- the @SQ names: an open-addressed table the host builds once -------------------------------------------------------
struct NameTab {
    const uint32_t *slot;  // mask + 1 entries: 0 empty, else tid + 1
    const uint32_t *off;   // n_refs + 1 offsets into names
    const uint8_t *names;
    uint32_t mask;
};
NP2_SAM_HD uint32_t name_hash(const uint8_t *t, uint32_t a, uint32_t b) { // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = a; i < b; ++i) h = (h ^ t[i]) * 16777619u;
    return h;
}
// tid of the name text[a, b); TID_NONE for "*", TID_UNKNOWN for a name the table lacks
NP2_SAM_HD int32_t name_lookup(const NameTab &nt, const uint8_t *t, uint32_t a, uint32_t b) {
    if (b - a == 1u && t[a] == (uint8_t)'*') return TID_NONE;
    for (uint32_t h = name_hash(t, a, b) & nt.mask;; h = (h + 1u) & nt.mask) { // (the table is at most half full)
        const uint32_t e = nt.slot[h];
        if (e == 0u) return TID_UNKNOWN;
        const uint32_t o = nt.off[e - 1u], len = nt.off[e] - o;
        if (len != b - a) continue;
        uint32_t k = 0;
        while (k < len && nt.names[o + k] == t[a + k]) ++k;
        if (k == len) return (int32_t)(e - 1u);
    }
}

// the four fields a single lane reads each
NP2_SAM_HD uint32_t parse_flag(const uint8_t *t, uint32_t a, uint32_t b, uint32_t *flag) {
    uint64_t v = 0;
    if (!parse_dec(t, a, b, 65535u, &v)) return E_FLAG;
    *flag = (uint32_t)v;
    return OK;
}
NP2_SAM_HD uint32_t parse_pos(const uint8_t *t, uint32_t a, uint32_t b, int32_t *pos) {
    uint64_t v = 0;
    if (!parse_dec(t, a, b, 2147483647u, &v)) return E_POS;
    *pos = (int32_t)v - 1;
    return OK;
}
NP2_SAM_HD uint32_t parse_mapq(const uint8_t *t, uint32_t a, uint32_t b, uint32_t *mapq) {
    uint64_t v = 0;
    if (!parse_dec(t, a, b, 255u, &v)) return E_MAPQ;
    *mapq = (uint32_t)v;
    return OK;
}
NP2_SAM_HD uint32_t parse_rname(const NameTab &nt, const uint8_t *t, uint32_t a, uint32_t b, int32_t *tid) {
    *tid = name_lookup(nt, t, a, b);
    return *tid == TID_UNKNOWN ? E_RNAME : OK;
}
NP2_SAM_HD uint32_t first_err(uint32_t a, uint32_t b) { return a == OK ? b : b == OK ? a : a < b ? a : b; }

// what k_sam_fields keeps of a line (32 bytes)
struct Line {
    uint32_t cig_a, cig_b; // the CIGAR field, text[cig_a, cig_b)
    uint32_t seq_a, l_seq; // the first SEQ byte; bases (0 for "*")
    int32_t tid, pos;      // tid: TID_EMPTY_LINE for a line without a byte
    uint32_t n_cigar;
    uint16_t flag;
    uint8_t mapq, err;
};
NP2_SAM_HD bool line_kept(const Line &ln) { return ln.err == OK && ln.tid >= 0 && !(ln.flag & 4u); }

// The line text[s, e) ('\n' and a '\r' before it already cut off) walked by one lane: the order of the steps and every rule
// are the wavefront's (k_sam_fields), which spreads the tab search and the CIGAR bytes over its lanes.
NP2_SAM_HD Line parse_line(const uint8_t *t, uint32_t s, uint32_t e, const NameTab &nt) {
    Line ln;
    ln.cig_a = ln.cig_b = ln.seq_a = ln.l_seq = 0, ln.tid = TID_NONE, ln.pos = -1, ln.n_cigar = 0, ln.flag = 0, ln.mapq = 0, ln.err = OK;
    if (e == s) {
        ln.tid = TID_EMPTY_LINE;
        return ln;
    }
    if (t[s] == (uint8_t)'@') {
        ln.err = E_HEADER_LATE;
        return ln;
    }
    uint32_t tab[N_TABS], n_tab = 0;
    for (uint32_t i = s; i < e && n_tab < N_TABS; ++i)
        if (t[i] == (uint8_t)'\t') tab[n_tab++] = i;
    if (n_tab < N_TABS) {
        ln.err = E_FIELDS;
        return ln;
    }
    uint32_t flag = 0, mapq = 0, err = OK;
    err = first_err(err, parse_flag(t, tab[0] + 1, tab[1], &flag));
    err = first_err(err, parse_rname(nt, t, tab[1] + 1, tab[2], &ln.tid));
    err = first_err(err, parse_pos(t, tab[2] + 1, tab[3], &ln.pos));
    err = first_err(err, parse_mapq(t, tab[3] + 1, tab[4], &mapq));
    ln.flag = (uint16_t)flag, ln.mapq = (uint8_t)mapq;
    ln.cig_a = tab[4] + 1, ln.cig_b = tab[5];
    if (ln.cig_b == ln.cig_a) {
        err = first_err(err, E_CIGAR);
    } else if (!(ln.cig_b - ln.cig_a == 1u && t[ln.cig_a] == (uint8_t)'*')) {
        for (uint32_t i = ln.cig_a; i < ln.cig_b; ++i) {
            uint32_t w;
            const uint32_t k = cigar_byte(t, ln.cig_a, ln.cig_b, i, &w);
            if (k == 2u) err = first_err(err, E_CIGAR);
            ln.n_cigar += k == 1u ? 1u : 0u;
        }
    }
    ln.seq_a = tab[8] + 1;
    ln.l_seq = tab[9] - ln.seq_a == 1u && t[ln.seq_a] == (uint8_t)'*' ? 0u : tab[9] - ln.seq_a;
    ln.err = (uint8_t)err;
    return ln;
}
// ... and its CIGAR words and packed SEQ (cigar: n_cigar words, seq4: (l_seq + 1) / 2 bytes), as k_sam_pack writes them
NP2_SAM_HD void pack_line(const uint8_t *t, const Line &ln, uint32_t *cigar, uint8_t *seq4) {
    uint32_t n = 0;
    if (ln.n_cigar)
        for (uint32_t i = ln.cig_a; i < ln.cig_b; ++i) {
            uint32_t w;
            if (cigar_byte(t, ln.cig_a, ln.cig_b, i, &w) == 1u) cigar[n++] = w;
        }
    for (uint32_t j = 0; j < (ln.l_seq + 1u) / 2u; ++j) {
        const uint32_t hi = base_code(t[ln.seq_a + 2u * j]);
        const uint32_t lo = 2u * j + 1u < ln.l_seq ? base_code(t[ln.seq_a + 2u * j + 1u]) : 0u;
        seq4[j] = (uint8_t)(hi << 4 | lo);
    }
}

// ---- host only: the header --------------------------------------------------------------------------------------------
struct Refs {
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    bool operator==(const Refs &o) const { return names == o.names && lens == o.lens; }
};
// One header line text[a, b) (it begins with '@').  Empty string: taken (an @SQ line added to refs, any other line ignored);
// otherwise what is wrong with it.
inline std::string header_line(const uint8_t *t, size_t a, size_t b, Refs &refs) {
    if (b - a < 3 || t[a + 1] != 'S' || t[a + 2] != 'Q' || (b - a > 3 && t[a + 3] != '\t')) return "";
    std::string sn;
    bool has_sn = false, has_ln = false;
    uint64_t ln = 0;
    size_t i = a + 3;
    while (i < b) { // fields behind the tag
        size_t j = ++i;
        while (j < b && t[j] != '\t') ++j;
        if (j - i >= 3 && t[i + 2] == ':') {
            if (t[i] == 'S' && t[i + 1] == 'N' && !has_sn) sn.assign((const char *)t + i + 3, j - i - 3), has_sn = true;
            if (t[i] == 'L' && t[i + 1] == 'N' && !has_ln) {
                if (!parse_dec(t, (uint32_t)(i + 3), (uint32_t)j, 0xFFFFFFFFull, &ln)) return "an @SQ line whose LN is not a number below 2^32";
                has_ln = true;
            }
        }
        i = j;
    }
    if (!has_sn || sn.empty() || !has_ln) return "an @SQ line without SN or LN";
    for (const std::string &n : refs.names)
        if (n == sn) return "the @SQ name " + sn + " is given twice";
    refs.names.push_back(sn), refs.lens.push_back((uint32_t)ln);
    return "";
}

// NP2_SAM_KEEP_ALL: is the header line text[a, b) carried into the BAM's header text as it stands?  Every line but @HD and @SQ
// (the writer makes those itself).
inline bool header_line_is_carried(const uint8_t *t, size_t a, size_t b) {
    if (b - a < 3) return true;
    const bool hd = t[a + 1] == 'H' && t[a + 2] == 'D', sq = t[a + 1] == 'S' && t[a + 2] == 'Q';
    return !((hd || sq) && (b - a == 3 || t[a + 3] == '\t'));
}

// the table of NameTab over `refs`, as host arrays (names concatenated; slots: a power of two, at least twice the names)
struct NameTabHost {
    std::vector<uint32_t> slot, off;
    std::vector<uint8_t> names;
    uint32_t mask = 0;
    explicit NameTabHost(const Refs &refs) {
        uint32_t cap = 4;
        while (cap < 2 * refs.names.size() + 2) cap <<= 1;
        mask = cap - 1;
        slot.assign(cap, 0u);
        off.push_back(0u);
        for (const std::string &n : refs.names) {
            names.insert(names.end(), n.begin(), n.end());
            off.push_back((uint32_t)names.size());
        }
        names.push_back(0); // (never an empty array)
        for (uint32_t i = 0; i < refs.names.size(); ++i) {
            uint32_t h = name_hash(names.data(), off[i], off[i + 1]) & mask;
            while (slot[h]) h = (h + 1u) & mask;
            slot[h] = i + 1u;
        }
    }
    NameTab view() const { return NameTab{slot.data(), off.data(), names.data(), mask}; }
};

} // namespace np2sam
