// DEFLATE (RFC 1951) encoding of one BGZF block's bytes, shared by the GPU deflater (np2_deflate.hip: one wavefront per
// block) and its host twin (np2_deflate_host.cpp behind np2_bgzf_deflate_host, tests/tools/deflate_core_test.cpp): the
// mirror of np2_inflate_core.hpp.  The reference writes its compressed outputs through gzip on the host (its recipe's
// sr.R1.clean.fastq.gz); here the block is compressed where the bytes already are.
//
// The code is written as PHASES: m.lanes(f) runs f(lane) for each of the 64 lanes and ends in a wavefront barrier — on the
// device every lane calls f with its own index, the host machine loops over 0 .. 63 — and m.lead(f) runs f once.  Whatever a
// phase reads of shared state was written in an earlier phase, and where several lanes write one word in one phase they do
// it with an operation whose result does not depend on their order (add, max, or).  So the bytes that come out are a
// function of the block's bytes alone, and the same on both sides.
//
// One block of n <= 65280 bytes:
//   1. LZ77.  The block is walked in stripes of 64 x 64 bytes, lane l owning the 64-byte segment l of each stripe; in round
//      r every lane stands at byte r of its segment.  It looks its next 8 bytes up in a 4096-entry hash table of positions
//      (the table as the previous round left it), takes the candidate if it lies before its own position, no further back
//      than 32768, and if the bytes there really are the same for at least MIN_MATCH bytes; a match ends at its segment's
//      end at the latest.  Then, behind the barrier, all lanes enter their positions, the highest winning a slot.
//      Tokens go to `tok` (one word per input byte), their symbols into the two histograms.
//   2. One dynamic Huffman block: both codes limited to 15 bits, the code length code to 7, HLIT / HDIST / HCLEN trimmed.
//   3. If that would be no smaller than n + 5 bytes: a stored block.  Else every lane counts the bits of its segments, a
//      prefix sum gives it its bit offsets, and it writes its bits: the words it shares with a neighbour by OR into words
//      this call has zeroed, the others by plain stores.
//   n == 0: the fixed block with nothing but the end code (03 00), what the canonical BGZF EOF block carries.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_DEF_HD __host__ __device__ __forceinline__
#else
#define NP2_DEF_HD inline
#endif

namespace np2def {

static constexpr uint32_t MAX_BLOCK = 65280;   // input bytes of a block (0xff00, htslib's)
static constexpr uint32_t SLOT_BYTES = 65536;  // a BGZF block: 18 header bytes, at most MAX_BLOCK + 5 of DEFLATE, 8 of trailer
static constexpr uint32_t HDR_BYTES = 18, TRL_BYTES = 8;
static constexpr uint32_t SEG = 64;            // bytes of a lane's segment
static constexpr uint32_t STRIPE = 64 * SEG;   // bytes all lanes cover together
static constexpr uint32_t HASH_BITS = 12, HASH_SLOTS = 1u << HASH_BITS;
static constexpr uint32_t HASH_BYTES = 8;      // bytes hashed; also the fewest a match is accepted with
static constexpr uint32_t MIN_MATCH = 8;       // (greedy matches of 4 - 7 bytes cost more than literals under a 2-bit code on DNA)
static constexpr uint32_t MAX_DIST = 32768;
static constexpr uint32_t NLIT = 286, NDIST = 30, NCLEN = 19;
static constexpr uint32_t TOK_WORDS = 65536;   // words of token scratch per block

// a token word: 0 = literal (the byte is read from the input again), else (length << 16) | (distance - 1)
NP2_DEF_HD uint32_t tok_match(uint32_t len, uint32_t dist) { return (len << 16) | (dist - 1u); }
// token index of position p: inside a stripe the 64 lanes of a round lie side by side
NP2_DEF_HD uint32_t tok_index(uint32_t p) {
    const uint32_t o = p & (STRIPE - 1u);
    return (p & ~(STRIPE - 1u)) | ((o & (SEG - 1u)) << 6) | (o >> 6);
}

// length 3 .. 258 -> symbol - 257, and distance 1 .. 32768 -> symbol (RFC 1951 3.2.5)
NP2_DEF_HD uint32_t len_sym(uint32_t len) {
    if (len == 258) return 28;
    const uint32_t v = len - 3u;
    if (v < 8) return v;
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(v); // >= 3
    return ((hb - 1u) << 2) + ((v >> (hb - 2u)) & 3u);
}
NP2_DEF_HD uint32_t len_sym_extra(uint32_t s) { return (s < 8 || s == 28) ? 0u : (s - 4u) >> 2; }
NP2_DEF_HD uint32_t len_sym_base(uint32_t s) {
    const uint32_t eb = len_sym_extra(s);
    return s == 28 ? 258u : (s < 8 ? 3u + s : 3u + ((4u + (s & 3u)) << eb));
}
NP2_DEF_HD uint32_t dist_sym(uint32_t dist) {
    const uint32_t v = dist - 1u;
    if (v < 4) return v;
    const uint32_t hb = 31u - (uint32_t)__builtin_clz(v); // >= 2
    return (hb << 1) + ((v >> (hb - 1u)) & 1u);
}
NP2_DEF_HD uint32_t dist_sym_extra(uint32_t s) { return s < 4 ? 0u : (s - 2u) >> 1; }
NP2_DEF_HD uint32_t dist_sym_base(uint32_t s) {
    const uint32_t eb = dist_sym_extra(s);
    return s < 4 ? 1u + s : 1u + ((2u + (s & 1u)) << eb);
}
NP2_DEF_HD uint32_t bit_reverse(uint32_t c, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((c >> i) & 1u) << (n - 1u - i);
    return r;
}
NP2_DEF_HD uint32_t clen_order(uint32_t i) { // RFC 1951 3.2.7
    const uint64_t lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) |
                        (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
    const uint64_t hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
    return i < 12 ? (uint32_t)((lo >> (5 * i)) & 31u) : (uint32_t)((hi >> (5 * (i - 12))) & 31u);
}
NP2_DEF_HD uint64_t load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
NP2_DEF_HD uint32_t hash8(uint64_t x) { return (uint32_t)((x * 0x9E3779B97F4A7C15ull) >> (64u - HASH_BITS)); }

// What a block's wavefront shares (LDS on the device).  The hash table is dead once the tokens stand, and the code
// builder's arrays take its place.
struct Shared {
    union {
        uint32_t hash[HASH_SLOTS]; // position + 1 of the latest 8 bytes with this hash; 0: none
        struct {
            uint32_t a[288];      // the builder's in-place array (frequencies -> parents -> depths)
            uint16_t sorted[288]; // used symbols by (frequency, symbol) ascending
            uint16_t rle[320];    // the code length sequence as symbols of the code length code: symbol | extra << 8
            uint32_t n_rle;
            uint32_t seg_bits[64];
        } b;
    };
    uint32_t lfreq[288], dfreq[32], cfreq[NCLEN];
    uint16_t lcode[288], dcode[32], ccode[NCLEN]; // bit-reversed: ready to be ORed into the stream
    uint8_t llen[288], dlen[32], clen[NCLEN];
    uint32_t hlit, hdist, hclen, hdr_bits, body_bits;
    uint32_t dummy[2], n_dummy; // symbols build_code added to make a code of two
};

// ---- the Huffman code of freq[0, n): len[] <= maxbits, code[] bit-reversed --------------------------------------------
// Every lane ranks some symbols (a rank sort: no order of arrival in it); the leader then runs Moffat and Katajainen's
// in-place minimum-redundancy lengths over the sorted frequencies, moves the codes longer than maxbits up (the Kraft sum
// repaired from the longest lengths down) and hands the lengths out, the shortest to the most frequent symbol.
// A code always has two symbols at least (as zlib's: a decoder need not take a one-symbol code).
template <class M>
NP2_DEF_HD void build_code(M &m, Shared &S, uint32_t *freq, uint32_t n, uint32_t maxbits, uint8_t *len, uint16_t *code) {
    m.lead([&] {
        uint32_t used = 0;
        for (uint32_t s = 0; s < n; ++s) used += freq[s] != 0;
        S.n_dummy = 0;
        for (uint32_t s = 0; used < 2 && s < n; ++s)
            if (!freq[s]) freq[s] = 1, ++used, S.dummy[S.n_dummy++] = s;
    });
    m.lanes([&](uint32_t lane) {
        for (uint32_t s = lane; s < n; s += 64) {
            len[s] = 0, code[s] = 0;
            const uint32_t f = freq[s];
            if (!f) continue;
            uint32_t rank = 0;
            for (uint32_t t = 0; t < n; ++t) {
                const uint32_t g = freq[t];
                rank += (g != 0 && (g < f || (g == f && t < s))) ? 1u : 0u;
            }
            S.b.sorted[rank] = (uint16_t)s;
        }
    });
    m.lead([&] {
        uint32_t *A = S.b.a;
        int32_t nu = 0;
        for (uint32_t s = 0; s < n; ++s) nu += freq[s] != 0;
        for (int32_t i = 0; i < nu; ++i) A[i] = freq[S.b.sorted[i]];
        // (Moffat & Katajainen, "In-place calculation of minimum-redundancy codes", 1995; nu >= 2)
        A[0] += A[1];
        int32_t root = 0, leaf = 2, next;
        for (next = 1; next < nu - 1; ++next) {
            if (leaf >= nu || A[root] < A[leaf]) A[next] = A[root], A[root++] = (uint32_t)next;
            else A[next] = A[leaf++];
            if (leaf >= nu || (root < next && A[root] < A[leaf])) A[next] += A[root], A[root++] = (uint32_t)next;
            else A[next] += A[leaf++];
        }
        A[nu - 2] = 0;
        for (next = nu - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int32_t avbl = 1, usd = 0, dpth = 0;
        root = nu - 2, next = nu - 1;
        while (avbl > 0) {
            while (root >= 0 && (int32_t)A[root] == dpth) ++usd, --root;
            while (avbl > usd) A[next--] = (uint32_t)dpth, --avbl;
            avbl = 2 * usd, ++dpth, usd = 0;
        }
        // A[i]: length of the i-th rarest symbol.  Codes per length, the limit enforced.
        uint32_t cnt[34];
        for (uint32_t b = 0; b < 34; ++b) cnt[b] = 0;
        for (int32_t i = 0; i < nu; ++i) ++cnt[A[i] < 33 ? A[i] : 33];
        for (uint32_t b = maxbits + 1; b < 34; ++b) cnt[maxbits] += cnt[b];
        uint32_t total = 0;
        for (uint32_t b = maxbits; b >= 1; --b) total += cnt[b] << (maxbits - b);
        while (total > (1u << maxbits)) {
            --cnt[maxbits];
            for (uint32_t b = maxbits - 1; b >= 1; --b)
                if (cnt[b]) {
                    --cnt[b], cnt[b + 1] += 2;
                    break;
                }
            --total;
        }
        int32_t j = nu;
        for (uint32_t b = 1; b <= maxbits; ++b)
            for (uint32_t l = cnt[b]; l; --l) len[S.b.sorted[--j]] = (uint8_t)b;
        // canonical codes in symbol order
        uint32_t nextc[17], c = 0;
        cnt[0] = 0;
        for (uint32_t b = 1; b <= maxbits; ++b) c = (c + cnt[b - 1]) << 1, nextc[b] = c;
        for (uint32_t s = 0; s < n; ++s)
            if (len[s]) code[s] = (uint16_t)bit_reverse(nextc[len[s]]++, len[s]);
        for (uint32_t d = 0; d < S.n_dummy; ++d) freq[S.dummy[d]] = 0; // (they keep their codes; no token stands for them)
    });
}

// ---- a lane's bit writer ----------------------------------------------------------------------------------------------------
// Bits from stream bit `at` on (counted from bit 0 of words[0]).  The first word a writer touches and the one it ends in
// may be shared with other writers: OR.  A word in between is this writer's alone: a plain store.
template <class M> struct BitWriter {
    M &m;
    uint32_t *words;
    uint32_t w;      // word being filled
    uint64_t acc;    // its bits so far, and those beyond
    uint32_t nacc;   // valid bits in acc
    bool first;
    NP2_DEF_HD BitWriter(M &mm, uint32_t *wd, uint32_t at) : m(mm), words(wd), w(at >> 5), acc(0), nacc(at & 31u), first(true) {}
    NP2_DEF_HD void put(uint32_t bits, uint32_t n) { // n <= 32, nacc < 32 on entry
        acc |= (uint64_t)bits << nacc;
        nacc += n;
        if (nacc >= 32u) {
            if (first) m.word_or(words + w, (uint32_t)acc);
            else m.word_set(words + w, (uint32_t)acc);
            first = false;
            ++w, acc >>= 32, nacc -= 32u;
        }
    }
    NP2_DEF_HD void finish() {
        if (nacc) m.word_or(words + w, (uint32_t)acc);
    }
};

// struct Machine {
//     template <class F> void lanes(F f);   // f(lane) for the 64 lanes, then a barrier
//     template <class F> void lead(F f);    // f() once, then a barrier
//     struct Lane { uint32_t skip, h; };    // what a lane keeps between phases
//     Lane &priv(uint32_t lane);
//     void hist_add(uint32_t *p);           // ++*p               (shared memory, several lanes at once)
//     void slot_max(uint32_t *p, uint32_t v);   // *p = max(*p, v)    (shared memory)
//     void word_or(uint32_t *p, uint32_t v);    // *p |= v            (the output, several lanes at once)
//     void word_set(uint32_t *p, uint32_t v);   // *p = v             (the output, a word of one lane's)
//     void zeroed();                        // the output's zero words are in place before any lane ORs into them
// };
//
// in[0, n) -> a complete DEFLATE stream (one final block) whose bit 0 is stream bit `bit0` of `words` (bit0 a multiple of 8).
// The function zeroes every word it writes bits into, from word bit0 / 32 on: the bytes of that first word in front of the
// stream are the caller's to write AFTERWARDS.  tok: TOK_WORDS words of scratch.  Returns the stream's bytes, at most n + 5.
template <class M> NP2_DEF_HD uint32_t deflate_block(M &m, Shared &S, const uint8_t *in, uint32_t n, uint32_t *words, uint32_t bit0, uint32_t *tok) {
    uint8_t *out = reinterpret_cast<uint8_t *>(words) + (bit0 >> 3);
    if (n == 0) {
        m.lead([&] { out[0] = 3, out[1] = 0; });
        return 2;
    }
    // ---- 1. tokens and histograms ----
    m.lanes([&](uint32_t lane) {
        for (uint32_t i = lane; i < HASH_SLOTS; i += 64) S.hash[i] = 0;
        for (uint32_t i = lane; i < 288; i += 64) S.lfreq[i] = 0;
        if (lane < 32) S.dfreq[lane] = 0;
        if (lane < NCLEN) S.cfreq[lane] = 0;
    });
    for (uint32_t base = 0; base < n; base += STRIPE) {
        m.lanes([&](uint32_t lane) { m.priv(lane).skip = 0; });
        const uint32_t rounds = n - base < SEG ? n - base : SEG; // (a last stripe shorter than a segment)
        for (uint32_t r = 0; r < rounds; ++r) {
            m.lanes([&](uint32_t lane) {
                auto &L = m.priv(lane);
                const uint32_t p = base + lane * SEG + r;
                L.h = 0xFFFFFFFFu;
                if (p >= n) return;
                uint64_t mine = 0;
                uint32_t cand = 0;
                if (p + HASH_BYTES <= n) {
                    mine = load64(in + p);
                    L.h = hash8(mine);
                    cand = S.hash[L.h];
                }
                if (r < L.skip) { // inside the match taken earlier
                    tok[tok_index(p)] = 0;
                    return;
                }
                uint32_t t = 0;
                if (cand && r + HASH_BYTES <= SEG && cand - 1u < p && p - (cand - 1u) <= MAX_DIST && load64(in + (cand - 1u)) == mine) {
                    const uint32_t c = cand - 1u;
                    uint32_t room = SEG - r; // to the segment's end ...
                    if (n - p < room) room = n - p; // ... and the block's
                    uint32_t len = HASH_BYTES;
                    bool differ = false;
                    while (!differ && len + 8u <= room) {
                        const uint64_t x = load64(in + c + len) ^ load64(in + p + len);
                        if (x) len += (uint32_t)__builtin_ctzll(x) >> 3, differ = true;
                        else len += 8u;
                    }
                    while (!differ && len < room && in[c + len] == in[p + len]) ++len;
                    if (len >= MIN_MATCH) t = tok_match(len, p - c), L.skip = r + len;
                }
                tok[tok_index(p)] = t;
                if (t) {
                    m.hist_add(&S.lfreq[257u + len_sym(t >> 16)]);
                    m.hist_add(&S.dfreq[dist_sym((t & 0xFFFFu) + 1u)]);
                } else {
                    m.hist_add(&S.lfreq[in[p]]);
                }
            });
            m.lanes([&](uint32_t lane) {
                const uint32_t h = m.priv(lane).h;
                if (h != 0xFFFFFFFFu) m.slot_max(&S.hash[h], base + lane * SEG + r + 1u);
            });
        }
    }
    m.lead([&] { S.lfreq[256] = 1; });
    // ---- 2. the codes and the block header ----
    build_code(m, S, S.lfreq, NLIT, 15, S.llen, S.lcode);
    build_code(m, S, S.dfreq, NDIST, 15, S.dlen, S.dcode);
    m.lead([&] {
        uint32_t hlit = NLIT, hdist = NDIST;
        while (hlit > 257 && !S.llen[hlit - 1]) --hlit;
        while (hdist > 1 && !S.dlen[hdist - 1]) --hdist;
        S.hlit = hlit, S.hdist = hdist;
        // the two length arrays as one sequence, run-length coded (16: previous x 3-6, 17: zeros x 3-10, 18: zeros x 11-138)
        const uint32_t total = hlit + hdist;
        auto at = [&](uint32_t i) -> uint32_t { return i < hlit ? S.llen[i] : S.dlen[i - hlit]; };
        uint32_t nr = 0;
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = at(i);
            uint32_t run = 1;
            while (i + run < total && at(i + run) == v) ++run;
            uint32_t left = run;
            if (v == 0) {
                while (left >= 11) {
                    const uint32_t k = left < 138 ? left : 138;
                    S.b.rle[nr++] = (uint16_t)(18u | ((k - 11u) << 8)), left -= k;
                }
                if (left >= 3) S.b.rle[nr++] = (uint16_t)(17u | ((left - 3u) << 8)), left = 0;
            } else if (left >= 4) {
                S.b.rle[nr++] = (uint16_t)v, --left;
                while (left >= 3) {
                    const uint32_t k = left < 6 ? left : 6;
                    S.b.rle[nr++] = (uint16_t)(16u | ((k - 3u) << 8)), left -= k;
                }
            }
            for (; left; --left) S.b.rle[nr++] = (uint16_t)v;
            i += run;
        }
        S.b.n_rle = nr;
        for (uint32_t k = 0; k < nr; ++k) ++S.cfreq[S.b.rle[k] & 255u];
    });
    build_code(m, S, S.cfreq, NCLEN, 7, S.clen, S.ccode); // (the builder's arrays lie beside rle[], not over it)
    m.lead([&] {
        uint32_t hclen = NCLEN;
        while (hclen > 4 && !S.clen[clen_order(hclen - 1)]) --hclen;
        S.hclen = hclen;
        uint32_t hb = 3 + 14 + 3 * hclen;
        for (uint32_t k = 0; k < S.b.n_rle; ++k) {
            const uint32_t s = S.b.rle[k] & 255u;
            hb += S.clen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
        }
        S.hdr_bits = hb;
        uint32_t body = 0;
        for (uint32_t s = 0; s < NLIT; ++s) body += S.lfreq[s] * (S.llen[s] + (s > 256 ? len_sym_extra(s - 257u) : 0u));
        for (uint32_t s = 0; s < NDIST; ++s) body += S.dfreq[s] * (S.dlen[s] + dist_sym_extra(s));
        S.body_bits = body;
    });
    const uint32_t dyn_bytes = (S.hdr_bits + S.body_bits + 7u) >> 3;
    if (dyn_bytes >= n + 5u) { // ---- 3a. stored ----
        m.lanes([&](uint32_t lane) {
            if (lane == 0) {
                out[0] = 1;
                out[1] = (uint8_t)(n & 255u), out[2] = (uint8_t)(n >> 8);
                out[3] = (uint8_t)(~n & 255u), out[4] = (uint8_t)((~n >> 8) & 255u);
            }
            for (uint32_t i = lane; i < n; i += 64) out[5u + i] = in[i];
        });
        return n + 5u;
    }
    // ---- 3b. the bit stream ----
    const uint32_t w0 = bit0 >> 5;
    const uint32_t w_end = (bit0 + S.hdr_bits + S.body_bits + 31u) >> 5;
    m.lanes([&](uint32_t lane) {
        for (uint32_t w = w0 + lane; w < w_end; w += 64) m.word_set(words + w, 0u);
    });
    m.zeroed();
    m.lead([&] {
        BitWriter<M> bw(m, words, bit0);
        bw.first = true;
        auto put_or = [&](uint32_t bits, uint32_t nb) { // (the header's words: all by OR, the first is shared with the caller's bytes)
            bw.put(bits, nb);
            bw.first = true;
        };
        put_or(1u | (2u << 1), 3);
        put_or((S.hlit - 257u) | ((S.hdist - 1u) << 5) | ((S.hclen - 4u) << 10), 14);
        for (uint32_t i = 0; i < S.hclen; ++i) put_or(S.clen[clen_order(i)], 3);
        for (uint32_t k = 0; k < S.b.n_rle; ++k) {
            const uint32_t s = S.b.rle[k] & 255u, x = S.b.rle[k] >> 8;
            put_or(S.ccode[s], S.clen[s]);
            if (s >= 16) put_or(x, s == 16 ? 2u : s == 17 ? 3u : 7u);
        }
        bw.finish();
    });
    uint32_t at = bit0 + S.hdr_bits; // (the same in every lane: read from shared memory behind a barrier)
    for (uint32_t base = 0; base < n; base += STRIPE) {
        const bool last_stripe = base + STRIPE >= n;
        // the lane that holds the block's last byte appends the end code
        const uint32_t end_lane = (n - 1u - base) / SEG;
        auto walk = [&](uint32_t lane, auto &&lit, auto &&match) {
            const uint32_t lo = base + lane * SEG;
            const uint32_t hi = lo + SEG < n ? lo + SEG : n;
            for (uint32_t p = lo; p < hi;) {
                const uint32_t t = tok[tok_index(p)];
                if (!t) lit((uint32_t)in[p]), ++p;
                else match(t >> 16, (t & 0xFFFFu) + 1u), p += t >> 16;
            }
        };
        m.lanes([&](uint32_t lane) {
            uint32_t bits = 0;
            walk(lane, [&](uint32_t b) { bits += S.llen[b]; },
                 [&](uint32_t len, uint32_t dist) {
                     const uint32_t ls = len_sym(len), ds = dist_sym(dist);
                     bits += S.llen[257u + ls] + len_sym_extra(ls) + S.dlen[ds] + dist_sym_extra(ds);
                 });
            if (last_stripe && lane == end_lane) bits += S.llen[256];
            S.b.seg_bits[lane] = bits;
        });
        m.lanes([&](uint32_t lane) {
            uint32_t off = at;
            for (uint32_t l = 0; l < lane; ++l) off += S.b.seg_bits[l];
            BitWriter<M> bw(m, words, off);
            walk(lane, [&](uint32_t b) { bw.put(S.lcode[b], S.llen[b]); },
                 [&](uint32_t len, uint32_t dist) {
                     const uint32_t ls = len_sym(len), ds = dist_sym(dist);
                     bw.put(S.lcode[257u + ls], S.llen[257u + ls]);
                     bw.put(len - len_sym_base(ls), len_sym_extra(ls));
                     bw.put(S.dcode[ds], S.dlen[ds]);
                     bw.put(dist - dist_sym_base(ds), dist_sym_extra(ds));
                 });
            if (last_stripe && lane == end_lane) bw.put(S.lcode[256], S.llen[256]);
            bw.finish();
        });
        uint32_t sum = 0;
        for (uint32_t l = 0; l < 64; ++l) sum += S.b.seg_bits[l];
        at += sum;
        m.lanes([](uint32_t) {}); // (seg_bits is rewritten by the next stripe)
    }
    return (at - bit0 + 7u) >> 3;
}

// The host twin's machine: the 64 lanes of a phase one after the other.
struct HostMachine {
    struct Lane {
        uint32_t skip, h;
    };
    Lane lane_state[64];
    template <class F> void lanes(F f) {
        for (uint32_t l = 0; l < 64; ++l) f(l);
    }
    template <class F> void lead(F f) { f(); }
    Lane &priv(uint32_t lane) { return lane_state[lane]; }
    void hist_add(uint32_t *p) { ++*p; }
    void slot_max(uint32_t *p, uint32_t v) { *p = *p > v ? *p : v; }
    void word_or(uint32_t *p, uint32_t v) { *p |= v; }
    void word_set(uint32_t *p, uint32_t v) { *p = v; }
    void zeroed() {}
};

} // namespace np2def
