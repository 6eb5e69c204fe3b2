// The host half of the phasing vote (nextpolish2_amd/csrc/np2_vote_host.hpp: vote_merge, vote_rows_from_pairs, vote_decide
// and, under them, the threaded graph code of np2_phase_host.hpp) without a device and without the library: a program of its
// own, built with the thread sanitizer and with the address and undefined-behaviour sanitizers
// (tests/test_vote_host_tools_cpu.py).
//
//     vote_host_test rows | merge | threads | recorded <dir> <n_reads>
//
// rows, merge: prints "ok" and exits 0, or names the failed checks and exits 1.  threads: prints the hash of the losers of
// a large generated vote, once decided from its pair list and once from its rows (NP2_VOTE_THREADS is read once per
// process: the test runs the program per thread count and compares).  recorded: decides the vote whose arrays lie in <dir>
// as raw little-endian files, whole and cut in two, and writes the losers next to them.
#include "../../include/np2.h"
#include "../../nextpolish2_amd/csrc/np2_vote_host.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>

using namespace np2h;

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

struct Vote { // one np2_vote_t and the arrays it points to
    std::vector<uint64_t> key;
    std::vector<uint32_t> cnt, read_id, first_pos;
    std::vector<int32_t> ref_w;
    std::vector<uint8_t> flags;
    void pair(uint32_t a, uint32_t b, uint32_t same, uint32_t neg) {
        key.push_back((uint64_t)a << 32 | b);
        cnt.push_back(same | neg << 16);
    }
    void read(uint32_t id, uint32_t pos, int32_t w, uint8_t fl) {
        read_id.push_back(id), first_pos.push_back(pos), ref_w.push_back(w), flags.push_back(fl);
    }
    np2_vote_t c() const {
        return np2_vote_t{key.size(), key.data(), cnt.data(), (uint32_t)read_id.size(), read_id.data(), first_pos.data(), ref_w.data(), flags.data()};
    }
};

// -> the status the library would return; the losers of a decided vote
struct Outcome {
    int rc = NP2_OK;
    std::vector<uint32_t> losers;
    bool operator==(const Outcome &o) const { return rc == o.rc && losers == o.losers; }
};
static Outcome decide(const VoteData &vd, bool use_all) {
    Outcome o;
    try {
        o.losers = vote_decide(vd, use_all);
    } catch (const Np2Error &e) {
        o.rc = e.code;
    }
    return o;
}
// (one sorted vote is viewed, not copied: `vs` has to outlive what is done with `vd`)
static int merge(const std::vector<Vote> &vs, uint32_t n_reads, VoteData &vd) {
    std::vector<np2_vote_t> c;
    for (const Vote &v : vs) c.push_back(v.c());
    return vote_merge(c.data(), (int)c.size(), n_reads, vd);
}
static Outcome decide_votes(const std::vector<Vote> &vs, uint32_t n_reads, bool use_all, bool as_rows = false) {
    VoteData vd;
    Outcome o;
    o.rc = merge(vs, n_reads, vd);
    if (o.rc != NP2_OK) return o;
    if (as_rows && !vote_rows_from_pairs(vd, use_all)) {
        o.rc = NP2_E_UNSUPPORTED;
        return o;
    }
    return decide(vd, use_all);
}

// A small vote as one unsharded pass would deliver it: reads 1 .. n_reads - 1, some of them with a per-read record, pairs
// among the voting ones (sorted, inside `band`), agreeing / disagreeing region counts, weights against the contig for
// some, a few flagged; reads with a record that never vote enter no pair.
static Vote small_vote(std::mt19937 &rng, uint32_t n_reads, uint32_t band) {
    Vote v;
    std::vector<uint8_t> votes(n_reads, 0), record(n_reads, 0);
    for (uint32_t r = 1; r < n_reads; ++r) record[r] = rng() % 8 != 0, votes[r] = record[r] && rng() % 6 != 0;
    for (uint32_t a = 1; a < n_reads; ++a)
        for (uint32_t b = a + 1; b < n_reads && b - a - 1 < band; ++b)
            if (votes[a] && votes[b] && rng() % 4 == 0) {
                const uint32_t same = rng() % 4, neg = rng() % 5;
                if (same | neg) v.pair(a, b, same, neg);
            }
    std::vector<uint8_t> in_pair(n_reads, 0);
    for (uint64_t k : v.key) in_pair[k >> 32] = in_pair[(uint32_t)k] = 1;
    for (uint32_t r = 1; r < n_reads; ++r) {
        if (!record[r]) continue;
        const bool seen = rng() % 2;
        const uint8_t fl = (uint8_t)((in_pair[r] ? 1 : 0) | (seen ? 2 : 0) | (rng() % 10 == 0 ? 4 : 0));
        v.read(r, in_pair[r] ? 100 + rng() % 100000 : 0xFFFFFFFFu, seen ? (int32_t)(rng() % 7) - 3 : 0, fl);
    }
    return v;
}

static void rows_scenario() {
    std::mt19937 rng(7);
    int decided = 0;
    for (int t = 0; t < 300; ++t) {
        const uint32_t n_reads = 12 + rng() % 49;
        const Vote v = small_vote(rng, n_reads, 1 + rng() % 40);
        for (bool use_all : {false, true}) {
            const Outcome pairs = decide_votes({v}, n_reads, use_all), rows = decide_votes({v}, n_reads, use_all, true);
            CHECK(pairs == rows);
            CHECK(pairs.rc == NP2_OK || pairs.rc == NP2_E_REFPANIC);
            decided += pairs.rc == NP2_OK;
        }
    }
    CHECK(decided > 300); // (most votes are decided, not refused as the reference's panics)
    // what the band does not hold, and what is no sorted pair list
    auto refused = [](std::vector<std::pair<uint32_t, uint32_t>> ps, uint32_t n_reads) {
        std::vector<Vote> vs(1);
        Vote &v = vs[0];
        std::vector<uint8_t> seen(n_reads, 0);
        for (auto &p : ps) v.pair(p.first, p.second, 1, 0), seen[p.first] = seen[p.second] = 1;
        for (uint32_t r = 0; r < n_reads; ++r)
            if (seen[r]) v.read(r, 1000 + r, 0, 1);
        VoteData vd;
        if (merge(vs, n_reads, vd) != NP2_OK) return false;
        if (ps.size() > 1 && ps[0] > ps[1]) vd.own(), std::swap(vd.pair_key[0], vd.pair_key[1]); // (vote_merge sorts: undo it)
        return !vote_rows_from_pairs(vd, false);
    };
    CHECK(!refused({{1, EDGE_BAND + 1}}, EDGE_BAND + 8)); // b - a - 1 == EDGE_BAND - 1: the last column of the band
    CHECK(refused({{1, EDGE_BAND + 2}}, EDGE_BAND + 8));  // b - a - 1 == EDGE_BAND
    CHECK(refused({{5, 5}}, 16));
    CHECK(refused({{6, 5}}, 16));
    CHECK(refused({{3, 4}, {2, 9}}, 16));
    CHECK(!refused({{2, 9}, {3, 4}}, 16));
    // pairs with an endpoint that never voted are counted, not listed
    {
        std::vector<Vote> vs(1);
        Vote &v = vs[0];
        v.pair(1, 2, 2, 0), v.pair(2, 3, 1, 0), v.pair(3, 5, 1, 1), v.pair(4, 5, 0, 1);
        for (uint32_t r : {1u, 2u, 5u}) v.read(r, 500 + r, 0, 1);
        v.read(3, 0xFFFFFFFFu, 1, 2); // a record, but no vote; read 4 has no record at all
        VoteData vd;
        CHECK(merge(vs, 8, vd) == NP2_OK);
        CHECK(vote_rows_from_pairs(vd, false));
        CHECK(vd.n_nokey == 3);
        CHECK(vd.off[8] == 2 && vd.off[2] - vd.off[1] == 1 && vd.off[3] - vd.off[2] == 1); // only (1, 2) is listed, twice
        CHECK(decide(vd, false).rc == NP2_E_DEVICE);
    }
}

// `v` dealt out over n_shards shards of consecutive reads: a pair goes to the shard of its lower read, unless both reads lie
// within `halo` reads of a cut — then its counts are split between the two shards at the cut; a read's record goes to its
// shard, a halo read's to both (weights split, flags dealt out, the first vote kept by one of them)
static std::vector<Vote> cut_vote(std::mt19937 &rng, const Vote &v, uint32_t n_reads, uint32_t n_shards, uint32_t halo) {
    std::vector<Vote> out(n_shards);
    auto shard_of = [&](uint32_t r) { return std::min<uint32_t>(n_shards - 1, (uint32_t)((uint64_t)r * n_shards / n_reads)); };
    auto near_cut = [&](uint32_t r) -> int { // the cut (1 .. n_shards - 1) the read lies close to, or 0
        for (uint32_t c = 1; c < n_shards; ++c) {
            const uint32_t at = (uint32_t)(((uint64_t)c * n_reads + n_shards - 1) / n_shards); // first read of shard c
            if (r + halo >= at && r < at + halo) return (int)c;
        }
        return 0;
    };
    for (size_t i = 0; i < v.key.size(); ++i) {
        const uint32_t a = (uint32_t)(v.key[i] >> 32), b = (uint32_t)v.key[i], same = v.cnt[i] & 0xFFFFu, neg = v.cnt[i] >> 16;
        const int c = near_cut(a);
        if (c && c == near_cut(b)) {
            const uint32_t s1 = rng() % (same + 1), n1 = rng() % (neg + 1);
            if (s1 | n1) out[c - 1].pair(a, b, s1, n1);
            if ((same - s1) | (neg - n1)) out[c].pair(a, b, same - s1, neg - n1);
        } else {
            out[shard_of(a)].pair(a, b, same, neg);
        }
    }
    for (size_t i = 0; i < v.read_id.size(); ++i) {
        const uint32_t r = v.read_id[i];
        const int c = near_cut(r);
        if (!c) {
            out[shard_of(r)].read(r, v.first_pos[i], v.ref_w[i], v.flags[i]);
            continue;
        }
        const bool votes = v.flags[i] & 1, first_left = rng() % 2;
        const int32_t w1 = (int32_t)(rng() % 5) - 2;
        uint8_t f1 = (uint8_t)(v.flags[i] & (rng() % 8)), f2 = (uint8_t)(v.flags[i] & ~f1 & 6);
        if (rng() % 2) f2 |= v.flags[i] & 6; // (a flag may also come from both)
        // the first vote is the rightmost region over the shards: one keeps it, the other one votes further left or not at all
        const uint32_t lower = votes && v.first_pos[i] > 1 && rng() % 2 ? 1 + rng() % (v.first_pos[i] - 1) : 0xFFFFFFFFu;
        f1 = (uint8_t)((f1 & 6) | (votes && (first_left || lower != 0xFFFFFFFFu) ? 1 : 0));
        f2 = (uint8_t)((f2 & 6) | (votes && (!first_left || lower != 0xFFFFFFFFu) ? 1 : 0));
        out[c - 1].read(r, !(f1 & 1) ? 0xFFFFFFFFu : first_left ? v.first_pos[i] : lower, w1, f1);
        out[c].read(r, !(f2 & 1) ? 0xFFFFFFFFu : first_left ? lower : v.first_pos[i], v.ref_w[i] - w1, f2);
    }
    return out;
}

static void merge_scenario() {
    std::mt19937 rng(11);
    size_t shared = 0;
    for (int t = 0; t < 200; ++t) {
        const uint32_t n_reads = 30 + rng() % 70, n_shards = 2 + t % 2;
        const Vote v = small_vote(rng, n_reads, 1 + rng() % 40);
        for (bool use_all : {false, true}) {
            const Outcome whole = decide_votes({v}, n_reads, use_all);
            std::vector<Vote> cut = cut_vote(rng, v, n_reads, n_shards, 1 + rng() % 8);
            size_t n_cut = 0;
            for (const Vote &c : cut) n_cut += c.key.size();
            shared += n_cut - v.key.size();
            CHECK(decide_votes(cut, n_reads, use_all) == whole);
            CHECK(decide_votes(cut, n_reads, use_all, true) == whole);
            // an unsorted shard, some of its pairs in two pieces: the same answer as its sorted form
            Vote &u = cut[rng() % n_shards];
            for (size_t i = 0, n = u.key.size(); i < n; ++i) {
                const uint32_t same = u.cnt[i] & 0xFFFFu, neg = u.cnt[i] >> 16;
                if (rng() % 4 || !same || !neg) continue;
                u.cnt[i] = same;
                u.key.push_back(u.key[i]), u.cnt.push_back(neg << 16);
            }
            for (size_t i = u.key.size(); i > 1; --i) {
                const size_t j = rng() % i;
                std::swap(u.key[i - 1], u.key[j]), std::swap(u.cnt[i - 1], u.cnt[j]);
            }
            CHECK(decide_votes(cut, n_reads, use_all) == whole);
        }
    }
    CHECK(shared > 200); // (pairs that both shards at a cut hold: their counts were added)
    // refusals, at both places where counts are added (the merge of two sorted votes, the duplicates of an unsorted one)
    auto one = [](std::vector<std::pair<uint64_t, uint32_t>> ps, std::vector<uint32_t> ids) {
        Vote v;
        for (auto &p : ps) v.key.push_back(p.first), v.cnt.push_back(p.second);
        for (uint32_t r : ids) v.read(r, 100 + r, 0, 1);
        return v;
    };
    const uint64_t k12 = (uint64_t)1 << 32 | 2, k23 = (uint64_t)2 << 32 | 3;
    VoteData vd;
    CHECK(merge({one({{k12, 0xFFFFu}}, {1, 2}), one({{k12, 1u}}, {})}, 8, vd) == NP2_E_UNSUPPORTED);
    CHECK(merge({one({{k12, 0xFFFFu << 16}}, {1, 2}), one({{k12, 1u << 16}}, {})}, 8, vd) == NP2_E_UNSUPPORTED);
    CHECK(merge({one({{k12, 0xFFFEu | 0xFFFEu << 16}}, {1, 2}), one({{k12, 1u | 1u << 16}}, {})}, 8, vd) == NP2_OK);
    CHECK(vd.n_pairs() == 1 && vd.cnts()[0] == 0xFFFFFFFFu);
    CHECK(merge({one({{k23, 1u}, {k12, 0xFFFFu}, {k12, 1u}}, {1, 2, 3})}, 8, vd) == NP2_E_UNSUPPORTED);
    CHECK(merge({one({{k23, 1u}, {k12, 0xFFFFu << 16}, {k12, 1u << 16}}, {1, 2, 3})}, 8, vd) == NP2_E_UNSUPPORTED);
    CHECK(merge({one({{k23, 1u}, {k12, 2u}, {k12, 1u << 16}}, {1, 2, 3})}, 8, vd) == NP2_OK);
    CHECK(vd.n_pairs() == 2 && vd.keys()[0] == k12 && vd.cnts()[0] == (2u | 1u << 16) && !vd.view_key);
    CHECK(merge({one({{(uint64_t)1 << 32 | 8, 1u}}, {1})}, 8, vd) == NP2_E_ARG);
    CHECK(merge({one({{(uint64_t)8 << 32 | 9, 1u}}, {1})}, 8, vd) == NP2_E_ARG);
    CHECK(merge({one({{k12, 1u}}, {1, 2, 8})}, 8, vd) == NP2_E_ARG);
    CHECK(merge({one({{k12, 1u}}, {1, 2}), one({}, {7, 9})}, 8, vd) == NP2_E_ARG);
    // one sorted vote is not copied
    const std::vector<Vote> s{one({{k12, 1u}, {k23, 2u}}, {1, 2, 3})};
    CHECK(merge(s, 8, vd) == NP2_OK);
    CHECK(vd.view_key == s[0].key.data() && vd.view_cnt == s[0].cnt.data() && vd.view_n == 2 && vd.pair_key.empty());
    CHECK(vd.any && vd.first_key[2] == 0xFFFFFFFEu - 102 && vd.first_key[4] == 0xFFFFFFFFu);
}

static uint64_t hash_of(const std::vector<uint32_t> &v) { // FNV-1a over the ids
    uint64_t h = 1469598103934665603ull;
    for (uint32_t x : v)
        for (int i = 0; i < 4; ++i) h = (h ^ ((x >> (8 * i)) & 0xFFu)) * 1099511628211ull;
    return h;
}

// a diploid pileup's vote at a size where every threaded path of the host vote runs: 60 000 reads of two haplotypes, each
// paired with 20 of the 40 reads above it — agreeing with its own haplotype, disagreeing with the other, 3 % noise —,
// a weight against the contig for every third read, 2 % of the other haplotype's reads flagged
static int threads_scenario() {
    const uint32_t n_reads = 60001;
    std::mt19937 rng(3);
    Vote v;
    std::vector<uint8_t> hap(n_reads);
    for (auto &h : hap) h = rng() & 1;
    for (uint32_t a = 1; a < n_reads; ++a)
        for (uint32_t d = 1; d <= 40; ++d) {
            if ((rng() & 1) || a + d >= n_reads) continue;
            const bool agree = (hap[a] == hap[a + d]) != (rng() % 100 < 3);
            v.pair(a, a + d, agree ? 1 + rng() % 3 : 0, agree ? 0 : 1 + rng() % 4);
        }
    for (uint32_t r = 1; r < n_reads; ++r) {
        const bool seen = r % 3 == 0;
        v.read(r, 0x7FFFFFFFu - r * 16, seen ? (hap[r] ? -2 : 2) : 0, (uint8_t)(1 | (seen ? 2 : 0) | (hap[r] && rng() % 50 == 0 ? 4 : 0)));
    }
    if (v.key.size() < (1u << 18) || 2 * v.key.size() < (1u << 20)) return fprintf(stderr, "generated vote too small\n"), 1;
    const Outcome pairs = decide_votes({v}, n_reads, false), rows = decide_votes({v}, n_reads, false, true);
    if (pairs.rc != NP2_OK || rows.rc != NP2_OK || pairs.losers.size() < 1000)
        return fprintf(stderr, "not decided: %d %d, %zu losers\n", pairs.rc, rows.rc, pairs.losers.size()), 1;
    printf("pairs %016llx\nrows %016llx\n", (unsigned long long)hash_of(pairs.losers), (unsigned long long)hash_of(rows.losers));
    return 0;
}

template <class T> static bool load(const std::string &path, std::vector<T> &v) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    const bool ok = n >= 0 && (size_t)n % sizeof(T) == 0 && fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}
static bool store(const std::string &path, const std::vector<uint32_t> &v) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), 4, v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}
static int recorded_scenario(const std::string &dir, uint32_t n_reads) {
    Vote v;
    if (!load(dir + "/pair_key.u64", v.key) || !load(dir + "/pair_cnt.u32", v.cnt) || !load(dir + "/read_id.u32", v.read_id) ||
        !load(dir + "/first_pos.u32", v.first_pos) || !load(dir + "/ref_w.i32", v.ref_w) || !load(dir + "/flags.u8", v.flags) ||
        v.key.size() != v.cnt.size() || v.read_id.size() != v.first_pos.size() || v.read_id.size() != v.ref_w.size() ||
        v.read_id.size() != v.flags.size())
        return fprintf(stderr, "cannot read the vote's arrays from %s\n", dir.c_str()), 1;
    const Outcome whole = decide_votes({v}, n_reads, false);
    // cut in two: the pairs split in the middle, the per-read records with the first half
    Vote a = v, b;
    const size_t h = v.key.size() / 2;
    a.key.resize(h), a.cnt.resize(h);
    b.key.assign(v.key.begin() + (long)h, v.key.end()), b.cnt.assign(v.cnt.begin() + (long)h, v.cnt.end());
    const Outcome cut = decide_votes({a, b}, n_reads, false);
    if (whole.rc != NP2_OK || cut.rc != NP2_OK) return fprintf(stderr, "not decided: %d %d\n", whole.rc, cut.rc), 1;
    if (!store(dir + "/losers_whole.u32", whole.losers) || !store(dir + "/losers_cut.u32", cut.losers)) return fprintf(stderr, "cannot write the losers\n"), 1;
    return 0;
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "rows") rows_scenario();
    else if (what == "merge") merge_scenario();
    else if (what == "threads") return threads_scenario();
    else if (what == "recorded" && argc == 4) failures += recorded_scenario(argv[2], (uint32_t)strtoul(argv[3], nullptr, 10));
    else return fprintf(stderr, "usage: vote_host_test rows | merge | threads | recorded <dir> <n_reads>\n"), 2;
    if (failures) return fprintf(stderr, "%d check(s) failed\n", failures), 1;
    printf("ok\n");
    return 0;
}
