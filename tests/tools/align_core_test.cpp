// The aligner's rule (csrc/np2_align_core.hpp, through the one-read-at-a-time host program of csrc/np2_align_cpu.hpp) built with
// a plain C++ compiler, for tests/test_align_cpu.py: with and without the address and undefined-behaviour sanitizers.
//   align_core_test ASM_STREAM READ_STREAM k w max_occ lookback max_gap bandwidth min_cnt min_score
//                   match mismatch gap_open gap_ext band end_bonus ext_max max_cells
// prints the nine counts, then per read "tid flag pos end mapq n_cigar nm as CIGAR" (CIGAR "*" when there is none).
//   align_core_test finish REFERENCE READ t_start RAW_CIGAR
// runs the rule's last pass (ends, left-alignment, pos, NM, AS with the default scores) on a hand-made alignment of the whole
// read to the reference from t_start on and prints "pos end nm as CIGAR".
//   align_core_test core PAIRS_FILE band [match mismatch gap_open gap_ext]
// treats each line "REFERENCE READ" of the file as the bases between two pins: the trim and the class (np2aln::classify) and,
// for a core, the banded matrix (dp_slot) with the default scores or the given ones; prints "kind over pre suf tl ql score" per
// line (tl, ql: the core's sides; score 0 without a matrix).
//   align_core_test chains CASE_FILE
// runs align_read on caller-built hits and chains, as np2_align_chains_host does behind its checks.  The file: a line "k match
// mismatch gap_open gap_ext band end_bonus ext_max max_cells", a line with the number of contigs, one contig per line, a line
// with the number of reads, then per read "SEQ tid rev mapq n r q r q ..." (tid -1 and n 0: unmapped).  Prints what the first
// form prints.
// With a last argument "sam" the first form prints the SAM text instead (reads named r0, r1, ..., sequences 1, 2, ...).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_align_cpu.hpp"

static bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

static std::string cigar_text(const uint32_t *w, uint32_t n) {
    std::string s;
    for (uint32_t i = 0; i < n; ++i) s += std::to_string(w[i] >> 4) + "MIDNS"[w[i] & 15u];
    return n ? s : "*";
}

static int finish(char **argv) {
    const std::string t = argv[2], q = argv[3];
    const uint32_t t_start = (uint32_t)strtoul(argv[4], nullptr, 10);
    std::vector<uint32_t> a;
    for (const char *p = argv[5]; *p;) {
        char *e;
        const uint32_t len = (uint32_t)strtoul(p, &e, 10);
        const char *op = strchr("MIDNS", *e);
        if (!op || !*e) return 2;
        a.push_back(len << 4 | (uint32_t)(op - "MIDNS"));
        p = e + 1;
    }
    const np2aln::Opts o{1, 4, 6, 2, 32, 5, 2048, 1u << 23};
    const np2aln::Seqs s{(const uint8_t *)t.data(), (uint32_t)t.size(), (const uint8_t *)q.data(), (uint32_t)q.size(), 0};
    std::vector<uint32_t> b(2 * a.size() + 2);
    np2aln::Rec rec{};
    np2aln::finish_ops(s, a.data(), (uint32_t)a.size(), t_start, o, b.data(), &rec);
    np2aln::score_ops(s, b.data(), rec.n_cigar, rec.pos, o, 0, 1, &rec.nm, &rec.as, &rec.end);
    printf("%u %u %u %d %s\n", rec.pos, rec.end, rec.nm, rec.as, cigar_text(b.data(), rec.n_cigar).c_str());
    return 0;
}

static int core(int argc, char **argv) {
    np2aln::Opts o{1, 4, 6, 2, (uint32_t)strtoul(argv[3], nullptr, 10), 5, 2048, 1u << 23};
    if (argc == 8) {
        uint32_t *f[4] = {&o.match, &o.mismatch, &o.gap_open, &o.gap_ext};
        for (int i = 0; i < 4; ++i) *f[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
    }
    if (const char *bad = np2aln::check_opts(o)) {
        fprintf(stderr, "argument: %s\n", bad);
        return 3;
    }
    std::vector<uint8_t> text;
    if (!slurp(argv[2], text)) {
        fprintf(stderr, "cannot read the pairs\n");
        return 2;
    }
    std::vector<uint8_t> tb;
    std::vector<int32_t> H, F;
    for (size_t at = 0; at < text.size();) { // lines "REFERENCE READ"
        const size_t sp = std::find(text.begin() + (std::ptrdiff_t)at, text.end(), (uint8_t)' ') - text.begin();
        const size_t nl = std::find(text.begin() + (std::ptrdiff_t)at, text.end(), (uint8_t)'\n') - text.begin();
        if (sp >= nl || nl >= text.size()) return 2;
        const np2aln::Seqs s{text.data() + at, (uint32_t)(sp - at), text.data() + sp + 1, (uint32_t)(nl - sp - 1), 0};
        np2aln::Slot x{};
        x.tl = s.tlen, x.ql = s.qlen, x.kind = np2aln::K_RAW;
        const uint64_t cells = np2aln::classify(s, x, o, o.max_cells);
        np2aln::Res res{};
        if (cells) {
            tb.assign(cells, 0);
            res = np2aln::dp_slot(s, x, 0, o, tb.data(), H, F);
        }
        printf("%u %u %u %u %u %u %d\n", x.kind, x.over, x.pre, x.suf, x.tl, x.ql, res.score);
        at = nl + 1;
    }
    return 0;
}

static void print_rec(std::string &out, const np2aln::Rec &rec, const std::vector<uint32_t> &cigar) {
    char line[160];
    snprintf(line, sizeof line, "%d %u %u %u %u %u %u %d ", rec.tid, rec.flag, rec.pos, rec.end, rec.mapq, rec.n_cigar, rec.nm, rec.as);
    out += line + cigar_text(cigar.data(), rec.n_cigar) + "\n";
}

static int chains(char **argv) {
    std::vector<uint8_t> text;
    if (!slurp(argv[2], text)) {
        fprintf(stderr, "cannot read the case\n");
        return 2;
    }
    text.push_back(0);
    const char *p = (const char *)text.data();
    const auto number = [&]() { // the next whole number (a leading '-' allowed)
        char *e;
        const long long v = strtoll(p, &e, 10);
        if (e == p) {
            fprintf(stderr, "a number is missing\n");
            exit(2);
        }
        p = e;
        return v;
    };
    const auto word = [&]() {
        while (*p == ' ' || *p == '\n') ++p;
        const char *b = p;
        while (*p && *p != ' ' && *p != '\n') ++p;
        return std::string(b, p);
    };
    const uint32_t k = (uint32_t)number();
    np2aln::Opts ao{};
    uint32_t *afields[8] = {&ao.match, &ao.mismatch, &ao.gap_open, &ao.gap_ext, &ao.band, &ao.end_bonus, &ao.ext_max, &ao.max_cells};
    for (int i = 0; i < 8; ++i) *afields[i] = (uint32_t)number();
    if (const char *bad = np2aln::check_opts(ao)) {
        fprintf(stderr, "argument: %s\n", bad);
        return 3;
    }
    std::vector<std::string> contigs((size_t)number());
    for (std::string &c : contigs) c = word();
    const size_t n_reads = (size_t)number();
    np2aln::Scratch w;
    uint64_t c[np2aln::C_N] = {};
    std::string out;
    for (size_t i = 0; i < n_reads; ++i) {
        const std::string seq = word();
        np2map::Hit h{};
        h.tid = (int32_t)number(), h.rev = (uint32_t)number(), h.mapq = (uint32_t)number(), h.n = (uint32_t)number();
        h.qlen = (uint32_t)seq.size();
        std::vector<uint32_t> chain(2 * (size_t)h.n), cigar;
        for (uint32_t &x : chain) x = (uint32_t)number();
        np2aln::Rec rec = np2aln::unaligned_rec();
        if (h.tid >= 0) {
            if ((size_t)h.tid >= contigs.size() || h.n < 1) return 2;
            const std::string &t = contigs[(size_t)h.tid];
            for (uint32_t a = 0; a < h.n; ++a)
                if (chain[2 * a] + 1 < k || chain[2 * a] >= t.size() || chain[2 * a + 1] + 1 < k || chain[2 * a + 1] >= seq.size()) return 2;
            rec = np2aln::align_read((const uint8_t *)t.data(), (uint32_t)t.size(), (const uint8_t *)seq.data(), h, chain.data(), k, ao, ao.max_cells, w,
                                     cigar, c);
        }
        print_rec(out, rec, cigar);
    }
    for (int i = 0; i < np2aln::C_N; ++i) printf("%llu%c", (unsigned long long)c[i], i + 1 < np2aln::C_N ? ' ' : '\n');
    fputs(out.c_str(), stdout);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "finish")) return finish(argv);
    if ((argc == 4 || argc == 8) && !strcmp(argv[1], "core")) return core(argc, argv);
    if (argc == 3 && !strcmp(argv[1], "chains")) return chains(argv);
    const bool sam = argc == 20 && !strcmp(argv[19], "sam");
    if (argc != 19 && !sam) {
        fprintf(stderr, "usage: align_core_test ASM_STREAM READ_STREAM (8 mapping options) (8 alignment options)\n");
        return 2;
    }
    std::vector<uint8_t> a, r;
    if (!slurp(argv[1], a) || !slurp(argv[2], r)) {
        fprintf(stderr, "cannot read the streams\n");
        return 2;
    }
    np2map::Opts o{};
    uint32_t *fields[8] = {&o.k, &o.w, &o.max_occ, &o.lookback, &o.max_gap, &o.bandwidth, &o.min_cnt, &o.min_score};
    for (int i = 0; i < 8; ++i) *fields[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
    np2aln::Opts ao{};
    uint32_t *afields[8] = {&ao.match, &ao.mismatch, &ao.gap_open, &ao.gap_ext, &ao.band, &ao.end_bonus, &ao.ext_max, &ao.max_cells};
    for (int i = 0; i < 8; ++i) *afields[i] = (uint32_t)strtoul(argv[11 + i], nullptr, 10);
    bool unsupported = false;
    if (const char *bad = np2map::check_opts(o, &unsupported)) {
        fprintf(stderr, "%s: %s\n", unsupported ? "unsupported" : "argument", bad);
        return 3;
    }
    if (const char *bad = np2aln::check_opts(ao)) {
        fprintf(stderr, "argument: %s\n", bad);
        return 3;
    }
    std::vector<uint64_t> a_ends, r_ends;
    if (!np2map::stream_ends(a.data(), a.size(), a_ends) || !np2map::stream_ends(r.data(), r.size(), r_ends)) {
        fprintf(stderr, "a stream does not end in a newline\n");
        return 3;
    }
    np2map::HostIndex ix;
    ix.build(a.data(), a_ends, o.k, o.w);
    np2map::ReadCounts rc;
    np2aln::Scratch w;
    uint64_t c[np2aln::C_N] = {};
    std::string out;
    std::vector<std::string> names;
    std::vector<uint64_t> lens;
    for (size_t i = 0; i < a_ends.size(); ++i) names.push_back(std::to_string(i + 1)), lens.push_back(a_ends[i] - (i ? a_ends[i - 1] + 1 : 0));
    if (sam) np2aln::sam_header(out, names, lens);
    uint64_t from = 0;
    for (size_t i = 0; i < r_ends.size(); ++i) {
        np2map::Hit h;
        std::vector<uint32_t> chain, cigar;
        np2map::map_read(ix, r.data() + from, (uint32_t)(r_ends[i] - from), o, &h, &chain, &rc);
        np2aln::Rec rec = np2aln::unaligned_rec();
        if (h.tid >= 0) {
            const uint64_t t_at = h.tid ? a_ends[(size_t)h.tid - 1] + 1 : 0;
            rec = np2aln::align_read(a.data() + t_at, (uint32_t)(a_ends[(size_t)h.tid] - t_at), r.data() + from, h, chain.data(), o.k, ao,
                                     ao.max_cells, w, cigar, c);
        }
        if (sam) {
            const std::string qname = "r" + std::to_string(i);
            np2aln::sam_line(out, qname.data(), qname.size(), rec, h, cigar.data(), r.data() + from, (uint32_t)(r_ends[i] - from),
                             rec.tid >= 0 ? &names[(size_t)rec.tid] : nullptr);
            from = r_ends[i] + 1;
            continue;
        }
        from = r_ends[i] + 1;
        print_rec(out, rec, cigar);
    }
    if (!sam)
        for (int i = 0; i < np2aln::C_N; ++i) printf("%llu%c", (unsigned long long)c[i], i + 1 < np2aln::C_N ? ' ' : '\n');
    fputs(out.c_str(), stdout);
    return 0;
}
