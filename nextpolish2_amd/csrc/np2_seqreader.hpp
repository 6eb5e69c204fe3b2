// The sequence-file reader of the k-mer counter and of the read binner (np2_kcount_host.cpp, np2_bin_host.cpp): FASTA
// (multi-line joined) / FASTQ (the 4-line rule) / one-sequence-per-line text, plain or gzip (zlib's gzread: multi-member
// files work through it), into the separator stream: every read's bytes as they stand, '\r' dropped, one '\n' after each
// read; empty reads are kept, a last line needs no newline.  A caller that wants the records' names passes `hdr`; one that
// wants the FASTQ quality lines passes `qual` and receives a second stream of the same shape (parse_file_qual).
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "np2_abi.hpp"

namespace np2seq {
using np2h::Np2Error;

// ---------------------------------------------------------------------------------------------------------------
// sequence text -> separator stream
// ---------------------------------------------------------------------------------------------------------------
struct SeqParser {
    enum Fmt { UNKNOWN, FASTA, FASTQ, LINES } fmt = UNKNOWN;
    uint32_t line = 0;   // FASTQ: line of the record, 0 .. 3 (the 4-line rule: a quality line may begin with '@' or '>')
    bool bol = true;     // at the beginning of a line
    bool skip = false;   // the current line holds no sequence
    bool blank = false;  // FASTQ: a blank line between records (does not advance `line`)
    bool open = false;   // FASTA: a record has begun and its separator is still owed
    bool head = false;   // the current line names a record (FASTA '>' line, FASTQ line 0)
    template <class Put> void feed(const uint8_t *p, size_t n, Put &&put) {
        feed(p, n, put, [](const uint8_t *, size_t, bool) {});
    }
    // hdr(nullptr, 0, true): a record begins (FASTA / FASTQ: at its header line; one sequence per line: at every line);
    // hdr(bytes, n, false): the next bytes of its header line, '>' / '@' included, in as many calls as the input arrives in
    template <class Put, class Hdr> void feed(const uint8_t *p, size_t n, Put &&put, Hdr &&hdr) {
        feed(p, n, put, hdr, [](const uint8_t *, size_t) {});
    }
    // qual(bytes, n): the bytes of FASTQ line 3 without '\r', and one '\n' where `put` got the record's separator: the
    // quality stream has the length and the separator offsets of the sequence stream when every record's two lines agree
    template <class Put, class Hdr, class Qual> void feed(const uint8_t *p, size_t n, Put &&put, Hdr &&hdr, Qual &&qual) {
        static const uint8_t NL = '\n';
        size_t i = 0;
        while (i < n) {
            if (bol) {
                const uint8_t c = p[i];
                if (fmt == UNKNOWN) {
                    if (c == '\n' || c == '\r') {
                        ++i;
                        continue;
                    }
                    fmt = c == '>' ? FASTA : c == '@' ? FASTQ : LINES;
                }
                if (fmt == FASTA) {
                    skip = c == '>';
                    if (skip) {
                        if (open) put(&NL, 1);
                        open = true;
                    }
                    head = skip;
                } else if (fmt == FASTQ) {
                    blank = line == 0 && (c == '\n' || c == '\r');
                    skip = blank || line != 1;
                    head = line == 0 && !blank;
                } else {
                    skip = false;
                    head = false;
                }
                if (head || fmt == LINES) hdr(nullptr, 0, true);
                bol = false;
            }
            const uint8_t *e = (const uint8_t *)memchr(p + i, '\n', n - i);
            const size_t end = e ? (size_t)(e - p) : n;
            if (head && end > i) hdr(p + i, end - i, false);
            auto without_cr = [&](auto &sink) { // the line's bytes without '\r'
                size_t a = i;
                while (a < end) {
                    const uint8_t *cr = (const uint8_t *)memchr(p + a, '\r', end - a);
                    const size_t b = cr ? (size_t)(cr - p) : end;
                    if (b > a) sink(p + a, b - a);
                    a = b + 1;
                }
            };
            if (!skip) without_cr(put);
            else if (fmt == FASTQ && line == 3) without_cr(qual);
            i = end;
            if (e) {
                ++i;
                bol = true;
                if (fmt == FASTQ) {
                    if (line == 1) put(&NL, 1);
                    if (line == 3) qual(&NL, 1);
                    if (!blank) line = (line + 1) & 3u;
                } else if (fmt == LINES) {
                    put(&NL, 1);
                }
            }
        }
    }
    template <class Put> void finish(Put &&put) { // a last line without newline
        static const uint8_t NL = '\n';
        if (fmt == FASTA ? open : fmt == FASTQ ? (!bol && line == 1) : (fmt == LINES && !bol)) put(&NL, 1);
        open = false;
    }
    template <class Put, class Qual> void finish(Put &&put, Qual &&qual) { // ... and a last quality line without one (or none)
        static const uint8_t NL = '\n';
        const bool owed = fmt == FASTQ && line == 3;
        finish(put);
        if (owed) qual(&NL, 1);
    }
};

// a whole file, 1 MiB at a time: chunk(bytes, n) until the end (true) or until stop() says so (false); throws NP2_E_ARG
// for a file that cannot be opened or a damaged / truncated gzip
template <class Chunk> bool read_chunks(const std::string &path, const std::function<bool()> &stop, Chunk &&chunk) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) throw Np2Error(NP2_E_ARG, "cannot open " + path);
    std::unique_ptr<gzFile_s, int (*)(gzFile)> guard(f, gzclose);
    gzbuffer(f, 1 << 20);
    std::vector<uint8_t> buf((size_t)1 << 20);
    for (;;) {
        if (stop && stop()) return false;
        const int got = gzread(f, buf.data(), (unsigned)buf.size());
        int zerr = Z_OK;
        const char *zmsg = gzerror(f, &zerr);
        if (got < 0 || (zerr != Z_OK && zerr != Z_STREAM_END))
            throw Np2Error(NP2_E_ARG, path + ": cannot read the sequence file (" + (zmsg && *zmsg ? zmsg : "damaged or truncated gzip") + ")");
        if (got == 0) return true;
        chunk(buf.data(), (size_t)got);
    }
}
// a whole file through the parser
template <class Put, class Hdr> void parse_file(const std::string &path, Put &&put, const std::function<bool()> &stop, Hdr &&hdr) {
    SeqParser ps;
    if (read_chunks(path, stop, [&](const uint8_t *p, size_t n) { ps.feed(p, n, put, hdr); })) ps.finish(put);
}
template <class Put> void parse_file(const std::string &path, Put &&put, const std::function<bool()> &stop) {
    parse_file(path, put, stop, [](const uint8_t *, size_t, bool) {});
}

// What a quality-filtering call checks of every FASTQ record while its two lines go by: the quality line is as long as
// the sequence.  The sinks call seq_bytes / seq_end / qual_bytes / qual_end; NP2_E_ARG names the file and the 1-based record.
struct RecordCheck {
    std::string path;
    uint64_t record = 0; // complete records of this file
    uint64_t sl = 0, ql = 0;
    bool seq_done = false;
    [[noreturn]] void mismatch() const {
        throw Np2Error(NP2_E_ARG, path + ": record " + std::to_string(record + 1) + ": the quality line is not as long as the sequence");
    }
    void seq_bytes(size_t n) { sl += n; }
    void seq_end() { seq_done = true; }
    void qual_bytes(size_t n) {
        if (!seq_done || ql + n > sl) mismatch();
        ql += n;
    }
    void qual_end() {
        if (!seq_done || ql != sl) mismatch();
        ++record, sl = ql = 0, seq_done = false;
    }
    void file_end() const { // a sequence line the file has no quality line for
        if (seq_done || sl) mismatch();
    }
    void file_begin(const std::string &p) { path = p, record = 0, sl = ql = 0, seq_done = false; }
};

// A whole FASTQ file through the parser with its quality lines: put(bytes, n) and qual(bytes, n) receive the two streams
// (a separator arrives as one '\n' of its own).  NP2_E_ARG, naming the file: FASTA or one sequence per line.  The caller
// checks the records (RecordCheck) in its sinks and at the end.
template <class Put, class Qual, class Hdr>
void parse_file_qual(const std::string &path, Put &&put, Qual &&qual, const std::function<bool()> &stop, Hdr &&hdr) {
    SeqParser ps;
    const bool whole = read_chunks(path, stop, [&](const uint8_t *p, size_t n) {
        if (ps.fmt == SeqParser::UNKNOWN)
            for (size_t i = 0; i < n; ++i)
                if (p[i] != '\n' && p[i] != '\r') {
                    if (p[i] != '@')
                        throw Np2Error(NP2_E_ARG, path + ": quality filtering needs FASTQ input, and this is " +
                                                      (p[i] == '>' ? "FASTA" : "one sequence per line"));
                    break;
                }
        ps.feed(p, n, put, hdr, qual);
    });
    if (whole) ps.finish(put, qual);
}

// Keeps the name of the record the reader is in, from its `hdr` calls: the header up to the first whitespace, without
// '>' / '@'.  close() is called where the record's separator is put and hands the name out; a record without a name (a
// file of one sequence per line has none) is named by its 1-based number in the file.
struct NameCollector {
    std::string cur;
    bool done = true, lead = false;
    uint64_t n_closed = 0;
    void operator()(const uint8_t *p, size_t n, bool begin) {
        if (begin) {
            cur.clear();
            done = false, lead = true;
            return;
        }
        if (done) return;
        size_t i = 0;
        if (lead && n) ++i, lead = false; // '>' / '@'
        for (; i < n; ++i) {
            const uint8_t c = p[i];
            if (c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f') {
                done = true;
                return;
            }
            cur.push_back((char)c);
        }
    }
    std::string close() {
        ++n_closed;
        std::string s = cur.empty() ? std::to_string(n_closed) : cur;
        cur.clear();
        done = true;
        return s;
    }
};

} // namespace np2seq
