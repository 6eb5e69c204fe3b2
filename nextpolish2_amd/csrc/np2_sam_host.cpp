// Host driver of the SAM reader (include/np2_io.h: np2_sam_*; kernels: np2_sam.hip).
//
// A reader thread takes the bytes of the files as they stand (zlib's gzread: plain and gzip alike, "-" is standard input)
// into pinned pieces that end at a line boundary, reads the header lines of each file on the way and hands the rest over;
// the calling thread copies a piece to the device, finds its lines, judges them, asks for the three totals, grows the resident
// buffers where they are short (a larger block and a device-to-device copy, after a look at the free memory) and packs.
// An input that is a BAM (include/np2_io.h: "BAM input") goes the same way with other pieces: whole BGZF blocks as they lie in
// the file, which the calling thread uploads, inflates and checks (k_bgzf_inflate, k_bgzf_crc32) behind the bytes of a record
// the piece before left unfinished, walks (k_bamin_walk), judges (k_bamin_fields), scans and packs (k_bamin_pack) into the same
// resident buffers.
// After the last piece: keys -> stable sort -> records and CIGAR words gathered into sorted order.  The sorted keys come
// back to the host once; a contig's range is a binary search in them.
#include "../../include/np2_io.h"
#include "np2_bamfile.hpp"
#include "np2_bamin.hpp"
#include "np2_bgzf.hpp"
#include "np2_ctx.hpp"
#include "np2_inflate.hpp"
#include "np2_inflate_core.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_sam.hpp"
#include "np2_sam_accum.hpp"
#include "np2_sam_handle.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <zlib.h>
#include <unistd.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>

namespace {
using np2h::Np2Error;

struct Hooks {
    size_t piece = (size_t)32 << 20;
    bool profile = false; // NP2_SAM_PROFILE: one line on stderr with the kernels' times apart (tools/sam_probe.py)
    Hooks() { // read once per call, like the other NP2_* switches
        piece = (size_t)np2h::test_hook("NP2_SAM_TEST_PIECE", 64, 1ll << 30, (long long)piece);
        profile = getenv("NP2_SAM_PROFILE") != nullptr;
    }
};

// where the bytes come from: a file (plain or gzip), standard input, or host memory
struct Source {
    gzFile f = nullptr;
    const uint8_t *mem = nullptr;
    size_t mem_n = 0, mem_at = 0;
    std::string name;
    ~Source() {
        if (f) gzclose(f);
    }
    void open(const std::string &path) {
        name = path == "-" ? "standard input" : path;
        f = path == "-" ? gzdopen(dup(0), "rb") : gzopen(path.c_str(), "rb");
        if (!f) throw Np2Error(NP2_E_ARG, "cannot open " + name);
        gzbuffer(f, 1 << 20);
    }
    size_t read(uint8_t *dst, size_t n) { // 0: the end
        if (!f) {
            const size_t take = std::min(n, mem_n - mem_at);
            if (take) memcpy(dst, mem + mem_at, take);
            mem_at += take;
            return take;
        }
        const int got = gzread(f, dst, (unsigned)std::min<size_t>(n, (size_t)1 << 30));
        int zerr = Z_OK;
        const char *zmsg = gzerror(f, &zerr);
        if (got < 0 || (zerr != Z_OK && zerr != Z_STREAM_END))
            throw Np2Error(NP2_E_ARG, name + ": cannot read the SAM text (" + (zmsg && *zmsg ? zmsg : "damaged or truncated gzip") + ")");
        return (size_t)got;
    }
};

struct Piece {
    int buf = -1;
    size_t off = 0, n = 0;  // the alignment lines of the piece: bytes [off, off + n) of its buffer, ending with '\n'
    int file = 0;
    uint64_t first_line = 0; // 1-based number, in its file, of the line at `off`
    // a piece of a BAM: bytes [0, n) of the buffer are whole BGZF blocks, the file's bytes from file_off on
    bool bam = false, last = false; // last: the file ends with this piece
    uint64_t file_off = 0;
    uint32_t skip = 0;                   // inflated bytes in front of the first record (the end of the header: the file's first piece)
    std::vector<np2h::BgzfBlock> blks;   // the blocks that hold bytes; out_off counts from the piece's first block
    uint32_t n_blocks = 0;               // ... and all of them
};

// the reader thread: pieces in input order through a two-buffer queue
struct Reader {
    const Hooks &hooks;
    std::vector<std::string> paths; // empty: `mem`
    std::vector<char> is_bam;       // per path (np2_sam_open_ex sniffs the files before the reader starts)
    uint64_t bam_files = 0;
    const uint8_t *mem = nullptr;
    size_t mem_n = 0;
    static constexpr int NBUF = 2;
    np2h::PinnedBuf pinned[NBUF];
    uint8_t *pin[NBUF] = {nullptr, nullptr};
    size_t piece = 0;

    std::mutex mu;
    std::condition_variable cv;
    std::deque<Piece> ready;
    std::vector<int> idle;
    bool done = false, stop = false;
    int err_code = 0;
    std::string err_msg;
    np2sam::Refs refs; // of the first file, set before its first piece is handed over
    bool have_refs = false;
    uint64_t lines = 0; // of all files, when done
    std::vector<std::string> extra; // the header lines other than @HD and @SQ, in input order, each once, without '\r' and '\n'
    std::thread th;

    explicit Reader(const Hooks &h) : hooks(h) {}
    ~Reader() {
        {
            std::lock_guard<std::mutex> l(mu);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    void start(size_t bytes_bound) { // bytes_bound: what the input can hold at most, 0 when that is not known
        piece = hooks.piece;
        if (bytes_bound) piece = std::min(piece, std::max<size_t>(bytes_bound + 1, 64));
        const bool any_bam = std::find(is_bam.begin(), is_bam.end(), (char)1) != is_bam.end();
        for (int b = 0; b < NBUF; ++b) { // (a piece of a BAM holds at least one whole block, of up to 64 KiB)
            pin[b] = (uint8_t *)pinned[b].ensure(piece + 64 + (any_bam ? 65536 : 0));
            idle.push_back(b);
        }
        th = std::thread([this] { run(); });
    }
    int acquire() {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return stop || !idle.empty(); });
        if (stop) return -1;
        const int b = idle.back();
        idle.pop_back();
        return b;
    }
    void release(int b) {
        {
            std::lock_guard<std::mutex> l(mu);
            idle.push_back(b);
        }
        cv.notify_all();
    }
    // the calling thread: the next piece (false: the input is through, or the reader failed: see err_code)
    bool next(Piece &p) {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return done || !ready.empty(); });
        if (ready.empty()) return false;
        p = ready.front();
        ready.pop_front();
        return true;
    }
    void file_refs(const np2sam::Refs &r, const std::string &name) {
        std::lock_guard<std::mutex> l(mu);
        if (!have_refs) {
            refs = r, have_refs = true;
        } else if (!(refs == r)) {
            throw Np2Error(NP2_E_ARG, name + ": its @SQ lines differ from those of the first file");
        }
    }
    void one_file(Source &src, int file) {
        np2sam::Refs r;
        bool in_header = true, refs_done = false, eof = false;
        uint64_t line_no = 0; // lines of this file handed over or read as header
        std::vector<uint8_t> carry;
        while (!eof) {
            const int b = acquire();
            if (b < 0) return;
            uint8_t *buf = pin[b];
            size_t fill = carry.size();
            if (fill) memcpy(buf, carry.data(), fill);
            carry.clear();
            while (fill < piece && !eof) {
                const size_t got = src.read(buf + fill, piece - fill);
                eof = got == 0;
                fill += got;
            }
            if (in_header && line_no == 0 && fill >= 4 && !memcmp(buf, "BAM\1", 4)) { // (gzread inflated it: a file was sniffed before)
                release(b);
                throw Np2Error(NP2_E_UNSUPPORTED, src.name + " is a BAM: a BAM is read from a file, not from a stream (SAM text may come from one)");
            }
            if (eof && fill && buf[fill - 1] != '\n') buf[fill++] = '\n'; // (the buffers hold piece + 64 bytes)
            size_t cut = fill;
            while (cut && buf[cut - 1] != '\n') --cut;
            if (fill && !cut) {
                release(b);
                throw Np2Error(NP2_E_UNSUPPORTED, src.name + ": line " + std::to_string(line_no + 1) + " does not fit a piece of " +
                                                      std::to_string(piece) + " bytes");
            }
            carry.assign(buf + cut, buf + fill);
            size_t at = 0;
            while (in_header && at < cut) {
                const size_t nl = (const uint8_t *)memchr(buf + at, '\n', cut - at) - buf;
                const size_t end = nl > at && buf[nl - 1] == '\r' ? nl - 1 : nl;
                if (end > at && buf[at] != '@') {
                    in_header = false;
                    break;
                }
                if (end > at) {
                    const std::string bad = np2sam::header_line(buf, at, end, r);
                    if (!bad.empty()) {
                        release(b);
                        throw Np2Error(NP2_E_ARG, src.name + ": line " + std::to_string(line_no + 1) + ": " + bad);
                    }
                    if (np2sam::header_line_is_carried(buf, at, end)) {
                        std::string line((const char *)buf + at, end - at);
                        std::lock_guard<std::mutex> l(mu);
                        if (std::find(extra.begin(), extra.end(), line) == extra.end()) extra.push_back(std::move(line));
                    }
                }
                at = nl + 1, ++line_no;
            }
            if (!refs_done && (!in_header || eof)) { // the header is through
                try {
                    file_refs(r, src.name);
                } catch (...) {
                    release(b);
                    throw;
                }
                refs_done = true;
            }
            if (at < cut) {
                Piece p;
                p.buf = b, p.off = at, p.n = cut - at, p.file = file, p.first_line = line_no + 1;
                line_no += (uint64_t)std::count(buf + at, buf + cut, (uint8_t)'\n');
                {
                    std::lock_guard<std::mutex> l(mu);
                    ready.push_back(p);
                }
                cv.notify_all();
            } else {
                release(b);
            }
        }
        std::lock_guard<std::mutex> l(mu);
        lines += line_no;
    }
    // A BAM: the header on the host, then whole blocks into the pieces.  A piece ends before the block with which the summed
    // ISIZE would pass the piece size (or the file bytes the buffer's size); it always holds one block.
    void one_bam(const std::string &path, int file) {
        struct Fd {
            int fd = -1;
            ~Fd() {
                if (fd >= 0) close(fd);
            }
        } f;
        f.fd = open(path.c_str(), O_RDONLY);
        struct stat st;
        if (f.fd < 0 || fstat(f.fd, &st) != 0) throw Np2Error(NP2_E_ARG, "cannot open " + path);
        const uint64_t file_len = (uint64_t)st.st_size;
        np2sam::Refs r;
        std::vector<std::string> lines;
        uint64_t pos = 0;
        uint32_t skip = 0;
        np2h::bam_read_header(f.fd, file_len, path, r, lines, &pos, &skip);
        file_refs(r, path);
        {
            std::lock_guard<std::mutex> l(mu);
            ++bam_files;
            for (std::string &line : lines)
                if (std::find(extra.begin(), extra.end(), line) == extra.end()) extra.push_back(std::move(line));
        }
        const size_t room = piece + 65536;
        bool first = true;
        while (first || pos < file_len) {
            const int b = acquire();
            if (b < 0) return;
            uint8_t *buf = pin[b];
            Piece p;
            p.buf = b, p.file = file, p.bam = true, p.file_off = pos, p.skip = first ? skip : 0u;
            first = false;
            size_t fill = 0;
            uint64_t inflated = 0;
            try {
                while (pos < file_len) {
                    uint8_t head[18 + 65536], tail[8];
                    const size_t avail = (size_t)std::min<uint64_t>(file_len - pos, 18);
                    if (!np2h::pread_full(f.fd, head, avail, pos)) throw Np2Error(NP2_E_ARG, "cannot read the file");
                    np2h::BgzfHeader h = np2h::bgzf_header(head, avail, file_len - pos);
                    if (h.need) {
                        if (!np2h::pread_full(f.fd, head, h.need, pos)) throw Np2Error(NP2_E_ARG, "cannot read the file");
                        h = np2h::bgzf_header(head, h.need, file_len - pos);
                    }
                    if (!np2h::pread_full(f.fd, tail, 8, pos + h.bsize - 8)) throw Np2Error(NP2_E_ARG, "cannot read the file");
                    const np2h::BgzfTrailer t = np2h::bgzf_trailer(tail);
                    if (t.isize > 65536) throw Np2Error(NP2_E_ARG, "a BGZF block of more than 65536 bytes (block at file offset " + std::to_string(pos) + ")");
                    if (p.n_blocks && (fill + h.bsize > room || inflated + t.isize > piece)) break;
                    if (!np2h::pread_full(f.fd, buf + fill, h.bsize, pos)) throw Np2Error(NP2_E_ARG, "cannot read the file");
                    if (t.isize) p.blks.push_back(np2h::BgzfBlock{pos, inflated, h.hdr_len, h.clen, t.isize, h.bsize, t.crc});
                    ++p.n_blocks, fill += h.bsize, inflated += t.isize, pos += h.bsize;
                }
            } catch (const Np2Error &e) {
                release(b);
                throw Np2Error(e.code, path + ": " + e.what());
            }
            p.n = fill, p.last = pos >= file_len;
            {
                std::lock_guard<std::mutex> l(mu);
                ready.push_back(std::move(p));
            }
            cv.notify_all();
        }
    }
    void run() {
        try {
            if (paths.empty()) {
                Source src;
                src.mem = mem, src.mem_n = mem_n, src.name = "the text";
                one_file(src, 0);
            }
            for (size_t i = 0; i < paths.size(); ++i) {
                if (i < is_bam.size() && is_bam[i]) {
                    one_bam(paths[i], (int)i);
                    continue;
                }
                Source src;
                src.open(paths[i]);
                one_file(src, (int)i);
            }
        } catch (...) {
            std::lock_guard<std::mutex> l(mu);
            np2h::current_error(err_code, err_msg);
        }
        {
            std::lock_guard<std::mutex> l(mu);
            done = true;
        }
        cv.notify_all();
    }
};

using np2h::elapsed;

// text -> the handle's resident arrays
struct Build : np2h::SamAccum { // (the input-order arrays, their growth and finish(): np2_sam_accum.hpp)
    np2_ctx *cx;
    Hooks hooks;
    uint32_t tie = 1;
    // NP2_SAM_KEEP_NAMES: the lengths of a piece's names, their scan, the first bad line
    DevBuf<uint32_t> d_nname, d_nmoff, d_nbad;
    // NP2_SAM_KEEP_ALL: the sizes of a piece's tails and their scan
    DevBuf<uint32_t> d_tsize, d_taux, d_toff;
    np2h::DevEvent e_t0, e_t1;
    // one piece
    DevBuf<uint8_t> d_text;
    DevBuf<uint32_t> d_end, d_kept, d_ncig, d_nseq, d_koff, d_coff, d_soff;
    DevBuf<np2sam::Line> d_lines;
    DevBuf<np2::SamCtr> d_ctr;
    // the name table
    DevBuf<uint32_t> d_slot, d_noff;
    DevBuf<uint8_t> d_names;
    np2sam::NameTab nt{};
    bool have_nt = false;
    np2h::PinnedBuf pin;
    np2h::DevEvent e_mid;
    float lines_ms = 0;    // k_sam_lines alone, of parse_ms
    // a BAM's pieces: the file bytes, the block table with the CRC32 words behind it, the blocks' status words and the count of
    // failed ones, the inflated stream of this piece and of the one before (whose unfinished record is copied over), the walk
    DevBuf<uint8_t> d_comp, d_inf[2];
    DevBuf<np2::InfBlock> d_blk;
    DevBuf<uint32_t> d_status, d_starts, d_info;
    DevBuf<np2::BaminCtr> d_bctr;
    np2h::PinnedBuf pin_tab;
    np2h::DevEvent e_b0, e_b1, e_b2;
    int cur = 0;             // d_inf[cur] takes this piece
    uint32_t carry_at = 0, carry_n = 0; // the unfinished record: bytes [carry_at, carry_at + carry_n) of d_inf[cur ^ 1]
    int bam_file = -1;       // the file whose pieces are coming in
    uint64_t file_recs = 0;  // records of that file before this piece
    uint64_t text_bytes = 0;

    Build(np2_ctx *c, np2_sam &s) : np2h::SamAccum(s, c->stream), cx(c) {
        d_text.cached = d_end.cached = d_kept.cached = d_ncig.cached = d_nseq.cached = d_koff.cached = d_coff.cached = true;
        d_soff.cached = d_lines.cached = d_ctr.cached = d_slot.cached = d_noff.cached = d_names.cached = true;
        d_nname.cached = d_nmoff.cached = d_nbad.cached = true;
        d_comp.cached = d_inf[0].cached = d_inf[1].cached = d_blk.cached = d_status.cached = d_starts.cached = d_info.cached = d_bctr.cached = true;
        d_tsize.cached = d_taux.cached = d_toff.cached = true;
        e_mid.make(), e_t0.make(), e_t1.make(), e_b0.make(), e_b1.make(), e_b2.make();
    }
    ~Build() { (void)hipStreamSynchronize(st); }

    void name_table(const np2sam::Refs &refs) {
        const np2sam::NameTabHost h(refs);
        d_slot.ensure(h.slot.size()), d_noff.ensure(h.off.size()), d_names.ensure(h.names.size());
        HIPCHK(hipMemcpyAsync(d_slot.p, h.slot.data(), h.slot.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_noff.p, h.off.data(), h.off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_names.p, h.names.data(), h.names.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // (pageable sources: `h` goes away)
        nt = np2sam::NameTab{d_slot.p, d_noff.p, d_names.p, h.mask};
        have_nt = true;
    }

    // one piece: `text` (pinned) holds n bytes of whole lines; `where` names the file, first_line its first line
    void piece(const uint8_t *text, size_t n, const std::string &where, uint64_t first_line, const std::function<void()> &text_copied) {
        if (n >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "a piece of SAM text of 2 GiB or more");
        d_text.ensure(n + np2::SAM_TEXT_PAD);
        d_end.ensure(n);
        d_ctr.ensure(1);
        np2::SamCtr *h = (np2::SamCtr *)pin.ensure(256); // the counters, the three totals, the offending line
        uint32_t *h_tot = (uint32_t *)(h + 1);
        h->n_lines = 0, h->first_err = 0xFFFFFFFFu, h->n_empty = 0, h->err = 0;
        HIPCHK(hipMemcpyAsync(d_ctr.p, h, sizeof *h, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_text.p + n, 0, np2::SAM_TEXT_PAD, st));
        Lookback lb = np2h::next_lookback(cx, np2::sam_line_blocks(n)); // (the first one of a context fills its status words on the stream)
        lb.err = &d_ctr.p->err;
        HIPCHK(hipEventRecord(e0.e, st));
        try {
            np2::launch_sam_lines(st, lb, d_text.p, (uint32_t)n, d_end.p, d_ctr.p);
            HIPCHK(hipGetLastError());
        } catch (...) { // (tickets were issued for a launch that may not have run: the next descriptor starts over)
            cx->lb_dirty = true;
            throw;
        }
        HIPCHK(hipEventRecord(e_mid.e, st));
        HIPCHK(hipMemcpyAsync(h, d_ctr.p, sizeof *h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const float ms_lines = elapsed(e0, e_mid);
        lines_ms += ms_lines, text_bytes += n;
        text_copied(); // the pinned buffer goes back to the reader
        if (h->err) throw Np2Error(NP2_E_DEVICE, "np2_sam: a look-back wait gave up");
        const uint32_t n_lines = h->n_lines;
        if (n_lines == 0 || n_lines > n) throw Np2Error(NP2_E_DEVICE, "np2_sam: line counter out of range");
        const size_t m = (size_t)n_lines + 1;
        d_lines.ensure(m), d_kept.ensure(m), d_ncig.ensure(m), d_nseq.ensure(m), d_koff.ensure(m), d_coff.ensure(m), d_soff.ensure(m);
        const size_t tmp_bytes = np2::prim_temp_bytes(m);
        d_tmp.ensure(tmp_bytes);
        HIPCHK(hipEventRecord(e0.e, st)); // (the stream was idle while the host read the line count)
        np2::launch_sam_fields(st, d_text.p, d_end.p, n_lines, nt, d_lines.p, d_kept.p, d_ncig.p, d_nseq.p, d_ctr.p);
        if (np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_kept.p, d_koff.p, m) ||
            np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_ncig.p, d_coff.p, m) ||
            np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_nseq.p, d_soff.p, m))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        HIPCHK(hipEventRecord(e1.e, st));
        HIPCHK(hipMemcpyAsync(h, d_ctr.p, sizeof *h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_tot + 0, d_koff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_tot + 1, d_coff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_tot + 2, d_soff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        sam.stats.parse_ms += ms_lines + elapsed(e0, e1);
        if (h->first_err != 0xFFFFFFFFu) { // the first offending line of the first offending piece
            if (h->first_err >= n_lines) throw Np2Error(NP2_E_DEVICE, "np2_sam: error line out of range");
            np2sam::Line *bad = (np2sam::Line *)(h_tot + 4);
            HIPCHK(hipMemcpyAsync(bad, d_lines.p + h->first_err, sizeof *bad, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            throw Np2Error(NP2_E_ARG, where + ": line " + std::to_string(first_line + h->first_err) + ": " + np2sam::err_text(bad->err));
        }
        const uint64_t kept = h_tot[0], n_cig = h_tot[1], n_seq = h_tot[2];
        if (h->n_empty > n_lines || kept > n_lines - h->n_empty) throw Np2Error(NP2_E_DEVICE, "np2_sam: record counters out of range");
        n_records += n_lines - h->n_empty;
        check_room(kept, n_cig);
        uint64_t n_name = 0, n_tail = 0;
        if (keep_names && kept) { // the names' lengths and where they go; a bad one speaks after every other error of the piece
            uint32_t *h_name = h_tot + 16; // [0]: the first bad line, [1]: the bytes of all names
            d_nname.ensure(m), d_nmoff.ensure(m), d_nbad.ensure(1);
            h_name[0] = 0xFFFFFFFFu;
            HIPCHK(hipMemcpyAsync(d_nbad.p, h_name, 4, hipMemcpyHostToDevice, st));
            np2::launch_sam_name_len(st, d_text.p, d_end.p, d_lines.p, n_lines, d_nname.p, d_nbad.p);
            if (np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_nname.p, d_nmoff.p, m)) throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
            if (keep_all) { // the tails' sizes; a bad field ranks with a bad name: the first such line of the piece speaks
                d_tsize.ensure(m), d_taux.ensure(m), d_toff.ensure(m);
                HIPCHK(hipEventRecord(e_t0.e, st));
                np2::launch_sam_tail_len(st, d_text.p, d_end.p, d_lines.p, n_lines, nt, d_tsize.p, d_taux.p, d_nbad.p);
                if (np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_tsize.p, d_toff.p, m)) throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
                HIPCHK(hipEventRecord(e_t1.e, st));
                HIPCHK(hipMemcpyAsync(h_name + 2, d_toff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipMemcpyAsync(h_name, d_nbad.p, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_name + 1, d_nmoff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            if (keep_all) sam.tail_len_ms += elapsed(e_t0, e_t1);
            if (h_name[0] != 0xFFFFFFFFu) {
                if (h_name[0] >= n_lines) throw Np2Error(NP2_E_DEVICE, "np2_sam: error line out of range");
                const std::string at = where + ": line " + std::to_string(first_line + h_name[0]) + ": ";
                if (keep_all) bad_tail(h_name[0], n, at); // (throws, unless the name is what is wrong)
                throw Np2Error(NP2_E_ARG, at + "QNAME is empty or longer than 254 bytes");
            }
            n_name = h_name[1];
            if (n_name > kept * 254u) throw Np2Error(NP2_E_DEVICE, "np2_sam: name bytes out of range");
            if (keep_all) {
                n_tail = h_name[2];
                if (n_tail % 4u || n_tail < kept * np2tail::HEAD_BYTES || n_tail > 4ull * n + kept * (np2tail::HEAD_BYTES + 4ull))
                    throw Np2Error(NP2_E_DEVICE, "np2_sam: tail bytes out of range");
            }
        }
        if (kept) {
            reserve(kept, n_cig, n_seq, n_name, n_tail);
            HIPCHK(hipEventRecord(e0.e, st));
            np2::launch_sam_pack(st, d_text.p, d_lines.p, n_lines, d_koff.p, d_coff.p, d_soff.p, n_recs, n_cigar, seq_bytes, tie, recs_in.p,
                                 tids_in.p, keys_in.p, cigar_in.p, sam.seq4.p);
            if (keep_names)
                np2::launch_sam_name_copy(st, d_text.p, d_end.p, d_lines.p, n_lines, d_koff.p, d_nmoff.p, n_recs, name_bytes, sam.names.p, nref_in.p);
            HIPCHK(hipEventRecord(e1.e, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            sam.stats.pack_ms += elapsed(e0, e1);
            if (keep_all) {
                HIPCHK(hipEventRecord(e_t0.e, st));
                np2::launch_sam_tail_emit(st, d_text.p, d_end.p, d_lines.p, n_lines, nt, d_koff.p, d_toff.p, d_taux.p, n_recs, tail_bytes, sam.tails.p,
                                          tref_in.p);
                HIPCHK(hipEventRecord(e_t1.e, st));
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipGetLastError());
                sam.tail_emit_ms += elapsed(e_t0, e_t1);
            }
        }
        advance(kept, n_cig, n_seq, n_name, n_tail);
    }

    // One piece of a BAM: `comp` (pinned) holds the file's bytes from p.file_off on, p.blks the blocks in them that hold bytes.
    void bam_piece(const uint8_t *comp, const Piece &p, const std::string &where, const std::function<void()> &comp_copied) {
        namespace bi = np2bamin;
        if (p.file != bam_file) bam_file = p.file, file_recs = 0, carry_n = 0;
        const size_t n_blk = p.blks.size();
        const uint64_t inflated = n_blk ? p.blks.back().out_off + p.blks.back().isize : 0, n = carry_n + inflated;
        if (n >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "a piece of BAM records of 2 GiB or more");
        const uint32_t n_ref = (uint32_t)sam.refs.names.size();
        const uint32_t flags = (keep_all ? bi::KEEP_ALL : 0u) | (keep_names ? bi::KEEP_NAMES : 0u);
        uint8_t *inf = d_inf[cur].ensure(n + np2::BAMIN_PAD);
        if (carry_n) HIPCHK(hipMemcpyAsync(inf, d_inf[cur ^ 1].p + carry_at, carry_n, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(inf + n, 0, np2::BAMIN_PAD, st));
        sam.bamin.blocks += p.n_blocks, sam.bamin.comp_bytes += p.n, sam.bamin.inflated_bytes += inflated;
        uint32_t *h_words = (uint32_t *)pin.ensure(256);
        bool copied = false;
        if (n_blk) {
            d_comp.ensure(p.n + 64), d_blk.ensure(n_blk + (n_blk * 4 + sizeof(np2::InfBlock) - 1) / sizeof(np2::InfBlock)), d_status.ensure(n_blk + 2);
            np2::InfBlock *h_tb = (np2::InfBlock *)pin_tab.ensure(n_blk * (sizeof(np2::InfBlock) + 4));
            uint32_t *h_crc = (uint32_t *)(h_tb + n_blk); // (the CRC32 words travel behind the table, in the same copy)
            for (size_t i = 0; i < n_blk; ++i) {
                const np2h::BgzfBlock &b = p.blks[i];
                h_tb[i] = np2::InfBlock{b.file_off - p.file_off + b.hdr_len, carry_n + b.out_off, b.clen, b.isize};
                h_crc[i] = b.crc;
            }
            HIPCHK(hipMemcpyAsync(d_comp.p, comp, p.n, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_blk.p, h_tb, n_blk * (sizeof(np2::InfBlock) + 4), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(d_status.p, 0, (n_blk + 2) * 4, st));
            HIPCHK(hipEventRecord(e_b0.e, st));
            np2::launch_bgzf_inflate(st, d_blk.p, (uint32_t)n_blk, d_comp.p, inf, d_status.p, d_status.p + n_blk);
            HIPCHK(hipEventRecord(e_b1.e, st));
            const bool crc = np2h::bgzf_crc_on();
            if (crc) np2::launch_bgzf_crc32(st, d_blk.p, (uint32_t)n_blk, (const uint32_t *)(d_blk.p + n_blk), inf, d_status.p, d_status.p + n_blk);
            HIPCHK(hipEventRecord(e_b2.e, st));
            HIPCHK(hipMemcpyAsync(h_words, d_status.p + n_blk, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            comp_copied(), copied = true; // the pinned buffer goes back to the reader
            sam.bamin.inflate_ms += elapsed(e_b0, e_b1);
            if (crc) sam.bamin.crc_ms += elapsed(e_b1, e_b2);
            if (h_words[0]) { // the first block that failed speaks
                std::vector<uint32_t> stv(n_blk);
                HIPCHK(hipMemcpy(stv.data(), d_status.p, n_blk * 4, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < n_blk; ++i)
                    if (stv[i] != np2inf::ST_OK)
                        throw Np2Error(NP2_E_ARG, where + ": " + (stv[i] == np2inf::ST_CRC_MISMATCH ? np2h::crc_msg(p.blks[i].file_off) :
                                                                  "BGZF inflate failed (block at file offset " + std::to_string(p.blks[i].file_off) + ")"));
                throw Np2Error(NP2_E_DEVICE, "np2_sam: the count of failed BGZF blocks has no block to it");
            }
        }
        if (!copied) comp_copied();
        // the walk
        d_starts.ensure(n / 36 + 2), d_bctr.ensure(1);
        np2::BaminCtr *h = (np2::BaminCtr *)h_words;
        uint32_t *h_tot = (uint32_t *)(h + 1);
        h->count = 0, h->flags = 0, h->first_err = 0xFFFFFFFFu, h->tail_at = 0;
        HIPCHK(hipMemcpyAsync(d_bctr.p, h, sizeof *h, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(e0.e, st));
        np2::launch_bamin_walk(st, inf, p.skip, (uint32_t)n, (uint32_t)std::min<size_t>(hooks.piece, 1u << 30), d_starts.p, d_bctr.p);
        HIPCHK(hipEventRecord(e1.e, st));
        HIPCHK(hipMemcpyAsync(h, d_bctr.p, sizeof *h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        sam.bamin.walk_ms += elapsed(e0, e1);
        const uint32_t count = h->count, walk_flags = h->flags, tail_at = h->tail_at;
        if (count > n / 36 + 1 || tail_at > n) throw Np2Error(NP2_E_DEVICE, "np2_sam: record walk out of range");
        uint64_t kept = 0, n_cig = 0, n_seq = 0, n_name = 0, n_tail = 0;
        if (count) {
            const size_t m = (size_t)count + 1;
            d_info.ensure(m), d_kept.ensure(m), d_ncig.ensure(m), d_nseq.ensure(m), d_koff.ensure(m), d_coff.ensure(m), d_soff.ensure(m);
            if (keep_names) d_nname.ensure(m), d_nmoff.ensure(m);
            if (keep_all) d_tsize.ensure(m), d_toff.ensure(m);
            const size_t tmp_bytes = np2::prim_temp_bytes(m);
            d_tmp.ensure(tmp_bytes);
            HIPCHK(hipEventRecord(e0.e, st));
            np2::launch_bamin_fields(st, inf, d_starts.p, count, walk_flags, n_ref, flags, d_info.p, d_kept.p, d_ncig.p, d_nseq.p, d_nname.p, d_tsize.p, d_bctr.p);
            if (np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_kept.p, d_koff.p, m) ||
                np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_ncig.p, d_coff.p, m) ||
                np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_nseq.p, d_soff.p, m) ||
                (keep_names && np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_nname.p, d_nmoff.p, m)) ||
                (keep_all && np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, d_tsize.p, d_toff.p, m)))
                throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
            HIPCHK(hipEventRecord(e1.e, st));
            h_tot[3] = h_tot[4] = 0;
            HIPCHK(hipMemcpyAsync(h, d_bctr.p, sizeof *h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_tot + 0, d_koff.p + count, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_tot + 1, d_coff.p + count, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_tot + 2, d_soff.p + count, 4, hipMemcpyDeviceToHost, st));
            if (keep_names) HIPCHK(hipMemcpyAsync(h_tot + 3, d_nmoff.p + count, 4, hipMemcpyDeviceToHost, st));
            if (keep_all) HIPCHK(hipMemcpyAsync(h_tot + 4, d_toff.p + count, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            sam.bamin.fields_ms += elapsed(e0, e1);
            if (h->first_err != 0xFFFFFFFFu) { // the first refused record of the first offending piece
                if (h->first_err >= count) throw Np2Error(NP2_E_DEVICE, "np2_sam: refused record out of range");
                HIPCHK(hipMemcpyAsync(h_tot + 8, d_info.p + h->first_err, 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                const uint32_t w = h_tot[8] & 255u;
                std::string msg = where + ": " + bi::record_message(file_recs + h->first_err, w);
                if (w == bi::W_PIECE) msg += " of " + std::to_string(hooks.piece) + " bytes";
                throw Np2Error(bi::where_status(w), msg);
            }
            kept = h_tot[0], n_cig = h_tot[1], n_seq = h_tot[2], n_name = h_tot[3], n_tail = h_tot[4];
            if (kept > count || n_cig > n / 4 || n_seq > n || n_name > kept * 254u || n_tail % 4u || n_tail > n + kept * (np2tail::HEAD_BYTES + 4ull))
                throw Np2Error(NP2_E_DEVICE, "np2_sam: record counters out of range");
            check_room(kept, n_cig);
        }
        if (kept) {
            reserve(kept, n_cig, n_seq, n_name, n_tail);
            const np2::BaminOut out{d_koff.p, d_coff.p, d_soff.p, d_nmoff.p, d_toff.p, n_recs, n_cigar, seq_bytes, name_bytes, tail_bytes, recs_in.p,
                                    tids_in.p, keys_in.p, cigar_in.p, sam.seq4.p, sam.names.p, nref_in.p, sam.tails.p, tref_in.p};
            HIPCHK(hipEventRecord(e0.e, st));
            np2::launch_bamin_pack(st, inf, d_starts.p, d_info.p, count, n_ref, flags, tie, out);
            HIPCHK(hipEventRecord(e1.e, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipGetLastError());
            sam.bamin.pack_ms += elapsed(e0, e1);
        }
        n_records += count, file_recs += count, sam.bamin.records += count;
        advance(kept, n_cig, n_seq, n_name, n_tail);
        carry_at = tail_at, carry_n = (uint32_t)n - tail_at, cur ^= 1;
        if (p.last && carry_n) {
            const uint32_t w = carry_n < 4u ? bi::W_GARBAGE : bi::W_TRUNC;
            carry_n = 0;
            throw Np2Error(NP2_E_ARG, where + ": " + bi::record_message(file_recs, w));
        }
    }

    // Line `r` of the piece (n bytes, still in d_text) has a bad name or a bad tail: the host reads the line and walks it with the
    // one-lane text of the rule to say which field.  Returns when the tail is good (the name is what is wrong).
    void bad_tail(uint32_t r, size_t n, const std::string &at) {
        uint32_t ends[2] = {0, 0};
        if (r) HIPCHK(hipMemcpyAsync(ends, d_end.p + r - 1, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ends + 1, d_end.p + r, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const uint32_t s = r ? ends[0] + 1u : 0u;
        if (s > ends[1] || ends[1] > n) throw Np2Error(NP2_E_DEVICE, "np2_sam: error line out of range");
        std::vector<uint8_t> line(ends[1] - s + 1u);
        if (ends[1] > s) HIPCHK(hipMemcpyAsync(line.data(), d_text.p + s, ends[1] - s, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        uint32_t e = ends[1] - s;
        if (e && line[e - 1] == '\r') --e;
        const np2sam::NameTabHost nth(sam.refs);
        np2h::throw_tail_error(line.data(), e, nth.view(), at);
    }

    void report() const {
        if (!hooks.profile) return;
        fprintf(stderr, "np2_sam: %llu bytes of alignment lines: k_sam_lines %.3f ms, k_sam_fields + scans %.3f ms, k_sam_pack %.3f ms, sort + k_sam_gather %.3f ms, waited for the reader %.3f ms\n",
                (unsigned long long)text_bytes, lines_ms, sam.stats.parse_ms - lines_ms, sam.stats.pack_ms, sam.stats.sort_ms, sam.stats.read_ms);
    }
};

// everything: `rd` has its source set and has not been started
void build(np2_ctx *cx, np2_sam &sam, Reader &rd, const np2_sam_opts_t *opts, size_t bytes_bound, uint32_t flags = 0) {
    HIPCHK(hipSetDevice(cx->device));
    sam.device = cx->device;
    Build b(cx, sam);
    b.tie = opts ? (opts->tie_by_strand ? 1u : 0u) : 1u;
    b.keep_all = (flags & NP2_SAM_KEEP_ALL) != 0;
    b.keep_names = b.keep_all || (flags & NP2_SAM_KEEP_NAMES) != 0;
    rd.start(bytes_bound);
    Piece p;
    for (;;) {
        const double t0 = np2h::now_ms();
        const bool got = rd.next(p);
        sam.stats.read_ms += (float)(np2h::now_ms() - t0);
        if (!got) break;
        if (!b.have_nt) {
            std::lock_guard<std::mutex> l(rd.mu);
            sam.refs = rd.refs;
        }
        if (!b.have_nt && !p.bam) b.name_table(sam.refs); // (a BAM's records carry numbers, not names)
        const std::string where = rd.paths.empty() ? "the text" : rd.paths[p.file] == "-" ? "standard input" : rd.paths[p.file];
        bool back = false;
        try {
            if (p.bam) b.bam_piece(rd.pin[p.buf], p, where, [&] { rd.release(p.buf), back = true; });
            else b.piece(rd.pin[p.buf] + p.off, p.n, where, p.first_line, [&] { rd.release(p.buf), back = true; });
        } catch (...) {
            if (!back) {
                (void)hipStreamSynchronize(cx->stream); // (the copy out of the pinned buffer may be in flight)
                rd.release(p.buf);
            }
            throw;
        }
    }
    {
        std::lock_guard<std::mutex> l(rd.mu);
        if (rd.err_code) throw Np2Error(rd.err_code, rd.err_msg);
        sam.refs = rd.refs;
        sam.stats.lines = rd.lines + sam.bamin.records;
        sam.bamin.files = rd.bam_files;
        if (b.keep_all)
            for (const std::string &l : rd.extra) sam.extra_header += l + "\n";
    }
    if (b.keep_all) sam.header_text = np2h::bam_header_text(sam.refs, sam.extra_header);
    b.finish();
    b.report();
}

// the resident arrays copied back into malloc'ed blocks (np2_free); an error returns none
void export_arrays(hipStream_t st, const np2_sam &sam, np2_bamrec_t **recs, int32_t **tids, uint32_t **cigar, uint8_t **seq4, uint64_t *n_recs) {
    void *h[4] = {nullptr, nullptr, nullptr, nullptr};
    const void *d[4] = {sam.recs.p, sam.tids.p, sam.cigar.p, sam.seq4.p};
    const size_t bytes[4] = {(size_t)sam.n_recs * sizeof(np2_bamrec_t), (size_t)sam.n_recs * 4, (size_t)sam.n_cigar * 4, (size_t)sam.seq_bytes};
    try {
        for (int i = 0; i < 4; ++i) {
            if (!bytes[i]) continue;
            h[i] = malloc(bytes[i]);
            if (!h[i]) throw Np2Error(NP2_E_NOMEM, "out of memory for the parsed records");
            HIPCHK(hipMemcpyAsync(h[i], d[i], bytes[i], hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
    } catch (...) {
        (void)hipStreamSynchronize(st);
        for (void *p : h) free(p);
        throw;
    }
    *recs = (np2_bamrec_t *)h[0], *tids = (int32_t *)h[1], *cigar = (uint32_t *)h[2], *seq4 = (uint8_t *)h[3];
    *n_recs = sam.n_recs;
}

int ref_tid(const np2_sam *s, const char *name) {
    for (size_t i = 0; i < s->refs.names.size(); ++i)
        if (s->refs.names[i] == name) return (int)i;
    return -1;
}

} // namespace

extern "C" {

int np2_sam_open(np2_ctx_t *cx, const char *const *paths, int n_paths, const np2_sam_opts_t *opts, np2_sam_t **out) {
    return np2_sam_open_ex(cx, paths, n_paths, opts, 0u, out);
}

int np2_sam_open_ex(np2_ctx_t *cx, const char *const *paths, int n_paths, const np2_sam_opts_t *opts, uint32_t flags, np2_sam_t **out) {
    if (out) *out = nullptr;
    bool touched = false;
    return np2h::abi_guard([&] {
        // the arguments and the files, before the first device call
        if (!cx || !out || !paths || n_paths < 1) throw Np2Error(NP2_E_ARG, "np2_sam_open: NULL argument or no path");
        if (flags & ~(uint32_t)(NP2_SAM_KEEP_NAMES | NP2_SAM_KEEP_ALL)) throw Np2Error(NP2_E_ARG, "np2_sam_open_ex: unknown flag bits");
        Hooks hooks;
        Reader rd(hooks);
        int n_stdin = 0;
        for (int i = 0; i < n_paths; ++i) {
            if (!paths[i]) throw Np2Error(NP2_E_ARG, "np2_sam_open: a path is NULL");
            rd.paths.push_back(paths[i]);
            rd.is_bam.push_back(0);
            if (rd.paths.back() == "-") {
                if (++n_stdin > 1) throw Np2Error(NP2_E_ARG, "np2_sam_open: standard input is given twice");
                continue;
            }
            FILE *f = fopen(paths[i], "rb");
            if (!f) throw Np2Error(NP2_E_ARG, std::string("cannot open ") + paths[i] + (flags & NP2_SAM_KEEP_ALL ? " (np2_sam_open_ex, flag NP2_SAM_KEEP_ALL)" : ""));
            fclose(f);
            rd.is_bam.back() = np2h::is_bam_file(paths[i]) ? 1 : 0;
        }
        touched = true;
        std::unique_ptr<np2_sam> sam(new np2_sam());
        build(cx, *sam, rd, opts, 0, flags);
        *out = sam.release();
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            cx->err = msg;
        }
        np2h::io_set_error(code, msg);
    });
}

void np2_sam_close(np2_sam_t *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}
int np2_sam_n_refs(np2_sam_t *s) { return s ? (int)s->refs.names.size() : 0; }
const char *np2_sam_ref_name(np2_sam_t *s, int tid, uint32_t *len) {
    if (!s || tid < 0 || (size_t)tid >= s->refs.names.size()) return nullptr;
    if (len) *len = s->refs.lens[tid];
    return s->refs.names[tid].c_str();
}
int np2_sam_stats(np2_sam_t *s, np2_sam_stats_t *stats) {
    if (!s || !stats) return NP2_E_ARG;
    *stats = s->stats;
    return NP2_OK;
}

int np2_contig_from_sam(np2_ctx_t *cx, np2_sam_t *sam, const char *name, const uint8_t *ref, uint32_t L, const np2_front_opts_t *opts,
                        np2_contig_t **out) {
    if (out) *out = nullptr;
    bool touched = false;
    return np2h::abi_guard([&] {
        // checked before anything of the context or the handle is looked at
        if (!cx || !sam || !name || !ref || !opts || !out) throw Np2Error(NP2_E_ARG, "np2_contig_from_sam: NULL argument");
        if (opts->use_secondary)
            throw Np2Error(NP2_E_UNSUPPORTED, "np2_contig_from_sam: a secondary record takes the SEQ of its read's primary record, which is "
                                              "found by name: use a BAM for -S");
        const int tid = ref_tid(sam, name);
        if (tid < 0) throw Np2Error(NP2_E_ARG, std::string("the SAM header has no @SQ line for ") + name);
        if (cx->device != sam->device) throw Np2Error(NP2_E_ARG, "np2_contig_from_sam: the context is on another device than the SAM");
        touched = true;
        HIPCHK(hipSetDevice(cx->device));
        const uint64_t lo = (uint64_t)tid << 33, hi = (uint64_t)(tid + 1) << 33;
        const size_t a = std::lower_bound(sam->keys.begin(), sam->keys.end(), lo) - sam->keys.begin();
        const size_t b = std::lower_bound(sam->keys.begin(), sam->keys.end(), hi) - sam->keys.begin();
        std::vector<np2_bamrec_t> recs(b - a);
        std::vector<uint32_t> cigar;
        if (b > a) {
            const std::vector<uint32_t> words = np2h::d2h(cx, sam->recs.p + a * np2::SAM_REC_WORDS, (b - a) * np2::SAM_REC_WORDS);
            memcpy((void *)recs.data(), words.data(), words.size() * 4);
            const uint64_t c0 = recs.front().cigar_off, c1 = recs.back().cigar_off + recs.back().n_cigar;
            if (c1 < c0 || c1 > sam->n_cigar) throw Np2Error(NP2_E_DEVICE, "np2_sam: CIGAR offsets out of range");
            cigar = np2h::d2h(cx, sam->cigar.p + c0, c1 - c0);
            for (np2_bamrec_t &r : recs) r.cigar_off -= c0;
        }
        cigar.push_back(0); // (never a NULL array)
        np2h::contig_from_device_seq(cx, ref, L, recs.data(), (uint32_t)recs.size(), cigar.data(), sam->seq4.p, sam->seq_bytes, opts, out);
        np2h::flush_timings(cx);
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            np2h::flush_timings(cx);
            cx->err = msg;
        }
        np2h::io_set_error(code, msg);
    });
}

int np2_sam_parse_bytes(int device, const uint8_t *text, uint64_t n, const np2_sam_opts_t *opts, np2_bamrec_t **recs, int32_t **tids,
                        uint32_t **cigar, uint8_t **seq4, uint64_t *n_recs, np2_sam_stats_t *stats) {
    np2_ctx_t *cx = nullptr;
    const int rc = np2h::abi_guard([&] {
        if (!recs || !tids || !cigar || !seq4 || !n_recs || (n && !text)) throw Np2Error(NP2_E_ARG, "np2_sam_parse_bytes: NULL argument");
        *recs = nullptr, *tids = nullptr, *cigar = nullptr, *seq4 = nullptr, *n_recs = 0;
        if (np2_ctx_create(&cx, device, nullptr, 0) != NP2_OK) throw Np2Error(NP2_E_DEVICE, "np2_sam_parse_bytes: no context on that device");
        Hooks hooks;
        Reader rd(hooks);
        rd.mem = text, rd.mem_n = n;
        np2_sam sam;
        build(cx, sam, rd, opts, n);
        export_arrays(cx->stream, sam, recs, tids, cigar, seq4, n_recs);
        if (stats) *stats = sam.stats;
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (cx) (void)hipStreamSynchronize(cx->stream);
        np2h::io_set_error(code, msg);
    });
    if (cx) np2_ctx_destroy(cx);
    return rc;
}

int np2_sam_export(np2_ctx_t *cx, np2_sam_t *sam, np2_bamrec_t **recs, int32_t **tids, uint32_t **cigar, uint8_t **seq4, uint64_t *n_recs) {
    bool touched = false;
    return np2h::abi_guard([&] {
        if (!cx || !sam || !recs || !tids || !cigar || !seq4 || !n_recs) throw Np2Error(NP2_E_ARG, "np2_sam_export: NULL argument");
        *recs = nullptr, *tids = nullptr, *cigar = nullptr, *seq4 = nullptr, *n_recs = 0;
        if (cx->device != sam->device) throw Np2Error(NP2_E_ARG, "np2_sam_export: the context is on another device than the SAM");
        touched = true;
        HIPCHK(hipSetDevice(cx->device));
        export_arrays(cx->stream, *sam, recs, tids, cigar, seq4, n_recs);
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) cx->err = msg;
        np2h::io_set_error(code, msg);
    });
}

} // extern "C"
