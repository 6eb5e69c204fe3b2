// Host side of NP2_SAM_KEEP_ALL (include/np2_io.h): what a bad tail's message says, the host-only door np2_sam_tails_host, which
// runs the one-lane text of the rule (np2_samtail_core.hpp: tail_line) over SAM text in memory, and the small exports of a
// resident handle (np2_sam_export_tails, np2_sam_header_text, np2_sam_tail_stats).  The kernels are in np2_sam.hip.
#include "../../include/np2_io.h"
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_sam_handle.hpp"

#include <algorithm>

namespace {
using np2h::Np2Error;
namespace tl = np2tail;

// the QNAME of a line the lean parse took: the bytes before its first tab
bool name_ok(const uint8_t *t, uint32_t e) {
    uint32_t i = 0;
    while (i < e && t[i] != '\t') ++i;
    return i >= 1 && i <= 254;
}

// what error word `w` of line text[0, e) says, with the field's name or TAG
std::string tail_message(const uint8_t *t, uint32_t e, const np2sam::Line &ln, uint32_t w) {
    const uint32_t f = tl::word_field(w), k = tl::word_kind(w);
    static const char *fixed[4] = {"RNEXT", "PNEXT", "TLEN", "QUAL"};
    if (f < tl::F_OPT) return std::string(fixed[f]) + ": " + tl::kind_text(k);
    tl::Spots sp;
    std::string tag;
    if (tl::find_spots(t, e, ln, &sp)) {
        uint32_t a = sp.qual_b;
        for (uint32_t j = 0; j < f - tl::F_OPT && a < e; ++j)
            for (++a; a < e && t[a] != '\t';) ++a;
        if (a + 2 < e && k != tl::T_SHORT && k != tl::T_TAG) tag = std::string(" (") + (char)t[a + 1] + (char)t[a + 2] + ")";
    }
    return "optional field " + std::to_string(f - tl::F_OPT + 1) + tag + ": " + tl::kind_text(k);
}
int word_status(uint32_t w) { return tl::word_kind(w) == tl::T_WINDOW ? NP2_E_UNSUPPORTED : NP2_E_ARG; }

struct FreeList { // malloc'ed blocks that go back on an error
    std::vector<void *> p;
    ~FreeList() {
        for (void *x : p) free(x);
    }
    void *take(size_t bytes) {
        void *x = malloc(bytes ? bytes : 1);
        if (!x) throw Np2Error(NP2_E_NOMEM, "np2_sam_tails_host: out of memory");
        p.push_back(x);
        return x;
    }
};

} // namespace

namespace np2h {
void throw_tail_error(const uint8_t *line, uint32_t e, const np2sam::NameTab &nt, const std::string &at) {
    const np2sam::Line ln = np2sam::parse_line(line, 0, e, nt);
    if (ln.err != np2sam::OK || !np2sam::line_kept(ln) || !name_ok(line, e)) return;
    uint32_t size = 0, aux = 0;
    bool hq = false;
    const uint32_t w = tl::tail_line(line, e, ln, nt, &size, &aux, &hq, nullptr);
    if (w) throw Np2Error(word_status(w), at + tail_message(line, e, ln, w));
}
} // namespace np2h

extern "C" {

int np2_sam_tails_host(const uint8_t *text, uint64_t n, uint8_t **tails, uint64_t *tail_bytes, uint64_t **tail_ref, int32_t **status,
                       uint32_t **where, uint64_t *n_lines, char **header_text, uint64_t *header_bytes) {
    return np2h::abi_guard([&] {
        if (!tails || !tail_bytes || !tail_ref || !status || !where || !n_lines || (n && !text) || (header_text && !header_bytes))
            throw Np2Error(NP2_E_ARG, "np2_sam_tails_host: NULL argument");
        *tails = nullptr, *tail_ref = nullptr, *status = nullptr, *where = nullptr, *tail_bytes = 0, *n_lines = 0;
        if (header_text) *header_text = nullptr, *header_bytes = 0;
        if (n >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "np2_sam_tails_host: 2 GiB of text or more");
        // the header
        np2sam::Refs refs;
        std::vector<std::string> extra;
        struct Span { uint32_t a, e; uint64_t no; };
        std::vector<Span> lines; // the alignment lines that are not empty
        bool in_header = true;
        uint64_t no = 0;
        for (uint64_t at = 0; at < n;) {
            const uint8_t *nl = (const uint8_t *)memchr(text + at, '\n', n - at);
            const uint64_t end = nl ? (uint64_t)(nl - text) : n, e = end > at && text[end - 1] == '\r' ? end - 1 : end;
            ++no;
            if (e > at) {
                if (in_header && text[at] == '@') {
                    const std::string bad = np2sam::header_line(text, at, e, refs);
                    if (!bad.empty()) throw Np2Error(NP2_E_ARG, "the text: line " + std::to_string(no) + ": " + bad);
                    if (np2sam::header_line_is_carried(text, at, e)) {
                        std::string l((const char *)text + at, e - at);
                        if (std::find(extra.begin(), extra.end(), l) == extra.end()) extra.push_back(std::move(l));
                    }
                } else {
                    in_header = false;
                    lines.push_back(Span{(uint32_t)at, (uint32_t)e, no});
                }
            }
            at = end + 1;
        }
        const np2sam::NameTabHost nth(refs);
        const np2sam::NameTab nt = nth.view();
        const size_t m = lines.size();
        FreeList mem;
        uint64_t *ref = (uint64_t *)mem.take(m * 8);
        int32_t *st = (int32_t *)mem.take(m * 4);
        uint32_t *wh = (uint32_t *)mem.take(m * 4);
        std::vector<np2sam::Line> parsed(m);
        uint64_t total = 0;
        size_t first_lean = m, first_tail = m;
        for (size_t i = 0; i < m; ++i) { // sizes and errors
            const uint8_t *t = text + lines[i].a;
            const uint32_t e = lines[i].e - lines[i].a;
            np2sam::Line &ln = parsed[i] = np2sam::parse_line(t, 0, e, nt);
            ref[i] = ~0ull, st[i] = 0, wh[i] = 0;
            if (ln.err != np2sam::OK) {
                st[i] = NP2_E_ARG;
                first_lean = std::min(first_lean, i);
            } else if (!np2sam::line_kept(ln)) {
                st[i] = 1;
            } else if (!name_ok(t, e)) {
                st[i] = NP2_E_ARG, wh[i] = tl::T_QNAME;
                first_tail = std::min(first_tail, i);
            } else {
                uint32_t size = 0, aux = 0;
                bool hq = false;
                wh[i] = tl::tail_line(t, e, ln, nt, &size, &aux, &hq, nullptr);
                if (wh[i]) {
                    st[i] = word_status(wh[i]);
                    first_tail = std::min(first_tail, i);
                } else {
                    ref[i] = tl::tail_ref(total, hq);
                    total += tl::pad4(size);
                }
            }
        }
        uint8_t *out = (uint8_t *)mem.take(total);
        for (size_t i = 0; i < m; ++i) {
            if (st[i] != 0) continue;
            uint32_t size = 0, aux = 0;
            bool hq = false;
            (void)tl::tail_line(text + lines[i].a, lines[i].e - lines[i].a, parsed[i], nt, &size, &aux, &hq, out + tl::tail_off(ref[i]));
        }
        if (header_text) {
            std::string ex;
            for (const std::string &l : extra) ex += l + "\n";
            const std::string h = np2h::bam_header_text(refs, ex);
            char *c = (char *)mem.take(h.size() + 1);
            memcpy(c, h.c_str(), h.size() + 1);
            *header_text = c, *header_bytes = h.size();
        }
        *tails = out, *tail_bytes = total, *tail_ref = ref, *status = st, *where = wh, *n_lines = m;
        mem.p.clear();
        // the line that speaks: the first one the lean parse refuses, else the first with a bad name or tail
        const size_t bad = first_lean < m ? first_lean : first_tail;
        if (bad < m) {
            const uint8_t *t = text + lines[bad].a;
            const uint32_t e = lines[bad].e - lines[bad].a;
            const std::string at = "the text: line " + std::to_string(lines[bad].no) + ": ";
            np2h::io_set_error(st[bad], at + (first_lean < m ? std::string(np2sam::err_text(parsed[bad].err)) :
                                                  wh[bad] == tl::T_QNAME ? std::string("QNAME is empty or longer than 254 bytes") :
                                                                          tail_message(t, e, parsed[bad], wh[bad])));
            return st[bad];
        }
        return (int)NP2_OK;
    }, np2h::io_set_error);
}

int np2_sam_export_tails(np2_ctx_t *cx, np2_sam_t *sam, uint8_t **tails, uint64_t *tail_bytes, uint64_t **tail_ref, uint64_t *n_recs) {
    bool touched = false;
    return np2h::abi_guard([&] {
        if (!cx || !sam || !tails || !tail_bytes || !tail_ref || !n_recs) throw Np2Error(NP2_E_ARG, "np2_sam_export_tails: NULL argument");
        *tails = nullptr, *tail_ref = nullptr, *tail_bytes = 0, *n_recs = 0;
        if (!sam->has_tails) throw Np2Error(NP2_E_ARG, "np2_sam_export_tails: the SAM was opened without its tails (np2_sam_open_ex with NP2_SAM_KEEP_ALL)");
        if (cx->device != sam->device) throw Np2Error(NP2_E_ARG, "np2_sam_export_tails: the context is on another device than the SAM");
        touched = true;
        HIPCHK(hipSetDevice(cx->device));
        std::unique_ptr<uint8_t, void (*)(void *)> a((uint8_t *)malloc(sam->tail_bytes + 1), free);
        std::unique_ptr<uint64_t, void (*)(void *)> b((uint64_t *)malloc((sam->n_recs + 1) * 8), free);
        if (!a || !b) throw Np2Error(NP2_E_NOMEM, "out of memory for the tails");
        if (sam->tail_bytes) HIPCHK(hipMemcpyAsync(a.get(), sam->tails.p, sam->tail_bytes, hipMemcpyDeviceToHost, cx->stream));
        if (sam->n_recs) HIPCHK(hipMemcpyAsync(b.get(), sam->tail_ref.p, sam->n_recs * 8, hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        *tail_bytes = sam->tail_bytes, *n_recs = sam->n_recs;
        *tails = a.release(), *tail_ref = b.release();
        return NP2_OK;
    }, [&](int code, const std::string &msg) {
        if (touched) {
            (void)hipStreamSynchronize(cx->stream);
            cx->err = msg;
        }
        np2h::io_set_error(code, msg);
    });
}

int np2_sam_header_text(np2_sam_t *sam, const char **text, uint64_t *n) {
    return np2h::abi_guard([&] {
        if (!sam || !text || !n) throw Np2Error(NP2_E_ARG, "np2_sam_header_text: NULL argument");
        *text = nullptr, *n = 0;
        if (!sam->has_tails) throw Np2Error(NP2_E_ARG, "np2_sam_header_text: the SAM was opened without its header lines (np2_sam_open_ex with NP2_SAM_KEEP_ALL)");
        *text = sam->header_text.c_str(), *n = sam->header_text.size();
        return NP2_OK;
    }, np2h::io_set_error);
}

int np2_sam_tail_stats(np2_sam_t *sam, float *len_ms, float *emit_ms, uint64_t *tail_bytes) {
    if (!sam) return NP2_E_ARG;
    if (len_ms) *len_ms = sam->tail_len_ms;
    if (emit_ms) *emit_ms = sam->tail_emit_ms;
    if (tail_bytes) *tail_bytes = sam->tail_bytes;
    return NP2_OK;
}

} // extern "C"
