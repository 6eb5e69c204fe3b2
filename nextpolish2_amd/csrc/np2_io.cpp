// Input side of the hot path (include/np2_io.h): the entry points' error slot, FASTA[.gz], yak v2 dumps and the context made
// straight from dump files.  The indexed BAM is np2_bamfile.cpp (handle, host reader), np2_fetch_gpu.cpp (device reader),
// np2_frontend.cpp (records -> pileup) and np2_bamread.cpp (the entry points over them).
#include "np2_bamfile.hpp"
#include "np2_kcount.hpp"

#include <zlib.h>
#include <execinfo.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

thread_local std::string g_io_err;
int io_fail(int code, const std::string &m) {
    g_io_err = m;
    return code;
}

// ---------------------------------------------------------------------------------------------
// FASTA[.gz] (kseq semantics: name = header up to the first whitespace, sequence lines concatenated)
// ---------------------------------------------------------------------------------------------
struct Fasta {
    gzFile f = nullptr;
    std::string name, seq, pending; // pending = next header line
    std::vector<char> buf;
    ~Fasta() {
        if (f) gzclose(f);
    }
    bool getline(std::string &out) {
        out.clear();
        for (;;) {
            if (!gzgets(f, buf.data(), (int)buf.size())) return !out.empty();
            size_t n = strlen(buf.data());
            out.append(buf.data(), n);
            if (n && buf[n - 1] == '\n') break;
        }
        while (!out.empty() && (out.back() == '\n' || out.back() == '\r')) out.pop_back();
        return true;
    }
};

// NP2_SEGV_TRACE=1: print the native stack of a crashing thread (field debugging; off by default)
void np2_segv_handler(int sig) {
    void *frames[64];
    const int n = backtrace(frames, 64);
    const char msg[] = "np2: fatal signal, native stack:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
struct SegvTraceInit {
    SegvTraceInit() {
        if (getenv("NP2_SEGV_TRACE"))
            for (int sig : {SIGSEGV, SIGBUS, SIGABRT}) signal(sig, np2_segv_handler);
    }
} g_segv_trace_init;

// The dumps straight into HBM tables (what np2_yak_load + np2_ctx_create do through host arrays): each file is read
// once, in 8 MiB pieces, into pinned staging and copied to the device while the next piece is being read; the insert
// kernel then builds the table from the file image itself (bucket headers skipped by offset).  One host thread, one
// stream per dump.  A 12 Mb genome's two dumps (2 x 104 MB) are tables 0.1 s sooner than through pageable host
// arrays; a human-scale dump (tens of GB) never needs its host copy at all.
struct YakFile {
    std::string path;
    int fd = -1;
    uint32_t k = 0, pre = 0;
    size_t size = 0;
    np2h::YakTable table;
    int code = NP2_OK;
    std::string msg;
    ~YakFile() {
        if (fd >= 0) close(fd);
    }
};
void yak_file_to_table(YakFile &yf, int device, hipStream_t given) {
    hipStream_t st = given; // (one of the new context's idle streams, or our own)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void *pin[2] = {nullptr, nullptr};
    auto fail = [&](int code, const std::string &m) { yf.code = code, yf.msg = m; };
    const bool prof = getenv("NP2_IO_PROFILE") != nullptr;
    auto body = [&]() {
        const double t0 = np2h::now_ms();
        HIPCHK(hipSetDevice(device));
        const size_t nb = (size_t)1 << yf.pre;
        // bucket headers: 1024 small reads at positions that depend on one another (page cache)
        std::vector<uint64_t> off(nb + 1);
        uint64_t mx = 0;
        size_t at = 16; // file offset of the next bucket header
        const size_t body_words = (yf.size - 16) / 8; // the device image: the file from byte 16 on, whole words
        for (size_t b = 0; b < nb; ++b) {
            uint8_t h8[8];
            if (at + 8 > yf.size || pread(yf.fd, h8, 8, (off_t)at) != 8) return fail(NP2_E_ARG, "Failed to parse the dump file");
            const uint64_t n = le32(h8 + 4); // (first u32, the capacity bits, is ignored like the reference, kmer.rs:143-147)
            const uint64_t take = std::min<uint64_t>(n, (yf.size - at - 8) / 8); // UnexpectedEof ends the bucket (kmer.rs:151-155)
            off[b] = (at - 16) / 8 + 1;
            mx = std::max(mx, take);
            at += 8 + take * 8;
            if (b + 1 == nb) off[nb] = off[b] + take + 1;
        }
        uint32_t cl = 4;
        while ((1ull << cl) < mx * 2 + 2) ++cl;
        const size_t slots = nb << cl;
        const double t1 = np2h::now_ms();
        double ta[6] = {t1, t1, t1, t1, t1, t1};
        if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        ta[0] = np2h::now_ms();
        yf.table.k = yf.k;
        yf.table.cap_log2 = cl;
        yf.table.table = std::make_shared<np2h::DevBuf<uint64_t>>();
        yf.table.table->ensure(slots);
        ta[1] = np2h::now_ms();
        HIPCHK(hipMemsetAsync(yf.table.table->p, 0xFF, slots * 8, st));
        ta[2] = np2h::now_ms();
        np2h::DevBuf<uint64_t> d_raw, d_off;
        np2h::DevBuf<uint32_t> d_dup;
        d_raw.ensure(body_words + 1);
        ta[3] = np2h::now_ms();
        d_off.ensure(nb + 1);
        d_dup.ensure(1);
        HIPCHK(hipMemsetAsync(d_dup.p, 0, 4, st));
        ta[4] = np2h::now_ms();
        const size_t PIECE = (size_t)8 << 20;
        for (int i = 0; i < 2; ++i) {
            pin[i] = np2h::pinned_pool().get(PIECE);
            if (!pin[i]) throw np2h::Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
            HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        const double t2 = np2h::now_ms();
        if (prof)
            fprintf(stderr, "  yak k=%u allocations: stream %.1f ms, table (%.1f GB) %.1f ms, memset call %.1f ms, file image (%.1f GB) %.1f ms, "
                            "small buffers %.1f ms, pinned pieces + events %.1f ms\n", yf.k, ta[0] - t1, slots * 8 / 1e9, ta[1] - ta[0],
                    ta[2] - ta[1], body_words * 8 / 1e9, ta[3] - ta[2], ta[4] - ta[3], t2 - ta[4]);
        if (!staged_upload(pin, ev, PIECE, 8, body_words * 8, (uint8_t *)d_raw.p, st, [&](uint8_t *stage, size_t o, size_t n) { return pread_full(yf.fd, stage, n, 16 + o); }, no_look))
            return fail(NP2_E_ARG, "Failed to parse the dump file");
        const double t3 = np2h::now_ms();
        // (the offsets are tiny: through the first staging piece once its last copy has drained)
        HIPCHK(hipStreamSynchronize(st));
        memcpy(pin[0], off.data(), (nb + 1) * 8);
        HIPCHK(hipMemcpyAsync(d_off.p, pin[0], (nb + 1) * 8, hipMemcpyHostToDevice, st));
        np2::launch_yak_insert(st, d_raw.p, d_off.p, (uint32_t)nb, mx, yf.table.table->p, cl, d_dup.p, 1);
        uint32_t *dup = (uint32_t *)pin[1];
        HIPCHK(hipMemcpyAsync(dup, d_dup.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (*dup) { // a repeated key (yak writes none): a slot per word, the winner chosen at lookup (kmer.rs:148-167)
            yf.table.ord = std::make_shared<np2h::DevBuf<uint32_t>>();
            yf.table.ord->ensure(slots);
            HIPCHK(hipMemsetAsync(yf.table.table->p, 0xFF, slots * 8, st));
            np2::launch_yak_insert_dup(st, d_raw.p, d_off.p, (uint32_t)nb, mx, yf.table.table->p, cl, yf.table.ord->p, 1);
            HIPCHK(hipStreamSynchronize(st));
        }
        if (prof)
            fprintf(stderr, "yak dump -> table (k=%u, %.0f MB): bucket headers %.2f ms, device + staging allocations %.2f ms, read + copy %.2f ms, "
                            "insert %.2f ms\n", yf.k, yf.size / 1e6, t1 - t0, t2 - t1, t3 - t2, np2h::now_ms() - t3);
    };
    try {
        body();
    } catch (const np2h::Np2Error &e) {
        fail(e.code, e.what());
    } catch (const std::exception &e) {
        fail(NP2_E_NOMEM, e.what());
    }
    if (st) (void)hipStreamSynchronize(st);
    for (int i = 0; i < 2; ++i) {
        if (pin[i]) np2h::pinned_pool().put(pin[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    if (st && st != given) (void)hipStreamDestroy(st);
}

} // namespace
// (the message slot for the entry points of other translation units: np2_bamfile.cpp, np2_kcount_host.cpp, ...)
int np2h::io_set_error(int code, const std::string &m) { return io_fail(code, m); }

struct np2_fasta {
    Fasta f;
};

extern "C" {

const char *np2_io_last_error(void) { return g_io_err.c_str(); }

// ---- FASTA ---------------------------------------------------------------------------------------
int np2_fasta_open(const char *path, np2_fasta_t **out) {
    return np2h::abi_guard([&] {
        std::unique_ptr<np2_fasta> h(new np2_fasta());
        h->f.f = gzopen(path, "rb");
        if (!h->f.f) return io_fail(NP2_E_ARG, std::string("cannot open ") + path);
        gzbuffer(h->f.f, 1 << 20);
        h->f.buf.resize(1 << 16);
        std::string line;
        while (h->f.getline(line)) // skip to the first header
            if (!line.empty() && line[0] == '>') {
                h->f.pending = line;
                break;
            }
        *out = h.release();
        return NP2_OK;
    }, io_fail);
}
int np2_fasta_next(np2_fasta_t *h, const char **name, const uint8_t **seq, uint64_t *len) {
    return np2h::abi_guard([&] {
        Fasta &f = h->f;
        if (f.pending.empty()) return 0;
        size_t e = 1;
        while (e < f.pending.size() && !isspace((unsigned char)f.pending[e])) ++e;
        f.name = f.pending.substr(1, e - 1);
        f.pending.clear();
        f.seq.clear();
        std::string line;
        while (f.getline(line)) {
            if (!line.empty() && line[0] == '>') {
                f.pending = line;
                break;
            }
            f.seq += line;
        }
        *name = f.name.c_str();
        *seq = (const uint8_t *)f.seq.data();
        *len = f.seq.size();
        return 1;
    }, io_fail);
}
void np2_fasta_close(np2_fasta_t *h) { delete h; }

// ---- yak v2 (kmer.rs:72-170) -----------------------------------------------------------------------
int np2_yak_load(const char *path, np2_yak_t *out) {
    return np2h::abi_guard([&] {
        std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(path, "rb"), fclose);
        if (!f) return io_fail(NP2_E_ARG, std::string("cannot open ") + path);
        uint8_t hd[16];
        if (fread(hd, 1, 16, f.get()) != 16 || memcmp(hd, "YAK\2", 4) != 0)
            return io_fail(NP2_E_ARG, "The input binary k-mer dump file is incompatible.");
        const uint32_t k = le32(hd + 4), pre = le32(hd + 8), cbits = le32(hd + 12);
        if (cbits != 10) return io_fail(NP2_E_ARG, "different YAK_COUNTER_BITS");
        if (pre > 20) return io_fail(NP2_E_UNSUPPORTED, "yak prefix bits too large");
        const size_t nb = (size_t)1 << pre;
        // every word of the file is read ONCE, straight into the array that is handed out (the file's size bounds it): a
        // human-scale dump is tens of GB, and the command line loads its dumps while the first contigs are being read
        struct stat st;
        if (fstat(fileno(f.get()), &st) != 0) return io_fail(NP2_E_ARG, std::string("cannot stat ") + path);
        const size_t max_words = (size_t)st.st_size / 8 + 1;
        std::unique_ptr<uint64_t, void (*)(void *)> w((uint64_t *)malloc(max_words * 8), free), off((uint64_t *)malloc((nb + 1) * 8), free);
        if (!w || !off) return io_fail(NP2_E_NOMEM, "out of memory loading the k-mer dump");
        off.get()[0] = 0;
        size_t have = 0;
        for (size_t b = 0; b < nb; ++b) {
            uint8_t h8[8];
            if (fread(h8, 1, 8, f.get()) != 8) return io_fail(NP2_E_ARG, "Failed to parse the dump file");
            const uint32_t n = le32(h8 + 4); // first u32 (capacity bits) is ignored like the reference (kmer.rs:143-147)
            const size_t want = std::min<size_t>(n, max_words - have);
            const size_t got = fread(w.get() + have, 8, want, f.get());
            have += got; // UnexpectedEof ends the bucket (kmer.rs:151-155)
            off.get()[b + 1] = have;
        }
        out->k = k;
        out->pre = pre;
        out->n_words = have;
        out->words = w.release();
        out->bucket_off = off.release();
        return NP2_OK;
    }, io_fail);
}
void np2_yak_free(np2_yak_t *y) {
    if (!y) return;
    free((void *)y->words);
    free((void *)y->bucket_off);
    y->words = nullptr;
    y->bucket_off = nullptr;
}

int np2_ctx_create_from_files(np2_ctx_t **out, int device, const char *const *paths, int n_paths) {
    if (!out) return NP2_E_ARG;
    *out = nullptr;
    return np2h::abi_guard([&] {
        if (n_paths < 0 || n_paths > NP2_MAX_YAK || (n_paths && !paths)) return io_fail(NP2_E_ARG, "n_yak must be in [0, 15]");
        std::unique_ptr<np2_ctx, void (*)(np2_ctx_t *)> cx(nullptr, np2_ctx_destroy);
        std::vector<std::unique_ptr<YakFile>> files; // (after the context: its tables are released before its device state goes)
        for (int i = 0; i < n_paths; ++i) {
            std::unique_ptr<YakFile> yf(new YakFile());
            yf->path = paths[i];
            yf->fd = open(paths[i], O_RDONLY);
            if (yf->fd < 0) return io_fail(NP2_E_ARG, std::string("cannot open ") + paths[i]);
            struct stat st;
            uint8_t hd[16];
            if (fstat(yf->fd, &st) != 0) return io_fail(NP2_E_ARG, std::string("cannot stat ") + paths[i]);
            yf->size = (size_t)st.st_size;
            if (pread(yf->fd, hd, 16, 0) != 16 || memcmp(hd, "YAK\2", 4) != 0)
                return io_fail(NP2_E_ARG, "The input binary k-mer dump file is incompatible.");
            yf->k = le32(hd + 4), yf->pre = le32(hd + 8);
            if (le32(hd + 12) != 10) return io_fail(NP2_E_ARG, "different YAK_COUNTER_BITS");
            if (yf->k >= 32 || yf->k < 2) return io_fail(NP2_E_UNSUPPORTED, "yak k must be in [2, 32) (main.rs:1433-1434)");
            if (yf->pre != 10) return io_fail(NP2_E_UNSUPPORTED, "yak pre must be 10 (kmer.rs:52-54,123-125)");
            files.push_back(std::move(yf));
        }
        std::stable_sort(files.begin(), files.end(), [](const std::unique_ptr<YakFile> &a, const std::unique_ptr<YakFile> &b) { return a->k < b->k; }); // option.rs:238
        np2_ctx_t *made = nullptr;
        const int rc = np2_ctx_create(&made, device, nullptr, 0);
        if (rc != NP2_OK) return io_fail(rc, "np2_ctx_create failed (see stderr)");
        cx.reset(made);
        {
            std::vector<std::thread> th;
            hipStream_t own[2] = {cx->stream, cx->stream_out}; // idle until the context's first call
            for (size_t i = 1; i < files.size(); ++i)
                th.emplace_back([&, i] { yak_file_to_table(*files[i], device, i < 2 ? own[i] : nullptr); });
            if (!files.empty()) yak_file_to_table(*files[0], device, own[0]);
            for (auto &t : th) t.join();
        }
        for (auto &yf : files)
            if (yf->code != NP2_OK) return io_fail(yf->code, yf->path + ": " + yf->msg);
        for (auto &yf : files) cx->yaks.push_back(yf->table);
        *out = cx.release();
        return NP2_OK;
    }, io_fail);
}
}
