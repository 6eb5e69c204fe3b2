// Host plumbing the drivers share: the queue of pinned pieces between reader threads and the device thread, the writer
// that cuts a separator stream into pieces with a halo, and the packer that lays a set of strings on tile boundaries of a
// staging buffer.  Host-only: no HIP here and no memory of its own for pieces (the caller hands the buffers in), so that a
// plain C++ compiler builds it (tests/tools/pieces_test.cpp, under the thread and address sanitizers).
#pragma once
#include "np2_abi.hpp"
#include "np2_kcount_core.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace np2h {

using np2kc::HALO;

// A piece on the device is HALO bytes, n bytes and separators up to the next multiple of 16 (the kernels load 16-byte
// words): pads `buf` (which has the room) and returns how many bytes go up.
inline size_t pad_piece(uint8_t *buf, size_t n) {
    const size_t padded = (HALO + n + 15) & ~(size_t)15;
    memset(buf + HALO + n, '\n', padded - (HALO + n));
    return padded;
}

// ---------------------------------------------------------------------------------------------------------------
// pieces between reader threads and the device thread
// ---------------------------------------------------------------------------------------------------------------
template <class P> struct PieceQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<P *> full, idle;
    int producers = 0;
    bool abort = false;
    int err_code = NP2_OK;
    std::string err;
    P *take_idle() { // reader side; nullptr: the run was given up
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return abort || !idle.empty(); });
        if (abort) return nullptr;
        P *p = idle.front();
        idle.pop_front();
        return p;
    }
    void give_full(P *p) {
        std::lock_guard<std::mutex> l(mu);
        full.push_back(p);
        cv.notify_all();
    }
    P *take_full() { // device side; nullptr: every reader has finished and nothing is left
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return !full.empty() || producers == 0; });
        if (full.empty()) return nullptr;
        P *p = full.front();
        full.pop_front();
        return p;
    }
    void give_idle(P *p) {
        std::lock_guard<std::mutex> l(mu);
        idle.push_back(p);
        cv.notify_all();
    }
    void producer_done(int code, const std::string &m) { // the first error wins and ends the run
        std::lock_guard<std::mutex> l(mu);
        if (code != NP2_OK && err_code == NP2_OK) err_code = code, err = m, abort = true;
        --producers;
        cv.notify_all();
    }
    void give_up() {
        std::lock_guard<std::mutex> l(mu);
        abort = true;
        cv.notify_all();
    }
};

// The reader threads of a run.  Whatever way the device thread leaves, the queues are given up and the threads joined
// before anything they use goes away: declare it after the queues and the pieces.
template <class P> struct Readers {
    std::vector<PieceQueue<P> *> queues;
    std::vector<std::thread> th;
    Readers() = default;
    Readers(Readers &&) = default;
    ~Readers() {
        for (auto *q : queues) q->give_up();
        for (auto &t : th) t.join();
    }
    template <class Body> void start(PieceQueue<P> *q, Body body, size_t ti) {
        th.emplace_back([q, body, ti] {
            int code = NP2_OK;
            std::string msg;
            try {
                body(ti);
            } catch (...) {
                try {
                    current_error(code, msg);
                } catch (...) { // (the status still gets through)
                }
            }
            q->producer_done(code, msg);
        });
    }
};
// n_threads readers on one queue: pieces come out as they fill.  body(ti) runs on thread ti; what it throws becomes the
// queue's (err_code, err).
template <class P, class Body> Readers<P> run_readers(size_t n_threads, PieceQueue<P> &q, Body body) {
    Readers<P> r;
    r.queues.push_back(&q);
    q.producers = (int)n_threads;
    for (size_t ti = 0; ti < n_threads; ++ti) r.start(&q, body, ti);
    return r;
}
// ... and a queue each: a reader's pieces come out in its own order.
template <class P, class Body> Readers<P> run_readers(size_t n_threads, std::vector<PieceQueue<P>> &qs, Body body) {
    Readers<P> r;
    for (size_t ti = 0; ti < n_threads; ++ti) qs[ti].producers = 1, r.queues.push_back(&qs[ti]);
    for (size_t ti = 0; ti < n_threads; ++ti) r.start(&qs[ti], body, ti);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// a stream into pieces of `cap` bytes, each with the stream's last HALO bytes in front
// ---------------------------------------------------------------------------------------------------------------
// P has `uint8_t *buf` (HALO bytes, then `cap` bytes) and `size_t n`.  Where the pieces come from and go to is the
// caller's: a PieceQueue, or buffers of its own.
template <class P> struct HaloWriter {
    size_t cap;
    std::function<P *()> take;       // an empty piece; nullptr: the run was given up
    std::function<void(P *)> full;   // a piece with bytes in it
    std::function<void(P *)> unused; // a piece nothing was written to
    std::function<void(P &)> on_fresh; // (optional) what else a piece forgets when it is taken
    P *cur = nullptr;
    uint8_t tail[HALO];
    bool dead = false;
    explicit HaloWriter(size_t cap_) : cap(cap_) { memset(tail, '\n', HALO); }
    HaloWriter(PieceQueue<P> &q, size_t cap_) : HaloWriter(cap_) {
        take = [&q] { return q.take_idle(); };
        full = [&q](P *p) { q.give_full(p); };
        unused = [&q](P *p) { q.give_idle(p); };
    }
    bool fresh() {
        cur = take();
        if (!cur) return !(dead = true);
        memcpy(cur->buf, tail, HALO);
        cur->n = 0;
        if (on_fresh) on_fresh(*cur);
        return true;
    }
    void flush(bool even_empty = false) {
        if (!cur) return;
        if (cur->n == 0 && !even_empty) {
            unused(cur);
        } else {
            memcpy(tail, cur->buf + cur->n, HALO); // the last HALO bytes of halo + data
            full(cur);
        }
        cur = nullptr;
    }
    void put(const uint8_t *p, size_t n) {
        while (n && !dead) {
            if (!cur && !fresh()) return;
            const size_t take_n = std::min(n, cap - cur->n);
            memcpy(cur->buf + HALO + cur->n, p, take_n);
            cur->n += take_n, p += take_n, n -= take_n;
            if (cur->n == cap) flush();
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------
// a set of strings through a staging buffer of `cap_tiles` tiles
// ---------------------------------------------------------------------------------------------------------------
// the checks every *_strings entry point makes of its set: off[0 .. n] ascending, strs there when a byte is asked for
inline void check_string_set(const char *who, const uint8_t *strs, const uint64_t *off, uint64_t n) {
    if (n && !off) throw Np2Error(NP2_E_ARG, std::string(who) + ": off is NULL with n > 0");
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) throw Np2Error(NP2_E_ARG, std::string(who) + ": off is descending at sequence " + std::to_string(i));
    if (n && off[n] > off[0] && !strs) throw Np2Error(NP2_E_ARG, std::string(who) + ": strs is NULL with a non-zero length");
}

// A piece: whole tiles of consecutive sequences, each starting at a tile boundary and padded with `pad` to the next one; a
// sequence longer than what is left of the piece goes on in the next one, whose halo then holds the `halo` bytes before
// it (else `pad`).  hd[t] is tile t's descriptor: its span's index in `spans`, with `first_flag` on a sequence's first
// tile.  A sequence's bitmap (a bit a base, `tile_bits` bytes a tile) starts where the one before it ends; an empty
// sequence has no tile.
struct StringPieces {
    struct Span { // a sequence's tiles in the piece, from tile0 on: the piece's counters `index in spans` are its own
        uint64_t seq, bit_at, bit_bytes;
        uint32_t tile0;
    };
    const uint8_t *strs;
    const uint64_t *off;
    uint64_t n;
    uint32_t cap, tile, halo, first_flag, tile_bits;
    uint8_t pad;
    std::vector<uint8_t> hs;  // halo, then nt tiles
    std::vector<uint32_t> hd; // nt descriptors
    std::vector<Span> spans;
    uint32_t nt = 0;
    uint64_t i = 0, p = 0, bit_base = 0; // sequence, bytes of it already handed out, its first bitmap byte

    StringPieces(const uint8_t *strs_, const uint64_t *off_, uint64_t n_, uint32_t cap_tiles, uint32_t tile_, uint32_t halo_, uint8_t pad_,
                 uint32_t first_flag_, uint32_t tile_bits_)
        : strs(strs_), off(off_), n(n_), cap(cap_tiles), tile(tile_), halo(halo_), first_flag(first_flag_), tile_bits(tile_bits_), pad(pad_),
          hs(halo_ + (size_t)cap_tiles * tile_), hd(cap_tiles) {}
    bool next() { // false: the set is through
        nt = 0;
        spans.clear();
        if (i >= n) return false;
        if (p && p < off[i + 1] - off[i])
            memcpy(hs.data(), strs + off[i] + p - halo, halo);
        else
            memset(hs.data(), pad, halo);
        while (i < n && nt < cap) {
            const uint64_t len = off[i + 1] - off[i];
            if (p >= len) {
                bit_base += (len + 7) / 8;
                ++i;
                p = 0;
                continue;
            }
            const uint32_t take = (uint32_t)std::min<uint64_t>((len - p + tile - 1) / tile, cap - nt);
            const uint64_t bytes = std::min<uint64_t>(len - p, (uint64_t)take * tile);
            uint8_t *dst = hs.data() + halo + (size_t)nt * tile;
            memcpy(dst, strs + off[i] + p, bytes);
            memset(dst + bytes, pad, (size_t)take * tile - bytes);
            for (uint32_t x = 0; x < take; ++x) hd[nt + x] = (uint32_t)spans.size() | (p == 0 && x == 0 ? first_flag : 0u);
            spans.push_back({i, bit_base + p / 8, std::min<uint64_t>((len + 7) / 8 - p / 8, (uint64_t)take * tile_bits), nt});
            nt += take;
            p += (uint64_t)take * tile;
        }
        return nt != 0;
    }
};

} // namespace np2h
