// A FASTQ file read by a thread of its own into batches of records: what lets the paired reader (np2_sradapt_host.hpp:
// pair_files) walk R1 and R2 in step.  Host-only, no HIP: a plain C++ compiler builds it (tests/tools/recordfeed_test.cpp,
// under the thread and address sanitizers).
#pragma once
#include "np2_seqreader.hpp"

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

namespace np2h {

// One FASTQ file read by a thread of its own, its records handed over a bounded queue in batches.  A batch is three flat
// buffers (headers, bases, qualities) and the records' lengths: nothing is allocated per record.
struct RecordFeed {
    struct Batch {
        std::string hdr, seq, qual;
        std::vector<uint32_t> hdr_len, len; // per record: header bytes, bases (= quality bytes)
        void clear() { hdr.clear(), seq.clear(), qual.clear(), hdr_len.clear(), len.clear(); }
    };
    struct Rec { // a view into the consumer's batch, good until the next next()
        const uint8_t *hdr, *seq, *qual;
        size_t hdr_len, len;
    };
    static constexpr size_t BATCH_RECORDS = 2048, MAX_BATCHES = 4;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Batch> q, spare; // filled batches; emptied ones on their way back
    bool done = false, stop = false;
    int code = NP2_OK;
    std::string msg;
    std::thread th;
    Batch have; // the consumer's batch
    size_t at = 0, at_hdr = 0, at_seq = 0;
    Rec rec{};
    uint64_t taken = 0; // records handed out

    ~RecordFeed() {
        {
            std::lock_guard<std::mutex> l(mu);
            stop = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
    bool give(Batch &batch) { // false: the consumer has gone
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return stop || q.size() < MAX_BATCHES; });
        if (stop) return false;
        q.emplace_back(std::move(batch));
        if (!spare.empty()) {
            batch = std::move(spare.front());
            spare.pop_front();
        } else {
            batch = Batch();
        }
        cv.notify_all();
        return true;
    }
    void start(const std::string &path, bool want_hdr) {
        th = std::thread([this, path, want_hdr] {
            try {
                np2seq::RecordCheck chk;
                chk.file_begin(path);
                Batch batch;
                size_t hdr0 = 0; // where the open record's header begins in batch.hdr
                bool gone = false;
                np2seq::parse_file_qual(
                    path,
                    [&](const uint8_t *p, size_t n) {
                        if (n == 1 && *p == '\n') chk.seq_end();
                        else chk.seq_bytes(n), batch.seq.append((const char *)p, n);
                    },
                    [&](const uint8_t *p, size_t n) {
                        if (n == 1 && *p == '\n') {
                            const uint32_t len = (uint32_t)chk.sl;
                            chk.qual_end();
                            while (batch.hdr.size() > hdr0 && batch.hdr.back() == '\r') batch.hdr.pop_back();
                            batch.hdr_len.push_back((uint32_t)(batch.hdr.size() - hdr0)), batch.len.push_back(len);
                            hdr0 = batch.hdr.size();
                            if (batch.len.size() >= BATCH_RECORDS) {
                                if (!give(batch)) gone = true;
                                batch.clear(), hdr0 = 0;
                            }
                        } else {
                            chk.qual_bytes(n), batch.qual.append((const char *)p, n);
                        }
                    },
                    [&] { return gone; },
                    [&](const uint8_t *p, size_t n, bool begin) {
                        if (!want_hdr) return;
                        if (begin) batch.hdr.resize(hdr0);
                        else batch.hdr.append((const char *)p, n);
                    });
                if (!gone) {
                    chk.file_end();
                    if (!batch.len.empty()) (void)give(batch);
                }
            } catch (...) {
                std::lock_guard<std::mutex> l(mu);
                try {
                    current_error(code, msg);
                } catch (...) {
                    code = NP2_E_NOMEM;
                }
            }
            std::lock_guard<std::mutex> l(mu);
            done = true;
            cv.notify_all();
        });
    }
    // the file's next record, or nullptr at its end; what the reader threw is thrown here
    const Rec *next() {
        if (at == have.len.size()) {
            std::unique_lock<std::mutex> l(mu);
            cv.wait(l, [&] { return done || !q.empty(); });
            if (q.empty()) {
                if (code != NP2_OK) throw Np2Error(code, msg);
                return nullptr;
            }
            have.clear();
            spare.emplace_back(std::move(have));
            have = std::move(q.front());
            q.pop_front();
            at = at_hdr = at_seq = 0;
            cv.notify_all();
        }
        rec = Rec{(const uint8_t *)have.hdr.data() + at_hdr, (const uint8_t *)have.seq.data() + at_seq, (const uint8_t *)have.qual.data() + at_seq,
                  have.hdr_len[at], have.len[at]};
        at_hdr += rec.hdr_len, at_seq += rec.len;
        ++at, ++taken;
        return &rec;
    }
};

} // namespace np2h
