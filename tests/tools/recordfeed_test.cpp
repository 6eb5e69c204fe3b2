// The paired reader's record feed (csrc/np2_recordfeed.hpp: a thread per FASTQ file, record batches over a bounded queue) as
// a stand-alone host program, built with the thread sanitizer and with the address and undefined-behaviour sanitizers by
// tests/test_sradapt_cpu.py.
//   in_step R1 R2    the records of both files in step, mate 1 then mate 2, one line each: header TAB bases TAB qualities;
//                    then "end <records of R1> <records of R2>" (one file may go on after the other has ended)
//   leave R1 R2 N    the consumer goes after N records of each file while the readers are still at work; prints "left"
// A reader's error is printed as "error <code> <message>" where the consumer meets it.
#include "../../nextpolish2_amd/csrc/np2_recordfeed.hpp"

#include <cstdio>
#include <cstdlib>

using np2h::RecordFeed;

static void line(const RecordFeed::Rec &r) {
    std::fwrite(r.hdr, 1, r.hdr_len, stdout), std::fputc('\t', stdout);
    std::fwrite(r.seq, 1, r.len, stdout), std::fputc('\t', stdout);
    std::fwrite(r.qual, 1, r.len, stdout), std::fputc('\n', stdout);
}

int main(int argc, char **argv) {
    if (argc < 4) return std::fprintf(stderr, "usage: recordfeed_test in_step|leave R1 R2 [N]\n"), 2;
    const std::string what = argv[1];
    const long stop_after = argc > 4 ? std::atol(argv[4]) : -1;
    try {
        RecordFeed f1, f2;
        f1.start(argv[2], true), f2.start(argv[3], true);
        for (long i = 0; what != "leave" || i < stop_after; ++i) {
            const RecordFeed::Rec *r1 = f1.next(), *r2 = f2.next();
            if (!r1 && !r2) break;
            if (what == "leave") continue;
            if (r1) line(*r1);
            if (r2) line(*r2);
        }
        if (what == "leave") std::printf("left\n");
        else std::printf("end %llu %llu\n", (unsigned long long)f1.taken, (unsigned long long)f2.taken);
    } catch (const np2h::Np2Error &e) {
        std::printf("error %d %s\n", e.code, e.what());
    }
    return 0;
}
