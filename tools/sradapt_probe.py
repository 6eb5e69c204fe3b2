"""Cost of the short-read adapter trimmer (csrc/np2_sradapt.hip) on the device; the figures of profiles/sradapt_cost.txt come
from here.

    python tools/sradapt_probe.py all [--mb 12.1 --cov 60 --files 16 --dir DIR --reps 3]

The workload is tools/srqc_probe.py's (tools/kcount_probe.py sim's 150-base reads as FASTQ with qualities), its 16 files
read as 8 pairs R1 R2 R1 R2 ...  The reads of two files are not mates: nearly no pair has an overlap, so every wavefront
scores every candidate shift before it gives up -- the overlap search's most expensive case.  Recorded:
  - k_sradapt's HIP-event time summed over the pieces (np2_sradapt_last_stats) and bases/s, beside k_srqc's
    (np2_srqc_last_stats) and k_kcount's for one k (np2_kcount_last_stats) on the same reads, and the ratio to k_srqc;
  - files -> two dumps (k = 21, 31; min_count 2) wall time with --sr_qc alone and with --sr_qc --sr_adapter, from plain text
    and from gzip, with the time the counting thread waited for its readers (read_ms).  The run without --sr_adapter is the
    code path of the commit before the trimmer: it is the yardstick on the same box and the same files."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nextpolish2_amd import io as np2io  # noqa: E402
from srqc_probe import simulate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all"])
    ap.add_argument("--mb", type=float, default=12.1)
    ap.add_argument("--cov", type=float, default=60.0)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.files % 2:
        ap.error("--files must be even: the files are read as pairs")
    qc, ad = np2io.SrQc.recipe(), np2io.SrAdapt(pair=True)
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        plain, gz = simulate(a.mb, a.cov, a.files, td)
        one = os.path.join(td, "one.k21.yak")
        for rep in range(a.reps):  # kernels, one k
            np2io.count_kmers_to_files(plain, [21], [one], min_count=1, qc=qc)
            kq, sq = np2io.kcount_last_stats(), np2io.srqc_last_stats()
            np2io.count_kmers_to_files(plain, [21], [one], min_count=1, qc=qc, ad=ad)
            ka, sa = np2io.kcount_last_stats(), np2io.sradapt_last_stats()
            print(f"kernels (k = 21): k_sradapt {sa['kernel_ms']:.2f} ms = {sa['bases_in'] / sa['kernel_ms'] / 1e6:.1f} G bases/s; "
                  f"k_srqc {sq['kernel_ms']:.2f} ms = {sq['bases_in'] / sq['kernel_ms'] / 1e6:.1f} G bases/s; ratio {sa['kernel_ms'] / sq['kernel_ms']:.2f}; "
                  f"k_kcount after k_sradapt {ka['kernel_ms']:.2f} ms, after k_srqc {kq['kernel_ms']:.2f} ms; " + np2io.sradapt_stats_text(sa), flush=True)
        outs = [os.path.join(td, f"w.k{k}.yak") for k in (21, 31)]
        for label, paths in (("plain", plain), ("gzip", gz)):
            for name, adapter in (("--sr_qc", None), ("--sr_qc --sr_adapter", ad)):
                for rep in range(a.reps):
                    t0 = time.perf_counter()
                    np2io.count_kmers_to_files(paths, [21, 31], outs, min_count=2, qc=qc, ad=adapter)
                    wall = time.perf_counter() - t0
                    st = np2io.kcount_last_stats()
                    ms = (np2io.sradapt_last_stats() if adapter is not None else np2io.srqc_last_stats())["kernel_ms"]
                    print(f"{label}, {name}: files -> two dumps (k = 21, 31; min_count 2) wall {wall:.3f} s: count kernels {st['kernel_ms'] / 1e3:.3f} s, "
                          f"{'k_sradapt' if adapter is not None else 'k_srqc'} {ms / 1e3:.3f} s, waiting for readers (read_ms) {st['read_ms'] / 1e3:.3f} s, "
                          f"growths {st['growths']}, passes {st['passes']}", flush=True)


if __name__ == "__main__":
    main()
