"""Cost of the short-read quality filter (csrc/np2_srqc.hip) on the device; the figures of profiles/srqc_cost.txt come from here.

    python tools/srqc_probe.py all [--mb 12.1 --cov 60 --files 16 --dir DIR --reps 3]

The workload is tools/kcount_probe.py sim's (simulated 150-base reads of a yeast-sized synthetic assembly, both strands,
0.5 % substitutions) written as FASTQ with qualities: 70 % of the reads good throughout, 25 % with bad ends, 5 % bad
throughout.  Recorded:
  - the filter kernel's HIP-event time summed over the pieces (np2_srqc_last_stats) beside k_kcount's for one k on the same
    pieces (np2_kcount_last_stats), in one run, and bases/s for both;
  - files -> two dumps (k = 21, 31; min_count 2) wall time with and without the filter, from plain text and from gzip, with
    the time the counting thread waited for its readers (read_ms).  The run without the filter is the code path of the
    commit before the filter, byte for byte: it is the yardstick on the same box and the same files."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import io as np2io  # noqa: E402


def simulate(mb, cov, n_files, d):
    rng = np.random.default_rng(1)
    L = int(mb * 1e6)
    genome = rng.integers(0, 4, size=L, dtype=np.uint8)
    n_reads = int(L * cov / 150)
    comp = np.array([3, 2, 1, 0], np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    plain = []
    t0 = time.perf_counter()
    for f in range(n_files):
        n = n_reads // n_files
        st = rng.integers(0, L - 150, size=n)
        r = genome[st[:, None] + np.arange(150)[None, :]]
        rc = rng.random(n) < 0.5
        r[rc] = comp[r[rc][:, ::-1]]
        err = rng.random(r.shape) < 0.005
        r[err] = rng.integers(0, 4, size=int(err.sum()), dtype=np.uint8)
        q = rng.integers(30, 41, size=(n, 150)).astype(np.uint8)
        kind = rng.random(n)
        ends = np.flatnonzero(kind < 0.25)
        q[ends, :12] = rng.integers(2, 15, size=(len(ends), 12))
        q[ends, -20:] = rng.integers(2, 15, size=(len(ends), 20))
        bad = np.flatnonzero(kind > 0.95)
        q[bad] = rng.integers(2, 15, size=(len(bad), 150))
        # @rNNNNNNNN \n 150 bases \n + \n 150 qualities \n
        txt = np.empty((n, 10 + 1 + 150 + 1 + 2 + 150 + 1), np.uint8)
        txt[:, 0] = ord("@")
        txt[:, 1] = ord("r")
        ids = np.arange(n)
        for dgt in range(8):
            txt[:, 9 - dgt] = 48 + (ids // 10 ** dgt) % 10
        txt[:, 10] = 10
        txt[:, 11:161] = letters[r]
        txt[:, 161] = 10
        txt[:, 162] = ord("+")
        txt[:, 163] = 10
        txt[:, 164:314] = q + 33
        txt[:, 314] = 10
        p = os.path.join(d, f"sim.{f}.fq")
        txt.tofile(p)
        plain.append(p)
    procs = [subprocess.Popen(["gzip", "-1", "-k", "-f", p]) for p in plain]
    for pr in procs:
        assert pr.wait() == 0
    gz = [p + ".gz" for p in plain]
    print(f"simulated {n_reads // n_files * n_files} FASTQ reads of 150 bases ({mb} Mb x {cov}) in {n_files} files, plain "
          f"{sum(map(os.path.getsize, plain)) / 1e6:.0f} MB, gzip -1 {sum(map(os.path.getsize, gz)) / 1e6:.0f} MB ({time.perf_counter() - t0:.0f} s)", flush=True)
    return plain, gz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all"])
    ap.add_argument("--mb", type=float, default=12.1)
    ap.add_argument("--cov", type=float, default=60.0)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    qc = np2io.SrQc.recipe()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        plain, gz = simulate(a.mb, a.cov, a.files, td)
        one = os.path.join(td, "one.k21.yak")
        for rep in range(a.reps):  # kernels, one k, the same pieces
            np2io.count_kmers_to_files(plain, [21], [one], min_count=1, qc=qc)
            kc, sq = np2io.kcount_last_stats(), np2io.srqc_last_stats()
            pieces = -(-(sq["bases_in"] + sq["reads"]) // (8 << 20))
            print(f"kernels (k = 21, ~{pieces} pieces of 8 MiB): filter {sq['kernel_ms']:.2f} ms = {sq['bases_in'] / sq['kernel_ms'] / 1e6:.1f} G bases/s "
                  f"({sq['kernel_ms'] / pieces:.3f} ms per piece); k_kcount on the masked pieces {kc['kernel_ms']:.2f} ms = "
                  f"{sq['bases_in'] / kc['kernel_ms'] / 1e6:.1f} G bases/s ({kc['kmers']} k-mers); "
                  + np2io.srqc_stats_text(sq), flush=True)
        np2io.count_kmers_to_files(plain, [21], [one], min_count=1)
        kc = np2io.kcount_last_stats()
        print(f"kernels, no filter (k = 21): k_kcount {kc['kernel_ms']:.2f} ms ({kc['kmers']} k-mers)", flush=True)
        outs = [os.path.join(td, f"w.k{k}.yak") for k in (21, 31)]
        for label, paths in (("plain", plain), ("gzip", gz)):
            for name, q in (("without --sr_qc", None), ("with --sr_qc", qc)):
                for rep in range(a.reps):
                    t0 = time.perf_counter()
                    np2io.count_kmers_to_files(paths, [21, 31], outs, min_count=2, qc=q)
                    wall = time.perf_counter() - t0
                    st = np2io.kcount_last_stats()
                    extra = f", filter kernel {np2io.srqc_last_stats()['kernel_ms'] / 1e3:.3f} s" if q is not None else ""
                    print(f"{label}, {name}: files -> two dumps (k = 21, 31; min_count 2) wall {wall:.3f} s: count kernels {st['kernel_ms'] / 1e3:.3f} s"
                          f"{extra}, waiting for readers (read_ms) {st['read_ms'] / 1e3:.3f} s, growths {st['growths']}, passes {st['passes']}", flush=True)


if __name__ == "__main__":
    main()
