"""Cost of the read binner (csrc/np2_bin.hip) on the device; the figures of profiles/bin_cost.txt come from here.

    python tools/bin_probe.py all [--out FILE]      # every step below, one child process each under its own time limit
    python tools/bin_probe.py hifi [--mb 64]        # k_bin_* on 15 kb reads cut from a synthetic diploid genome, k = 21
    python tools/bin_probe.py short [--mb 16]       # ... on 150-base reads
    python tools/bin_probe.py files [--mb 64]       # read files -> TSV wall time (np2_bin_files), plain FASTA and gzip FASTQ

The yardstick is k_trio_scan: in the same process and alternating with the binner, np2_trio_strings on the same reads as
sequences of their own (tile-aligned staging: every read from a tile boundary) against the same two tables; both report
the HIP-event time of their kernels.  The parental k-mers sit inside tables of --words words each (tools/trio_probe.py's
parent_table).  `all` stops at the first step that fails or runs out of time: nothing more is started on the device
after that."""
import argparse
import gzip
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

K = 21
STEP_LIMITS = {"hifi": 420, "short": 420, "files": 420}  # seconds


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def make_reads(genome_mb, total_mb, read_len, seed=5):
    """(Synth, reads): reads of about `read_len` bases cut alternately from the two haplotypes, `total_mb` MB in all"""
    from nextpolish2_amd.synth import Synth
    s = Synth(int(genome_mb * 1e6), depth=1, seed=seed, diploid=True)
    rng = np.random.default_rng(seed)
    n = min(len(s.hap1), len(s.hap2))
    reads, left, i = [], int(total_mb * 1e6), 0
    while left > 0:
        ln = max(50, int(rng.normal(read_len, read_len * 0.1)))
        a = int(rng.integers(0, n - ln))
        reads.append((s.hap1 if i % 2 == 0 else s.hap2)[a:a + ln])
        left -= ln + 1
        i += 1
    return s, reads


def tables_of(s, words):
    from trio_probe import parent_table
    t0 = time.time()
    yaks = [parent_table(s.hap1 + b"\n", words, 1), parent_table(s.hap2 + b"\n", words, 2)]
    print(f"tables: {len(yaks[0].words) / 1e6:.0f} M and {len(yaks[1].words) / 1e6:.0f} M words made in {time.time() - t0:.1f} s", flush=True)
    return yaks


def scan_leg(label, a, read_len):
    from nextpolish2_amd import Polisher
    s, reads = make_reads(a.genome_mb, a.mb, read_len)
    pol = Polisher(tables_of(s, a.words))
    stream = b"".join(r + b"\n" for r in reads)
    b = pol.bin_stream(0, 1, stream, stats=True)  # (warm: staging blocks, code objects)
    t = pol.trio_strings(0, 1, reads)
    same = np.array_equal(b.stats.astype(np.uint64), t.stats)
    bin_ms, trio_ms, ratio = [], [], []
    for _ in range(a.reps):  # alternating
        rb = pol.bin_stream(0, 1, stream)
        rt = pol.trio_strings(0, 1, reads)
        bin_ms.append(rb.kernel_ms)
        trio_ms.append(rt.kernel_ms)
        ratio.append(rb.kernel_ms / rt.kernel_ms)
    n = int(t.stats[:, 0].sum())
    counts = {c: b.classes.count(c.encode()) for c in "pma0"}
    print(f"{label}: {len(reads)} reads, {len(stream)} stream bytes, {n} k-mers, classes {counts}, tallies equal to np2_trio_strings: {same}", flush=True)
    print(f"  binner (k_bin_owner + k_bin_scan + k_bin_join + k_bin_classify) G k-mers/s: {spread([n / ms / 1e6 for ms in bin_ms])}", flush=True)
    print(f"  k_trio_scan + k_trio_join, same reads tile-aligned, G k-mers/s: {spread([n / ms / 1e6 for ms in trio_ms])}", flush=True)
    print(f"  binner kernel time / trio kernel time: {spread(ratio)}", flush=True)
    pol.close()


def leg_hifi(a):
    scan_leg(f"15 kb reads, {a.mb:g} MB, tables of {a.words:g} words", a, 15000)


def leg_short(a):
    scan_leg(f"150-base reads, {a.mb:g} MB, tables of {a.words:g} words", a, 150)


def leg_files(a):
    from nextpolish2_amd import Polisher, io as np2io
    s, reads = make_reads(a.genome_mb, a.mb, 15000)
    pol = Polisher(tables_of(s, a.words))
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        fa, fq = td + "/reads.fa", td + "/reads.fq.gz"
        with open(fa, "wb") as f:
            for i, r in enumerate(reads):
                f.write(b">read%d\n%s\n" % (i, r))
        with gzip.open(fq, "wb", compresslevel=1) as f:
            for i, r in enumerate(reads):
                f.write(b"@read%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
        np2io.bin_files(pol, [fa], tsv=td + "/warm.tsv")
        walls = {"plain FASTA -> TSV": [], "plain FASTA -> TSV + lists + both bins": [], "gzip FASTQ -> TSV": []}
        kernel = []
        for i in range(a.runs):  # alternating
            t0 = time.perf_counter()
            _, ms = np2io.bin_files(pol, [fa], tsv=td + f"/a{i}.tsv")
            walls["plain FASTA -> TSV"].append(time.perf_counter() - t0)
            kernel.append(ms / 1e3)
            t0 = time.perf_counter()
            np2io.bin_files(pol, [fa], tsv=td + f"/b{i}.tsv", pat_list=td + "/p.list", mat_list=td + "/m.list", pat_fa=td + "/p.fa", mat_fa=td + "/m.fa")
            walls["plain FASTA -> TSV + lists + both bins"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            np2io.bin_files(pol, [fq], tsv=td + f"/c{i}.tsv")
            walls["gzip FASTQ -> TSV"].append(time.perf_counter() - t0)
        same = open(td + "/a0.tsv", "rb").read() == open(td + "/b0.tsv", "rb").read() == open(td + "/c0.tsv", "rb").read()
        print(f"files, {len(reads)} reads of 15 kb, {os.path.getsize(fa) / 1e6:.0f} MB plain, {os.path.getsize(fq) / 1e6:.0f} MB gzip; the three reports identical: {same}", flush=True)
        for what, w in walls.items():
            print(f"  {what}: wall s {spread(w)}", flush=True)
        print(f"  of which kernels (plain FASTA -> TSV): s {spread(kernel)}", flush=True)
    pol.close()


def run_all(a):
    """one child per step, each under its own time limit; the first failure ends the run"""
    out = open(a.out, "a") if a.out else None
    for step in ("hifi", "short", "files"):
        cmd = [sys.executable, os.path.abspath(__file__), step, "--reps", str(a.reps), "--runs", str(a.runs), "--words", str(a.words),
               "--genome_mb", str(a.genome_mb)]
        if a.dir:
            cmd += ["--dir", a.dir]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMITS[step])
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {step}: no result within {STEP_LIMITS[step]} s\n", 124
        text = f"== {step} (exit {rc})\n{text}"
        print(text, flush=True)
        if out:
            out.write(text)
            out.flush()
        if rc != 0:
            return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "hifi", "short", "files"])
    p.add_argument("--mb", type=float, default=None, help="MB of reads [hifi, files: 64; short: 16]")
    p.add_argument("--genome_mb", type=float, default=12, help="Mb of the synthetic diploid genome the reads are cut from [12]")
    p.add_argument("--words", type=float, default=2e7, help="words of each parental table [2e7]")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--dir", default=None, help="where the files step writes its inputs [the system's temporary directory]")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    if a.mb is None:
        a.mb = 16 if a.step == "short" else 64
    {"hifi": leg_hifi, "short": leg_short, "files": leg_files}[a.step](a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
