"""Cost of the k-mer QV scan (csrc/np2_qv.hip) on the device; the figures of profiles/qv_cost.txt come from here.

    python tools/qv_probe.py asm [--mb 12 --reps 5]     # the scan kernel on a synthetic diploid assembly, k = 21 and 31
    python tools/qv_probe.py contig [--mb 60]           # ... on one long contig
    python tools/qv_probe.py big [--words 1e9]          # ... with the assembly's k-mers inside a table of 10^9 words (k = 21)
    python tools/qv_probe.py cli [--runs 5]             # files -> FASTA wall time on the yeast-sized assembly with / without --qv

Scan rates are k-mers per second of the kernel alone (HIP events: np2_qv_strings' kernel_ms).  Beside each, in the same
process and alternating with it, the count kernel's rate on the same bytes (np2_kcount_bytes, np2_kcount_last_stats) as
context: that kernel updates a table, this one only reads one."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import Polisher, io as np2io  # noqa: E402
from nextpolish2_amd._types import Yak  # noqa: E402
from nextpolish2_amd.synth import Synth  # noqa: E402


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def scan_leg(label, pol, tables, contigs, reps, count=True):
    stream = b"\n".join(contigs) + b"\n"
    for t, k in tables:
        scan, cnt, n_kmers, n_absent = [], [], 0, 0
        pol.qv_strings(t, contigs, 1)  # (warm: staging blocks, code object)
        for _ in range(reps):
            r = pol.qv_strings(t, contigs, 1)
            n_kmers, n_absent = r.n_kmers, r.n_absent
            scan.append(n_kmers / r.kernel_ms / 1e6)
            if count:
                np2io.count_kmers(stream, [k])
                st = np2io.kcount_last_stats()
                cnt.append(st["kmers"] / st["kernel_ms"] / 1e6)
        r = pol.qv_strings(t, contigs, 1, hist=True, bits=True)
        print(f"{label} k={k}: {n_kmers} k-mers, {n_absent} absent; scan kernel G k-mers/s: {spread(scan)}; "
              f"with histogram and bitmap {r.n_kmers / r.kernel_ms / 1e6:.3f}"
              + (f"; count kernel (k_kcount) on the same bytes G k-mers/s: {spread(cnt)}" if count else ""), flush=True)


def synth_contigs(mb, pieces, seed=5):
    s = Synth(int(mb * 1e6), depth=1, seed=seed, diploid=True)
    asm = s.pileup.ref.tobytes()
    cuts = [0] + sorted(int(x) for x in np.random.default_rng(seed).integers(1, len(asm), size=pieces - 1)) + [len(asm)]
    return s, [asm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def leg_asm(a):
    s, contigs = synth_contigs(a.mb, 17)
    pol = Polisher([s.yak(21), s.yak(31)])
    scan_leg(f"synthetic diploid assembly, {a.mb:g} Mb in 17 contigs", pol, [(0, 21), (1, 31)], contigs, a.reps)


def leg_contig(a):
    s, contigs = synth_contigs(a.mb, 1)
    pol = Polisher([s.yak(21), s.yak(31)])
    scan_leg(f"one {a.mb:g} Mb contig", pol, [(0, 21), (1, 31)], contigs, a.reps)


def leg_big(a):
    """the assembly's own k = 21 words inside a fabricated table of `words` words (tools/yak_probe.py's recipe: uniform
    over the buckets, distinct keys; filler keys have bit 43 set, a k = 21 key has 32 bits)"""
    s, contigs = synth_contigs(a.mb, 17)
    real = s.yak(21)
    n = int(a.words)
    per = n // 1024
    rng = np.random.default_rng(1)
    t0 = time.time()
    keys = rng.integers(0, 1 << 43, size=per * 1024, dtype=np.uint64) | np.uint64(1 << 43)
    keys = (keys.reshape(1024, per) | (np.arange(per, dtype=np.uint64) << np.uint64(44))[None, :])
    filler = (keys << np.uint64(10)) | rng.integers(5, 1000, size=(1024, per), dtype=np.uint64)
    ro = real.bucket_off.astype(np.int64)
    words = np.concatenate([x for b in range(1024) for x in (filler[b], real.words[ro[b]:ro[b + 1]])])
    off = (np.arange(1025, dtype=np.uint64) * np.uint64(per)) + real.bucket_off
    print(f"table: {len(words) / 1e6:.0f} M words ({len(words) * 8 / 1e9:.1f} GB) fabricated in {time.time() - t0:.1f} s", flush=True)
    pol = Polisher([Yak(21, words, off)])
    small = Polisher([real])
    # (k_kcount builds its own table from the bytes it counts: its rate does not depend on the table scanned, so it is
    # recorded once, beside the small table's figure)
    scan_leg(f"{a.mb:g} Mb assembly, its own table ({len(real.words) / 1e6:.1f} M words)", small, [(0, 21)], contigs, a.reps)
    scan_leg(f"{a.mb:g} Mb assembly, table of {len(words) / 1e6:.0f} M words", pol, [(0, 21)], contigs, a.reps, count=False)


def leg_cli(a):
    from bench import YEAST, make_assembly
    from nextpolish2_amd import cli
    from nextpolish2_amd.bamio import write_bam_raw
    syn = make_assembly(list(YEAST), 30, 1, True)
    yaks = [Synth.yak_assembly(syn, k) for k in (21, 31)]
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        bam, fa = td + "/a.bam", td + "/a.fa"
        write_bam_raw(bam, [(s.pileup.name, s.pileup.L) for s in syn], [s.bam_records(i) for i, s in enumerate(syn)])
        with open(fa, "wb") as f:
            for s in syn:
                f.write(b">%s\n%s\n" % (s.pileup.name.encode(), s.pileup.ref.tobytes()))
        yk = []
        for y in yaks:
            yk.append(td + f"/k{y.k}.yak")
            np2io.write_yak(yk[-1], y)
        base = [bam, fa] + yk + ["-t", "2", "-L", "20000"]
        walls = {"plain": [], "qv": [], "qv+bed": []}
        cli.main(base + ["-o", td + "/warm.fa"])
        for i in range(a.runs):  # alternating
            for what, extra in (("plain", []), ("qv", ["--qv", td + f"/q{i}.tsv"]), ("qv+bed", ["--qv", td + f"/b{i}.tsv", "--qv_bed", td + f"/b{i}"])):
                t0 = time.perf_counter()
                cli.main(base + extra + ["-o", td + f"/o.{what}.{i}.fa"])
                walls[what].append(time.perf_counter() - t0)
        same = open(td + "/o.plain.0.fa", "rb").read() == open(td + "/o.qv.0.fa", "rb").read() == open(td + "/o.qv+bed.0.fa", "rb").read()
        for what, w in walls.items():
            print(f"files -> FASTA, yeast-sized assembly, {what}: wall s {spread(w)}", flush=True)
        print(f"FASTA identical with and without --qv: {same}")
        print(open(td + "/q0.tsv").read().splitlines()[-2:], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["asm", "contig", "big", "cli"])
    ap.add_argument("--mb", type=float, default=None)
    ap.add_argument("--words", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.mb is None:
        a.mb = 60.0 if a.what == "contig" else 12.0
    {"asm": leg_asm, "contig": leg_contig, "big": leg_big, "cli": leg_cli}[a.what](a)


if __name__ == "__main__":
    main()
