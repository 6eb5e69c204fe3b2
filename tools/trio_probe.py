"""Cost of the trio scan (csrc/np2_trio.hip) on the device; the figures of profiles/trio_cost.txt come from here.

    python tools/trio_probe.py all [--out FILE]        # every step below, one child process each under its own time limit
    python tools/trio_probe.py asm [--mb 12]           # k_trio_scan + k_trio_join on a synthetic diploid assembly, k = 21
    python tools/trio_probe.py contig [--mb 60]        # ... on one long contig
    python tools/trio_probe.py cli [--runs 5]          # files -> FASTA wall time on the yeast-sized assembly with / without --trio

The yardstick is k_qv_scan: in the same process and alternating with the trio scan, the QV scan of the same bytes against
each of the two tables (np2_qv_strings' kernel_ms).  The trio scan reads the bytes once and probes twice, so its time
should not exceed the sum of the two QV scans; the ratio is printed with the spread of the repeats.  The parental k-mers
sit inside tables of --words words each (filler keys as in tools/qv_probe.py: bit 43 set, a k = 21 key has 32 bits).
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 21
STEP_LIMITS = {"asm": 420, "contig": 420, "cli": 540}  # seconds


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def chimera(h1, h2, block):
    n = min(len(h1), len(h2))
    return b"".join((h1 if (a // block) % 2 == 0 else h2)[a:a + block] for a in range(0, n, block))


def parent_table(hap_stream, words, seed):
    """one parent's k-mers (counted on the device, every count times five) inside a table of `words` words"""
    from nextpolish2_amd import io as np2io
    from nextpolish2_amd._types import Yak
    real = np2io.count_kmers(hap_stream, [K])[0]
    rw = (real.words & ~np.uint64(1023)) | np.minimum((real.words & np.uint64(1023)) * np.uint64(5), np.uint64(1023))
    per = max(0, int(words) - len(rw)) // 1024
    if per == 0:
        return Yak(K, rw, real.bucket_off)
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 43, size=per * 1024, dtype=np.uint64) | np.uint64(1 << 43)
    keys = keys.reshape(1024, per) | (np.arange(per, dtype=np.uint64) << np.uint64(44))[None, :]
    filler = (keys << np.uint64(10)) | rng.integers(5, 1000, size=(1024, per), dtype=np.uint64)
    ro = real.bucket_off.astype(np.int64)
    w = np.concatenate([x for b in range(1024) for x in (filler[b], rw[ro[b]:ro[b + 1]])])
    return Yak(K, w, (np.arange(1025, dtype=np.uint64) * np.uint64(per)) + real.bucket_off)


def scan_leg(label, a, pieces):
    from nextpolish2_amd import Polisher
    from nextpolish2_amd.synth import Synth
    s = Synth(int(a.mb * 1e6), depth=1, seed=5, diploid=True)
    asm = chimera(s.hap1, s.hap2, 1_000_000)
    cuts = [0] + sorted(int(x) for x in np.random.default_rng(5).integers(1, len(asm), size=pieces - 1)) + [len(asm)]
    contigs = [asm[x:y] for x, y in zip(cuts[:-1], cuts[1:])]
    t0 = time.time()
    yaks = [parent_table(s.hap1 + b"\n", a.words, 1), parent_table(s.hap2 + b"\n", a.words, 2)]
    print(f"tables: {len(yaks[0].words) / 1e6:.0f} M and {len(yaks[1].words) / 1e6:.0f} M words made in {time.time() - t0:.1f} s", flush=True)
    pol = Polisher(yaks)
    pol.trio_strings(0, 1, contigs)  # (warm: staging blocks, code objects)
    pol.qv_strings(0, contigs, 1)
    trio_ms, qv_ms, ratio = [], [[], []], []
    for _ in range(a.reps):  # alternating
        r = pol.trio_strings(0, 1, contigs)
        q = [pol.qv_strings(t, contigs, 1) for t in (0, 1)]
        trio_ms.append(r.kernel_ms)
        for t in (0, 1):
            qv_ms[t].append(q[t].kernel_ms)
        ratio.append(r.kernel_ms / (q[0].kernel_ms + q[1].kernel_ms))
    n = r.total[0]
    rb = pol.trio_strings(0, 1, contigs, bits=True)
    print(f"{label}: {n} k-mers, {r.total[1]} paternal and {r.total[2]} maternal markers, {r.n_switch} switches", flush=True)
    print(f"  trio scan (k_trio_scan + k_trio_join) G k-mers/s: {spread([n / ms / 1e6 for ms in trio_ms])}; with both bitmaps {n / rb.kernel_ms / 1e6:.3f}", flush=True)
    for t, who in ((0, "paternal"), (1, "maternal")):
        print(f"  k_qv_scan, same bytes, {who} table G k-mers/s: {spread([n / ms / 1e6 for ms in qv_ms[t]])}", flush=True)
    print(f"  trio time / (QV paternal + QV maternal): {spread(ratio)}", flush=True)
    pol.close()


def leg_asm(a):
    scan_leg(f"synthetic diploid assembly, {a.mb:g} Mb in 17 contigs, tables of {a.words:g} words", a, 17)


def leg_contig(a):
    scan_leg(f"one {a.mb:g} Mb contig, tables of {a.words:g} words", a, 1)


def leg_cli(a):
    from bench import YEAST, make_assembly
    from nextpolish2_amd import cli, io as np2io
    from nextpolish2_amd.bamio import write_bam_raw
    from nextpolish2_amd.synth import Synth
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
        parents = []
        for who, haps in (("pat", [s.hap1 for s in syn]), ("mat", [s.hap2 for s in syn])):
            parents.append(td + f"/{who}.yak")
            np2io.write_yak(parents[-1], parent_table(b"\n".join(haps) + b"\n", 0, 0))
        base = [bam, fa] + yk + ["-t", "2", "-L", "20000"]
        trio_args = ["--trio_pat", parents[0], "--trio_mat", parents[1]]
        walls = {"plain": [], "trio": [], "trio+bed": []}
        cli.main(base + ["-o", td + "/warm.fa"])
        for i in range(a.runs):  # alternating
            for what, extra in (("plain", []), ("trio", ["--trio", td + f"/t{i}.tsv"] + trio_args),
                                ("trio+bed", ["--trio", td + f"/b{i}.tsv", "--trio_bed", td + f"/b{i}"] + trio_args)):
                t0 = time.perf_counter()
                cli.main(base + extra + ["-o", td + f"/o.{what}.{i}.fa"])
                walls[what].append(time.perf_counter() - t0)
        same = open(td + "/o.plain.0.fa", "rb").read() == open(td + "/o.trio.0.fa", "rb").read() == open(td + "/o.trio+bed.0.fa", "rb").read()
        for what, w in walls.items():
            print(f"files -> FASTA, yeast-sized assembly, {what}: wall s {spread(w)}", flush=True)
        print(f"FASTA identical with and without --trio: {same}")
        print(open(td + "/t0.tsv").read().splitlines()[-1], flush=True)


def run_all(a):
    """one child per step, each under its own time limit; the first failure ends the run"""
    out = open(a.out, "a") if a.out else None
    for step in ("asm", "contig", "cli"):
        cmd = [sys.executable, os.path.abspath(__file__), step, "--reps", str(a.reps), "--runs", str(a.runs), "--words", str(a.words)]
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
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["all", "asm", "contig", "cli"])
    ap.add_argument("--mb", type=float, default=None)
    ap.add_argument("--words", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mb is None:
        a.mb = 60.0 if a.what == "contig" else 12.0
    if a.what == "all":
        return run_all(a)
    {"asm": leg_asm, "contig": leg_contig, "cli": leg_cli}[a.what](a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
