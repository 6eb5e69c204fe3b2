"""Cost of the k-mer completeness join (csrc/np2_cmp.hip) on the device; the figures of profiles/cmp_cost.txt come from here.

    python tools/cmp_probe.py join [--mb 12 --reps 5]      # np2_cmp_strings beside np2_qv_strings, same tables, same assembly
    python tools/cmp_probe.py kernels [--mb 12 --k 21]     # the same calls under rocprofv3 --kernel-trace --stats: per kernel
    python tools/cmp_probe.py cli [--runs 5]               # files -> FASTA wall time on the yeast-sized assembly with / without --cmp
    python tools/cmp_probe.py all [--out FILE]             # every step as a child process under its own time limit

join: HIP-event times as the entry points report them (np2_cmp_strings' kernel_ms is k_cmp_join + k_cmp_asm_only; the count
of the set that precedes them is np2_kcount_last_stats').  kernels: one k per trace, so that a kernel's row of the statistics
is one shape; k_cmp_join's rate is given in slots of the reads' table per second (the bytes it streams, 8 per slot) and in
probes per second (its live words, one random 8-byte read of the set's table each and a few more where a chain is longer),
k_qv_scan's in k-mers per second (one probe of the reads' table each)."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import Polisher, io as np2io  # noqa: E402
from nextpolish2_amd.completeness import completeness_text  # noqa: E402
from nextpolish2_amd.synth import Synth  # noqa: E402

STEP_LIMITS = {"join": 200, "kernels": 300, "cli": 200}
MIN_COUNT = 2


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def table_slots(y):
    """slots of a Yak's table in HBM (np2_ctx_create: 1024 sub-tables of the smallest power of two >= 2 * largest bucket + 2,
    at least 16)"""
    mx = int(np.diff(y.bucket_off.astype(np.int64)).max()) if len(y.words) else 0
    cl = 4
    while (1 << cl) < 2 * mx + 2:
        cl += 1
    return 1024 << cl


def synth_contigs(mb, pieces, seed=5):
    s = Synth(int(mb * 1e6), depth=1, seed=seed, diploid=True)
    asm = s.pileup.ref.tobytes()
    cuts = [0] + sorted(int(x) for x in np.random.default_rng(seed).integers(1, len(asm), size=pieces - 1)) + [len(asm)]
    return s, [asm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def leg_join(a):
    s, contigs = synth_contigs(a.mb, 17)
    ks = [a.k] if a.k else [21, 31]
    yaks = [s.yak(k) for k in ks]
    pol = Polisher(yaks)
    figures = {}
    for t, k in enumerate(ks):
        pol.cmp_strings(t, contigs, MIN_COUNT)  # (warm: the counter's buffers, code objects)
        pol.qv_strings(t, contigs, MIN_COUNT)
        join_ms, count_ms, qv_ms = [], [], []
        for _ in range(a.reps):  # alternating
            r = pol.cmp_strings(t, contigs, MIN_COUNT)
            join_ms.append(r.kernel_ms)
            count_ms.append(np2io.kcount_last_stats()["kernel_ms"])
            q = pol.qv_strings(t, contigs, MIN_COUNT)
            qv_ms.append(q.kernel_ms)
        rs = pol.cmp_strings(t, contigs, MIN_COUNT, spectra=True)
        slots = table_slots(yaks[t])
        figures[k] = {"read_slots": slots, "read_words": len(yaks[t].words), "n_read": r.n_read, "n_asm": r.n_asm, "qv_kmers": q.n_kmers,
                      "calls": a.reps + 2}
        print(f"{a.mb:g} Mb assembly in 17 contigs, k={k}, min_count {MIN_COUNT}: reads' table {len(yaks[t].words) / 1e6:.1f} M words in "
              f"{slots / 1e6:.0f} M slots ({slots * 8 / 1e6:.0f} MB); n_read {r.n_read}, n_found {r.n_found}, completeness "
              f"{completeness_text(r.n_found, r.n_read)}, n_asm {r.n_asm}, n_asm_only {r.n_asm_only}; spectrum rows "
              f"{[int(x) for x in rs.spectra.sum(axis=1)]}\n"
              f"  k_cmp_join + k_cmp_asm_only ms: {spread(join_ms)}; with the spectrum copied back {rs.kernel_ms:.3f}\n"
              f"  the count of the set before them (k_kcount and growths) ms: {spread(count_ms)}\n"
              f"  k_qv_scan on the same sequences and table ms: {spread(qv_ms)} = G k-mers/s "
              f"{spread([q.n_kmers / m / 1e6 for m in qv_ms])}", flush=True)
    pol.close()
    print("FIGURES " + json.dumps(figures), flush=True)


def leg_kernels(a):
    """leg_join for one k as a child under rocprofv3 --kernel-trace --stats (kernel tracing alone, no counters)"""
    for k in ([a.k] if a.k else [21, 31]):
        with tempfile.TemporaryDirectory(dir=a.dir) as td:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "kt", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "join", "--mb", str(a.mb), "--reps", str(a.reps), "--k", str(k)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMITS["kernels"] - 30)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-3000:])
                return r.returncode
            fig = [json.loads(ln[len("FIGURES "):]) for ln in r.stdout.splitlines() if ln.startswith("FIGURES ")][0][str(k)]
            rows = {}
            for row in csv.DictReader(open(os.path.join(td, "kt_kernel_stats.csv"))):
                for name in ("k_cmp_join", "k_cmp_asm_only", "k_qv_scan", "k_kcount"):
                    if f"np2::{name}(" in row["Name"] or row["Name"].startswith(name + "(") or f"{len(name)}{name}E" in row["Name"]:
                        rows[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
        print(f"{a.mb:g} Mb assembly, k={k}, kernel trace (average over the calls of the run; a traced run's host side is slower, its "
              f"kernels are not):", flush=True)
        if "k_cmp_join" in rows:
            n, us = rows["k_cmp_join"]
            print(f"  k_cmp_join      {n} calls, {us:9.1f} us: {fig['read_slots'] / us / 1e3:.2f} G slots/s ({fig['read_slots'] * 8 / us / 1e6:.3f} TB/s "
                  f"streamed), {fig['n_read'] / us / 1e3:.2f} G probes/s", flush=True)
        if "k_cmp_asm_only" in rows:
            n, us = rows["k_cmp_asm_only"]
            print(f"  k_cmp_asm_only  {n} calls, {us:9.1f} us: {fig['n_asm'] / us / 1e3:.2f} G probes/s", flush=True)
        if "k_qv_scan" in rows:
            n, us = rows["k_qv_scan"]
            print(f"  k_qv_scan       {n} calls, {us:9.1f} us: {fig['qv_kmers'] / us / 1e3:.2f} G k-mers/s", flush=True)
        if "k_kcount" in rows:
            n, us = rows["k_kcount"]
            print(f"  k_kcount        {n} calls, {us:9.1f} us a piece (the set counted before every join)", flush=True)
    return 0


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
        legs = (("plain", lambda i: []), ("cmp", lambda i: ["--cmp", td + f"/c{i}.tsv"]),
                ("cmp+spectra", lambda i: ["--cmp", td + f"/s{i}.tsv", "--cmp_spectra", td + f"/s{i}"]))
        walls = {what: [] for what, _ in legs}
        cli.main(base + ["-o", td + "/warm.fa"])
        for i in range(a.runs):  # alternating
            for what, extra in legs:
                t0 = time.perf_counter()
                cli.main(base + extra(i) + ["-o", td + f"/o.{what}.{i}.fa"])
                walls[what].append(time.perf_counter() - t0)
        same = open(td + "/o.plain.0.fa", "rb").read() == open(td + "/o.cmp.0.fa", "rb").read() == open(td + "/o.cmp+spectra.0.fa", "rb").read()
        for what, w in walls.items():
            print(f"files -> FASTA, yeast-sized assembly, {what}: wall s {spread(w)}", flush=True)
        print(f"FASTA identical with and without --cmp: {same}")
        print(open(td + "/c0.tsv").read(), flush=True)


def run_all(a):
    """one child per step, each under its own time limit; the first failure ends the run"""
    out = open(a.out, "a") if a.out else None
    for step in ("join", "kernels", "cli"):
        cmd = [sys.executable, os.path.abspath(__file__), step, "--reps", str(a.reps), "--runs", str(a.runs), "--mb", str(a.mb)]
        if a.dir:
            cmd += ["--dir", a.dir]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMITS[step])
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {step}: no result within {STEP_LIMITS[step]} s\n", 124
        text = f"== {step} (exit {rc})\n" + "".join(ln + "\n" for ln in text.splitlines() if not ln.startswith("FIGURES "))
        print(text, flush=True)
        if out:
            out.write(text)
            out.flush()
        if rc != 0:
            return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "join", "kernels", "cli"])
    p.add_argument("--mb", type=float, default=12.0, help="Mb of the synthetic diploid assembly [12]")
    p.add_argument("--k", type=int, default=0, help="join, kernels: this k alone [21 and 31]")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="where temporary files go [the system's temporary directory]")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"join": leg_join, "kernels": leg_kernels, "cli": leg_cli}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
