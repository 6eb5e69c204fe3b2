"""Cost of the repetitive k-mer list (csrc/np2_rep.hip) on the device; the figures of profiles/rep_cost.txt come from here.

    python tools/rep_probe.py count [--reps 7]         # k_rep_count beside k_kcount on the same bytes, with / without the run collapse
    python tools/rep_probe.py select [--reps 7]        # selection and compaction times against the table size (k = 8 .. 16)
    python tools/rep_probe.py files [--runs 5]         # gzip FASTA -> list wall time
    python tools/rep_probe.py all [--out FILE]         # every step as a child process under its own time limit

Inputs: the contigs of bench.py's default workload (the yeast-sized synthetic assembly, 12 Mb) and one long low-complexity
contig (homopolymers, di- and trinucleotide satellites, a 171-base repeat unit with 2 % divergence, 24 Mb).  Times are HIP
events as the entry points report them (np2_rep_stats_t, np2_kcount_last_stats): count_ms is the sum over the pieces'
launches, select_ms the pass (or two) over the counters, emit_ms sizes + scan + scatter.  Every figure is given as median,
min and max over --reps calls after one warm-up call; the two count variants and k_kcount alternate."""
import argparse
import gzip
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import api, io as np2io  # noqa: E402

STEP_LIMITS = {"count": 240, "select": 240, "files": 180}
K = 15


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def assembly_stream():
    """the default workload's contigs as one separator stream"""
    from bench import YEAST, make_assembly
    syn = make_assembly(list(YEAST), 1, 1, True)
    return b"\n".join(s.pileup.ref.tobytes() for s in syn) + b"\n"


def low_complexity_stream(mb=24.0, seed=7):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    unit = letters[rng.integers(0, 4, 171)]
    parts, n = [], 0
    while n < mb * 1e6:
        kind = int(rng.integers(0, 4))
        length = int(rng.integers(2000, 200000))
        if kind == 0:
            p = np.full(length, letters[rng.integers(0, 4)], np.uint8)
        elif kind == 1:
            p = np.tile(letters[rng.integers(0, 4, int(rng.integers(2, 4)))], length // 2)[:length]
        elif kind == 2:
            p = np.tile(unit, length // 171 + 1)[:length].copy()
            err = rng.random(length) < 0.02
            p[err] = letters[rng.integers(0, 4, int(err.sum()))]
        else:
            p = letters[rng.integers(0, 4, length // 8)]
        parts.append(p)
        n += len(p)
    return np.concatenate(parts).tobytes() + b"\n"


def leg_count(a):
    for label, stream in (("12 Mb synthetic assembly", assembly_stream()), ("24 Mb low-complexity contig", low_complexity_stream())):
        variants = (("k_rep_count, run collapse", None), ("k_rep_count, one add per k-mer", "1"))
        ms = {v[0]: [] for v in variants}
        ms["k_kcount"] = []
        kmers = {}
        for rep in range(a.reps + 1):  # (the first round warms up: code objects, the pinned pool)
            for what, env in variants:
                if env is None:
                    os.environ.pop("NP2_REP_NO_COLLAPSE", None)
                else:
                    os.environ["NP2_REP_NO_COLLAPSE"] = env
                _, _, st = api.rep_bytes(stream, k=K)
                kmers[what] = st["kmers"]
                if rep:
                    ms[what].append(st["count_ms"])
            os.environ.pop("NP2_REP_NO_COLLAPSE", None)
            np2io.count_kmers(stream, [K])
            ks = np2io.kcount_last_stats()
            kmers["k_kcount"] = ks["kmers"]
            if rep:
                ms["k_kcount"].append(ks["kernel_ms"])
        print(f"{label}, {len(stream)} bytes, k = {K}: distinct {st['distinct']}, threshold {st['threshold']}, listed {st['listed']}, "
              f"max count {st['max_count']}", flush=True)
        for what, xs in ms.items():
            print(f"  {what}: {kmers[what]} k-mers, kernel ms {spread(xs)} = G k-mers/s {spread([kmers[what] / x / 1e6 for x in xs])}",
                  flush=True)


def leg_select(a):
    stream = assembly_stream()
    for k in (8, 12, 13, 14, 15, 16):
        sel, emit, st = [], [], None
        for rep in range(a.reps + 1):
            _, _, st = api.rep_bytes(stream, k=k)
            if rep:
                sel.append(st["select_ms"])
                emit.append(st["emit_ms"])
        table = 4 ** k * 4
        print(f"k = {k}: table {table / 2 ** 20:.0f} MiB, distinct {st['distinct']}, threshold {st['threshold']}, listed {st['listed']}\n"
              f"  selection ms {spread(sel)} = table GB/s {spread([table / x / 1e6 for x in sel])}\n"
              f"  compaction (sizes, scan, scatter) ms {spread(emit)}", flush=True)


def leg_files(a):
    stream = assembly_stream()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        fa = os.path.join(td, "asm.fa.gz")
        with gzip.open(fa, "wb", compresslevel=6) as f:
            for i, contig in enumerate(stream.split(b"\n")[:-1]):
                f.write(b">ctg%d\n" % i)
                f.write(b"\n".join(contig[j:j + 80] for j in range(0, len(contig), 80)) + b"\n")
        walls, st = [], None
        for run in range(a.runs + 1):
            t0 = time.perf_counter()
            st = api.rep_files([fa], os.path.join(td, "rep.txt"), k=K)
            if run:
                walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        with gzip.open(fa, "rb") as f:
            while f.read(1 << 20):
                pass
        unzip = time.perf_counter() - t0
        print(f"gzip FASTA of the 12 Mb assembly ({os.path.getsize(fa)} bytes) -> list, k = {K}: wall s {spread(walls)}; of the last "
              f"call count {st['count_ms']:.3f} ms, selection {st['select_ms']:.3f} ms, compaction {st['emit_ms']:.3f} ms in kernels; "
              f"Python's gzip alone reads the file in {unzip:.3f} s; listed {st['listed']} k-mers above {st['threshold']}", flush=True)


def run_all(a):
    """one child per step, each under its own time limit; the first failure ends the run"""
    out = open(a.out, "a") if a.out else None
    for step in ("count", "select", "files"):
        cmd = [sys.executable, os.path.abspath(__file__), step, "--reps", str(a.reps), "--runs", str(a.runs)]
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
    p.add_argument("step", choices=["all", "count", "select", "files"])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="where temporary files go [the system's temporary directory]")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"count": leg_count, "select": leg_select, "files": leg_files}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
