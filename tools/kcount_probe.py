"""Cost of the k-mer counter (csrc/np2_kcount.hip) on the device; the figures of profiles/kcount_cost.txt come from here.

    python tools/kcount_probe.py fixture                # the 66 196 test reads: 8.6 M k-mers, a measurement of OVERHEADS
    python tools/kcount_probe.py sim [--mb 12.1 --cov 60 --files 16 --dir DIR]
                                                        # simulated 150-base reads of a yeast-sized synthetic assembly

Per k (21, 31): the count kernel alone (HIP events around every launch, summed: np2_kcount_last_stats) in k-mers/s, and
beside it, in the same process, the dump loader's k_yak_insert (NP2_IO_PROFILE's "insert" line: one CAS per word, no
increment) on the table of the counted words, in words/s.  `sim` adds files -> dumps wall time for plain and gzip input
with the reader / kernel split, and the time zlib alone needs to decode the same files on the same number of threads."""
import argparse
import gzip
import os
import re
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import io as np2io  # noqa: E402

FIXTURE = [os.path.join(ROOT, "tests", "golden", "ref_bundle", f"sr.seq.{i}.gz") for i in range(3)]


def yak_insert_ms(dump):
    """k_yak_insert on this dump (a fresh process with NP2_IO_PROFILE: launch to completion, the flag's read-back included)"""
    code = f"from nextpolish2_amd import io\nio.polisher_from_yak_files([{dump!r}])\n"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PYTHONPATH=ROOT, NP2_IO_PROFILE="1"))
    m = re.search(r"insert ([0-9.]+) ms", r.stderr)
    return float(m.group(1)) if m else float("nan")


def count_leg(label, paths, td, reps=3, min_count=1, insert=True):
    for k in (21, 31):
        out = os.path.join(td, f"{label}.k{k}.yak")
        rows = []
        for _ in range(reps):
            t0 = time.perf_counter()
            np2io.count_kmers_to_files(paths, [k], [out], min_count=min_count)
            wall = time.perf_counter() - t0
            st = np2io.kcount_last_stats()
            rows.append((wall, st))
        for wall, st in rows:
            print(f"{label} k={k}: {st['kmers']} k-mers, {st['distinct']} distinct, growths {st['growths']}, spilled {st['spilled']}: "
                  f"count kernel {st['kernel_ms']:.2f} ms = {st['kmers'] / st['kernel_ms'] / 1e6:.2f} G k-mers/s; "
                  f"files -> dump wall {wall:.3f} s (waiting for readers {st['read_ms']:.0f} ms)", flush=True)
        if not insert:  # (under a profiler: this process starts no other)
            continue
        n_words = (os.path.getsize(out) - 16 - 8 * 1024) // 8
        ms = [yak_insert_ms(out) for _ in range(reps)]
        best = min(r[1]["kernel_ms"] for r in rows)
        kmers = rows[0][1]["kmers"]
        print(f"{label} k={k}: k_yak_insert of the {n_words} counted words: {', '.join(f'{m:.2f}' for m in ms)} ms = "
              f"{n_words / min(ms) / 1e6:.2f} G words/s;  count kernel per k-mer {1e6 * best / kmers:.3f} ns, "
              f"k_yak_insert per word {1e6 * min(ms) / n_words:.3f} ns, ratio {(best / kmers) / (min(ms) / n_words):.2f}", flush=True)


def simulate(mb, cov, n_files, d):
    rng = np.random.default_rng(1)
    L = int(mb * 1e6)
    genome = rng.integers(0, 4, size=L, dtype=np.uint8)
    n_reads = int(L * cov / 150)
    comp = np.array([3, 2, 1, 0], np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    plain, gz = [], []
    t0 = time.perf_counter()
    for f in range(n_files):
        n = n_reads // n_files
        st = rng.integers(0, L - 150, size=n)
        r = genome[st[:, None] + np.arange(150)[None, :]]
        rc = rng.random(n) < 0.5
        r[rc] = comp[r[rc][:, ::-1]]
        err = rng.random(r.shape) < 0.005
        r[err] = rng.integers(0, 4, size=int(err.sum()), dtype=np.uint8)
        txt = np.empty((n, 151), np.uint8)
        txt[:, :150] = letters[r]
        txt[:, 150] = 10
        p = os.path.join(d, f"sim.{f}.seq")
        txt.tofile(p)
        plain.append(p)
    procs = [subprocess.Popen(["gzip", "-1", "-k", "-f", p]) for p in plain]
    for pr in procs:
        assert pr.wait() == 0
    gz = [p + ".gz" for p in plain]
    print(f"simulated {n_reads // n_files * n_files} reads of 150 bases ({mb} Mb x {cov}) in {n_files} files, plain "
          f"{sum(map(os.path.getsize, plain)) / 1e6:.0f} MB, gzip -1 {sum(map(os.path.getsize, gz)) / 1e6:.0f} MB ({time.perf_counter() - t0:.0f} s)", flush=True)
    return plain, gz


def zlib_alone(paths):
    def dec(p):
        n = 0
        with gzip.open(p, "rb") as f:
            while True:
                b = f.read(1 << 22)
                if not b:
                    return n
                n += len(b)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(16, len(paths))) as ex:
        n = sum(ex.map(dec, paths))
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fixture", "sim"])
    ap.add_argument("--mb", type=float, default=12.1)
    ap.add_argument("--cov", type=float, default=60.0)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-insert", action="store_true", help="leave the k_yak_insert leg (child processes) out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        if a.what == "fixture":
            count_leg("fixture (overheads)", FIXTURE, td, a.reps, insert=not a.no_insert)
            return
        plain, gz = simulate(a.mb, a.cov, a.files, td)
        count_leg("sim plain", plain, td, a.reps, insert=not a.no_insert)
        for label, paths in (("plain", plain), ("gzip", gz)):
            outs = [os.path.join(td, f"w.k{k}.yak") for k in (21, 31)]
            t0 = time.perf_counter()
            np2io.count_kmers_to_files(paths, [21, 31], outs, min_count=2)
            wall = time.perf_counter() - t0
            st = np2io.kcount_last_stats()
            print(f"sim {label}: files -> two dumps (k = 21, 31; min_count 2) wall {wall:.2f} s: count kernels {st['kernel_ms'] / 1e3:.2f} s, "
                  f"waiting for readers {st['read_ms'] / 1e3:.2f} s, rest (upload, growth, emit, write) "
                  f"{wall - st['kernel_ms'] / 1e3 - st['read_ms'] / 1e3:.2f} s; growths {st['growths']}, passes {st['passes']}", flush=True)
        n, t = zlib_alone(gz)
        print(f"zlib alone: {n / 1e6:.0f} MB decoded from the gzip files on {min(16, len(gz))} threads in {t:.2f} s", flush=True)


if __name__ == "__main__":
    main()
