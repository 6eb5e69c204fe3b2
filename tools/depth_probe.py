"""Cost of the mapping-depth report (csrc/np2_depth.hip) on the device; the figures of profiles/depth_cost.txt come from here.

    python tools/depth_probe.py all [--out FILE]    # the BAM once, then one child process per fetch path under its own time limit
    python tools/depth_probe.py path --bam F --ref F --inflate gpu|libdeflate

The input is a synthetic E. coli-sized contig (4.64 Mb, 30 x simulated HiFi) written by bamio.write_bam_raw.  Per fetch path
(NP2_INFLATE=gpu: records found on the device; libdeflate: the host pool), in one process and alternating:
  - np2_depth_from_bam, wall time, and of it the depth kernels (k_depth_events, k_depth_scan, k_depth_runs, k_depth_keep:
    kernel_ms, HIP events);
  - the same with the per-base array brought back;
  - np2_contig_from_bam on the same BAM, wall time.
The fetch is shared, so the comparison shows what depth costs on top of it and beside the columnariser.  `all` stops at
the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

ECOLI = 4641652
STEP_LIMIT = 300  # seconds per child


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def make_inputs(td, length, depth):
    from nextpolish2_amd.bamio import write_bam_raw
    from nextpolish2_amd.synth import Synth
    t0 = time.time()
    s = Synth(length, depth=depth, seed=31, name="ecoli")
    bam, ref = td + "/ecoli.bam", td + "/ecoli.ref"
    write_bam_raw(bam, [(s.pileup.name, s.pileup.L)], [s.bam_records(0)])
    with open(ref, "wb") as f:
        f.write(s.pileup.ref.tobytes())
    print(f"input: {s.pileup.L} positions, {s.pileup.n_reads - 1} records, BAM of {os.path.getsize(bam) / 1e6:.1f} MB made in {time.time() - t0:.1f} s", flush=True)
    return bam, ref


def leg_path(a):
    from nextpolish2_amd import Polisher, io as np2io
    ref = open(a.ref, "rb").read()
    L = len(ref)
    pol = Polisher([])
    bam = np2io.Bam(a.bam)
    name = bam.refs()[0][0]
    runs, st, _ = np2io.depth_from_bam(pol, bam, name, L)  # (warm: staging blocks, code objects, the look-back state)
    np2io.contig_from_bam(pol, bam, name, ref).free()
    walls = {"np2_depth_from_bam": [], "np2_depth_from_bam, per-base array back": [], "np2_contig_from_bam": []}
    kernel = []
    for _ in range(a.runs):  # alternating
        t0 = time.perf_counter()
        _, s1, _ = np2io.depth_from_bam(pol, bam, name, L)
        walls["np2_depth_from_bam"].append((time.perf_counter() - t0) * 1e3)
        kernel.append(s1["kernel_ms"])
        t0 = time.perf_counter()
        np2io.depth_from_bam(pol, bam, name, L, want_depth=True)
        walls["np2_depth_from_bam, per-base array back"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        c = np2io.contig_from_bam(pol, bam, name, ref)
        walls["np2_contig_from_bam"].append((time.perf_counter() - t0) * 1e3)
        c.free()
    print(f"fetch path {a.inflate}: {st['records_seen']} records, {st['records_counted']} counted, mean depth {st['sum_depth'] / L:.2f}, max {st['max_depth']}, "
          f"{st['runs']} runs at -d 3, {st['runs_kept']} kept, {st['bases_kept']} of {L} positions", flush=True)
    for what, w in walls.items():
        print(f"  {what}: wall ms {spread(w)}", flush=True)
    print(f"  of which the depth kernels (kernel_ms): ms {spread(kernel)}; {L * 12 / statistics.median(kernel) / 1e6:.1f} GB/s over the 12 bytes per position "
          f"the scan and the run extraction move", flush=True)
    bam.close()
    pol.close()


def run_all(a):
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        import contextlib
        import io
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            bam, ref = make_inputs(td, a.length, a.depth)
        emit(buf.getvalue().rstrip())
        for mode in ("gpu", "libdeflate"):
            cmd = [sys.executable, os.path.abspath(__file__), "path", "--bam", bam, "--ref", ref, "--inflate", mode, "--runs", str(a.runs)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT, env=dict(os.environ, NP2_INFLATE=mode))
                text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
            except subprocess.TimeoutExpired as e:
                got = e.stdout or ""
                text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {mode}: no result within {STEP_LIMIT} s\n", 124
            emit(f"== {mode} (exit {rc})\n{text.rstrip()}")
            if rc != 0:
                return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "path"])
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--bam", default=None)
    p.add_argument("--ref", default=None)
    p.add_argument("--inflate", default="gpu", choices=["gpu", "libdeflate"], help="path: the value NP2_INFLATE is expected to hold (all sets it)")
    p.add_argument("--dir", default=None, help="where the inputs are written [the system's temporary directory]")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    if os.environ.get("NP2_INFLATE") != a.inflate:
        p.error("path: set NP2_INFLATE to the value of --inflate")
    leg_path(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
