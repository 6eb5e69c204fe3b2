"""Cost of the variant caller (csrc/np2_varcall.hip) on the device; the figures of profiles/varcall_cost.txt come from here.

    python tools/varcall_probe.py all [--out FILE]    # the BAM once, then one child process per fetch path under its own time limit
    python tools/varcall_probe.py path --bam F --ref F --inflate gpu|libdeflate

The input is the synthetic E. coli-sized contig of tools/depth_probe.py (4.64 Mb, 30 x simulated HiFi, written by
bamio.write_bam_raw).  Per fetch path (NP2_INFLATE=gpu: records found on the device; libdeflate: the host pool), in one
process and alternating:
  - np2_varcall_from_bam: wall time, the kernels and sorts together (kernel_ms) and apart (stage_ms: records, coverage scan,
    key sorts, alleles, calls counted, calls written; HIP events);
  - np2_depth_from_bam on the same BAM: wall time and its four kernels (kernel_ms);
  - np2_contig_from_bam on the same BAM: wall time, and of it records -> pileup (the line NP2_IO_PROFILE prints);
  - the module, BAM -> VCF, wall time (python -m nextpolish2_amd.varcall in this process: argument parsing to the closed file).
The fetch is shared by the three entry points, so the comparison shows what the caller costs on top of it and beside the
columnariser, which reads every SEQ nibble once as the record kernel does.  `all` stops at the first step that fails or runs
out of time: nothing more is started on the device after that."""
import argparse
import contextlib
import io
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from depth_probe import ECOLI, make_inputs, spread  # noqa: E402

STEP_LIMIT = 300  # seconds per child


@contextlib.contextmanager
def stderr_to(path):
    """the process's standard error (the library writes there) into a file"""
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "wb") as f:
        os.dup2(f.fileno(), 2)
    try:
        yield
    finally:
        sys.stderr.flush()
        os.dup2(saved, 2)
        os.close(saved)


def leg_path(a):
    from nextpolish2_amd import Polisher, api, io as np2io, varcall
    ref = open(a.ref, "rb").read()
    L = len(ref)
    pol = Polisher([])
    bam = np2io.Bam(a.bam)
    name = bam.refs()[0][0]
    td = os.path.dirname(a.bam)
    fa = os.path.join(td, "ecoli.fa")
    with open(fa, "wb") as f:
        f.write(b">" + name.encode() + b"\n" + ref + b"\n")
    calls, st, _, _ = api.varcall_from_bam(pol, bam, name, ref)  # (warm: staging blocks, code objects, the look-back state)
    np2io.depth_from_bam(pol, bam, name, L)
    np2io.contig_from_bam(pol, bam, name, ref).free()
    walls = {"np2_varcall_from_bam": [], "np2_depth_from_bam": [], "np2_contig_from_bam": [], "module, BAM -> VCF": []}
    kernel, depth_kernel, pileup = [], [], []
    stages = {k: [] for k in api.VARCALL_STAGES}
    prof = os.path.join(td, "profile.txt")
    for i in range(a.runs):  # alternating
        t0 = time.perf_counter()
        _, s1, _, _ = api.varcall_from_bam(pol, bam, name, ref)
        walls["np2_varcall_from_bam"].append((time.perf_counter() - t0) * 1e3)
        kernel.append(s1["kernel_ms"])
        for k, v in s1["stage_ms"].items():
            stages[k].append(v)
        t0 = time.perf_counter()
        _, s2, _ = np2io.depth_from_bam(pol, bam, name, L)
        walls["np2_depth_from_bam"].append((time.perf_counter() - t0) * 1e3)
        depth_kernel.append(s2["kernel_ms"])
        os.environ["NP2_IO_PROFILE"] = "1"
        with stderr_to(prof):
            t0 = time.perf_counter()
            c = np2io.contig_from_bam(pol, bam, name, ref)
            walls["np2_contig_from_bam"].append((time.perf_counter() - t0) * 1e3)
        del os.environ["NP2_IO_PROFILE"]
        c.free()
        m = re.search(r"records->pileup ([0-9.]+) ms", open(prof).read())
        if m:
            pileup.append(float(m.group(1)))
        vcf = os.path.join(td, "calls.%s.%d.vcf" % (a.inflate, i))
        with stderr_to(os.devnull):
            t0 = time.perf_counter()
            varcall.main([a.bam, fa, "-o", vcf])
            walls["module, BAM -> VCF"].append((time.perf_counter() - t0) * 1e3)
    print(f"fetch path {a.inflate}: {st['records_seen']} records, {st['records_counted']} counted, {st['events']} indel events in {st['alleles']} alleles, "
          f"{st['callable']} of {L} positions callable, {len(calls)} calls at the rule's defaults "
          f"({', '.join('%s %d' % (k, st[k]) for k in api.VARCALL_CALLS)})", flush=True)
    for what, w in walls.items():
        print(f"  {what}: wall ms {spread(w)}", flush=True)
    print(f"  the caller's kernels and sorts together (kernel_ms): ms {spread(kernel)}", flush=True)
    for k in api.VARCALL_STAGES:
        print(f"    {k}: ms {spread(stages[k])}", flush=True)
    print(f"  beside them, the four depth kernels (kernel_ms): ms {spread(depth_kernel)}", flush=True)
    if pileup:
        print(f"  and np2_contig_from_bam's records -> pileup: ms {spread(pileup)}; the caller's kernels are "
              f"{statistics.median(kernel) / statistics.median(pileup):.2f} x that", flush=True)
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
    p.add_argument("--runs", type=int, default=5)
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
