"""Cost of the SAM reader (csrc/np2_sam.hip, np2_sam_host.cpp) on the device; the figures of profiles/sam_cost.txt come from here.

    python tools/sam_probe.py all [--out FILE]    # the inputs once, then one child process per BAM fetch path under its own time limit
    python tools/sam_probe.py path --dir D --inflate gpu|libdeflate

The input is a synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi): bamio.write_bam_raw writes the sorted BAM and
its .bai, and the same records, shuffled, are written as SAM text, plain and gzip.  Per fetch path of the BAM
(NP2_INFLATE=gpu: records found on the device; libdeflate: the host pool), in one process and alternating:
  - files -> resident pileup through np2_sam_open + np2_contig_from_sam, wall time, from plain text and from gzip, and of
    it np2_sam_open alone; the HIP-event times of k_sam_lines, k_sam_fields (with the three scans) and k_sam_pack with
    their bytes/s over the text, of the sort with k_sam_gather, and read_ms, the time the device waited for the reader
    (NP2_SAM_PROFILE's line and np2_sam_stats);
  - np2_contig_from_bam on the same records, wall time.
The comparator is the BAM path, which had its sort and its index done for it: `samtools sort` and `samtools index` are not
timed here, no samtools being at hand.  `all` stops at the first step that fails or runs out of time: nothing more is started
on the device after that."""
import argparse
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

ECOLI = 4641652
STEP_LIMIT = 300  # seconds per child
PROFILE = re.compile(r"np2_sam: (\d+) bytes of alignment lines: k_sam_lines ([\d.]+) ms, k_sam_fields \+ scans ([\d.]+) ms, k_sam_pack ([\d.]+) ms, "
                     r"sort \+ k_sam_gather ([\d.]+) ms, waited for the reader ([\d.]+) ms")


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def make_inputs(td, length, depth):
    import numpy as np
    from nextpolish2_amd.bamio import read_bam, write_bam_raw, write_sam
    from nextpolish2_amd.synth import Synth
    t0 = time.time()
    s = Synth(length, depth=depth, seed=31, name="ecoli")
    bam = td + "/ecoli.bam"
    write_bam_raw(bam, [(s.pileup.name, s.pileup.L)], [s.bam_records(0)])
    with open(td + "/ecoli.ref", "wb") as f:
        f.write(s.pileup.ref.tobytes())
    refs, recs = read_bam(bam)
    shuffled = [recs[k] for k in np.random.default_rng(1).permutation(len(recs))]
    write_sam(td + "/ecoli.sam", refs, shuffled)
    write_sam(td + "/ecoli.sam.gz", refs, shuffled, gz=True)
    print(f"input: {s.pileup.L} positions, {len(recs)} records; BAM {os.path.getsize(bam) / 1e6:.1f} MB, SAM text {os.path.getsize(td + '/ecoli.sam') / 1e6:.1f} MB, "
          f"gzip {os.path.getsize(td + '/ecoli.sam.gz') / 1e6:.1f} MB; made in {time.time() - t0:.1f} s", flush=True)


def leg_path(a):
    import contextlib
    from nextpolish2_amd import Polisher, io as np2io
    ref = open(a.dir + "/ecoli.ref", "rb").read()
    pol = Polisher([])
    bam = np2io.Bam(a.dir + "/ecoli.bam")
    name = bam.refs()[0][0]

    def from_sam(path):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path])
        t1 = time.perf_counter()
        c = np2io.contig_from_sam(pol, sam, name, ref)
        t2 = time.perf_counter()
        st = sam.stats()
        c.free()
        sam.close()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, st

    np2io.contig_from_bam(pol, bam, name, ref).free()  # (warm: staging blocks, code objects, the look-back state)
    from_sam(a.dir + "/ecoli.sam")
    walls = {"SAM text -> resident pileup": [], "  of it np2_sam_open": [], "SAM gzip -> resident pileup": [], "  of it np2_sam_open (gzip)": [],
             "np2_contig_from_bam": []}
    stats = {"plain": [], "gzip": []}
    for _ in range(a.runs):  # alternating
        w, o, st = from_sam(a.dir + "/ecoli.sam")
        walls["SAM text -> resident pileup"].append(w), walls["  of it np2_sam_open"].append(o), stats["plain"].append(st)
        w, o, st = from_sam(a.dir + "/ecoli.sam.gz")
        walls["SAM gzip -> resident pileup"].append(w), walls["  of it np2_sam_open (gzip)"].append(o), stats["gzip"].append(st)
        t0 = time.perf_counter()
        c = np2io.contig_from_bam(pol, bam, name, ref)
        walls["np2_contig_from_bam"].append((time.perf_counter() - t0) * 1e3)
        c.free()
    st = stats["plain"][0]
    print(f"BAM fetch path {a.inflate}: {st['lines']} lines, {st['kept']} records kept, {st['cigar_words']} CIGAR words, {st['seq_bytes']} packed SEQ bytes", flush=True)
    for what, w in walls.items():
        print(f"  {what}: wall ms {spread(w)}", flush=True)
    text_bytes = os.path.getsize(a.dir + "/ecoli.sam")
    for kind in ("plain", "gzip"):
        for key in ("parse_ms", "pack_ms", "sort_ms", "read_ms"):
            xs = [s_[key] for s_ in stats[kind]]
            rate = f"; {text_bytes / statistics.median(xs) / 1e6:.1f} GB/s of text" if key in ("parse_ms", "pack_ms") and statistics.median(xs) > 0 else ""
            print(f"  {kind} {key}: {spread(xs)}{rate}", flush=True)
    bam.close()
    pol.close()
    with contextlib.suppress(Exception):
        sys.stderr.flush()


def report_profile(stderr_text, emit):
    """NP2_SAM_PROFILE's lines of a child: the three kernels apart"""
    rows = [tuple(float(x) for x in m.groups()) for m in PROFILE.finditer(stderr_text)]
    if not rows:
        return
    n = rows[0][0]
    for i, what in ((1, "k_sam_lines"), (2, "k_sam_fields + scans"), (3, "k_sam_pack"), (4, "sort + k_sam_gather")):
        xs = [r[i] for r in rows]
        rate = f"; {n / statistics.median(xs) / 1e6:.1f} GB/s over the {n / 1e6:.1f} MB of alignment lines" if i < 4 else ""  # (the sort moves no text)
        emit(f"  {what}: ms {spread(xs)}{rate}")


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
            make_inputs(td, a.length, a.depth)
        emit(buf.getvalue().rstrip())
        for mode in ("gpu", "libdeflate"):
            cmd = [sys.executable, os.path.abspath(__file__), "path", "--dir", td, "--inflate", mode, "--runs", str(a.runs)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT, env=dict(os.environ, NP2_INFLATE=mode, NP2_SAM_PROFILE="1"))
                text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
            except subprocess.TimeoutExpired as e:
                got = e.stdout or ""
                text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {mode}: no result within {STEP_LIMIT} s\n", 124
            emit(f"== {mode} (exit {rc})\n{text.rstrip()}")
            if rc != 0:
                return rc
            report_profile(r.stderr, emit)
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "path"])
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--inflate", default="gpu", choices=["gpu", "libdeflate"], help="path: the value NP2_INFLATE is expected to hold (all sets it)")
    p.add_argument("--dir", default=None, help="all: where the inputs are written [the system's temporary directory]; path: where they are")
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
