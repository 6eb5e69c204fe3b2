"""Cost of the BAM writer (csrc/np2_bamout.hip, np2_bamout_host.cpp) on the device; the figures of profiles/bamout_cost.txt come
from here.

    python tools/bamout_probe.py all [--out FILE]   # the inputs once, then one child process under its own time limit
    python tools/bamout_probe.py run --dir D

The input is tools/sam_probe.py's: a synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi), its records shuffled and
written as SAM text, plain and gzip.  In one process, alternating:
  - SAM text -> BAM + .bai (np2_sam_open_ex with the names kept + np2_sam_write_bam), wall time, from plain text and from gzip,
    and of it np2_sam_write_bam alone; beside SAM text -> resident pileup (np2_sam_open + np2_contig_from_sam) on the same input;
  - the HIP-event times np2_bamout_stats_t carries: k_bam_sizes with its scan, k_bam_emit, the deflate kernel, the index kernels,
    the bytes/s of the two over the stream, and the ratio of k_bam_emit to the deflate kernel on the same bytes;
  - np2_contig_from_bam on the written file, on the fetch path NP2_INFLATE names or the default.
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
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
sys.path.insert(0, HERE)

STEP_LIMIT = 300  # seconds per child


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def leg_run(a):
    from nextpolish2_amd import Polisher, io as np2io
    ref = open(a.dir + "/ecoli.ref", "rb").read()
    pol = Polisher([])
    out = a.dir + "/written.bam"

    def to_bam(path):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path], keep_names=True)
        t1 = time.perf_counter()
        st = sam.write_bam(pol, out)
        t2 = time.perf_counter()
        sam.close()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3, st

    def to_pileup(path):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path])
        c = np2io.contig_from_sam(pol, sam, sam.refs()[0][0], ref)
        ms = (time.perf_counter() - t0) * 1e3
        c.free()
        sam.close()
        return ms

    to_bam(a.dir + "/ecoli.sam"), to_pileup(a.dir + "/ecoli.sam")  # (warm: staging blocks, code objects, the writer's batches)
    walls = {k: [] for k in ("SAM text -> BAM + .bai", "  of it np2_sam_write_bam", "SAM gzip -> BAM + .bai", "  of it np2_sam_write_bam (gzip)",
                             "SAM text -> resident pileup", "SAM gzip -> resident pileup", "np2_contig_from_bam on the written file")}
    stats = []
    for _ in range(a.runs):  # alternating
        w, b, st = to_bam(a.dir + "/ecoli.sam")
        walls["SAM text -> BAM + .bai"].append(w), walls["  of it np2_sam_write_bam"].append(b), stats.append(st)
        w, b, st = to_bam(a.dir + "/ecoli.sam.gz")
        walls["SAM gzip -> BAM + .bai"].append(w), walls["  of it np2_sam_write_bam (gzip)"].append(b), stats.append(st)
        walls["SAM text -> resident pileup"].append(to_pileup(a.dir + "/ecoli.sam"))
        walls["SAM gzip -> resident pileup"].append(to_pileup(a.dir + "/ecoli.sam.gz"))
        bam = np2io.Bam(out)
        t0 = time.perf_counter()
        c = np2io.contig_from_bam(pol, bam, bam.refs()[0][0], ref)
        walls["np2_contig_from_bam on the written file"].append((time.perf_counter() - t0) * 1e3)
        c.free()
        bam.close()
    st = stats[0]
    print(f"{st['records']} records, stream {st['stream_bytes'] / 1e6:.1f} MB in {st['blocks']} blocks -> file {st['file_bytes'] / 1e6:.1f} MB; "
          f".bai {os.path.getsize(out + '.bai')} bytes, {st['bins']} bins, {st['chunks']} chunks", flush=True)
    for what, w in walls.items():
        print(f"  {what}: wall ms {spread(w)}", flush=True)
    for key, what in (("sizes_ms", "k_bam_sizes + scan"), ("emit_ms", "k_bam_emit"), ("deflate_ms", "k_bgzf_deflate"), ("index_ms", "index kernels, scans and sort")):
        xs = [s[key] for s in stats]
        rate = f"; {st['stream_bytes'] / statistics.median(xs) / 1e6:.1f} GB/s of the stream" if key in ("emit_ms", "deflate_ms") and statistics.median(xs) > 0 else ""
        print(f"  {what}: ms {spread(xs)}{rate}", flush=True)
    ratios = [s["emit_ms"] / s["deflate_ms"] for s in stats if s["deflate_ms"] > 0]
    print(f"  k_bam_emit / k_bgzf_deflate on the same bytes: {spread(ratios)}", flush=True)
    pol.close()


def run_all(a):
    import sam_probe
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
            sam_probe.make_inputs(td, a.length, a.depth)
        emit(buf.getvalue().rstrip())
        cmd = [sys.executable, os.path.abspath(__file__), "run", "--dir", td, "--runs", str(a.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nno result within {STEP_LIMIT} s\n", 124
        emit(f"== BAM writer (exit {rc})\n{text.rstrip()}")
        return rc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "run"])
    p.add_argument("--length", type=int, default=4641652, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the inputs are written [the system's temporary directory]; run: where they are")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    leg_run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
