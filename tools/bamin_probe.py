"""Cost of BAM input (csrc/np2_bamin.hip and the BAM pieces of np2_sam_host.cpp) on the device; the figures of
profiles/bamin_cost.txt come from here.

    python tools/bamin_probe.py all [--out FILE]   # the inputs once, then one child process under its own time limit
    python tools/bamin_probe.py run --dir D

The input is tools/bamout_probe.py's: a synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi, 10 705 records), its
records shuffled and written as SAM text, plain and gzip, lean and with qualities and a minimap2-like tag set.  The BAM of the
same records is written by this project's own writer (np2_sam_write_bam: blocks of 65280 bytes), lean from the lean text and full
from the decorated one; the reader reads no index and does not care that this file is sorted.  In one process, alternating:
  - BAM -> sorted BAM + .bai, SAM text -> the same, SAM gzip -> the same: wall time of np2_sam_open_ex + np2_sam_write_bam;
  - the HIP-event times np2_bamin_stats_t carries (inflate, CRC, walk, fields + scans, pack), GB/s of the inflated stream for
    each, and the walk as a share of the inflate.
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import gzip
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

STEP_LIMIT = 400  # seconds per child


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def leg_run(a):
    from nextpolish2_amd import Polisher, io as np2io
    pol = Polisher([])
    out = a.dir + "/written.bam"

    def to_bam(path, full):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path], keep_names=True, keep_all=full)
        t1 = time.perf_counter()
        sam.write_bam(pol, out)
        t2 = time.perf_counter()
        st = dict(sam.bamin_stats(), read_ms=sam.stats()["read_ms"], open_ms=(t1 - t0) * 1e3, wall_ms=(t2 - t0) * 1e3)
        sam.close()
        return st

    for full, stem in ((False, "ecoli"), (True, "ecoli.full")):
        text, gz, bam = f"{a.dir}/{stem}.sam", f"{a.dir}/{stem}.sam.gz", f"{a.dir}/{stem}.in.bam"
        to_bam(text, full)  # (warm; and the input BAM is what it wrote)
        shutil.copy(out, bam)
        to_bam(bam, full), to_bam(gz, full)
        runs = {"BAM": [], "SAM text": [], "SAM gzip": []}
        for _ in range(a.runs):  # alternating
            runs["BAM"].append(to_bam(bam, full)), runs["SAM text"].append(to_bam(text, full)), runs["SAM gzip"].append(to_bam(gz, full))
        st = runs["BAM"][0]
        print(f"{'full (qualities and tags)' if full else 'lean'}: {st['records']} records; BAM {st['comp_bytes'] / 1e6:.1f} MB in {st['blocks']} blocks "
              f"-> {st['inflated_bytes'] / 1e6:.1f} MB inflated; SAM text {os.path.getsize(text) / 1e6:.1f} MB, gzip {os.path.getsize(gz) / 1e6:.1f} MB", flush=True)
        for what, rs in runs.items():
            print(f"  {what} -> sorted BAM + .bai: wall ms {spread([r['wall_ms'] for r in rs])}; of it np2_sam_open_ex {spread([r['open_ms'] for r in rs])}, "
                  f"waiting for the reader {spread([r['read_ms'] for r in rs])}", flush=True)
        med = {}
        for key, what in (("inflate_ms", "k_bgzf_inflate"), ("crc_ms", "k_bgzf_crc32"), ("walk_ms", "k_bamin_walk"), ("fields_ms", "k_bamin_fields + scans"),
                          ("pack_ms", "k_bamin_pack")):
            xs = [r[key] for r in runs["BAM"]]
            med[key] = statistics.median(xs)
            print(f"  {what}: ms {spread(xs)}; {st['inflated_bytes'] / max(med[key], 1e-9) / 1e6:.2f} GB/s of the inflated stream", flush=True)
        print(f"  k_bamin_walk / k_bgzf_inflate: {med['walk_ms'] / max(med['inflate_ms'], 1e-9):.2f}; "
              f"the five kernels together {sum(med.values()):.3f} ms of np2_sam_open_ex's {statistics.median(r['open_ms'] for r in runs['BAM']):.3f} ms", flush=True)
    pol.close()


def run_all(a):
    import bamout_probe
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
        bamout_probe.decorate_text(td + "/ecoli.sam", td + "/ecoli.full.sam")
        with open(td + "/ecoli.full.sam", "rb") as f, gzip.open(td + "/ecoli.full.sam.gz", "wb", compresslevel=1) as g:  # (level 1: made on the measuring box)
            shutil.copyfileobj(f, g, 1 << 22)
        cmd = [sys.executable, os.path.abspath(__file__), "run", "--dir", td, "--runs", str(a.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nno result within {STEP_LIMIT} s\n", 124
        emit(f"== BAM input beside SAM text, plain and gzip (exit {rc})\n{text.rstrip()}")
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
