"""Cost of the aligner's opt-in outputs (csrc/np2_aligntags.hip: k_align_tags_size, scans, k_align_tags_emit; the quality bytes on
the host side of np2_map_host.cpp); the figures of profiles/aligntags_cost.txt come from here.

    python tools/aligntags_probe.py all [--out FILE] [--parent TREE]  # the inputs once, then one child process per step
    python tools/aligntags_probe.py flags --dir D                      # FASTQ -> SAM without a flag and with each flag
    python tools/aligntags_probe.py noflag --dir D [--tree TREE]       # FASTA -> SAM without a flag: wall time and assemble_ms

The input is tools/map_probe.py's synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi), its reads written once more as
FASTQ with seeded qualities.  Every figure is median, min and max over --runs calls after one warm-up call.
  flags:  np2_map_align_files[_x] to a plain SAM, the flag sets alternating inside every run of one process: wall seconds,
          assemble_ms (k_align_ops_count, scan, k_align_ops_emit and their copies), tags_ms (the tag kernels, their three scans
          and the copies of their outputs), write_ms, the SAM's bytes and the tag stats' counts.
  noflag: the call every earlier release has, from --tree (another built checkout of the project, its own library under its own
          Python layer) or from this one: `all --parent TREE` runs the two alternating, one child process each, three times.
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from map_probe import ECOLI, STEP_LIMIT, spread  # noqa: E402

SETS = (("none", {}), ("qual", dict(qual=True)), ("md", dict(md=True)), ("cs", dict(cs=True)), ("eqx", dict(eqx=True)),
        ("qual md", dict(qual=True, md=True)), ("all", dict(qual=True, md=True, cs=True, eqx=True)))


def make_fastq(td, seed=41):
    rng = np.random.default_rng(seed)
    n = 0
    with open(td + "/reads.fa", "rb") as f, open(td + "/reads.fastq", "wb") as out:
        for head in f:
            seq = f.readline().rstrip(b"\n")
            out.write(b"@" + head[1:] + seq + b"\n+\n" + rng.integers(33, 127, len(seq), dtype=np.uint8).tobytes() + b"\n")
            n += 1
    print(f"reads.fastq: {n} reads, {os.path.getsize(td + '/reads.fastq')} bytes", flush=True)


def leg_flags(a):
    from nextpolish2_amd import io as np2io
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    res = {label: dict(wall=[], assemble_ms=[], tags_ms=[], write_ms=[], read_ms=[]) for label, _ in SETS}
    last = {}
    for run in range(a.runs + 1):
        for label, kw in SETS:
            t0 = time.perf_counter()
            st = np2io.map_align_files(ix, [a.dir + "/reads.fastq"], a.dir + "/map.sam", **kw)
            wall = time.perf_counter() - t0
            ast, tst = np2io.align_last_stats(), np2io.align_last_tag_stats()
            last[label] = (st, tst, os.path.getsize(a.dir + "/map.sam"))
            if run:
                r = res[label]
                r["wall"].append(wall), r["assemble_ms"].append(ast["assemble_ms"]), r["tags_ms"].append(tst["tags_ms"])
                r["write_ms"].append(ast["write_ms"]), r["read_ms"].append(st["read_ms"])
    ix.close()
    for label, _ in SETS:
        st, tst, size = last[label]
        print(f"[{label}] {st['reads']} reads, {st['mapped']} mapped, {st['groups']} groups, SAM {size} bytes; md_bytes {tst['md_bytes']}, "
              f"cs_bytes {tst['cs_bytes']}, eqx_words {tst['eqx_words']}, qual_reads {tst['qual_reads']}", flush=True)
        for f, xs in res[label].items():
            print(f"  {f} {spread(xs)}", flush=True)


def leg_noflag(a):
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    from nextpolish2_amd import api
    from nextpolish2_amd import io as np2io
    print(f"library: {api.LIB_PATH}", flush=True)
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    walls, asm_ms = [], []
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        np2io.map_align_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.sam")
        wall = time.perf_counter() - t0
        if run:
            walls.append(wall), asm_ms.append(np2io.align_last_stats()["assemble_ms"])
    ix.close()
    print(f"  wall s {spread(walls)}\n  assemble_ms {spread(asm_ms)}", flush=True)


def run_all(a):
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    def child(label, cmd):
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {label}: no result within {STEP_LIMIT} s\n", 124
        emit(f"== {label} (exit {rc})\n{text}")
        return rc

    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        r = subprocess.run([sys.executable, os.path.join(HERE, "map_probe.py"), "inputs", "--dir", td, "--length", str(a.length), "--depth", str(a.depth)],
                           capture_output=True, text=True, timeout=900)
        emit(r.stdout + (r.stderr[-3000:] if r.returncode else ""))
        if r.returncode:
            return r.returncode
        make_fastq(td)
        me = [sys.executable, os.path.abspath(__file__)]
        rc = child("flags", me + ["flags", "--dir", td, "--runs", str(a.runs)])
        if rc:
            return rc
        if a.parent:
            for k in range(3):
                for label, tree in (("parent", ["--tree", os.path.abspath(a.parent)]), ("head", [])):
                    rc = child(f"noflag {label} {k + 1}", me + ["noflag", "--dir", td, "--runs", str(a.runs)] + tree)
                    if rc:
                        return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "flags", "noflag"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; the steps: where the inputs are")
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    p.add_argument("--parent", default=None, help="all: another built checkout to run `noflag` from, alternating with this one")
    p.add_argument("--tree", default=None, help="noflag: the checkout whose package and library are used [this one]")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"flags": leg_flags, "noflag": leg_noflag}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
