"""Cost of the aligner (csrc/np2_align.hip, the align stages of np2_map_host.cpp) on the device; the figures of
profiles/align_cost.txt come from here.

    python tools/align_probe.py all [--out FILE]     # the inputs once, then one child process per step under its own time limit
    python tools/align_probe.py stages --dir D       # files -> SAM beside files -> PAF: wall time, the stages' HIP-event times
    python tools/align_probe.py bundle               # the committed bundle: map -a, polish, distance to the bundle's own polish

The input of `stages` is tools/map_probe.py's: the synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi).  Every figure
is median, min and max over --runs calls after one warm-up call.
  stages: np2_map_align_files to a plain SAM: wall seconds beside np2_map_files' on the same reads, the mapper's stage times,
          pins_ms, classify_ms, dp_ms, assemble_ms (HIP events, summed over groups) and write_ms; cores/s and cells/s are over
          dp_ms; the SAM's share of wall time is write_ms / wall.
  bundle: tests/golden's assembly and the 574 reads of its BAM through np2_map_align_files and the polisher (cli); the polished
          contig is then aligned to the bundle's expected.fa.gz by np2_map_align_host as one read, and NM plus the clipped bases
          is the number of bases by which the two differ.
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from map_probe import ECOLI, STEP_LIMIT, make_inputs, spread  # noqa: E402

ALIGN_MS = ("pins_ms", "classify_ms", "dp_ms", "assemble_ms", "write_ms")
MAP_MS = ("sketch_ms", "seed_ms", "sort_ms", "chain_ms", "read_ms")


def leg_stages(a):
    from nextpolish2_amd import io as np2io
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    print(f"index: {ix.n_minimizers} minimizers of {sum(ix.lens)} bases, kernels and sort {ix.build_ms:.3f} ms", flush=True)
    walls, paf_walls, ms, st, ast = [], [], {}, None, None
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        np2io.map_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.paf")
        t1 = time.perf_counter()
        st = np2io.map_align_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.sam")
        t2 = time.perf_counter()
        ast = np2io.align_last_stats()
        if run:
            paf_walls.append(t1 - t0), walls.append(t2 - t1)
            for f in MAP_MS:
                ms.setdefault(f, []).append(st[f])
            for f in ALIGN_MS:
                ms.setdefault(f, []).append(ast[f])
    ix.close()
    print(f"reads FASTA ({os.path.getsize(a.dir + '/reads.fa')} bytes) -> SAM ({os.path.getsize(a.dir + '/map.sam')} bytes): {st['reads']} reads, "
          f"{st['mapped']} mapped, {st['anchors']} anchors, {st['pieces']} pieces, {st['groups']} groups", flush=True)
    print("  " + ", ".join(f"{f} {ast[f]}" for f in ("pins", "segments", "equal", "pure_gap", "snv", "cores", "cells", "clipped_bases", "overflow")),
          flush=True)
    print(f"  wall s, files -> SAM {spread(walls)}", flush=True)
    print(f"  wall s, files -> PAF {spread(paf_walls)}", flush=True)
    for f, xs in ms.items():
        print(f"  {f} {spread(xs)}", flush=True)
    print(f"  M cores/s over dp_ms {spread([ast['cores'] / x / 1e3 for x in ms['dp_ms']])}", flush=True)
    print(f"  G cells/s over dp_ms {spread([ast['cells'] / x / 1e6 for x in ms['dp_ms']])}", flush=True)
    print(f"  SAM formatting and writing, share of wall {spread([w / 1e3 / t for w, t in zip(ms['write_ms'], walls)])}", flush=True)


def leg_bundle(a):
    from nextpolish2_amd import io as np2io
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_model as mm
    golden = os.path.join(ROOT, "tests", "golden")
    asm, bundle = os.path.join(golden, "ref_test_asm.fa.gz"), os.path.join(golden, "ref_bundle")
    _, _, reads, names, _ = mm.bundle_reads(os.path.join(bundle, "hifi.map.sort.bam"))
    with tempfile.TemporaryDirectory() as td:
        with open(td + "/hifi.fa", "wb") as f:
            for n, r in zip(names, reads):
                f.write(b">" + n.encode() + b"\n" + r + b"\n")
        with np2io.MapIndex(asm) as ix:
            st = np2io.map_align_files(ix, [td + "/hifi.fa"], td + "/map.sam")
            ast = np2io.align_last_stats()
        print(f"bundle: {st['reads']} reads, {st['mapped']} mapped; " + ", ".join(f"{f} {ast[f]}" for f in ("pins", "segments", "equal", "pure_gap",
              "snv", "cores", "cells", "clipped_bases", "overflow")), flush=True)
        cmd = [sys.executable, "-m", "nextpolish2_amd.cli", "-L", "10000", td + "/map.sam", asm, bundle + "/k21.yak", bundle + "/k31.yak", "-o",
               td + "/out.fa", "--qv", td + "/qv.tsv"]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=STEP_LIMIT)
        if r.returncode:
            print(r.stderr[-3000:])
            return r.returncode
        print(open(td + "/qv.tsv").read(), flush=True)
        got = "".join(ln.strip() for ln in open(td + "/out.fa") if not ln.startswith(">")).encode()
        with gzip.open(bundle + "/expected.fa.gz", "rt") as f:
            want = "".join(ln.strip() for ln in f if not ln.startswith(">")).encode()
        with gzip.open(asm, "rt") as f:
            before = "".join(ln.strip() for ln in f if not ln.startswith(">")).encode()
        for label, seq in (("the input assembly", before), ("polished from map -a", got)):
            hits, recs, cigar, off = np2io.map_align_host([want], [seq.upper()])
            clip = sum(int(w) >> 4 for w in cigar if int(w) & 15 == 4)
            print(f"{label}: {len(seq)} bases against the bundle's expected {len(want)}: NM {int(recs[0]['nm'])} + {clip} clipped", flush=True)
    return 0


def run_all(a):
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        r = subprocess.run([sys.executable, os.path.join(HERE, "map_probe.py"), "inputs", "--dir", td, "--length", str(a.length), "--depth", str(a.depth)],
                           capture_output=True, text=True, timeout=900)
        emit(r.stdout + (r.stderr[-3000:] if r.returncode else ""))
        if r.returncode:
            return r.returncode
        for step in ("stages", "bundle"):
            cmd = [sys.executable, os.path.abspath(__file__), step, "--dir", td, "--runs", str(a.runs)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
                text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
            except subprocess.TimeoutExpired as e:
                got = e.stdout or ""
                text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {step}: no result within {STEP_LIMIT} s\n", 124
            emit(f"== {step} (exit {rc})\n{text}")
            if rc != 0:
                return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "stages", "bundle"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; stages: where the inputs are")
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"stages": leg_stages, "bundle": leg_bundle}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
