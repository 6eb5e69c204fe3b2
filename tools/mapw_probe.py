"""Cost of the mapper's weighted minimizer sampling (winnowmap -W; csrc/np2_map.hip k_map_sketch<.., WEIGHTED>, the bitmap in
np2_map_host.cpp); the figures of profiles/mapw_cost.txt come from here.

    python tools/mapw_probe.py all [--out FILE]  # the inputs once, then one child process per step under its own time limit
    python tools/mapw_probe.py sketch --dir D    # k_map_sketch unweighted and weighted, with and without the coarse level
    python tools/mapw_probe.py stages --dir D    # FASTA -> PAF wall time with and without the weights
    python tools/mapw_probe.py tandem --dir D    # a tandem-array assembly: what the weights change

The input is tools/map_probe.py's E. coli-sized simulated mapping (4.64 Mb, 30 x simulated HiFi: 10 705 reads, 139 Mb).  Every
figure is median, min and max over --runs calls after one warm-up call, the variants alternating in one process on the same
bytes.  k = 15 and w = 19 throughout (the weights need k <= 15).  The unweighted sketch at the default k = 19 beside the parent
commit's is tools/map_probe.py's `sketch` step, run from either tree.
  sketch: sketch_ms of np2_map_bytes (both passes of k_map_sketch and the tile scan, HIP events) against five indexes of the
          same assembly: unweighted; weighted by its --rep list (distinct=0.9998) and by a dense list (every k-mer of the
          assembly, min_count=0: a stress case; min_count=1 is reported for its size), each with the bitmap's coarse level and
          with NP2_MAP_TEST_COARSE=0.  Also each index's build_ms (the weighted ones include zeroing and setting the bitmap),
          its minimizers, and the reads' minimizers, anchors and dropped_occ.
  stages: np2_map_files to a plain PAF, unweighted and --rep weighted index alternating: wall seconds.
  tandem: 200 kb random + 2 400 copies of a 171-base monomer (every 4th with one substitution) + 200 kb random, 2 000 reads of
          3 kb, the list of 15-mers counted more than 10 times: minimizers, anchors, dropped_occ and reads at mapq >= 30.
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
K, W = 15, 19


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


class Coarse:
    """NP2_MAP_TEST_COARSE for the index builds inside (the hook is read once per call)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("NP2_MAP_TEST_COARSE")
        os.environ["NP2_MAP_TEST_COARSE"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["NP2_MAP_TEST_COARSE"]
        else:
            os.environ["NP2_MAP_TEST_COARSE"] = self.old


def leg_sketch(a):
    from nextpolish2_amd import api
    from nextpolish2_amd import io as np2io
    asm = np2io.seqfile_stream(a.dir + "/ecoli.fa")
    stream = np2io.seqfile_stream(a.dir + "/reads.fa")
    lists = {}
    for name, kw in (("rep", dict(distinct=0.9998)), ("min_count=1", dict(min_count=1)), ("dense", dict(min_count=0))):
        idx, _, st = api.rep_bytes(bytes(asm), k=K, **kw)
        lists[name] = idx
        print(f"list {name}: {len(idx)} of {st['distinct']} distinct {K}-mers listed (threshold {st['threshold']}, max count {st['max_count']}), "
              f"count {st['count_ms']:.3f} + select {st['select_ms']:.3f} + emit {st['emit_ms']:.3f} ms", flush=True)
    variants = [("unweighted", None, True), ("rep, coarse", "rep", True), ("rep, no coarse", "rep", False), ("dense, coarse", "dense", True),
                ("dense, no coarse", "dense", False)]
    ixs, build = {}, {v[0]: [] for v in variants}
    for run in range(a.runs + 1):  # the index builds, alternating; the last of each is kept
        for name, lst, coarse in variants:
            if name in ixs:
                ixs.pop(name).close()
            with Coarse(coarse):
                if lst is None:
                    ixs[name] = np2io.MapIndex(asm, k=K, w=W, stream=True)
                else:
                    with np2io.MapWeights(lists[lst], k=K) as wts:
                        ixs[name] = np2io.MapIndex(asm, k=K, w=W, stream=True, weights=wts)
            if run:
                build[name].append(ixs[name].build_ms)
    ms, last = {v[0]: [] for v in variants}, {}
    for run in range(a.runs + 1):
        for name, _, _ in variants:
            np2io.map_reads(ixs[name], stream)
            st = np2io.map_last_stats()
            last[name] = st
            if run:
                ms[name].append(st["sketch_ms"])
    n = len(stream)
    print(f"{n} bytes of reads, k = {K}, w = {W}", flush=True)
    base = statistics.median(ms["unweighted"])
    for name, _, _ in variants:
        st, ix = last[name], ixs[name]
        print(f"  {name}: k_map_sketch (count + scan + emit) ms {spread(ms[name])} = {statistics.median(ms[name]) / base:.3f} x unweighted; "
              f"index build ms {spread(build[name])}; index minimizers {ix.n_minimizers}, listed {ix.weights_listed}; reads: "
              f"{st['minimizers']} minimizers, {st['anchors']} anchors, {st['dropped_occ']} dropped by occurrence, {st['mapped']} mapped", flush=True)
    for ix in ixs.values():
        ix.close()


def leg_stages(a):
    from nextpolish2_amd import io as np2io
    with np2io.MapWeights.from_assembly(a.dir + "/ecoli.fa", k=K) as wts:
        plain = np2io.MapIndex(a.dir + "/ecoli.fa", k=K, w=W)
        weighted = np2io.MapIndex(a.dir + "/ecoli.fa", k=K, w=W, weights=wts)
    walls = {"unweighted": [], "weighted (--rep)": []}
    for run in range(a.runs + 1):
        for name, ix in (("unweighted", plain), ("weighted (--rep)", weighted)):
            t0 = time.perf_counter()
            st = np2io.map_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.paf")
            if run:
                walls[name].append(time.perf_counter() - t0)
    print(f"reads FASTA ({os.path.getsize(a.dir + '/reads.fa')} bytes) -> PAF, {st['reads']} reads, k = {K}, w = {W}, {weighted.weights_listed} listed",
          flush=True)
    for name, xs in walls.items():
        print(f"  {name}: wall s {spread(xs)}", flush=True)
    plain.close(), weighted.close()


def leg_tandem(a):
    import numpy as np
    from nextpolish2_amd import api
    from nextpolish2_amd import io as np2io
    rng = np.random.default_rng(5)
    rand = lambda n: bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])
    unit, copies = rand(171), []
    for i in range(2400):
        u = bytearray(unit)
        if i % 4 == 3:
            at = int(rng.integers(0, 171))
            u[at] = b"ACGT"[(b"ACGT".index(bytes([u[at]])) + 1 + int(rng.integers(0, 3))) % 4]
        copies.append(bytes(u))
    c = rand(200000) + b"".join(copies) + rand(200000)
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    reads, inside = [], []
    for i in range(2000):
        at = int(rng.integers(0, len(c) - 3000))
        s = c[at:at + 3000]
        reads.append(s.translate(rc)[::-1] if i % 2 else s)
        inside.append(200000 <= at and at + 3000 <= 200000 + 2400 * 171)
    inside = np.array(inside)
    idx, _, st = api.rep_bytes(c + b"\n", k=K, min_count=10)
    print(f"tandem assembly of {len(c)} bases, {len(reads)} reads of 3 kb ({int(inside.sum())} inside the array), {len(idx)} {K}-mers counted more "
          f"than 10 times", flush=True)
    for name, lst in (("unweighted", []), ("weighted", idx)):
        with np2io.MapWeights(lst, k=K) as wts, np2io.MapIndex([c], k=K, w=W, stream=True, weights=wts) as ix:
            hits = ix.map(reads)
            st = np2io.map_last_stats()
            print(f"  {name}: index minimizers {ix.n_minimizers}; reads: {st['minimizers']} minimizers, {st['anchors']} anchors, {st['dropped_occ']} "
                  f"dropped by occurrence, {st['mapped']} mapped; inside the array {int(np.count_nonzero(hits['mapq'][inside] >= 30))} of "
                  f"{int(inside.sum())} at mapq >= 30 and {int(np.count_nonzero(hits['mapq'][inside] == 60))} at 60; sketch_ms {st['sketch_ms']:.3f}",
                  flush=True)


def run_all(a):
    import map_probe
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        r = subprocess.run([sys.executable, map_probe.__file__, "inputs", "--dir", td, "--length", str(a.length), "--depth", str(a.depth)],
                           capture_output=True, text=True, timeout=900)
        emit(r.stdout + (r.stderr[-3000:] if r.returncode else ""))
        if r.returncode:
            return r.returncode
        for step in ("sketch", "stages", "tandem"):
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
    p.add_argument("step", choices=["all", "sketch", "stages", "tandem"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; a step: where the inputs are")
    p.add_argument("--length", type=int, default=4641652, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"sketch": leg_sketch, "stages": leg_stages, "tandem": leg_tandem}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
