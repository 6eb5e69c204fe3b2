"""Cost of the mapper's further chains (csrc/np2_map.hip k_map_chain_more; np2_io.h, "More chains"), and the default path beside
another tree's; the figures of profiles/mapmulti_cost.txt come from here.

    python tools/mapmulti_probe.py all [--other TREE] [--out FILE]  # the inputs once, then one child process per step
    python tools/mapmulti_probe.py default --dir D [--tree TREE]    # without the new options: chain_ms, assemble_ms, wall times
    python tools/mapmulti_probe.py cost --dir D                     # more_ms beside chain_ms on the same anchors
    python tools/mapmulti_probe.py tandem --dir D                   # the same on a tandem-array assembly, -W weighted
    python tools/mapmulti_probe.py segdup --dir D                   # the same on a four-copy segmental duplication
    python tools/mapmulti_probe.py align --dir D                    # the aligner's stages with units on that assembly

The input is tools/map_probe.py's E. coli-sized simulated mapping (4.64 Mb, 30 x simulated HiFi: 10 705 reads, 139 Mb).  Every
figure is median, min and max over --runs calls after one warm-up call.
  default: np2_map_files to a plain PAF and np2_map_align_files to a plain SAM at the default options: chain_ms, assemble_ms and
           wall seconds.  It uses nothing this change adds, so `--tree TREE` runs it on another checkout's built package (the
           parent commit's); `all --other TREE` alternates child processes of the two trees, three of each, on one box.
  cost:    np2_map_bytes_m on the reads in memory: single chain, --supp --secondary 5 (max_chains 10) and --supp --secondary 15
           (max_chains 16), the latter also with --pri_ratio 0 (every secondary kept), alternating: chain_ms (k_map_chain and
           the hits' copy), more_ms (k_map_chain_more, the scan of the unit counts, the packing and the units' copy), their
           ratio, the units and the counts.  The re-sweep is the wave-wide form (64-anchor blocks, pointer jumping through
           LDS); the one-lane form exists only as the host twin.
  tandem:  tools/mapw_probe.py's tandem-array assembly (2 400 copies of a 171-base monomer between two 200 kb flanks, 2 000
           reads of 3 kb), the index weighted by the 15-mers counted more than 10 times and unweighted: the same variants.
  segdup:  a 50 kb segment four times in 0.95 Mb, each copy with substitutions at 0.5 % of its bases, 2 000 reads of 10 kb: a
           fifth of the reads lie in a copy and have three further chains of about a thousand anchors each.
  align:   the same assembly through the aligner, np2_map_align_bytes beside np2_map_align_bytes_m: the units and the aligner's
           pins_ms, classify_ms, dp_ms and assemble_ms.
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

STEP_LIMIT = 300  # seconds per child
VARIANTS = (("single chain", None), ("--supp --secondary 5 (max_chains 10)", dict(max_chains=10, supplementary=1, secondary_n=5)),
            ("--supp --secondary 15 (max_chains 16)", dict(max_chains=16, supplementary=1, secondary_n=15)),
            ("--supp --secondary 15 --pri_ratio 0 (max_chains 16)", dict(max_chains=16, supplementary=1, secondary_n=15, pri_pm=0)))


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def leg_default(a):
    from nextpolish2_amd import io as np2io
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    fig = {}
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        st = np2io.map_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.paf")
        paf = time.perf_counter() - t0
        t0 = time.perf_counter()
        np2io.map_align_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.sam")
        sam = time.perf_counter() - t0
        ast = np2io.align_last_stats()
        if run:
            for key, v in (("chain_ms", st["chain_ms"]), ("FASTA -> PAF wall s", paf), ("assemble_ms", ast["assemble_ms"]), ("dp_ms", ast["dp_ms"]),
                           ("FASTA -> SAM wall s", sam)):
                fig.setdefault(key, []).append(v)
    ix.close()
    print(f"tree {os.path.dirname(os.path.dirname(np2io.__file__))}: {st['reads']} reads, {st['anchors']} anchors", flush=True)
    for key, xs in fig.items():
        print(f"  {key}: {spread(xs)}; values {' '.join('%.3f' % x for x in xs)}", flush=True)


def variants_on(ix, reads, runs):
    from nextpolish2_amd import io as np2io
    chain, more, last = {}, {}, {}
    for run in range(runs + 1):
        for name, multi in VARIANTS:
            if multi is None:
                np2io.map_reads(ix, reads)
                mst = dict(more_ms=0.0)
            else:
                np2io.map_reads(ix, reads, multi=multi)
                mst = np2io.map_last_multi_stats()
            st = np2io.map_last_stats()
            last[name] = (st, mst)
            if run:
                chain.setdefault(name, []).append(st["chain_ms"]), more.setdefault(name, []).append(mst["more_ms"])
    for name, _ in VARIANTS:
        st, mst = last[name]
        line = f"  {name}: chain_ms {spread(chain[name])}; more_ms {spread(more[name])} = {statistics.median(more[name]) / statistics.median(chain[name]):.3f} x chain_ms"
        if len(mst) > 1:
            line += (f"; {mst['units']} units of {st['reads']} reads: {mst['selections']} further selections, {mst['dropped_min_cnt']} dropped by min_cnt, "
                     f"{mst['dropped_secondary']} secondaries not kept, {mst['kept_supplementary']} supplementary, {mst['kept_secondary']} secondary")
        print(line + f"; {st['anchors']} anchors, {st['groups']} groups", flush=True)


def leg_cost(a):
    from nextpolish2_amd import io as np2io
    stream = np2io.seqfile_stream(a.dir + "/reads.fa")
    with np2io.MapIndex(a.dir + "/ecoli.fa") as ix:
        print(f"E. coli-sized simulated mapping, {len(stream)} bytes of reads, k = {ix.k}, w = {ix.w}", flush=True)
        variants_on(ix, stream, a.runs)


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
    reads = []
    for i in range(2000):
        at = int(rng.integers(0, len(c) - 3000))
        s = c[at:at + 3000]
        reads.append(s.translate(rc)[::-1] if i % 2 else s)
    idx, _, _ = api.rep_bytes(c + b"\n", k=15, min_count=10)
    print(f"tandem assembly of {len(c)} bases, {len(reads)} reads of 3 kb, {len(idx)} 15-mers counted more than 10 times, k = 15, w = 19", flush=True)
    for name, lst in (("weighted (-W)", idx), ("unweighted", [])):
        print(f" {name}:", flush=True)
        with np2io.MapWeights(lst, k=15) as wts, np2io.MapIndex([c], k=15, w=19, stream=True, weights=wts) as ix:
            variants_on(ix, reads, a.runs)


def segdup_inputs():
    import numpy as np
    rng = np.random.default_rng(9)
    rand = lambda n: bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])
    seg = rand(50000)
    parts = [rand(150000)]
    for _ in range(4):  # four copies, each with its own substitutions at one base in 200
        u = bytearray(seg)
        for at in rng.integers(0, len(u), len(u) // 200):
            u[at] = b"ACGT"[(b"ACGT".index(bytes([u[at]])) + 1 + int(rng.integers(0, 3))) % 4]
        parts += [bytes(u), rand(150000)]
    c = b"".join(parts)
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for i in range(2000):
        at = int(rng.integers(0, len(c) - 10000))
        s = c[at:at + 10000]
        reads.append(s.translate(rc)[::-1] if i % 2 else s)
    print(f"segmental-duplication assembly of {len(c)} bases (a 50 kb segment four times, each copy 0.5 % from it), {len(reads)} reads of 10 kb, k = 19, w = 19",
          flush=True)
    return c, reads


def leg_segdup(a):
    from nextpolish2_amd import io as np2io
    c, reads = segdup_inputs()
    with np2io.MapIndex([c], stream=True) as ix:
        variants_on(ix, reads, a.runs)


def leg_align(a):
    """the aligner with units beside the single-chain run, on the segmental duplication: np2_map_align_bytes(_m)"""
    from nextpolish2_amd import io as np2io
    c, reads = segdup_inputs()
    fig, last = {}, {}
    with np2io.MapIndex([c], stream=True) as ix:
        for run in range(a.runs + 1):
            for name, multi in VARIANTS[:2] + VARIANTS[3:]:
                if multi is None:
                    ix.align(reads)
                    units = len(reads)
                else:
                    units = len(np2io.map_align_reads_m(ix, reads, multi)["recs"])
                ast = np2io.align_last_stats()
                last[name] = (units, ast)
                if run:
                    for f in ("pins_ms", "classify_ms", "dp_ms", "assemble_ms"):
                        fig.setdefault((name, f), []).append(ast[f])
    for name, _ in VARIANTS[:2] + VARIANTS[3:]:
        units, ast = last[name]
        print(f"  {name}: {units} units, {ast['cells']} cells, {ast['overflow']} overflowed; " +
              "; ".join(f"{f} {spread(fig[(name, f)])}" for f in ("pins_ms", "classify_ms", "dp_ms", "assemble_ms")), flush=True)


def run_all(a):
    sys.path.insert(0, HERE)
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
        me = os.path.abspath(__file__)
        steps = []
        for _ in range(3 if a.other else 1):
            if a.other:
                steps.append(("default (the other tree)", [me, "default", "--dir", td, "--runs", "2", "--tree", a.other]))
            steps.append(("default", [me, "default", "--dir", td, "--runs", "2" if a.other else str(a.runs)]))
        steps += [(step, [me, step, "--dir", td, "--runs", str(a.runs)]) for step in ("cost", "tandem", "segdup", "align")]
        for step, cmd in steps:
            try:
                r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
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
    p.add_argument("step", choices=["all", "default", "cost", "tandem", "segdup", "align"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; a step: where the inputs are")
    p.add_argument("--tree", default=ROOT, help="default: the checkout whose built package is measured [this one]")
    p.add_argument("--other", default=None, help="all: a second checkout (the parent commit's, built) whose `default` step alternates with this one's")
    p.add_argument("--length", type=int, default=4641652, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.step == "all":
        return run_all(a)
    return {"default": leg_default, "cost": leg_cost, "tandem": leg_tandem, "segdup": leg_segdup, "align": leg_align}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
