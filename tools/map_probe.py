"""Cost of the mapper (csrc/np2_map.hip, np2_map_host.cpp) on the device; the figures of profiles/map_cost.txt come from here.

    python tools/map_probe.py all [--out FILE]     # the inputs once, then one child process per step under its own time limit
    python tools/map_probe.py stages --dir D       # files -> PAF: wall time, the stages' HIP-event times, read_ms
    python tools/map_probe.py sketch --dir D       # k_map_sketch beside k_kcount on the same bytes

The input is the synthetic E. coli-sized mapping the SAM probes use (4.64 Mb, 30 x simulated HiFi, tools/sam_probe.py): the
contig as FASTA and its reads, put back on the strand they were read from, as FASTA.  Every figure is median, min and max over
--runs calls after one warm-up call.
  stages: np2_map_index_files once (build_ms), then np2_map_files to a plain PAF: wall seconds beside the stats' sketch_ms,
          seed_ms, sort_ms, chain_ms (HIP events, summed over batches), read_ms (the device thread's wait for its readers) and
          write_ms; anchors/s of the chain kernel is anchors / chain_ms.
  sketch: the reads' separator stream through np2_map_bytes (sketch_ms: both passes of k_map_sketch and the tile scan) and
          through np2_kcount_bytes at the same k (kernel_ms of k_kcount), alternating: both roll and hash every k-mer of the
          same bytes, the sketch twice (count and emit) and with a window test after it.
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

ECOLI = 4641652
STEP_LIMIT = 300  # seconds per child
K = 19


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def make_inputs(td, length, depth):
    from nextpolish2_amd.bamio import read_bam, write_bam_raw
    from nextpolish2_amd.synth import Synth
    t0 = time.time()
    s = Synth(length, depth=depth, seed=31, name="ecoli")
    bam = td + "/ecoli.bam"
    write_bam_raw(bam, [(s.pileup.name, s.pileup.L)], [s.bam_records(0)])
    _, recs = read_bam(bam)
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    with open(td + "/ecoli.fa", "wb") as f:
        f.write(b">ecoli\n" + s.pileup.ref.tobytes() + b"\n")
    n_bytes = 0
    with open(td + "/reads.fa", "wb") as f:
        for i, r in enumerate(recs):
            seq = r["seq"].encode()
            if r["flag"] & 16:
                seq = seq.translate(rc)[::-1]
            n_bytes += len(seq)
            f.write(b">r%d\n%s\n" % (i, seq))
    print(f"input: {s.pileup.L} positions, {len(recs)} reads, {n_bytes} bases; made in {time.time() - t0:.1f} s", flush=True)


def leg_stages(a):
    from nextpolish2_amd import io as np2io
    t0 = time.perf_counter()
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    print(f"index: {ix.n_minimizers} minimizers of {sum(ix.lens)} bases, kernels and sort {ix.build_ms:.3f} ms, wall {time.perf_counter() - t0:.3f} s "
          f"(the first device call of the process included)", flush=True)
    walls, ms, st = [], {}, None
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        st = np2io.map_files(ix, [a.dir + "/reads.fa"], a.dir + "/map.paf")
        if run:
            walls.append(time.perf_counter() - t0)
            for f in ("sketch_ms", "seed_ms", "sort_ms", "chain_ms", "read_ms", "write_ms"):
                ms.setdefault(f, []).append(st[f])
    ix.close()
    size = os.path.getsize(a.dir + "/reads.fa")
    print(f"reads FASTA ({size} bytes) -> PAF ({os.path.getsize(a.dir + '/map.paf')} bytes): {st['reads']} reads, {st['mapped']} mapped, "
          f"{st['minimizers']} minimizers, {st['anchors']} anchors, {st['dropped_occ']} dropped by occurrence, {st['pieces']} pieces, "
          f"{st['groups']} groups", flush=True)
    print(f"  wall s {spread(walls)}", flush=True)
    for f, xs in ms.items():
        print(f"  {f} {spread(xs)}", flush=True)
    print(f"  chain kernel M anchors/s {spread([st['anchors'] / x / 1e3 for x in ms['chain_ms']])}", flush=True)


def leg_sketch(a):
    from nextpolish2_amd import io as np2io
    stream = np2io.seqfile_stream(a.dir + "/reads.fa")
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    sk, kc = [], []
    for run in range(a.runs + 1):
        np2io.map_reads(ix, stream)
        st = np2io.map_last_stats()
        np2io.count_kmers(stream, [K])
        ks = np2io.kcount_last_stats()
        if run:
            sk.append(st["sketch_ms"])
            kc.append(ks["kernel_ms"])
    ix.close()
    n = len(stream)
    print(f"{n} bytes of reads, k = {K}, w = {ix.w}: {st['minimizers']} minimizers, {ks['kmers']} k-mers", flush=True)
    print(f"  k_map_sketch (count + scan + emit) ms {spread(sk)} = G bases/s {spread([n / x / 1e6 for x in sk])}", flush=True)
    print(f"  k_kcount ms {spread(kc)} = G bases/s {spread([n / x / 1e6 for x in kc])}", flush=True)


def run_all(a):
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "inputs", "--dir", td, "--length", str(a.length), "--depth", str(a.depth)],
                           capture_output=True, text=True, timeout=900)
        emit(r.stdout + (r.stderr[-3000:] if r.returncode else ""))
        if r.returncode:
            return r.returncode
        for step in ("stages", "sketch"):
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
    p.add_argument("step", choices=["all", "inputs", "stages", "sketch"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; a step: where the inputs are")
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    if a.step == "inputs":
        return make_inputs(a.dir, a.length, a.depth) or 0
    return {"stages": leg_stages, "sketch": leg_sketch}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
