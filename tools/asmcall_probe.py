"""Cost of the assembly-to-reference caller (csrc/np2_asmcall.hip) on the device; the figures of profiles/asmcall_cost.txt come
from here.

    python tools/asmcall_probe.py [--length 4641652] [--runs 5] [--out FILE]

The input is a seeded random E. coli-sized contig (the truth) and an edited copy of it (an SNV, a deletion of 1..3 or an
insertion of 1..3 bases about every 2 kb), cut into the module's default segments (10 kb, 2 kb overlap).  In one process and
alternating, after one warm round:
  - MapIndex.align over the segments: wall time and the mapper's and aligner's own stage times (chain_ms, dp_ms, assemble_ms;
    HIP events);
  - np2_asmcall over the resulting alignments: wall time, the kernels and the sort together (kernel_ms) and apart (stage_ms:
    walk counted, coverage scan, cov == 1 counts, event offsets, walk written, runs, filter, sort, gather; HIP events);
  - np2_varcall_from_records over the same alignments packed as BAM records (np2_align_pack_host, outside the timing): its
    record kernel k_vc_records (stage_ms["records"]) walks the same CIGAR words and bases once, as k_ac_walk does twice;
  - the module without its files (asmcall.call: tiling, index, align, call, text): wall time.
Nothing more is started on the device after a step that fails."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

ECOLI = 4641652


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def make_pair(length, every=2000, seed=31):
    """-> (truth, edited copy, number of edits)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    truth = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].tobytes()
    out, prev, n = [], 0, 0
    for x in range(every, length - every, every):
        kind, k = n % 3, 1 + n % 3
        if kind == 0:
            out += [truth[prev:x], b"ACGT"[(b"ACGT".index(truth[x]) + 1) % 4:][:1]]
            prev = x + 1
        elif kind == 1:
            out.append(truth[prev:x])
            prev = x + k
        else:
            out += [truth[prev:x], b"GATTACA"[:k]]
            prev = x
        n += 1
    out.append(truth[prev:])
    return truth, b"".join(out), n


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--length", type=int, default=ECOLI, help="bases of the synthetic contig [4641652]")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--out", default=None, help="append the output to this file")
    a = p.parse_args()
    from nextpolish2_amd import Polisher, api, asmcall, io as np2io
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    t0 = time.perf_counter()
    truth, edited, n_edits = make_pair(a.length)
    refs, contigs = [("truth", truth)], [("asm", edited)]
    tiles = asmcall.tile(len(edited), 10000, 2000)
    segs = [edited[s:e] for s, e, _, _ in tiles]
    emit(f"truth {len(truth)} bases, edited copy {len(edited)} bases with {n_edits} planted edits, {len(segs)} segments ({time.perf_counter() - t0:.1f} s to make)")
    pol = Polisher([])
    walls = {"MapIndex.align": [], "np2_asmcall": [], "np2_varcall_from_records": [], "module (asmcall.call)": []}
    chain, dp, assemble, kernel, vc_records = [], [], [], [], []
    stages = {k: [] for k in api.ASMCALL_STAGES}
    st = None
    with np2io.MapIndex([truth], stream=True, names=["truth"]) as index:
        for i in range(a.runs + 1):  # (round 0 warms: code objects, staging blocks, the look-back state)
            t0 = time.perf_counter()
            _, recs, cigar, cigar_off = index.align(segs)
            w_align = (time.perf_counter() - t0) * 1e3
            ms, als = np2io.map_last_stats(), np2io.align_last_stats()
            if i == 0:
                alns = asmcall.segment_alns(tiles, [0] * len(tiles), recs, cigar_off, __import__("numpy").cumsum([0] + [len(s) for s in segs[:-1]]))
                query = b"".join(segs)
                b_recs, _, b_cigar, b_seq4 = np2io.align_pack_host(recs, cigar, cigar_off, segs)
            t0 = time.perf_counter()
            runs, vars_, st, _ = api.asmcall(pol, [truth], query, alns, cigar)
            w_call = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            _, vst, _, _ = api.varcall_from_records(pol, truth, b_recs, b_cigar, b_seq4, min_depth=1, min_alt=1)
            w_vc = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            text, _, _ = asmcall.call(refs, contigs, pol=pol)
            w_mod = (time.perf_counter() - t0) * 1e3
            if i == 0:
                continue
            walls["MapIndex.align"].append(w_align), walls["np2_asmcall"].append(w_call), walls["np2_varcall_from_records"].append(w_vc)
            walls["module (asmcall.call)"].append(w_mod)
            chain.append(ms["chain_ms"]), dp.append(als["dp_ms"]), assemble.append(als["assemble_ms"]), kernel.append(st["kernel_ms"])
            vc_records.append(vst["stage_ms"]["records"])
            for k, v in st["stage_ms"].items():
                stages[k].append(v)
    pol.close()
    emit(f"{st['alns_admitted']} of {st['alns_seen']} segments admitted; {st['runs']} R runs, {st['r_bases']} R bases, {st['cov0_bases']} bases at coverage 0, "
         f"{st['cov2_bases']} at >= 2; kept {st['kept_snv']} SNV, {st['kept_del']} DEL, {st['kept_ins']} INS of {st['found_snv']}, {st['found_del']}, "
         f"{st['found_ins']} found; {text.count(chr(10))} lines of text")
    for what, w in walls.items():
        emit(f"  {what}: wall ms {spread(w)}")
    emit(f"  the caller's kernels and sort together (kernel_ms): ms {spread(kernel)}")
    for k in api.ASMCALL_STAGES:
        emit(f"    {k}: ms {spread(stages[k])}")
    emit(f"  beside them, over the same alignments: k_vc_records ms {spread(vc_records)}")
    emit(f"  and the mapper and aligner that made them: chain_ms {spread(chain)}; dp_ms {spread(dp)}; assemble_ms {spread(assemble)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
