"""The BAMs of test_bai_forms_cpu.py and test_gpu_bai_forms.py: four references, a few hundred records, a few linear-index
windows (16384 bases) and BGZF blocks each, with the window and block edges an index reader can get wrong made by hand.

  ctgA 70000  five windows, covered throughout; one record of 40000 M over four windows; a record with flag 0x4, a position
              and no CIGAR (span 0); a record whose span ends exactly on a window boundary and one that starts on one
  ctgB 90000  no record overlaps windows 0 and 1 (leading empty windows), window 3 is uncovered (an interior empty window)
  ctgC 25000  no record
  ctgD  3000  every record in window 0; they share a BGZF block with the tail of ctgB's

Each is written three ways (CUTS): blocks that end on record boundaries, blocks of 0xff00 bytes as samtools cuts them, and
blocks of 600 bytes, where length words and fixed fields straddle blocks.  build(dir) writes them with write_bam — whose
.bai the tests then replace by bai_model's forms — and returns what the tests share."""
import os

import numpy as np

from nextpolish2_amd.bamio import pileup_to_records, write_bam
from nextpolish2_amd.synth import Synth

W = 16384
REFS = [("ctgA", 70000), ("ctgB", 90000), ("ctgC", 25000), ("ctgD", 3000)]
CUTS = {"rec": None, "ff00": 0xff00, "b600": 600}
LONG_POS, LONG_LEN = 9000, 40000          # ctgA: windows 0 .. 2 and into 3
UNMAPPED_POS = 30000                      # ctgA: flag 0x4, placed, span 0
ENDS_ON_W = (2 * W - 2000, 2000)          # ctgA: (pos, M): the span ends exactly at 2 W
STARTS_ON_W = (3 * W, 1800)               # ctgA: starts exactly at 3 W
STRADDLED = 40                            # index of the record whose length word lies across a cut of the 600-byte blocks
B_COVERED = ((2 * W, 3 * W), (4 * W, 90000))  # ctgB: records lie wholly inside one of these


def front_opts():
    from nextpolish2_amd import io as np2io
    return np2io.FrontOpts(min_read_len=0, min_map_len=0, min_map_fra=0.0, max_clip_len=100000)


def _span(r):
    return sum(l for op, l in r["cigar"] if op in "MDN=X")


def records_and_refs():
    """-> (records sorted by (tid, pos), {tid: contig bytes})"""
    kw = dict(depth=8, read_len_mean=3500.0, read_len_sd=1200.0, read_len_min=1500)
    # (a synthetic assembly comes out a few bases off the length asked for: a little less is asked, and the contig filled up)
    sA = Synth(REFS[0][1] - 100, seed=501, name="ctgA", **kw)
    sB = Synth(REFS[1][1] - 100, seed=502, diploid=True, name="ctgB", **kw)
    sD = Synth(REFS[3][1] - 100, seed=504, depth=8, read_len_mean=1500.0, read_len_sd=200.0, read_len_min=1000, name="ctgD")
    refs = {}
    for tid, s in ((0, sA), (1, sB), (2, None), (3, sD)):
        seq = s.pileup.ref.tobytes() if s else b""
        assert len(seq) <= REFS[tid][1]
        refs[tid] = seq + bytes(np.random.default_rng(510 + tid).choice(np.frombuffer(b"ACGT", dtype=np.uint8), REFS[tid][1] - len(seq)))
    recs = pileup_to_records(sA.pileup, tid=0, rng=np.random.default_rng(1))
    recs += [r for r in pileup_to_records(sB.pileup, tid=1, rng=np.random.default_rng(2))
             if any(lo <= r["pos"] and r["pos"] + _span(r) <= hi for lo, hi in B_COVERED)]
    recs += pileup_to_records(sD.pileup, tid=3, rng=np.random.default_rng(3))
    a = refs[0].decode()
    for pos, n in ((LONG_POS, LONG_LEN), ENDS_ON_W, STARTS_ON_W):
        recs.append(dict(tid=0, pos=pos, mapq=60, flag=0, cigar=[("M", n)], seq=a[pos:pos + n]))
    recs.append(dict(tid=0, pos=UNMAPPED_POS, mapq=0, flag=4, cigar=[], seq=a[UNMAPPED_POS:UNMAPPED_POS + 1600]))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))  # (stable: ties stay in the order made)
    for i, r in enumerate(recs):
        r["name"] = b"q%d" % i
    # blocks of 600 bytes are cut at multiples of 600 from the first record on: longer names on three records put the length
    # word of STRADDLED-th record across such a cut (two bytes on either side), whatever the synthetic reads' lengths are
    size = lambda r: 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (len(r["seq"]) + 1) // 2 + len(r["seq"])
    pad = (598 - sum(size(r) for r in recs[:STRADDLED])) % 600
    for r in recs[STRADDLED - 3:STRADDLED]:
        r["name"] += b"x" * min(pad, 200)
        pad -= min(pad, 200)
    return recs, refs


def build(d):
    """writes <d>/<cut>.bam (+ write_bam's .bai) for every cut and <d>/ref<tid>.txt -> (records, refs, {cut: path})"""
    recs, refs = records_and_refs()
    paths = {}
    for cut, limit in CUTS.items():
        paths[cut] = os.path.join(str(d), cut + ".bam")
        write_bam(paths[cut], REFS, recs, block_limit=limit)
    for tid, seq in refs.items():
        with open(os.path.join(str(d), "ref%d.txt" % tid), "wb") as f:
            f.write(seq)
    return recs, refs, paths
