"""The rule of the BAM writer (include/np2_io.h: np2_sam_write_bam) in plain Python, for test_bamout_cpu.py and
test_gpu_bamout.py: the stream from bamio.encode_record, the bins from bamio.reg2bin, the virtual offset V and the index
from the rule's own words, with the blocks' file offsets C read by walking the BSIZE fields of the written file.  Also the
hand-built record lists both tests run."""
import struct

import numpy as np

from nextpolish2_amd.bamio import CIGAR_OPS, encode_record, reg2bin
from nextpolish2_amd.io import BAMREC_DTYPE

BLOCK = 65280
EOF_BLOCK = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def header(refs):
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in refs)
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for n, l in refs:
        out += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", l)
    return out


def sort_records(recs, tie="strand"):
    """the resident order: (tid, pos + 1, strand-or-0), ties in input order; unmapped records dropped"""
    kept = [r for r in recs if r["tid"] >= 0 and not r.get("flag", 0) & 4]
    return sorted(kept, key=lambda r: (r["tid"], r["pos"] + 1, (r.get("flag", 0) >> 4) & 1 if tie == "strand" else 0))


def span(r):
    return sum(l for op, l in r["cigar"] if op in "MDN=X")


def encode(r):
    return encode_record(r["tid"], r["pos"], r.get("mapq", 60), r.get("flag", 0), r["cigar"], r["seq"], r["name"])[0]


def stream(refs, recs):
    """-> (S, off): the stream of the sorted records, and where each begins (len(recs) + 1 entries)"""
    parts, off = [header(refs)], []
    at = len(parts[0])
    for r in recs:
        off.append(at)
        parts.append(encode(r))
        at += len(parts[-1])
    off.append(at)
    return b"".join(parts), off


def block_offsets(bam_bytes):
    """C: the file offset of every BGZF block, the EOF block's last, by walking BSIZE"""
    C, at = [], 0
    while at < len(bam_bytes):
        assert bam_bytes[at:at + 4] == b"\x1f\x8b\x08\x04" and bam_bytes[at + 12:at + 16] == b"BC\x02\x00", at
        C.append(at)
        at += struct.unpack_from("<H", bam_bytes, at + 16)[0] + 1
    assert at == len(bam_bytes) and bam_bytes[C[-1]:] == EOF_BLOCK
    return C


def bai(refs, recs, off, C):
    """the .bai of the rule: chunks are maximal runs of consecutive records of one (tid, bin)"""
    V = lambda u: C[u // BLOCK] << 16 | u % BLOCK
    bins = [dict() for _ in refs]
    lin = [dict() for _ in refs]
    prev = None
    for i, r in enumerate(recs):
        beg, end = V(off[i]), V(off[i + 1])
        p0, p1 = r["pos"], r["pos"] + max(span(r), 1)
        key = (r["tid"], reg2bin(p0, p1))
        if key == prev:
            bins[key[0]][key[1]][-1][1] = end
        else:
            bins[key[0]].setdefault(key[1], []).append([beg, end])
        prev = key
        for w in range(p0 >> 14, ((p1 - 1) >> 14) + 1):
            lin[r["tid"]].setdefault(w, beg)
    out = b"BAI\1" + struct.pack("<I", len(refs))
    for t in range(len(refs)):
        out += struct.pack("<I", len(bins[t]))
        for b, ch in sorted(bins[t].items()):
            out += struct.pack("<II", b, len(ch)) + b"".join(struct.pack("<QQ", x, y) for x, y in ch)
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        out += struct.pack("<I", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin[t].get(w, last)
            out += struct.pack("<Q", last)
    return out


def arrays(recs):
    """sorted record dicts -> what Sam.export and Sam.export_names return: (recs, tids, cigar, seq4, names, name_ref)"""
    from nextpolish2_amd.bamio import records_to_arrays
    arr, cig, seq4, _, _ = records_to_arrays(recs)
    names, ref = bytearray(), []
    for r in recs:
        ref.append(len(names) << 8 | len(r["name"]))
        names += r["name"]
    return (arr, np.array([r["tid"] for r in recs], dtype=np.int32), cig, seq4[:len(seq4) - 16].copy(),
            np.frombuffer(bytes(names), dtype=np.uint8), np.array(ref, dtype=np.uint64))


def check_files(refs, recs, bam_bytes, bai_bytes, what=""):
    """the two files against the rule: the blocks hold the model's stream cut every 65280 bytes, the index is the model's"""
    import zlib
    S, off = stream(refs, recs)
    C = block_offsets(bam_bytes)
    assert len(C) - 1 == (len(S) + BLOCK - 1) // BLOCK, (what, len(C), len(S))
    for b in range(len(C) - 1):
        assert zlib.decompress(bam_bytes[C[b]:C[b + 1]], 31) == S[b * BLOCK:(b + 1) * BLOCK], (what, "block", b)
    want = bai(refs, recs, off, C)
    assert bai_bytes == want, (what, "bai", len(bai_bytes), len(want))
    return S


# ---- the hand-built shapes -----------------------------------------------------------------------------------------------
BIG = 1 << 29
REFS = [("c1", BIG), ("c2", 5000), ("c3", 300000)]
BASES = "ACGT"


def rec(tid, pos, cigar, l_seq=None, name=b"q", flag=0, mapq=60, seed=0):
    """a record whose SEQ is l_seq bases (default: what the CIGAR consumes of the read), made from `seed`"""
    if l_seq is None:
        l_seq = sum(l for op, l in cigar if op in "MIS=X")
    seq = "".join(BASES[(seed + 7 * i + i // 5) & 3] for i in range(l_seq))
    return dict(tid=tid, pos=pos, cigar=cigar, seq=seq, name=name, flag=flag, mapq=mapq)


def size_of(r):
    return 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (len(r["seq"]) + 1) // 2 + len(r["seq"])


def filler(tid, pos, size, seed=0):
    """a record of exactly `size` bytes in the stream (size >= 60): one M operation, the name takes up the slack"""
    for l_seq in range(max(0, (size - 41 - 254) * 2 // 3 - 2), size):
        k = size - 41 - ((l_seq + 1) // 2 + l_seq)
        if 1 <= k <= 254 and l_seq >= 1:
            r = rec(tid, pos, [("M", l_seq)], name=b"f" * k, seed=seed)
            assert size_of(r) == size
            return r
    raise AssertionError(size)


def fill_to(recs, refs, target, tid, pos):
    """append fillers at (tid, pos ..) until the stream of `recs` is exactly `target` bytes long; returns the next free pos"""
    at = len(header(refs)) + sum(size_of(r) for r in recs)
    while at < target:
        left = target - at
        take = left if left <= 50000 else min(40000, left - 100)  # (what is left stays a size a filler can have)
        recs.append(filler(tid, pos, take, seed=pos))
        at += take
        pos += 1
    assert at == target, (at, target)
    return pos


def case_cuts():
    """byte 65280 k falls, in turn, into a record's block_size word, fixed fields, name, CIGAR words, SEQ bytes and 0xFF run"""
    recs, pos = [], 10
    # the target: 4 + 32 + (20 + 1) + 4 * 30 + 100 + 200 bytes; parts begin at 0, 4, 36, 57, 177, 277
    for k, inside in enumerate((2, 20, 45, 103, 200, 400), start=1):
        pos = fill_to(recs, REFS, BLOCK * k - inside, 0, pos)
        recs.append(rec(0, pos, [("M", 5), ("I", 1)] * 14 + [("M", 5), ("S", 111)], name=b"target_%013d" % k, seed=k))
        assert size_of(recs[-1]) == 477
        pos += 1
    return REFS, recs


def case_exact(blocks):
    """a stream of exactly `blocks` * 65280 bytes: the last record's end is V at the very end"""
    recs = []
    fill_to(recs, REFS, BLOCK * blocks, 0, 5)
    return REFS, recs


def case_long():
    """one record of 100 000 bases: three blocks, and three batches at one block a batch"""
    return REFS, [rec(0, 3, [("M", 100000)], name=b"long")]


def case_small():
    """l_seq 0, 1 and odd, CIGAR *, names of 1 and 254 bytes, 65535 CIGAR operations"""
    return REFS, [
        rec(0, 0, [("M", 10)], l_seq=0, name=b"s"),
        rec(0, 1, [("M", 1)], name=b"n" * 254),
        rec(0, 2, [("M", 3)], name=b"odd"),
        rec(0, 2, [], l_seq=7, name=b"star_cigar"),
        rec(0, 2, [], l_seq=0, name=b"star_both", flag=16),
        rec(0, 9, [("M", 1), ("I", 1)] * 32767 + [("M", 1)], name=b"many_ops"),
        rec(1, 4999, [("M", 1)], name=b"last_base"),
    ]


def case_bins():
    """windows and bins at their edges; c2, the middle reference, has no record"""
    return [("c1", BIG), ("c2", 5000), ("c3", 300000)], [
        rec(0, 10, [("M", 5)], name=b"bin4681_a"),
        rec(0, 100, [("M", 20000)], l_seq=4, name=b"bin585"),            # crosses 16384: one level up
        rec(0, 200, [("M", 5)], name=b"bin4681_b"),                       # the bin met again: a second chunk
        rec(0, 16380, [("M", 4)], name=b"ends_at_16384"),                 # [16380, 16384): window 0 alone
        rec(0, 16381, [("M", 4)], name=b"ends_at_16385"),                 # [16381, 16385): windows 0 and 1
        rec(0, 16383, [("M", 1), ("D", 1)], name=b"span_two"),            # [16383, 16385)
        rec(0, 5 * 16384 + 7, [("M", 3)], name=b"window_5"),              # windows 2 .. 4 stay empty
        rec(0, (1 << 17) - 1, [("M", 2)], l_seq=2, name=b"level4"),       # crosses 2^17: bin 73 + ..
        rec(0, (1 << 20) - 1, [("=", 1), ("X", 1)], name=b"level3"),      # crosses 2^20
        rec(0, (1 << 23) - 1, [("M", 1), ("N", 1)], name=b"level2"),      # crosses 2^23
        rec(0, (1 << 26) - 1, [("M", 2)], name=b"level1"),                # crosses 2^26: bin 0
        rec(0, BIG - 1, [("M", 1)], name=b"last_base"),                   # the last base BAI addresses
        rec(2, 100000, [("M", 50)], name=b"leading_empty_windows"),       # windows 0 .. 5 of c3 are empty
        rec(2, 100000, [("M", 50)], name=b"tie_reverse", flag=16),
        rec(2, 100000, [("M", 50)], name=b"tie_forward"),
        rec(2, 100000, [("S", 2), ("M", 40000)], l_seq=5, name=b"tie_long"),
    ]


CASES = {"empty": lambda: (REFS, []), "cuts": case_cuts, "exact_1": lambda: case_exact(1), "exact_2": lambda: case_exact(2),
         "long": case_long, "small": case_small, "bins": case_bins}

# name -> (refs, records, status): each refused before a file exists
E_ARG, E_UNSUPPORTED = -1, -4
REFUSED = {
    "n_cigar_65536": (REFS, [rec(0, 5, [("M", 1), ("I", 1)] * 32768, name=b"ops")], E_UNSUPPORTED),
    "pos_zero": (REFS, [rec(0, 3, [("M", 4)], name=b"ok"), rec(1, -1, [("M", 4)], name=b"unplaced")], E_ARG),
    "ln_too_large": ([("c1", BIG + 1)], [rec(0, 5, [("M", 4)], name=b"r")], E_UNSUPPORTED),
    "ends_behind_2_29": (REFS, [rec(0, BIG - 1, [("M", 2)], l_seq=2, name=b"r")], E_UNSUPPORTED),
}
