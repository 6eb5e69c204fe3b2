"""The rule of the full BAM (include/np2_io.h: NP2_SAM_KEEP_ALL) in plain Python, for test_bamfull_cpu.py and test_gpu_bamfull.py:
a SAM writer that emits QUAL, the mate fields, optional fields and extra header lines, and an encoder built on struct.pack
(a float is struct.pack("<f", float(text))).  The order, the blocks' offsets and the index are bamout_model's.

A record is a bamout_model record dict with, optionally: rnext (bytes: b"*", b"=" or a reference name), pnext and tlen (int, or
bytes to put malformed text), qual (bytes, None: "*"), tags (a list of bytes, each the text of one field, TAG:TYPE:VALUE)."""
import struct

import numpy as np

import bamout_model as bm
from bamout_model import BLOCK, bai, block_offsets, sort_records  # noqa: F401  (reused as they are)

HD = b"@HD\tVN:1.6\tSO:coordinate\n"


# ---- text ------------------------------------------------------------------------------------------------------------------
def _num(v):
    return v if isinstance(v, bytes) else b"%d" % v


def sam_line(refs, r, i=0, end=b"\n"):
    seq = r["seq"].encode("latin-1") if isinstance(r["seq"], str) else bytes(r["seq"])
    fields = [r.get("name", b"r%d" % i), b"%d" % r.get("flag", 0), refs[r["tid"]][0].encode() if r["tid"] >= 0 else b"*",
              b"%d" % (r["pos"] + 1), b"%d" % r.get("mapq", 60), "".join("%d%s" % (l, op) for op, l in r["cigar"]).encode() or b"*",
              r.get("rnext", b"*"), _num(r.get("pnext", 0)), _num(r.get("tlen", 0)), seq or b"*",
              r["qual"] if r.get("qual") is not None else b"*"] + list(r.get("tags", []))
    return b"\t".join(fields) + end


def sam_text(refs, recs, extra=(), hd=b"@HD\tVN:1.0\tSO:unsorted\n", end=b"\n"):
    """extra: header lines (without newline) behind the @SQ lines"""
    out = [hd] + [b"@SQ\tSN:%s\tLN:%d%s" % (n.encode(), l, end) for n, l in refs] + [l + end for l in extra]
    return b"".join(out) + b"".join(sam_line(refs, r, i, end) for i, r in enumerate(recs))


# ---- the optional fields ---------------------------------------------------------------------------------------------------
INT_TYPES = {"c": ("<b", -128, 127), "C": ("<B", 0, 255), "s": ("<h", -32768, 32767), "S": ("<H", 0, 65535),
             "i": ("<i", -2 ** 31, 2 ** 31 - 1), "I": ("<I", 0, 2 ** 32 - 1)}


def int_type(v):
    for t in ("CSI" if v >= 0 else "csi"):
        if INT_TYPES[t][1] <= v <= INT_TYPES[t][2]:
            return t
    raise ValueError(v)


def number(sub, text):
    if sub == "f":
        return struct.pack("<f", float(text))
    fmt, lo, hi = INT_TYPES[sub]
    v = int(text)
    assert lo <= v <= hi
    return struct.pack(fmt, v)


def aux(field):
    """one well-formed field's text -> its BAM bytes"""
    tag, typ, val = field[:2], chr(field[3]), field[5:].decode("latin-1")
    assert field[2:3] == b":" and field[4:5] == b":"
    if typ == "A":
        return tag + b"A" + val.encode("latin-1")
    if typ == "i":
        t = int_type(int(val))
        return tag + t.encode() + struct.pack(INT_TYPES[t][0], int(val))
    if typ == "f":
        return tag + b"f" + struct.pack("<f", float(val))
    if typ in "ZH":
        return tag + typ.encode() + val.encode("latin-1") + b"\0"
    assert typ == "B"
    sub, items = val[0], val[1:].split(",")[1:]
    return tag + b"B" + sub.encode() + struct.pack("<I", len(items)) + b"".join(number(sub, x) for x in items)


def tid_of(refs, name):
    return [n for n, _ in refs].index(name.decode())


def mates(refs, r):
    rn = r.get("rnext", b"*")
    ntid = -1 if rn == b"*" else r["tid"] if rn == b"=" else tid_of(refs, rn)
    return ntid, int(r.get("pnext", 0)) - 1, int(r.get("tlen", 0))


def tail(refs, r):
    """the tail the handle keeps of a record, padded to a word"""
    a = b"".join(aux(f) for f in r.get("tags", []))
    q = bytes(c - 33 for c in r["qual"]) if r.get("qual") is not None else b""
    t = struct.pack("<iiiI", *mates(refs, r), len(a)) + q + a
    return t + b"\0" * (-len(t) % 4)


def encode(refs, r):
    lean = bytearray(bm.encode(r))
    lean[24:36] = struct.pack("<iii", *mates(refs, r))
    l_seq = len(r["seq"])
    if r.get("qual") is not None:
        assert len(r["qual"]) == l_seq
        lean[len(lean) - l_seq:] = bytes(c - 33 for c in r["qual"])
    body = bytes(lean[4:]) + b"".join(aux(f) for f in r.get("tags", []))
    return struct.pack("<I", len(body)) + body


def header_text(refs, extras):
    """extras: per file, the header lines of the input (without line ends) other than the @SQ lines"""
    seen, out = set(), []
    for lines in extras:
        for l in lines:
            l = l.rstrip(b"\r")
            if l[:3] in (b"@HD", b"@SQ") and (len(l) == 3 or l[3:4] == b"\t") or l in seen:
                continue
            seen.add(l)
            out.append(l + b"\n")
    return HD + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), l) for n, l in refs) + b"".join(out)


def header(refs, extras=()):
    text = header_text(refs, extras)
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for n, l in refs:
        out += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", l)
    return out


def stream(refs, recs, extras=()):
    """-> (S, off) of the sorted records, as bamout_model.stream"""
    parts, off = [header(refs, extras)], []
    at = len(parts[0])
    for r in recs:
        off.append(at)
        parts.append(encode(refs, r))
        at += len(parts[-1])
    off.append(at)
    return b"".join(parts), off


def size_of(r):
    return bm.size_of(r) + sum(len(aux(f)) for f in r.get("tags", []))


def tails(refs, recs_in_input_order, order):
    """the tail bytes as the records were met, and tail_ref in the order `order` (indices into the input)"""
    buf, ref = bytearray(), []
    for r in recs_in_input_order:
        ref.append(len(buf) << 1 | (1 if r.get("qual") is not None else 0))
        buf += tail(refs, r)
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array([ref[i] for i in order], dtype=np.uint64)


def check_files(refs, recs, bam_bytes, bai_bytes, extras=(), what=""):
    import zlib
    S, off = stream(refs, recs, extras)
    C = block_offsets(bam_bytes)
    assert len(C) - 1 == (len(S) + BLOCK - 1) // BLOCK, (what, len(C), len(S))
    for b in range(len(C) - 1):
        assert zlib.decompress(bam_bytes[C[b]:C[b + 1]], 31) == S[b * BLOCK:(b + 1) * BLOCK], (what, "block", b)
    want = bai(refs, recs, off, C)
    assert bai_bytes == want, (what, "bai", len(bai_bytes), len(want))
    return S


# ---- decoration --------------------------------------------------------------------------------------------------------------
def qual_of(l_seq, seed=0):
    q = bytes(33 + (seed * 7 + i * 13 + i // 3) % 61 for i in range(l_seq))
    return b"+" if q == b"*" else q  # (a lone "*" means that there is none)


def decorate(recs, refs, seed=0):
    """qualities and a minimap2-like tag set on every record (in place); mates on some"""
    for i, r in enumerate(recs):
        n = len(r["seq"])
        r["qual"] = qual_of(n, seed + i) if n and i % 7 != 3 else None
        nm = (i * 37 + seed) % 300
        r["tags"] = [b"NM:i:%d" % nm, b"ms:i:%d" % (2 * n - nm), b"AS:i:%d" % (2 * n - 3 * nm), b"nn:i:0", b"tp:A:" + b"PS"[i % 2:i % 2 + 1],
                     b"cm:i:%d" % (n // 9), b"s1:i:%d" % (n - nm), b"s2:i:0", b"de:f:0.%04d" % (nm % 10000), b"rl:i:%d" % (i % 70000)]
        if i % 5 == 0:
            r["tags"].append(b"SA:Z:" + b",".join(b"%s,%d,+,%dM,60,%d;" % (refs[0][0].encode(), 100 + k, 50 + k, k) for k in range(i % 9 + 1)))
        if i % 3 == 0:
            r["tags"].append(b"MD:Z:" + b"".join(b"%dA" % (k % 40 + 1) for k in range(n // 40)) + b"7")
        if i % 4 == 1:
            r["rnext"], r["pnext"], r["tlen"] = b"=", r["pos"] + 50, (-1) ** i * (n + 50)
        elif i % 4 == 2 and len(refs) > 1:
            r["rnext"], r["pnext"], r["tlen"] = refs[(r["tid"] + 1) % len(refs)][0].encode(), 7 + i, 0
    return recs
