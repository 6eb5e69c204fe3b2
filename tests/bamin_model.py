"""The rule of BAM input (include/np2_io.h: "BAM input") in plain Python, for test_bamin_cpu.py and test_gpu_bamin.py: an
inflated BAM stream -> what the resident handle keeps of it, in input order, written on struct.unpack with no look at the
library's text of the rule; and the writers the tests build their BAM files with (bamfull_model's encoder, bamio's block cutter).

decode() returns what io.bamin_host returns: status and where per record; of the kept records recs (np2io.BAMREC_DTYPE),
tids, cigar, seq4, names, name_ref, tails, tail_ref."""
import io as pyio
import struct

import numpy as np

import bamfull_model as fm
from nextpolish2_amd import io as np2io
from nextpolish2_amd.bamio import _BgzfCut

E_ARG, E_UNSUPPORTED = -1, -4
(W_OK, W_SHORT, W_OVERRUN, W_REFID, W_POS, W_CIGAR, W_CG, W_NAME, W_NEXT_REFID, W_NEXT_POS, W_QUAL, W_AUX, W_TRUNC, W_GARBAGE,
 W_PIECE) = range(15)
SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def header_end(s):
    """-> (refs, offset of the first record)"""
    assert s[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", s, 4)
    n_ref, = struct.unpack_from("<I", s, 8 + l_text)
    at, refs = 12 + l_text, []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", s, at)
        refs.append((s[at + 4:at + 4 + l_name - 1].decode(), struct.unpack_from("<I", s, at + 4 + l_name)[0]))
        at += 8 + l_name
    return refs, at


def aux_ends(a):
    """do the optional fields end exactly at len(a)?"""
    i = 0
    while i < len(a):
        if len(a) - i < 3:
            return False
        t = chr(a[i + 2])
        i += 3
        if t in SIZES:
            i += SIZES[t]
        elif t in "ZH":
            nul = a.find(b"\0", i)
            if nul < 0:
                return False
            i = nul + 1
        elif t == "B":
            if len(a) - i < 5 or chr(a[i]) not in "cCsSiIf":
                return False
            i += 5 + SIZES[chr(a[i])] * struct.unpack_from("<I", a, i + 1)[0]
        else:
            return False
        if i > len(a):
            return False
    return True


def judge(rec, n_ref, names, full):
    """rec: a whole record, block_size word included -> (where, kept, fields dict)"""
    bs, = struct.unpack_from("<I", rec, 0)
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 4)
    need = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    if need > bs:
        return W_OVERRUN, False, None
    if tid < -1 or tid >= n_ref:
        return W_REFID, False, None
    if tid < 0 or flag & 4:
        return W_OK, False, None
    at = 36
    name, at = rec[at:at + l_name], at + l_name
    cigar, at = list(struct.unpack_from("<%dI" % n_cig, rec, at)), at + 4 * n_cig
    seq, at = bytearray(rec[at:at + (l_seq + 1) // 2]), at + (l_seq + 1) // 2
    qual, at = rec[at:at + l_seq], at + l_seq
    aux = rec[at:]
    if l_seq & 1:
        seq[-1] &= 0xF0
    bad = []
    if pos < -1:
        bad.append(W_POS)
    if any(w & 15 > 8 for w in cigar):
        bad.append(W_CIGAR)
    if n_cig == 2 and cigar[0] == (l_seq << 4 | 4) and cigar[1] & 15 == 3:
        bad.append(W_CG)
    if (names or full) and (l_name < 2 or name[-1:] != b"\0"):
        bad.append(W_NAME)
    has_qual = False
    if full:
        if ntid < -1 or ntid >= n_ref:
            bad.append(W_NEXT_REFID)
        if npos < -1:
            bad.append(W_NEXT_POS)
        if l_seq and qual != b"\xff" * l_seq:
            if max(qual) > 93:
                bad.append(W_QUAL)
            else:
                has_qual = True
        if not aux_ends(aux):
            bad.append(W_AUX)
    if bad:
        return min(bad), False, None
    return W_OK, True, dict(tid=tid, pos=pos, flag=flag, mapq=mapq, cigar=cigar, l_seq=l_seq, seq=bytes(seq), name=name[:-1], has_qual=has_qual,
                            tail=struct.pack("<iiiI", ntid, npos, tlen, len(aux)) + (qual if has_qual else b"") + aux)


def decode(s, keep_names=False, keep_all=False):
    refs, at = header_end(s)
    status, where, kept = [], [], []
    while at < len(s):
        if len(s) - at < 4:
            status.append(E_ARG), where.append(W_GARBAGE)
            break
        bs, = struct.unpack_from("<I", s, at)
        if bs < 32:
            status.append(E_ARG), where.append(W_SHORT)
            break
        if at + 4 + bs > len(s):
            status.append(E_ARG), where.append(W_TRUNC)
            break
        w, k, f = judge(s[at:at + 4 + bs], len(refs), keep_names, keep_all)
        at += 4 + bs
        where.append(w)
        status.append((E_UNSUPPORTED if w in (W_CG, W_PIECE) else E_ARG) if w else 0 if k else 1)
        if k:
            kept.append(f)
    recs = np.zeros(len(kept), np2io.BAMREC_DTYPE)
    cigar, seq4, names, tails, name_ref, tail_ref = [], bytearray(), bytearray(), bytearray(), [], []
    for i, f in enumerate(kept):
        recs[i]["pos"], recs[i]["flag"], recs[i]["mapq"], recs[i]["n_cigar"], recs[i]["l_seq"] = f["pos"], f["flag"], f["mapq"], len(f["cigar"]), f["l_seq"]
        recs[i]["cigar_off"], recs[i]["seq_off"] = len(cigar), len(seq4)
        cigar += f["cigar"]
        seq4 += f["seq"]
        if keep_names or keep_all:
            name_ref.append(len(names) << 8 | len(f["name"]))
            names += f["name"]
        if keep_all:
            tail_ref.append(len(tails) << 1 | (1 if f["has_qual"] else 0))
            tails += f["tail"] + b"\0" * (-len(f["tail"]) % 4)
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)
    return dict(status=np.array(status, np.int32), where=np.array(where, np.uint32), recs=recs, tids=np.array([f["tid"] for f in kept], np.int32),
                cigar=np.array(cigar, np.uint32), seq4=u8(seq4), names=u8(names), name_ref=np.array(name_ref, np.uint64), tails=u8(tails),
                tail_ref=np.array(tail_ref, np.uint64), first_bad=next((i for i, x in enumerate(status) if x < 0), None))


def same(a, b, what=""):
    """two decode()-shaped dicts hold the same"""
    for k in ("status", "where", "tids", "cigar", "seq4", "names", "name_ref", "tails", "tail_ref"):
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:16], b[k][:16])
    assert a["recs"].tobytes() == b["recs"].tobytes(), (what, "recs")


# ---- writers ----------------------------------------------------------------------------------------------------------------
def raw_record(tid=0, pos=10, name=b"q\0", cigar=((0, 4),), seq=b"\x12\x48", l_seq=None, qual=None, aux=b"", flag=0, mapq=60, ntid=-1, npos=-1,
               tlen=0, block_size=None, l_name=None, n_cigar=None):
    """a record from its raw parts, so that malformed ones can be put together; cigar: (op number, length) pairs"""
    l_seq = 2 * len(seq) if l_seq is None else l_seq
    qual = b"\xff" * l_seq if qual is None else qual
    cig = b"".join(struct.pack("<I", l << 4 | op) for op, l in cigar)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(name) if l_name is None else l_name, mapq, 0, len(cigar) if n_cigar is None else n_cigar, flag,
                       l_seq, ntid, npos, tlen) + name + cig + seq + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def inflated(refs, recs, extras=(), raw=False):
    """the stream of `recs` in the order given: record dicts through bamfull_model.encode, or bytes as they are"""
    return fm.header(refs, [extras] if extras else ()) + b"".join(r if raw or isinstance(r, bytes) else fm.encode(refs, r) for r in recs)


def bgzf(stream, cut=0xff00, level=6, eof=True, empty_after=None):
    """the stream as BGZF, a block cut every `cut` bytes wherever that falls; empty_after: an empty block behind that many blocks"""
    f = pyio.BytesIO()
    w = _BgzfCut(f, cut, level)
    if empty_after is None:
        w.write(stream)
    else:
        w.write(stream[:cut * empty_after])
        w._flush_block(b"")
        w.write(stream[cut * empty_after:])
    w.flush()
    if eof:
        w._flush_block(b"")
    return f.getvalue()


def block_bounds(stream_len, cut):
    """the inflated offsets at which blocks of `cut` bytes end"""
    return list(range(cut, stream_len, cut))
