"""A plain-Python model of the SAM rule of include/np2_io.h (np2_sam_*): text -> references, the kept records in sorted order
as the dicts bamio.write_bam takes, the np2_bamrec / tid / cigar / seq4 arrays as the device leaves them, the statistics, and
the error with its 1-based line.  Written from the rule's text, field by field with bytes.split and regular expressions; it
shares no code with csrc/np2_sam_core.hpp."""
import re

import numpy as np

from nextpolish2_amd import bamio

E_ARG, E_UNSUPPORTED = -1, -4
# why a line is refused; of several on one line the smallest speaks (csrc/np2_sam_core.hpp)
HEADER_LATE, FIELDS, FLAG, RNAME, POS, MAPQ, CIGAR = 1, 2, 3, 4, 5, 6, 7
_DEC = re.compile(rb"[0-9]+")
_CIGAR = re.compile(rb"(?:[0-9]+[MIDNSHP=X])+")
_CIGAR_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")


class SamError(Exception):
    def __init__(self, code, line, what, file=0):
        super().__init__(f"file {file} line {line}: {what}")
        self.code, self.line, self.what, self.file = code, line, what, file


def _dec(field, top):
    """the decimal number `field`, None when it is empty, holds a non-digit or exceeds top"""
    if not _DEC.fullmatch(field):
        return None
    v = int(field)
    return v if v <= top else None


def split_lines(text):
    """the lines of `text` without their '\\n' and without a '\\r' directly before it; a last line needs no newline"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def parse_line(line, tid_of):
    """one line behind the header -> None (no byte) | int (why it is refused) | the record as a dict with `kept`"""
    if not line:
        return None
    if line.startswith(b"@"):
        return HEADER_LATE
    f = line.split(b"\t")
    if len(f) < 11:
        return FIELDS
    errs = []
    flag = _dec(f[1], 65535)
    if flag is None:
        errs.append(FLAG)
    tid = -1 if f[2] == b"*" else tid_of.get(f[2])
    if tid is None:
        errs.append(RNAME)
    pos1 = _dec(f[3], 2 ** 31 - 1)
    if pos1 is None:
        errs.append(POS)
    mapq = _dec(f[4], 255)
    if mapq is None:
        errs.append(MAPQ)
    cigar = []
    if f[5] != b"*":
        if not _CIGAR.fullmatch(f[5]):
            errs.append(CIGAR)
        else:
            cigar = [(op.decode(), int(n)) for n, op in _CIGAR_OP.findall(f[5])]
            if any(n >= 2 ** 28 for _, n in cigar):
                errs.append(CIGAR)
    if errs:
        return min(errs)
    seq = "" if f[9] == b"*" else f[9].decode("latin-1")
    return dict(tid=tid, pos=pos1 - 1, mapq=mapq, flag=flag, cigar=cigar, seq=seq, name=f[0], kept=tid != -1 and not flag & 4)


def parse_header(lines):
    """-> (refs [(name, length)], number of header lines); SamError for an @SQ line the rule refuses"""
    refs, n = [], 0
    for n, ln in enumerate(lines):
        if ln and not ln.startswith(b"@"):
            break
        if ln.startswith(b"@SQ") and (len(ln) == 3 or ln[3:4] == b"\t"):
            tags = {}
            for t in ln.split(b"\t")[1:]:
                if len(t) >= 3 and t[2:3] == b":":
                    tags.setdefault(t[:2], t[3:])
            length = _dec(tags[b"LN"], 2 ** 32 - 1) if b"LN" in tags else None
            if not tags.get(b"SN") or b"LN" not in tags:
                raise SamError(E_ARG, n + 1, "an @SQ line without SN or LN")
            if length is None:
                raise SamError(E_ARG, n + 1, "LN is not a number")
            if tags[b"SN"] in [r[0].encode("latin-1") for r in refs]:
                raise SamError(E_ARG, n + 1, "a duplicate SN")
            refs.append((tags[b"SN"].decode("latin-1"), length))
    else:
        n = len(lines)
    return refs, n


class Result:
    """refs; records: the kept records in sorted order (dicts); order: their ordinals among the kept records in input order;
    lines_out: per line behind the headers, in input order, what parse_line gave; stats"""

    def arrays(self):
        """(recs, tids, cigar, seq4): the records in sorted order with cigar_off running in that order, the CIGAR words
        in that order, seq_off and seq4 as the kept records were met in the text"""
        kept_in = [r for r in self.lines_out if isinstance(r, dict) and r["kept"]]
        arr_in, cig_in, seq4, _, _ = bamio.records_to_arrays(kept_in)
        arr = arr_in[np.array(self.order, dtype=np.int64)].copy()
        cigar, off = [], 0
        for i, k in enumerate(self.order):
            a, n = int(arr_in[k]["cigar_off"]), int(arr_in[k]["n_cigar"])
            cigar.append(cig_in[a:a + n])
            arr[i]["cigar_off"] = off
            off += n
        tids = np.array([kept_in[k]["tid"] for k in self.order], dtype=np.int32)
        cig = np.concatenate(cigar).astype(np.uint32) if cigar else np.zeros(0, np.uint32)
        return arr, tids, cig, seq4[:self.stats["seq_bytes"]]


def model(texts, tie="strand"):
    """texts: the bytes of one file, or a list of them in argument order"""
    if isinstance(texts, (bytes, bytearray)):
        texts = [texts]
    assert tie in ("strand", "input")
    res = Result()
    res.refs, res.lines_out = None, []
    n_lines = 0
    for fi, text in enumerate(texts):
        lines = split_lines(bytes(text))
        n_lines += len(lines)
        try:
            refs, n_head = parse_header(lines)
        except SamError as e:
            e.file = fi
            raise
        if res.refs is None:
            res.refs = refs
        elif refs != res.refs:
            raise SamError(E_ARG, 0, "the @SQ lists differ", fi)
        tid_of = {n.encode("latin-1"): i for i, (n, _) in enumerate(res.refs)}
        for j in range(n_head, len(lines)):
            r = parse_line(lines[j], tid_of)
            if isinstance(r, int):
                raise SamError(E_ARG, j + 1, r, fi)
            res.lines_out.append(r)
    recs = [r for r in res.lines_out if r is not None]
    kept = [r for r in recs if r["kept"]]
    key = lambda r: (r["tid"], r["pos"] + 1, (r["flag"] >> 4) & 1 if tie == "strand" else 0)
    res.order = sorted(range(len(kept)), key=lambda k: key(kept[k]))  # (sorted is stable: ties keep input order)
    res.records = [kept[k] for k in res.order]
    res.stats = dict(lines=n_lines, records=len(recs), unmapped=len(recs) - len(kept), kept=len(kept),
                     cigar_words=sum(len(r["cigar"]) for r in kept), seq_bytes=sum((len(r["seq"]) + 1) // 2 for r in kept))
    return res


def sort_key_int(r, tie):
    """the 64-bit key of a kept record"""
    return r["tid"] << 33 | (r["pos"] + 1) << 1 | ((r["flag"] >> 4) & 1 if tie == "strand" else 0)
