"""An index-free scan of a BAM file and .bai writers in several forms, in plain Python (zlib, struct).  Nothing here
imports the product or reads the .bai next to a file: scan() walks the BGZF blocks and the records of the stream they
make, and its list of records with their virtual offsets is the expected answer of test_bai_forms_cpu.py and
test_gpu_bai_forms.py.

Virtual offsets: a stream position inside a block is (file offset of the block << 16) | offset inside it.  A position
that falls exactly on a block's end has two spellings: (next block, 0), which is what htslib's reader reports and what
scan() gives ("normalised"), and (this block, its inflated size), which a writer gets when it asks where it is before
it closes the block.

The forms of write_bai:

  own           what nextpolish2_amd.bamio.write_bam writes: records with flag 0x4 left out, bins ascending, a new chunk
                whenever a record's begin differs from the previous chunk's end AS SPELLED, empty linear windows taking the
                previous window's value (0 before the first).  write_bam notes a record's end before it closes a block, so
                an end on a block's end is spelled (this block, inflated size) here, while every begin is normalised; a
                chunk therefore never runs across a block that ends on a record boundary.  On a BAM write_bam wrote with
                its default blocks this reproduces its .bai byte for byte (the check that scan's offsets are right).
  htslib        as htslib's index writer is documented in the SAM specification (section 5.2, reg2bin) and its published
                source (hts_idx_push, compress_binning, update_loff, hts_idx_save): every placed record, bin =
                reg2bin(pos, pos + max(span, 1)); one chunk per run of consecutive records of a bin; from the deepest
                level up, a bin whose chunks span less than 0x10000 of compressed file offset goes into its parent if the
                parent exists; chunks sorted by begin and merged while prev.end >> 16 >= next.beg >> 16; bins in hash
                order (here: shuffled by `seed`); the pseudo-bin 37450 with (smallest begin, largest end) and (mapped,
                unmapped) per reference with records; an empty linear window takes the NEXT non-empty one's value; a
                trailing 8-byte count of unplaced reads.  THIS FORM IS WRITTEN FROM THE PUBLISHED DESCRIPTION AND IS NOT
                PINNED AGAINST AN HTSLIB BINARY: none exists where these tests are written or run.
  htslib_nometa the same without the pseudo-bin and the trailing count
  sparse        one chunk per placed record, unmerged; bins descending; empty linear windows hold 0, interior ones too
  end_at_isize  own, but every offset on a block's end — begins and linear entries too — spelled (this block, inflated size)
"""
import bisect
import random
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
SEQ16 = "=ACMGRSVTWYHKDBN"
FORMS = ("own", "htslib", "htslib_nometa", "sparse", "end_at_isize")
META_BIN = 37450
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)  # first bin of each level of the binning scheme


def reg2bin(beg, end):
    """SAM specification 5.3: the smallest bin that holds [beg, end)"""
    end -= 1
    for shift, level in ((14, 5), (17, 4), (20, 3), (23, 2), (26, 1)):
        if beg >> shift == end >> shift:
            return LEVEL_FIRST[level] + (beg >> shift)
    return 0


class Scan:
    """blocks: [(file offset, inflated size, stream offset)] of every BGZF block, the end-of-file marker included;
    refs: [(name, length)]; records: dicts in file order; file_len."""

    def __init__(self, blocks, refs, records, file_len):
        self.blocks, self.refs, self.records, self.file_len = blocks, refs, records, file_len
        self._full = [b for b in blocks if b[1]]  # the blocks that hold bytes
        self._ends = [b[2] + b[1] for b in self._full]

    def voff(self, spos, end_at_isize=False):
        """virtual offset of stream position spos; a position on a block's end as (next block, 0), or — end_at_isize —
        as (this block, inflated size)"""
        i = bisect.bisect_right(self._ends, spos)  # first block that ends beyond spos
        if end_at_isize and i > 0 and self._ends[i - 1] == spos:
            fo, isize, _ = self._full[i - 1]
            return (fo << 16) | isize
        if i < len(self._full):
            fo, _, so = self._full[i]
            return (fo << 16) | (spos - so)
        # the end of the stream: the block behind the last one that holds bytes (the end-of-file marker), or the file's end
        behind = [b for b in self.blocks if b[0] > self._full[-1][0]] if self._full else self.blocks
        return (behind[0][0] if behind else self.file_len) << 16

    def spos(self, v):
        """stream position a virtual offset names, in either spelling (None: not a block of the file, or beyond its bytes)"""
        for fo, isize, so in self.blocks:
            if fo == v >> 16:
                return so + (v & 0xFFFF) if (v & 0xFFFF) <= isize else None
        return None

    def of(self, tid):
        return [r for r in self.records if r["tid"] == tid]


def scan(path):
    with open(path, "rb") as f:
        data = f.read()
    blocks, parts, o, so = [], [], 0, 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", "not a BGZF block at %d" % o
        xlen, = struct.unpack_from("<H", data, o + 10)
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, x + 4)[0] + 1
            x += 4 + slen
        assert bsize is not None and o + bsize <= len(data)
        crc, isize = struct.unpack_from("<II", data, o + bsize - 8)
        raw = zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15)
        assert len(raw) == isize and zlib.crc32(raw) & 0xFFFFFFFF == crc
        blocks.append((o, isize, so))
        parts.append(raw)
        so += isize
        o += bsize
    st = b"".join(parts)
    assert st[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", st, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<I", st, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", st, p)
        refs.append((st[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<I", st, p + 4 + l_name)[0]))
        p += 8 + l_name
    sc = Scan(blocks, refs, [], len(data))
    while p < len(st):
        bs, = struct.unpack_from("<I", st, p)
        tid, pos, l_name, mapq, _bin, ncig, flag, l_seq = struct.unpack_from("<iiBBHHHI", st, p + 4)
        q = p + 36
        name = st[q:q + l_name - 1]
        q += l_name
        cw = struct.unpack_from("<%dI" % ncig, st, q)
        q += 4 * ncig
        nib = st[q:q + (l_seq + 1) // 2]
        seq = "".join(SEQ16[b >> 4] + SEQ16[b & 15] for b in nib)[:l_seq]
        cigar = [(CIGAR_OPS[w & 15], w >> 4) for w in cw]
        sc.records.append(dict(tid=tid, pos=pos, mapq=mapq, flag=flag, name=name, cigar=cigar, seq=seq,
                               span=sum(l for op, l in cigar if op in "MDN=X"), spos=p, send=p + 4 + bs,
                               beg=sc.voff(p), end=sc.voff(p + 4 + bs)))
        p += 4 + bs
    assert p == len(st)
    return sc


def fetch_rule(sc, tid, zone_lo, zone_hi):
    """the records fetch(tid, zone_lo, zone_hi) gives, as fetch_records and bam_chain state the rule: refID == tid and
    0 <= pos < min(L, zone_hi); for zone_lo > 0 also pos + span > zone_lo"""
    L = sc.refs[tid][1]
    return [r for r in sc.of(tid) if 0 <= r["pos"] < min(L, zone_hi) and (zone_lo == 0 or r["pos"] + r["span"] > zone_lo)]


def _windows(r):
    return range(r["pos"] >> 14, ((r["pos"] + max(r["span"], 1) - 1) >> 14) + 1)


def _own(sc, recs, all_at_isize):
    bins, lin = {}, {}
    for r in recs:
        if r["flag"] & 4:
            continue
        beg, end = sc.voff(r["spos"], all_at_isize), sc.voff(r["send"], True)
        ch = bins.setdefault(reg2bin(r["pos"], r["pos"] + max(r["span"], 1)), [])
        if ch and ch[-1][1] == beg:
            ch[-1][1] = end
        else:
            ch.append([beg, end])
        for w in _windows(r):
            lin.setdefault(w, beg)
    out, prev = [], 0
    for w in range(max(lin) + 1 if lin else 0):
        prev = lin.get(w, prev)
        out.append(prev)
    return [(b, [tuple(c) for c in ch]) for b, ch in sorted(bins.items())], out


def _sparse(sc, recs):
    bins, lin = {}, {}
    for r in recs:
        bins.setdefault(reg2bin(r["pos"], r["pos"] + max(r["span"], 1)), []).append((r["beg"], r["end"]))
        for w in _windows(r):
            lin.setdefault(w, r["beg"])
    return sorted(bins.items(), reverse=True), [lin.get(w, 0) for w in range(max(lin) + 1 if lin else 0)]


def _htslib(sc, recs, meta, rng):
    bins, lin, last_bin = {}, {}, None
    for r in recs:
        b = reg2bin(r["pos"], r["pos"] + max(r["span"], 1))
        if b == last_bin:
            bins[b][-1][1] = r["end"]
        else:
            bins.setdefault(b, []).append([r["beg"], r["end"]])
        last_bin = b
        for w in _windows(r):
            lin.setdefault(w, r["beg"])
    for level in range(5, 0, -1):  # compress_binning: small bins go into their parents, deepest level first
        for b in sorted(k for k in bins if k >= LEVEL_FIRST[level]):
            ch = bins[b]
            if level < 5:
                ch.sort()
            if (ch[-1][1] >> 16) - (ch[0][0] >> 16) < 0x10000 and (b - 1) >> 3 in bins:
                bins[(b - 1) >> 3] += ch
                del bins[b]
    for b, ch in bins.items():
        ch.sort()
        merged = [list(ch[0])]
        for beg, end in ch[1:]:
            if merged[-1][1] >> 16 >= beg >> 16:
                merged[-1][1] = max(merged[-1][1], end)
            else:
                merged.append([beg, end])
        bins[b] = merged
    out = [(b, [tuple(c) for c in ch]) for b, ch in bins.items()]
    if meta and recs:
        n_un = sum(1 for r in recs if r["flag"] & 4)
        out.append((META_BIN, [(min(r["beg"] for r in recs), max(r["end"] for r in recs)), (len(recs) - n_un, n_un)]))
    rng.shuffle(out)
    n_intv = max(lin) + 1 if lin else 0
    filled, nxt = [0] * n_intv, 0
    for w in range(n_intv - 1, -1, -1):  # update_loff: the last entry is always there; an empty one takes the next one's
        nxt = lin.get(w, nxt)
        filled[w] = nxt
    return out, filled


def index_of(sc, form, seed=0):
    """-> ([(bins [(bin, [(beg, end)])], linear [offset])] per reference, trailing bytes)"""
    assert form in FORMS
    rng = random.Random(seed)
    refs = []
    for tid in range(len(sc.refs)):
        recs = sc.of(tid)
        if form in ("own", "end_at_isize"):
            refs.append(_own(sc, recs, form == "end_at_isize"))
        elif form == "sparse":
            refs.append(_sparse(sc, recs))
        else:
            refs.append(_htslib(sc, recs, form == "htslib", rng))
    tail = struct.pack("<Q", sum(1 for r in sc.records if r["tid"] < 0)) if form == "htslib" else b""
    return refs, tail


def pack_bai(refs, tail=b""):
    out = [b"BAI\1", struct.pack("<I", len(refs))]
    for bins, lin in refs:
        out.append(struct.pack("<I", len(bins)))
        for b, ch in bins:
            out.append(struct.pack("<II", b, len(ch)))
            out += [struct.pack("<QQ", beg, end) for beg, end in ch]
        out.append(struct.pack("<I", len(lin)))
        out += [struct.pack("<Q", v) for v in lin]
    return b"".join(out) + tail


def unpack_bai(data):
    """the inverse of pack_bai -> (refs, tail); for tests that edit an index"""
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<I", data, 4)
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<I", data, p)
        p += 4
        bins = []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", data, p)
            p += 8
            bins.append((b, [struct.unpack_from("<QQ", data, p + 16 * i) for i in range(n_chunk)]))
            p += 16 * n_chunk
        n_intv, = struct.unpack_from("<I", data, p)
        p += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, p))))
        p += 8 * n_intv
    return refs, data[p:]


def ref_block_ends(refs):
    """byte offset in pack_bai(refs) just behind each reference's part (the cuts at which a prefix is a whole number of references)"""
    ends, p = [], 8
    for bins, lin in refs:
        p += 4 + sum(8 + 16 * len(ch) for _, ch in bins) + 4 + 8 * len(lin)
        ends.append(p)
    return ends


def write_bai(path, sc, form, seed=0):
    """writes <path>.bai for the BAM at `path` that `sc` is the scan of; -> the bytes"""
    refs, tail = index_of(sc, form, seed)
    data = pack_bai(refs, tail)
    with open(path + ".bai", "wb") as f:
        f.write(data)
    return data
