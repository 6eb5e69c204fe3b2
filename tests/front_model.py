"""The rule of the read front end in plain Python, one function per function of the reference (NextPolish2 v0.2.2
src/main.rs): a mapper's record and the contig -> the two aligned strings -> the trim to the first and last run of 8
equal columns -> the packed nibble stream.  Nothing here calls the oracle or the product; tests compare both with it."""

SEQ16 = "=ACMGRSVTWYHKDBN"  # what a BAM can carry: 4 bits a base
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3, "N": 5, "M": 6}  # SEQ_NUM (main.rs): everything else, '-' included, is 4


class UnknownCigar(Exception):
    """the reference panics with "Unknown cigar" (main.rs:430-432)"""


def bam_letter(ch):
    """a SEQ letter as the record carries it through a BAM: the 16-letter table without regard to case, N for the rest"""
    u = ch.upper()
    return u if u in SEQ16 else "N"


def columns(ref, rec):
    """Alignment::fill_with_cigar (main.rs:386-440): -> (t_aln, q_aln), the contig's and the read's row of every
    alignment column.  ref: the contig as str; rec: dict(pos, cigar [(op, len)], seq)."""
    t, q = [], []
    ts, qs = rec["pos"], 0
    seq = rec["seq"]
    for op, l in rec["cigar"]:
        if op == "S":                       # main.rs:395-402 (aln_q_s / aln_q_e only feed the clip filter)
            qs += l
        elif op in "M=X":                   # main.rs:403-411
            q += [bam_letter(c) for c in seq[qs:qs + l]]
            t += list(ref[ts:ts + l])
            assert len(q) == len(t), "SEQ or contig shorter than the CIGAR"
            qs += l
            ts += l
        elif op == "I":                     # main.rs:412-420
            q += [bam_letter(c) for c in seq[qs:qs + l]]
            t += ["-"] * l
            qs += l
        elif op == "D":                     # main.rs:421-428
            q += ["-"] * l
            t += list(ref[ts:ts + l])
            ts += l
        elif op == "H":                     # main.rs:429
            pass
        else:                               # main.rs:430-432
            raise UnknownCigar(op)
    return "".join(t), "".join(q)


def trim8(t, q):
    """Alignment::trim(8) (main.rs:447-513): -> (shift, new_len), the kept columns are [shift, new_len): from the first
    column of the first run of 8 byte-equal columns to the last column of the last such run; None without such a run
    (the reference sets shift = len: no column is left)."""
    n = len(t)
    run = 0
    shift = None
    for i in range(n):                      # main.rs:449-476
        run = run + 1 if t[i] == q[i] else 0
        if run == 8:
            shift = i + 1 - 8
            break
    if shift is None:                       # main.rs:510-512
        return None
    run = 0
    for i in range(n - 1, -1, -1):          # main.rs:478-509
        run = run + 1 if t[i] == q[i] else 0
        if run == 8:
            return shift, i + 8
    raise AssertionError("a run found forwards is found backwards")


def pack(pos, t, q, shift, new_len):
    """the target coordinates trim leaves and AlignSeq::new (main.rs:279-312): -> (aln_t_s, aln_t_e inclusive, n_cols,
    bytes).  A column's nibble is the read letter's code (A 0, C 1, G 2, T/U 3, N 5, M 6, anything else 4), | 8 where the
    contig's row is '-'; two a byte, high nibble first; then 0xF, and a whole 0xFF byte when n_cols is even."""
    aln_t_s = pos + sum(1 for c in t[:shift] if c != "-")
    n_cols = new_len - shift
    out = bytearray(((n_cols + 1) >> 1) + 1)    # main.rs:280-285
    aln_t_e = aln_t_s
    for i in range(n_cols):                     # main.rs:289-304
        b = _CODE.get(q[shift + i], 4)
        if t[shift + i] == "-":
            b |= 8
        elif i:
            aln_t_e += 1
        out[i >> 1] |= b << 4 if i & 1 == 0 else b
    out[n_cols >> 1] |= 0xFF if n_cols & 1 == 0 else 0x0F  # main.rs:306-310
    return aln_t_s, aln_t_e, n_cols, bytes(out[:(n_cols >> 1) + 1])


def front(ref, rec):
    """columns + trim8 + pack of one record: (shift, new_len, aln_t_s, aln_t_e, n_cols, bytes), or None (no anchor)"""
    t, q = columns(ref, rec)
    tr = trim8(t, q)
    if tr is None:
        return None
    return tr + pack(rec["pos"], t, q, *tr)
