"""A plain Python model of the aligner's opt-in outputs (include/np2_io.h: np2_map_align_*, "Tags"), written from the rule's text,
not from the C++: tags(t, q, cigar) -> (MD, cs, the CIGAR with M split into = and X); rebuild_reference, the inverse of MD, which
does not go through tags(); the hand-built records and the seeded random records that the CPU and the GPU tests share; and the
packing of a list of records into the buffers the tag doors take.

t: the reference's bytes from the record's pos on.  q: the read as aligned (its reverse complement for flag 16), index 0 the
first CIGAR column, soft clips included.  cigar: [(op letter, length)]."""
import re

import numpy as np

OPS = "MIDNSHP=X"
_ACGT = b"ACGTacgt"


def is_match(t, q):
    """a column is a match iff both bytes are ACGT in either case and the same base"""
    return t in _ACGT and q in _ACGT and (t | 32) == (q | 32)


def L(b):
    """MD's letter: A-Z kept, a-z upper-cased, any other byte N"""
    return b if 65 <= b <= 90 else b - 32 if 97 <= b <= 122 else ord("N")


def l(b):
    """cs's letter: letters lower-cased, any other byte n"""
    return b if 97 <= b <= 122 else b + 32 if 65 <= b <= 90 else ord("n")


def tags(t, q, cigar):
    """-> (md bytes, cs bytes, split cigar); an empty CIGAR has no text at all"""
    if not cigar:
        return b"", b"", []
    md, cs, split = bytearray(), bytearray(), []
    c = r = x = 0
    for op, n in cigar:
        if op == "M":
            run, cols = 0, []
            for i in range(n):
                tb, qb = t[r + i], q[x + i]
                if is_match(tb, qb):
                    c += 1
                    run += 1
                    cols.append("=")
                else:
                    md += b"%d" % c + bytes([L(tb)])
                    c = 0
                    if run:
                        cs += b":%d" % run
                        run = 0
                    cs += b"*" + bytes([l(tb), l(qb)])
                    cols.append("X")
            if run:
                cs += b":%d" % run
            for ch in cols:
                if split and split[-1][0] == ch and split[-1][2]:
                    split[-1][1] += 1
                else:
                    split.append([ch, 1, True])
            if split:
                split[-1][2] = False  # a run ends with its M word
            r += n
            x += n
        elif op == "D":
            md += b"%d^" % c + bytes(L(b) for b in t[r:r + n])
            c = 0
            cs += b"-" + bytes(l(b) for b in t[r:r + n])
            split.append([op, n, False])
            r += n
        elif op == "I":
            cs += b"+" + bytes(l(b) for b in q[x:x + n])
            split.append([op, n, False])
            x += n
        elif op == "S":
            split.append([op, n, False])
            x += n
        else:
            raise ValueError(op)
    md += b"%d" % c
    return bytes(md), bytes(cs), [(op, n) for op, n, _ in split]


def collapse(cigar):
    """= and X back to M, adjacent M merged: the CIGAR before the split"""
    out = []
    for op, n in cigar:
        op = "M" if op in "=X" else op
        if out and out[-1][0] == op == "M":
            out[-1] = (op, out[-1][1] + n)
        else:
            out.append((op, n))
    return out


def nm_of(split):
    """X columns + I bases + D bases of a split CIGAR"""
    return sum(n for op, n in split if op in "XID")


def rebuild_reference(seq, cigar, md):
    """the aligned reference bytes (the M / = / X and D columns, in order) from SEQ as in the SAM line, its CIGAR and its MD: it
    must equal L() of the assembly's slice [pos, end)"""
    toks = re.findall(rb"\d+|\^[A-Z]+|[A-Z]", md)
    assert b"".join(toks) == md and toks and toks[0].isdigit(), md
    it = iter(toks[1:])
    rem, out, x = int(toks[0]), bytearray(), 0

    def number():
        tok = next(it)
        assert tok.isdigit(), md
        return int(tok)

    for op, n in cigar:
        if op in "M=X":
            for _ in range(n):
                if rem:
                    out.append(L(seq[x]))
                    rem -= 1
                else:
                    tok = next(it)
                    assert len(tok) == 1 and not tok.isdigit(), md
                    out += tok
                    rem = number()
                x += 1
        elif op == "D":
            assert rem == 0, md
            tok = next(it)
            assert tok[:1] == b"^" and len(tok) == n + 1, md
            out += tok[1:]
            rem = number()
        elif op in "IS":
            x += n
    assert rem == 0 and next(it, None) is None, md
    return bytes(out)


def words(cigar):
    return np.array([n << 4 | OPS.index(op) for op, n in cigar], np.uint32)


def cigar_of(w):
    return [(OPS[int(v) & 15], int(v) >> 4) for v in w]


# ---- records ---------------------------------------------------------------------------------------------------------------------
_B = np.frombuffer(b"ACGT", np.uint8)


def rand(n, seed):
    return bytearray(bytes(_B[np.random.default_rng(seed).integers(0, 4, n)]))


def other(ch, step=1):
    return b"ACGT"[(b"ACGT".index(bytes([ch]).upper()) + step) % 4]


def record(cigar, seed, subs=(), t_edit=None, q_edit=None):
    """a record whose M columns all match except at the M-column indices `subs` (counted over the M columns only, negative from
    the end); t_edit / q_edit(t, q) change the two sides afterwards"""
    n_m = sum(n for op, n in cigar if op == "M")
    core = rand(n_m, seed)
    t, q, at = bytearray(), bytearray(), 0
    for i, (op, n) in enumerate(cigar):
        if op == "M":
            t += core[at:at + n]
            q += core[at:at + n]
            at += n
        elif op == "D":
            t += rand(n, seed * 131 + i)
        else:
            q += rand(n, seed * 137 + i)
    cols_t, cols_q, tp, qp = [], [], 0, 0
    for op, n in cigar:
        if op == "M":
            cols_t += range(tp, tp + n)
            cols_q += range(qp, qp + n)
        if op in "MD":
            tp += n
        if op in "MIS":
            qp += n
    for s in subs:
        q[cols_q[s]] = other(t[cols_t[s]])
    if t_edit:
        t_edit(t, q)
    if q_edit:
        q_edit(t, q)
    return bytes(t), bytes(q), list(cigar)


def _set(side, at, val):
    def edit(t, q):
        (t if side == "t" else q)[at:at + len(val)] = val
    return edit


def hand_cases():
    """name -> (t, q, cigar): each the smallest shape at which one branch of the walk, or one step of the 64-lane kernels, can go
    wrong"""
    C = {}
    for n in (1, 63, 64, 65, 127, 128, 129, 4097):
        C[f"m{n}"] = record([("M", n)], n)
    for at in (0, 63, 64, -1):
        C[f"sub_at_{at}"] = record([("M", 129)], 200 + at, subs=[at])
    C["sub_63_64"] = record([("M", 129)], 210, subs=[63, 64])
    C["subs_130"] = record([("M", 130)], 220, subs=range(130))
    C["subs_130_inside"] = record([("M", 300)], 221, subs=range(90, 220))
    for n in (9, 10, 99, 100, 999, 1000, 9999, 10000):
        C[f"count_{n}"] = record([("M", n + 2)], 300 + n, subs=[0, -1])  # 0, a letter, the count, a letter, 0
    C["i_between"] = record([("M", 40), ("I", 3), ("M", 50)], 400)
    C["d_then_sub"] = record([("M", 10), ("D", 2), ("M", 10)], 401, subs=[10], t_edit=_set("t", 10, b"ACT"),
                             q_edit=lambda t, q: q.__setitem__(10, ord("G")))
    for n in (1, 70):
        C[f"d{n}"] = record([("M", 70), ("D", n), ("M", 70)], 410 + n)
        C[f"i{n}"] = record([("M", 70), ("I", n), ("M", 70)], 420 + n)
    C["d70_i70"] = record([("M", 5), ("D", 70), ("M", 3), ("I", 70), ("M", 5)], 430, subs=[5])
    C["clips"] = record([("S", 7), ("M", 66), ("S", 130)], 440, subs=[65])
    C["only_clip_and_m1"] = record([("S", 1), ("M", 1)], 441)
    C["lower_t"] = record([("M", 80), ("D", 3), ("M", 20)], 450, subs=[3, 70], t_edit=lambda t, q: t.__setitem__(slice(None), bytes(t).lower()))
    C["lower_q"] = record([("M", 80), ("I", 3), ("M", 20)], 451, subs=[3, 70], q_edit=lambda t, q: q.__setitem__(slice(None), bytes(q).lower()))
    C["n_against_n"] = record([("M", 70)], 460, t_edit=_set("t", 5, b"N"), q_edit=lambda t, q: (q.__setitem__(5, ord("N")), q.__setitem__(66, ord("n"))))
    C["odd_reference_bytes"] = record([("M", 70), ("D", 4), ("M", 10)], 470,
                                      t_edit=lambda t, q: (t.__setitem__(2, ord("R")), t.__setitem__(64, ord("*")), t.__setitem__(65, 0x80),
                                                           t.__setitem__(slice(70, 74), b"r*\x80N")))
    C["odd_read_bytes"] = record([("M", 20), ("I", 3), ("M", 10)], 471, q_edit=lambda t, q: (q.__setitem__(1, ord("-")), q.__setitem__(slice(20, 23), b"n.\xff")))
    C["adjacent_words"] = record([("M", 10), ("M", 5), ("D", 2), ("D", 1), ("I", 2), ("I", 1), ("M", 4)], 480, subs=[9, 10])
    C["empty"] = (b"", b"", [])
    return C


def random_records(n=200, seed=7, max_len=300):
    """seeded records: 1 .. 8 words of up to max_len columns, substitutions at one column in 12, now and then lower case, N and
    bytes that are no letters"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cigar = []
        if rng.random() < 0.3:
            cigar.append(("S", int(rng.integers(1, max_len + 1))))
        for w in range(int(rng.integers(1, 9))):
            op = "M" if w % 2 == 0 else "DI"[int(rng.integers(0, 2))]
            cigar.append((op, int(rng.integers(1, max_len + 1))))
        if cigar[-1][0] != "M":
            cigar.append(("M", int(rng.integers(1, max_len + 1))))
        if rng.random() < 0.3:
            cigar.append(("S", int(rng.integers(1, max_len + 1))))
        n_m = sum(k for op, k in cigar if op == "M")
        subs = sorted(set(int(v) for v in rng.integers(0, n_m, max(1, n_m // 12)))) if rng.random() < 0.9 else []
        t, q, cigar = record(cigar, 1000 + i, subs=subs)
        t, q = bytearray(t), bytearray(q)
        for side in (t, q):
            if len(side) and rng.random() < 0.3:
                for at in rng.integers(0, len(side), 3):
                    side[int(at)] = (ord("N"), ord("n"), ord("*"), 0x80, ord("R"), ord("a"), ord("t"))[int(rng.integers(0, 7))]
            if rng.random() < 0.1:
                side[:] = bytes(side).lower()
        out.append((bytes(t), bytes(q), cigar))
    return out


def pack(records, pad=3):
    """records -> (ref, reads, t_off, q_off, cigars as word arrays): the two buffers the tag doors take, `pad` foreign bytes
    between the records' stretches so that a walk that runs over reads something else than the next record's first byte"""
    ref, reads, t_off, q_off = bytearray(), bytearray(), [], []
    for t, q, _ in records:
        t_off.append(len(ref))
        q_off.append(len(reads))
        ref += t + b"#" * pad
        reads += q + b"%" * pad
    return bytes(ref), bytes(reads), t_off, q_off, [words(c) for _, _, c in records]


def expected(records):
    """the model's (md list, cs list, split word arrays)"""
    got = [tags(t, q, c) for t, q, c in records]
    return [g[0] for g in got], [g[1] for g in got], [words(g[2]) for g in got]
