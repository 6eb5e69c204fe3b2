"""The short-read adapter rule as plain Python, written from its statement in include/np2_io.h (not from the C++): the
yardstick of tests/test_sradapt_cpu.py and tests/test_gpu_sradapt.py.  Also the seeded pair generator and the hand-written
edge pairs both share.  The quality rule (steps 1 - 3, the classes, the mask) is tests/srqc_model.py's.

  A base byte is case-folded; A/T and C/G are complements; any other byte is unknown and matches nothing.
  A. pair overlap: x = r1[a1:b1], y = r2[a2:b2], rcy = reverse complement of y.  For a shift s, x[i] faces rcy[i - s] over
     i in [max(0, s), min(n1, n2 + s)): l(s) positions, d(s) of them unknown or different.  Accepted: l(s) >= O and
     d(s) <= min(D, P * l(s) // 100).  Order s = 0, 1, 2, .., then -1, -2, ..; the first accepted wins.  T = n2 + s,
     b1 = a1 + min(n1, T), b2 = a2 + min(n2, T).  No search when a span is longer than 1024 or shorter than O.
  B. by sequence (reads A did not decide, spans of 4 .. 1024 bases): p = 0 .. n - 4, c = min(n - p, A), m(p) mismatches over c
     letters; the smallest p with m(p) <= c // 8 wins, b = a + p.
  C. the quality rule's classes over the new spans; in a pair the mate of a single failing read gets class 4."""
import numpy as np

import srqc_model as sm

DEFAULTS = dict(pair=True, overlap=30, diff=5, diffpct=20, seq=None, seq2=None)
STAT_NAMES = sm.STAT_NAMES + ("mate_failed", "pairs", "pairs_overlap", "pairs_unsearched", "trimmed_overlap", "trimmed_seq", "adapter_bases")
CLASS_NAMES = ("pass", "too_short", "too_many_n", "low_quality", "mate_failed")
MAX_SPAN = 1024
# the Illumina TruSeq read-through sequences (public; fastp's documentation names them)
ADAPTER1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ADAPTER2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"

_CODE = np.full(256, 4, np.uint8)  # A 0, C 1, G 2, T 3; 4: unknown
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i


def adopts(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def codes(s):
    return _CODE[np.frombuffer(s, np.uint8)]


def revcomp(s):
    return bytes(s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1])


def _diagonal_sums(m):
    """m: (r, c) of 0 / 1 -> v[s] = sum over j of m[j + s, j], s = 0 .. r - 1"""
    r, c = m.shape
    pad = np.zeros((r + c, c), np.int64)
    pad[:r] = m
    sr, sc = pad.strides
    return np.lib.stride_tricks.as_strided(pad, shape=(c, r), strides=(sr + sc, sr)).sum(axis=0)


def find_overlap(x, y, o):
    """the accepted shift, or None"""
    n1, n2, O, D, P = len(x), len(y), o["overlap"], o["diff"], o["diffpct"]
    if n1 > MAX_SPAN or n2 > MAX_SPAN or n1 < O or n2 < O:
        return None
    cx, cy = codes(x), codes(y)
    rc = np.where(cy < 4, 3 - cy, 4)[::-1]
    differ = ((cx[:, None] != rc[None, :]) | (cx[:, None] == 4) | (rc[None, :] == 4)).astype(np.int64)  # [i, j]: x[i] against rcy[j]
    fwd = _diagonal_sums(differ)  # s >= 0: x[j + s] faces rcy[j]
    for s in range(0, n1 - O + 1):
        ln = min(n1, n2 + s) - s
        if ln >= O and fwd[s] <= min(D, P * ln // 100):
            return s
    bwd = _diagonal_sums(differ.T)  # s = -t: x[i] faces rcy[i + t]
    for t in range(1, n2 - O + 1):
        ln = min(n1, n2 - t)
        if ln >= O and bwd[t] <= min(D, P * ln // 100):
            return -t
    return None


def find_adapter(r, adapter):
    """the winning p, or None"""
    n = len(r)
    if adapter is None or n < 4 or n > MAX_SPAN:
        return None
    ad = codes(adapter.encode())
    A = len(ad)
    padded = np.concatenate([codes(r), np.full(A, 5, np.uint8)])
    win = np.lib.stride_tricks.sliding_window_view(padded, A)[:n - 3]  # [p, j] = read[p + j]
    c = np.minimum(n - np.arange(n - 3), A)
    m = ((win != ad[None, :]) & (np.arange(A)[None, :] < c[:, None])).sum(axis=1)
    hit = np.flatnonzero(m <= c // 8)
    return int(hit[0]) if len(hit) else None


def _cls(s, q, a, b, qc):
    """step 4 of the quality rule over [a, b)"""
    p = np.maximum(np.frombuffer(q, np.uint8).astype(np.int64) - 33, 0)[a:b]
    sb = np.frombuffer(s, np.uint8)[a:b]
    ln, n_n, lowq = b - a, int(((sb == ord("N")) | (sb == ord("n"))).sum()), int((p < qc["qualified_q"]).sum())
    if ln < qc["min_len"] or ln == 0:
        return 1
    if n_n > qc["n_base_limit"]:
        return 2
    if 100 * lowq > qc["unqualified_percent"] * ln:
        return 3
    return 0


def _by_seq(s, a, b, adapter):
    p = find_adapter(s[a:b], adapter)
    return (b, 0) if p is None else (a + p, 2)


def judge_pair(r1, r2, qc, o):
    """two (s, q) -> two (begin, end, cls, how, insert)"""
    (s1, q1), (s2, q2) = r1, r2
    a1, b1, _ = sm.judge(s1, q1, qc)
    a2, b2, _ = sm.judge(s2, q2, qc)
    n1, n2 = b1 - a1, b2 - a2
    s = find_overlap(s1[a1:b1], s2[a2:b2], o)
    h1 = h2 = ins = 0
    if s is not None:
        ins = n2 + s
        if min(n1, ins) < n1:
            b1, h1 = a1 + ins, 1
        if min(n2, ins) < n2:
            b2, h2 = a2 + ins, 1
    else:
        b1, h1 = _by_seq(s1, a1, b1, o["seq"])
        b2, h2 = _by_seq(s2, a2, b2, o["seq2"] if o["seq2"] is not None else o["seq"])
    c1, c2 = _cls(s1, q1, a1, b1, qc), _cls(s2, q2, a2, b2, qc)
    if c1 != 0 and c2 == 0:
        c2 = 4
    elif c2 != 0 and c1 == 0:
        c1 = 4
    return (a1, b1, c1, h1, ins), (a2, b2, c2, h2, ins)


def judge_single(r, qc, o):
    s, q = r
    a, b, _ = sm.judge(s, q, qc)
    b, h = _by_seq(s, a, b, o["seq"])
    return a, b, _cls(s, q, a, b, qc), h, 0


def run(reads, qc, o):
    """reads: [(s, q)] (pair mode: mates adjacent) -> (results [(a, b, cls, how, insert)], masked stream, totals dict)"""
    res = []
    t = dict.fromkeys(STAT_NAMES, 0)
    if o["pair"]:
        assert len(reads) % 2 == 0
        for i in range(0, len(reads), 2):
            res.extend(judge_pair(reads[i], reads[i + 1], qc, o))
            spans = [sm.judge(s, q, qc) for s, q in reads[i:i + 2]]
            t["pairs"] += 1
            t["pairs_overlap"] += res[-1][4] != 0
            t["pairs_unsearched"] += any(b - a > MAX_SPAN for a, b, _ in spans)
    else:
        res = [judge_single(r, qc, o) for r in reads]
    out = []
    for (s, q), (a, b, cls, how, _) in zip(reads, res):
        out.append(b"N" * a + s[a:b] + b"N" * (len(s) - b) if cls == 0 else b"N" * len(s))
        t["reads"] += 1
        t[CLASS_NAMES[cls]] += 1
        t["bases_in"] += len(s)
        t["bases_out"] += b - a if cls == 0 else 0
        t["trimmed_overlap"] += how == 1
        t["trimmed_seq"] += how == 2
        t["adapter_bases"] += sm.judge(s, q, qc)[1] - b
    return res, b"".join(x + b"\n" for x in out), {k: int(v) for k, v in t.items()}


def clean_stream(reads, qc, o):
    """the kept substrings of the passing reads as reads of their own: what counting the masked stream must equal"""
    res, _, _ = run(reads, qc, o)
    return b"".join(s[a:b] + b"\n" for (s, _), (a, b, cls, _, _) in zip(reads, res) if cls == 0)


def clean_fastq_pair(rec1, rec2, qc, o):
    """two lists of (header, s, q) in step -> the two cleaned FASTQ texts: a pair is written only when both mates pass"""
    out1, out2 = [], []
    for (h1, s1, q1), (h2, s2, q2) in zip(rec1, rec2):
        r1, r2 = judge_pair((s1, q1), (s2, q2), qc, o)
        if r1[2] == 0 and r2[2] == 0:
            out1.append(h1 + b"\n" + s1[r1[0]:r1[1]] + b"\n+\n" + q1[r1[0]:r1[1]] + b"\n")
            out2.append(h2 + b"\n" + s2[r2[0]:r2[1]] + b"\n+\n" + q2[r2[0]:r2[1]] + b"\n")
    return b"".join(out1), b"".join(out2)


# ---- the generator -------------------------------------------------------------------------------------------------------------
M = 150
UNEQUAL = [(100, 150), (150, 75), (0, 150)]


def special_inserts(O=30, m=M):
    return [0, 1, O - 1, O, O + 1, m - 1, m, m + 1, 2 * m - O - 1, 2 * m - O, 2 * m - O + 1, 3 * m]


def _qualities(rng, prof, n):
    """srqc_model.generate's five profiles: good; bad; bad ends; values around the thresholds; 18 .. 22 throughout"""
    if prof == 0:
        return rng.integers(30, 41, size=n)
    if prof == 1:
        return rng.integers(2, 16, size=n)
    if prof == 2:
        p = rng.integers(30, 41, size=n)
        e1, e2 = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        p[:e1] = rng.integers(2, 19, size=min(e1, n))
        if e2:
            p[max(0, n - e2):] = rng.integers(2, 19, size=min(e2, n))
        return p
    if prof == 3:
        return rng.choice(np.array([2, 19, 20, 21, 40]), size=n)
    return rng.integers(18, 23, size=n)


def generate(n_pairs=4000, seed=21):
    """-> (reads [(s, q)] with mates adjacent, meta [dict(insert, m1, m2, clean)]).  Pair i cuts an insert of I bases from a
    random 30 kb genome (even i: special_inserts() in turn; odd i: random 0 .. 450) and reads m1 bases from its start and m2
    from the other strand's; past the insert's end a read goes on into ADAPTER1 / ADAPTER2 and then random bases.  m1 = m2 =
    150 except every tenth pair (UNEQUAL in turn).  Profile i % 7 % 5 of the qualities (two pairs in seven good, one in seven
    bad), 2 % N in all profiles but the first; every third pair has 1 % substitutions.  clean: no N, no substitution."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.choice(acgt, size=30000).tobytes()
    special = special_inserts()
    reads, meta = [], []
    for i in range(n_pairs):
        ins = special[(i // 2) % len(special)] if i % 2 == 0 else int(rng.integers(0, 451))
        m1, m2 = UNEQUAL[(i // 10) % 3] if i % 10 == 9 else (M, M)
        at = int(rng.integers(0, len(genome) - ins))
        frag = genome[at:at + ins]
        prof = i % 7 % 5
        clean = True
        pair = []
        for frag_s, adapter, m in ((frag, ADAPTER1, m1), (revcomp(frag), ADAPTER2, m2)):
            s = np.frombuffer((frag_s + adapter.encode() + rng.choice(acgt, size=M).tobytes())[:m], np.uint8).copy()
            if i % 3 == 2:
                err = rng.random(m) < 0.01
                s[err] = rng.choice(acgt, size=int(err.sum()))
                clean = False
            if prof != 0:
                s = np.where(rng.random(m) < 0.02, np.uint8(ord("n") if i % 11 == 0 else ord("N")), s)
                clean = False
            pair.append((s.astype(np.uint8).tobytes(), (_qualities(rng, prof, m) + 33).astype(np.uint8).tobytes()))
        reads.extend(pair)
        meta.append(dict(insert=ins, m1=m1, m2=m2, clean=clean, frag=frag))
    return reads, meta


def guard(reads, qc, o):
    """what the generator exercises under (qc, o): pairs with an accepted s < 0, s = 0, s > 0 without a trim, no accepted s;
    reads of class 4; reads with how == 2"""
    res, _, _ = run(reads, qc, o)
    neg = zero = pos_untrimmed = none = 0
    for i in range(0, len(reads), 2):
        (a1, _, _, h1, ins), (a2, _, _, h2, _) = res[i], res[i + 1]
        if ins == 0:
            none += 1
            continue
        n2 = sm.judge(*reads[i + 1], qc)
        s = ins - (n2[1] - n2[0])
        neg += s < 0
        zero += s == 0
        pos_untrimmed += s > 0 and h1 == 0 and h2 == 0
    return dict(neg=neg, zero=zero, pos_untrimmed=pos_untrimmed, none=none, cls4=sum(r[2] == 4 for r in res), how2=sum(r[3] == 2 for r in res))


# ---- hand-written pairs ----------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tobytes()


def _subst(s, positions):
    b = bytearray(s)
    for p in positions:
        b[p] = ord({"A": "C", "C": "G", "G": "T", "T": "A"}[chr(b[p])])
    return bytes(b)


def _good(s, ch=b"I"):
    return s, ch * len(s)


def _facing(x, rcy):
    """the pair whose mate 1 is x and whose mate 2's reverse complement is rcy"""
    return [_good(x), _good(revcomp(rcy))]


EDGE_ADAPTER = "AGATCGGAAGAGC"
EDGE_ADAPTER_4 = "AGAT"
EDGE_ADAPTER_64 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCACTTAGGCATCTCGTATGCCGTCTTCTGCTTG"
assert len(EDGE_ADAPTER_64) == 64


def edge_pairs(seed=3):
    """[(s, q)] with mates adjacent.  The cases are written for NEUTRAL quality options (a case's comment says which adapter
    options it is about); under any other options they are pairs like any others."""
    rng = np.random.default_rng(seed)
    out = []
    spread = [1, 6, 11, 16, 21, 26, 3, 8, 13, 18, 23, 28]
    # d at the limit and one above.  l = 30: D = 5 binds under D=5,P=20 (5 | 6), P binds under D=10,P=20 (6 | 7)
    r30 = _rand(rng, 30)
    for k in (5, 6, 7):
        out += _facing(r30, _subst(r30, spread[:k]))
    # l = 49 under D=10,P=20: P binds, 9 | 10
    r49 = _rand(rng, 49)
    for k in (9, 10):
        out += _facing(r49, _subst(r49, [4 * j + 1 for j in range(k)]))
    # an unknown base inside the overlap counts as a difference: 4 + N accepted, 5 + N refused, on either side
    for k in (4, 5):
        xn = bytearray(_subst(r30, spread[:k]))
        xn[15] = ord("N")
        out += _facing(bytes(xn), r30)
        y = bytearray(revcomp(_subst(r30, spread[:k])))
        y[9] = ord("n")
        out += [_good(r30), _good(bytes(y))]
    # many shifts qualify: the order picks s = 0 (and trims the longer mate 1), or the smallest accepted s > 0
    out += _facing(b"A" * 60, b"A" * 60)
    out += _facing(b"A" * 80, b"A" * 60)
    out += _facing(b"AC" * 40, b"AC" * 40)
    out += _facing(b"AC" * 40, b"CA" * 40)
    out += _facing(b"ac" * 40, b"CA" * 20)
    # s > 0 with n1 > T: mate 1 alone is trimmed
    g = _rand(rng, 120)
    out += _facing(g, g[20:80])
    # s < 0: read-through, both trimmed to the insert
    ins = _rand(rng, 70)
    out += [_good(ins + ADAPTER1.encode()[:30]), _good(revcomp(ins) + ADAPTER2.encode()[:30])]
    # kept spans at the cap
    for n in (1023, 1024, 1025):
        big = _rand(rng, n)
        out += _facing(big, big)
        out += _facing(big, big[:150])
        out += _facing(big[:150], big)
    # an empty mate, two empty mates
    out += [_good(b""), _good(g)]
    out += [_good(g), _good(b"")]
    out += [_good(b""), _good(b"")]
    # one mate failing each class under the recipe, the other passing: class 4
    other = _rand(rng, 100)
    out += [_good(_rand(rng, 20)), _good(other)]                                                  # too short after the trims
    nn = bytearray(_rand(rng, 100))
    nn[50] = ord("N")
    out += [_good(other), _good(bytes(nn))]                                                       # too many N
    out += [(_rand(rng, 100), b"I4" * 50), _good(other)]                                          # low quality
    # by sequence (no overlap: the mates are unrelated)
    ad = EDGE_ADAPTER.encode()
    body = _rand(rng, 60)
    out += [_good(ad + body), _good(other)]                                                       # p = 0
    out += [_good(body + ad[:4]), _good(other)]                                                   # p = n - 4
    out += [_good(body[:50] + ad[:10]), _good(other)]                                             # c < A at the end
    out += [_good(body[:50] + _subst(ad[:10], [3])), _good(other)]                                # c = 10: one mismatch allowed
    out += [_good(body[:50] + _subst(ad[:10], [3, 7])), _good(other)]                             # ... two are not
    out += [_good(body[:40] + _subst(ad, [5]) + body[40:]), _good(other)]                         # c = 13: 1 | 2
    out += [_good(body[:40] + _subst(ad, [5, 9]) + body[40:]), _good(other)]
    a64 = EDGE_ADAPTER_64.encode()
    out += [_good(body[:30] + _subst(a64, [2, 12, 22, 32, 42, 52, 62, 7]) + body[30:]), _good(other)]  # c = 64: 8 | 9
    out += [_good(body[:30] + _subst(a64, [2, 12, 22, 32, 42, 52, 62, 7, 17]) + body[30:]), _good(other)]
    out += [_good(other), _good(body[:30].lower() + a64.lower())]                                  # lower case, mate 2
    out += [_good(b"ACG"), _good(b"AGAT")]                                                         # n < 4, n = 4
    # every mate start at each byte offset of a word: lead pairs of 0 .. 3 bases in front of a read-through pair and a
    # by-sequence pair
    for lead in range(4):
        out += [_good(b"ACG"[:lead]), _good(b"")]
        out += [_good(ins + ADAPTER1.encode()[:31]), _good(revcomp(ins) + ADAPTER2.encode()[:29])]
        out += [_good(body[:41] + ad), _good(other[:50] + ad[:7])]
    return out


def text_case(reads, qc, o):
    """the input of tests/tools/sradapt_core_test.cpp"""
    flags = (1 if qc["cut_front"] else 0) | (2 if qc["cut_tail"] else 0)
    head = [qc["trim_front"], qc["trim_tail"], qc["cut_window"], qc["cut_mean_q"], qc["n_base_limit"], qc["qualified_q"],
            qc["unqualified_percent"], qc["min_len"], flags, 1 if o["pair"] else 0, o["overlap"], o["diff"], o["diffpct"], o["seq"] or "-", o["seq2"] or "-"]
    return " ".join(str(x) for x in head).encode() + b"\n" + b"".join(s + b"\n" + q + b"\n" for s, q in reads)
