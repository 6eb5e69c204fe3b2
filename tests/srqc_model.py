"""The short-read quality rule as plain Python, written from its statement in include/np2_io.h (not from the C++): the
yardstick of tests/test_srqc_cpu.py and tests/test_gpu_srqc.py.  Also the seeded read generator both share.

One read: n bases s, n quality bytes, p[i] = max(0, byte - 33).
  1. a = min(trim_front, n), b = max(a, n - trim_tail)
  2. cut_front (b > a): smallest i, a <= i, i + W <= b, sum p[i:i+W] >= M * W; none: a = b; else a = i, then skip N / n
  3. cut_tail (b > a): largest j, j <= b, j - W >= a, sum p[j-W:j] >= M * W; none: b = a; else b = j, then skip N / n back
  4. class: 1 if len < min_len or len == 0; 2 if nN > n_base_limit; 3 if 100 * lowq > U * len; else 0
  5. masked stream: failed reads and the bases of passing reads outside [a, b) become 'N'"""
import numpy as np

U32 = 2 ** 32 - 1
RECIPE = dict(trim_front=5, trim_tail=5, cut_front=True, cut_tail=True, cut_window=4, cut_mean_q=20, n_base_limit=0, qualified_q=20,
              unqualified_percent=40, min_len=15)
# every step switched off: each read passes whole
NEUTRAL = dict(trim_front=0, trim_tail=0, cut_front=False, cut_tail=False, cut_window=4, cut_mean_q=20, n_base_limit=U32, qualified_q=0,
               unqualified_percent=100, min_len=0)
# one option alone on top of NEUTRAL
SINGLES = [dict(trim_front=5), dict(trim_tail=5), dict(cut_front=True), dict(cut_tail=True), dict(n_base_limit=0),
           dict(qualified_q=20, unqualified_percent=40), dict(min_len=15)]
STAT_NAMES = ("reads", "pass", "too_short", "too_many_n", "low_quality", "bases_in", "bases_out")


def opts(base=None, **kw):
    o = dict(RECIPE if base is None else base)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def judge(s, q, o):
    """(a, b, class) of one read; s, q: bytes of equal length"""
    n = len(s)
    assert len(q) == n
    p = np.maximum(np.frombuffer(q, dtype=np.uint8).astype(np.int64) - 33, 0)
    sb = np.frombuffer(s, dtype=np.uint8)
    is_n = (sb == ord("N")) | (sb == ord("n"))
    W, M = o["cut_window"], o["cut_mean_q"]
    a = min(o["trim_front"], n)
    b = max(a, n - o["trim_tail"])
    c = np.concatenate([[0], np.cumsum(p)])
    if o["cut_front"] and b > a:
        hit = np.flatnonzero(c[a + W:b + 1] - c[a:b + 1 - W] >= M * W) if b - a >= W else []
        if len(hit) == 0:
            a = b
        else:
            a += int(hit[0])
            while a < b and is_n[a]:
                a += 1
    if o["cut_tail"] and b > a:
        hit = np.flatnonzero(c[a + W:b + 1] - c[a:b + 1 - W] >= M * W) if b - a >= W else []
        if len(hit) == 0:
            b = a
        else:
            b = a + int(hit[-1]) + W
            while b > a and is_n[b - 1]:
                b -= 1
    ln, n_n, lowq = b - a, int(is_n[a:b].sum()), int((p[a:b] < o["qualified_q"]).sum())
    if ln < o["min_len"] or ln == 0:
        cls = 1
    elif n_n > o["n_base_limit"]:
        cls = 2
    elif 100 * lowq > o["unqualified_percent"] * ln:
        cls = 3
    else:
        cls = 0
    return a, b, cls


def run(reads, o):
    """reads: [(s, q)] -> (results [(a, b, cls)], masked separator stream, totals dict)"""
    res, out = [], []
    t = dict.fromkeys(STAT_NAMES, 0)
    for s, q in reads:
        a, b, cls = judge(s, q, o)
        res.append((a, b, cls))
        out.append(b"N" * a + s[a:b] + b"N" * (len(s) - b) if cls == 0 else b"N" * len(s))
        t["reads"] += 1
        t[STAT_NAMES[1 + cls]] += 1
        t["bases_in"] += len(s)
        t["bases_out"] += b - a if cls == 0 else 0
    return res, b"".join(x + b"\n" for x in out), t


def clean_stream(reads, o):
    """the kept substrings as reads of their own: what counting the masked stream must equal"""
    res, _, _ = run(reads, o)
    return b"".join(s[a:b] + b"\n" for (s, _), (a, b, cls) in zip(reads, res) if cls == 0)


def clean_fastq(records, o):
    """records: [(header line without newline, s, q)] -> the cleaned FASTQ text"""
    out = []
    for h, s, q in records:
        a, b, cls = judge(s, q, o)
        if cls == 0:
            out.append(h + b"\n" + s[a:b] + b"\n+\n" + q[a:b] + b"\n")
    return b"".join(out)


def streams(reads):
    return b"".join(s + b"\n" for s, _ in reads), b"".join(q + b"\n" for _, q in reads)


def fastq(reads, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, q) for i, (s, q) in enumerate(reads))


# ---- the generator -------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 5, 9, 10, 11, 14, 15, 16, 24, 25, 26, 63, 64, 65, 127, 128, 129, 150, 255, 256, 257, 1000, 5000]
N_LIMITS = (0, 1, 5)  # read i is judged under n_base_limit = N_LIMITS[i % 3] wherever the mixture is asked for


def generate(n_reads=5000, seed=20):
    """Five quality profiles by i % 5 (good; bad; bad ends; values around the thresholds {2, 19, 20, 21, 40}; 18 .. 22
    throughout), 2 % N in all but the first, lengths from LENGTHS (even i, in turn) or random 0 .. 300 (odd i).  The bases
    are stretches of one random 30 kb sequence, so that k-mers repeat and a count threshold above 1 keeps some."""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=30000)
    reads = []
    for i in range(n_reads):
        n = LENGTHS[(i // 2) % len(LENGTHS)] if i % 2 == 0 else int(rng.integers(0, 301))
        at = int(rng.integers(0, len(genome) - n))
        s = genome[at:at + n]
        prof = i % 5
        if prof == 0:
            p = rng.integers(30, 41, size=n)
        elif prof == 1:
            p = rng.integers(2, 16, size=n)
        elif prof == 2:
            p = rng.integers(30, 41, size=n)
            e1, e2 = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            p[:e1] = rng.integers(2, 19, size=min(e1, n))
            if e2:
                p[max(0, n - e2):] = rng.integers(2, 19, size=min(e2, n))
        elif prof == 3:
            p = rng.choice(np.array([2, 19, 20, 21, 40]), size=n)
        else:
            p = rng.integers(18, 23, size=n)
        if prof != 0:
            s = np.where(rng.random(n) < 0.02, np.uint8(ord("n") if i % 7 == 0 else ord("N")), s)
        reads.append((s.astype(np.uint8).tobytes(), (p + 33).astype(np.uint8).tobytes()))
    return reads


def mixture(reads):
    """[(a, b, cls)] with read i under the recipe and n_base_limit = N_LIMITS[i % 3]"""
    os_ = [opts(n_base_limit=v) for v in N_LIMITS]
    return [judge(s, q, os_[i % 3]) for i, (s, q) in enumerate(reads)]


def guard(reads):
    """what the mixture exercises: classes, front cuts, tail cuts and emptied reads"""
    o = opts()
    res = mixture(reads)
    classes = [sum(1 for r in res if r[2] == c) for c in range(4)]
    cut_front = cut_tail = emptied = 0
    for (s, q), (a, b, cls) in zip(reads, res):
        n = len(s)
        a0 = min(o["trim_front"], n)
        b0 = max(a0, n - o["trim_tail"])
        if cls == 0 and a > a0:
            cut_front += 1
        if cls == 0 and b < b0:
            cut_tail += 1
        if n > 10 and b0 > a0 and a == b:
            emptied += 1
    return classes, cut_front, cut_tail, emptied


def edge_reads():
    """hand-written reads around every boundary of the rule (the core program's cases, as data)"""
    good, bad = b"I", b"#"  # phred 40, 2
    out = [(b"", b""), (b"A", good), (b"ACG", good * 3), (b"ACGT", good * 4), (b"ACGTA", good * 5)]
    for pos in range(12):  # a single bad base at each position of a 12-base read
        out.append((b"ACGTACGTACGT", good * pos + bad + good * (11 - pos)))
    body = b"ACGTACGTACGTACGTACGTACGTACGTAC"
    out.append((body[:5] + b"NN" + body[7:], bad * 5 + good * 25))            # N directly after the front cut
    out.append((body[:23] + b"Nn" + body[25:], good * 25 + bad * 5))          # N directly before the tail cut
    out.append((b"N" * 30, good * 30))
    out.append((body, bad * 30))
    out.append((body[:14] + b"N" + body[15:], good * 30))                     # one N: the limit 0 and 1
    for low in (7, 8, 9):                                                     # 100 * lowq against 40 * 20
        out.append((body[:20] + b"ACGTACGTAC", good * 5 + b"4" * low + good * (20 - low) + good * 5))
    for n in (23, 24, 25, 26):                                                # len around min_len = 15 after the trims
        out.append((body[:n], good * n))
    out.append((body, bytes([0x20]) * 10 + bytes([0x7E]) * 10 + bytes([0x21]) * 10))  # bytes below '!' and at the top
    for n in (999, 1000, 1001, 1009, 1010, 1011):                             # W = 1000: W - 1, W, W + 1 with and without the trims
        out.append(((body * 34)[:n], good * n))
    return out
