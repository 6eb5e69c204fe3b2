"""A numpy restatement of the mapper's weighted minimizer order (include/np2_io.h: np2_map_*, "Weights"), written from the
rule's text: a listed k-mer is ordered by key = M - s(s(s(M - h))), s(y) = y * y >> 2k, an unlisted one by its hash, and a
window's minimum is that of (key, h, position).  Everything else is tests/map_model.py's: this module swaps that model's
`sketch` for the weighted one while an index is built or reads are mapped, and touches nothing besides.  Also the list file's
rule (parse_list) and the canonical index of a k-mer's text."""
import contextlib
import gzip

import numpy as np

import map_model as mm

KW_MIN, KW_MAX = 11, 15
_LETTER = {c: i for i, c in enumerate("ACGT")}
_LETTER.update({c.lower(): i for c, i in list(_LETTER.items())})
_LETTER.update(U=3, u=3)


def index_of(kmer):
    """the canonical index v = min(fw, rv) of a k-mer's text (ACGTU in either case); ValueError for another letter"""
    fw = rv = 0
    k = len(kmer)
    for j, ch in enumerate(kmer):
        if ch not in _LETTER:
            raise ValueError(f"bad letter {ch!r}")
        c = _LETTER[ch]
        fw = fw << 2 | c
        rv |= (3 - c) << (2 * j)
    return min(fw, rv)


def text_of(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k))


def revcomp_index(v, k):
    r = 0
    for j in range(k):
        r = r << 2 | (3 - ((v >> (2 * j)) & 3))
    return r


def parse_list(data):
    """the list file's bytes (plain or gzip) -> (kw, sorted unique canonical indices); ValueError("line N: ...") as the rule
    says.  An empty file is (0, [])."""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    k, out = 0, set()
    for no, ln in enumerate(lines, 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        kmer = ln.split(b"\t", 1)[0].decode("latin-1")
        try:
            v = index_of(kmer)
        except ValueError as e:
            raise ValueError(f"line {no}: {e}")
        if k == 0:
            k = len(kmer)
        if len(kmer) != k or k == 0:
            raise ValueError(f"line {no}: length {len(kmer)}, not {k}")
        out.add(v)
    return k, sorted(out)


def kmers_v(seq, k):
    """per byte i: (ok, v, h, strand) of the k-mer that ends there; v = min(fw, rv), h = hash(v), or 2^64 - 1 where fw == rv"""
    c = mm._CODE[np.frombuffer(bytes(seq), np.uint8)]
    n = len(c)
    idx = np.arange(n)
    last_bad = np.maximum.accumulate(np.where(c < 4, -1, idx))
    ok = (idx - last_bad) >= k
    fw, rv = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    c64 = (c & 3).astype(np.uint64)
    for j in range(min(k, n)):
        sh = np.zeros(n, np.uint64)
        sh[j:] = c64[:n - j] if j else c64
        fw |= sh << np.uint64(2 * j)
        rv |= (np.uint64(3) - sh) << np.uint64(2 * (k - 1 - j))
    v = np.minimum(fw, rv)
    h = np.where(fw == rv, mm._INF, mm.hash64(v, (1 << (2 * k)) - 1))
    return ok, v, h, (fw > rv).astype(np.uint8)


def key_of(h, listed, k):
    """the ordering key of hashes h (uint64 array, h <= M) whose k-mers are listed where `listed` says so"""
    M = np.uint64((1 << (2 * k)) - 1)
    sh = np.uint64(2 * k)
    y = M - h
    for _ in range(3):
        y = (y * y) >> sh  # y < 2^30: the product is below 2^60
    return np.where(listed, M - y, h)


def sketch(seq, k, w, L):
    """map_model.sketch under the weight set L (a sorted uint64 array of canonical indices): (h, end position, strand)"""
    ok, v, h, strand = kmers_v(seq, k)
    n = len(ok)
    pal = h == mm._INF
    hh = np.where(pal, np.uint64(0), h)
    key = key_of(hh, np.isin(v, L), k)
    order = np.where(pal, mm._INF, (key << np.uint64(2 * k)) | hh)  # (key, h) as one integer below 2^60
    chosen = np.zeros(n, bool)
    edge = np.diff(np.concatenate(([0], ok.astype(np.int8), [0])))
    for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
        if b - a < w:
            continue
        win = np.lib.stride_tricks.sliding_window_view(order[a:b], w)
        arg = win.argmin(axis=1)  # the first of equal values: the leftmost
        at = a + np.arange(len(arg)) + arg
        chosen[at[~pal[at]]] = True
    pos = np.flatnonzero(chosen)
    return h[pos], pos.astype(np.int64), strand[pos]


def weight_array(L):
    return np.unique(np.asarray(sorted(L) if not isinstance(L, np.ndarray) else L, np.uint64))


@contextlib.contextmanager
def weighted(L):
    """inside: map_model sketches under L (an empty L: map_model as it stands)"""
    L = weight_array(L)
    if len(L) == 0:
        yield
        return
    plain = mm.sketch
    mm.sketch = lambda seq, k, w: sketch(seq, k, w, L)
    try:
        yield
    finally:
        mm.sketch = plain


def Index(seqs, k, w, L):
    with weighted(L):
        return mm.Index(seqs, k, w)


def map_reads(index, reads, L, info=None, **kw):
    with weighted(L):
        return mm.map_reads(index, reads, info=info, **kw)
