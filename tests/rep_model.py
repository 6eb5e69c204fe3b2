"""A numpy restatement of the repetitive k-mer rule (include/np2_io.h: np2_rep_*), independent of the C++: canonical
indices of a separator stream, unique + counts over them, the threshold rule, the listed (index, count) pairs and their text.
The tests compare the one-lane host program and the device against it."""
import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _ch, _c in zip(b"ACGTU", (0, 1, 2, 3, 3)):
    _CODE[_ch] = _CODE[_ch | 0x20] = _c


def canonical_indices(stream, k):
    """the index min(fw, rv) of every window of k bases, in stream order (uint32)"""
    c = _CODE[np.frombuffer(bytes(stream), dtype=np.uint8)]
    m = len(c) - k + 1
    if m <= 0:
        return np.zeros(0, np.uint32)
    bad = np.concatenate([[0], np.cumsum(c == 4)])
    ok = (bad[k:] - bad[:m]) == 0
    b = (c & 3).astype(np.uint64)
    fw, rv = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    for j in range(k):
        w = b[j:j + m]
        fw |= w << np.uint64(2 * (k - 1 - j))
        rv |= (np.uint64(3) - w) << np.uint64(2 * j)
    return np.minimum(fw, rv)[ok].astype(np.uint32)


def threshold(counts, distinct=0.9998, min_count=None):
    """counts: one entry per index with count > 0"""
    if min_count is not None:
        return int(min_count)
    D = len(counts)
    if D == 0:
        return 0
    target = int(float(distinct) * float(D))  # IEEE double, truncated
    values, occ = np.unique(counts, return_counts=True)
    cum = np.cumsum(occ)
    return int(values[np.searchsorted(cum, target, side="left")])  # the first occurring value with cum >= target


def table(stream, k):
    """-> (index, count): the indices with count > 0 in ascending order and their counts"""
    return np.unique(canonical_indices(stream, k), return_counts=True)


def listed(index, count, distinct=0.9998, min_count=None):
    """a table -> (index, count, stats): the listed pairs in ascending index, and every np2_rep_stats_t field except the times"""
    thr = threshold(count, distinct, min_count)
    keep = count > thr
    li, lc = index[keep].astype(np.uint32), count[keep].astype(np.uint32)
    stats = {"kmers": int(count.sum()), "distinct": int(len(index)), "listed": int(len(li)), "listed_occurrences": int(lc.sum()),
             "threshold": thr, "max_count": int(count.max()) if len(count) else 0}
    return li, lc, stats


def rep(stream, k, distinct=0.9998, min_count=None):
    return listed(*table(stream, k), distinct=distinct, min_count=min_count)


def text(index, count, k, both=False):
    """the list as the text file has it"""
    out = []
    for v, c in zip(index.tolist(), count.tolist()):
        s = "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))
        out.append(f"{s}\t{c}\n")
        rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
        if both and rc != s:
            out.append(f"{rc}\t{c}\n")
    return "".join(out)
