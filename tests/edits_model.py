"""Plain Python model of the edit rule in include/np2.h (np2_edits_*), written from the rule's six paragraphs and not from
the kernels: clean positions -> raw runs -> trimming -> kinds -> left-alignment -> k-mer support.  Slow on purpose."""
import bisect

import numpy as np

KINDS = ("SNV", "MNV", "INS", "DEL", "CPX")


def _up(b):
    return bytes(b).upper()  # (ASCII letters only: what "without regard to case" means in the rule)


def kind_of(ref, alt):
    if len(ref) == 1 and len(alt) == 1:
        return "SNV"
    if len(ref) == len(alt) and len(ref) > 1:
        return "MNV"
    if not ref:
        return "INS"
    if not alt:
        return "DEL"
    return "CPX"


def edits(ref, bases, pos):
    """-> (records, totals).  A record: dict(ref_pos, out_off, ref, alt, kind) after the shift, unanchored.  Raises
    ValueError where the entry point answers NP2_E_ARG."""
    ref, bases = bytes(ref), bytes(bases)
    pos = [int(p) for p in pos]
    L, n = len(ref), len(bases)
    assert len(pos) == n
    if any(p >= L for p in pos):
        raise ValueError("a position is not below the contig's length")
    if any(pos[i] > pos[i + 1] for i in range(n - 1)):
        raise ValueError("the positions decrease somewhere")
    totals = dict(has_span=0, first=0, last=0, raw_runs=0, same_runs=0, n_kind=[0] * 5, bases_inserted=0, bases_deleted=0, outside=L)
    if n == 0:
        return [], totals
    first, last = pos[0], pos[-1]
    totals.update(has_span=1, first=first, last=last, outside=L - (last - first + 1))
    U, B = _up(ref), _up(bases)
    groups = {}
    for i, p in enumerate(pos):
        groups.setdefault(p, []).append(i)

    def clean(p):
        g = groups.get(p, [])
        return len(g) == 1 and B[g[0]] == U[p]

    def first_out_at_or_after(s):
        return bisect.bisect_left(pos, s)  # (pos is sorted: the index of the first output base with pos >= s)

    recs = []
    prev_end = first
    p = first
    while p <= last:
        if clean(p):
            p += 1
            continue
        s = p
        while p + 1 <= last and not clean(p + 1):
            p += 1
        e = p
        p += 1
        totals["raw_runs"] += 1
        o_s = first_out_at_or_after(s)
        alt_idx = [i for q in range(s, e + 1) for i in groups.get(q, [])]
        assert alt_idx == list(range(o_s, o_s + len(alt_idx)))
        r, a = list(range(s, e + 1)), alt_idx  # indices into ref / bases
        while r and a and U[r[-1]] == B[a[-1]]:
            r.pop(), a.pop()
        while r and a and U[r[0]] == B[a[0]]:
            r.pop(0), a.pop(0)
            s += 1
            o_s += 1
        if not r and not a:
            totals["same_runs"] += 1
            continue
        REF, ALT = ref[s:s + len(r)], bases[o_s:o_s + len(a)]
        kind = kind_of(REF, ALT)
        end = s + len(REF)
        if kind in ("INS", "DEL"):
            X = ALT if kind == "INS" else REF
            while s > prev_end and U[s - 1] == _up(X)[-1]:
                X = X[-1:] + X[:-1]
                s -= 1
                o_s -= 1
            if kind == "INS":
                ALT = X
            else:
                REF = X
        recs.append(dict(ref_pos=s, out_off=o_s, ref=REF, alt=ALT, kind=kind))
        totals["n_kind"][KINDS.index(kind)] += 1
        totals["bases_inserted"] += max(len(ALT) - len(REF), 0)
        totals["bases_deleted"] += max(len(REF) - len(ALT), 0)
        prev_end = end
    return recs, totals


def apply(ref, recs, first, last):
    """the records applied to ref[first .. last] (case as the records and the contig have it)"""
    out, at = [], first
    for r in recs:
        out.append(bytes(ref[at:r["ref_pos"]]))
        out.append(bytes(r["alt"]))
        at = r["ref_pos"] + len(r["ref"])
    out.append(bytes(ref[at:last + 1]))
    return b"".join(out)


# ---- rule 6 ----------------------------------------------------------------------------------------------------------
_CODE = {c: i for i, c in enumerate(b"ACGT")}
_CODE.update({c: i for i, c in enumerate(b"acgt")})
_CODE[ord("U")] = _CODE[ord("u")] = 3


def hash64(key, mask):
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def kmer_hashes(seq, lo, hi, k):
    """table hashes of the valid k-mers wholly inside seq[lo:hi)"""
    mask = (1 << (2 * k)) - 1
    out = []
    for a in range(lo, hi - k + 1):
        w = seq[a:a + k]
        if any(c not in _CODE for c in w):
            continue
        fw = rv = 0
        for c in w:
            fw = (fw << 2) | _CODE[c]
        for c in reversed(w):
            rv = (rv << 2) | (3 - _CODE[c])
        out.append(hash64(min(fw, rv), mask))
    return out


class Table:
    """a yak dump's words as a lookup: hash -> stored count (the LAST word in file order of a key wins among those that
    pass min_count, kmer.rs:148-167)"""

    def __init__(self, yak):
        self.k = int(yak.k)
        self.words = {}
        off, words = np.asarray(yak.bucket_off), np.asarray(yak.words)
        for b in range(len(off) - 1):
            for w in words[int(off[b]):int(off[b + 1])]:
                w = int(w)
                self.words.setdefault(((w >> 10) << 10) | b, []).append(w & 1023)

    def count(self, h, min_count):
        c = 0
        for v in self.words.get(h, ()):
            if v >= min_count:
                c = v
        return c


def support(ref, bases, rec, table, min_count=1):
    """-> (n_in, absent_in, n_out, absent_out) of one record against one Table"""
    k = table.k
    res = []
    for seq, at, ln in ((bytes(ref), rec["ref_pos"], len(rec["ref"])), (bytes(bases), rec["out_off"], len(rec["alt"]))):
        hs = kmer_hashes(seq, max(0, at - (k - 1)), min(len(seq), at + ln + (k - 1)), k)
        res += [len(hs), sum(1 for h in hs if table.count(h, min_count) == 0)]
    return tuple(res)
