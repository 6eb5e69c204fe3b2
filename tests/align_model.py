"""A Python restatement of the aligner's rule (include/np2_io.h: np2_map_align_*), written from the rule's text and independent
of the C++: pins, the trim, banded Gotoh as three full tables with a value-driven walk back (no stored bits), the end extension's
choice of cell, the ends of the CIGAR, left-alignment on runs, the record and the SAM text.  Chains come from tests/map_model.py."""
import numpy as np

import map_model as mm

DEFAULTS = dict(match=1, mismatch=4, gap_open=6, gap_ext=2, band=32, end_bonus=5, ext_max=2048, max_cells=1 << 23)
REC_FIELDS = ("tid", "flag", "pos", "end", "mapq", "n_cigar", "nm", "as")
COUNT_FIELDS = ("pins", "segments", "equal", "pure_gap", "snv", "cores", "cells", "clipped_bases", "overflow")
MAX_W = 2048
NONE = -10 ** 9  # a cell outside the band or the matrix
OPS = "MIDNS"


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def codes(seq):
    return mm._CODE[np.frombuffer(bytes(seq), np.uint8)].tolist()


def rc_codes(c):
    return [3 - x if x < 4 else 4 for x in reversed(c)]


def same(a, b):
    return a < 4 and a == b


def pins_of(chain, k):
    """the chain's pins as (r, q) end positions"""
    out = []
    for r, q in chain.tolist():
        if not out or (r - k + 1 > out[-1][0] and q - k + 1 > out[-1][1]):
            out.append((r, q))
    return out


class Overflow(Exception):
    pass


def tables(T, Q, lo, W, o):
    """H, E, F of the band's cells, [row][slot]; slot L of row i is column i + lo + L"""
    tl, ql = len(T), len(Q)
    go, ge = o["gap_open"], o["gap_ext"]
    H = [[NONE] * W for _ in range(ql + 1)]
    E = [[NONE] * W for _ in range(ql + 1)]
    F = [[NONE] * W for _ in range(ql + 1)]

    def at(M, i, j):
        L = j - i - lo
        return M[i][L] if i >= 0 and 0 <= j <= tl and 0 <= L < W else NONE

    for i in range(ql + 1):
        for L in range(W):
            j = i + lo + L
            if j < 0 or j > tl:
                continue
            if i == 0 and j == 0:
                H[0][L] = 0
                continue
            e = max(at(E, i, j - 1), at(H, i, j - 1) - go) - ge
            f = max(at(F, i - 1, j), at(H, i - 1, j) - go) - ge
            d = NONE
            if i > 0 and j > 0 and at(H, i - 1, j - 1) > NONE // 2:
                d = at(H, i - 1, j - 1) + (o["match"] if same(T[j - 1], Q[i - 1]) else -o["mismatch"])
            E[i][L], F[i][L] = max(e, NONE), max(f, NONE)
            H[i][L] = max(d, E[i][L], F[i][L])
    return H, E, F, at


def walk(T, Q, lo, W, o, tabs, ei, ej):
    """columns from (0, 0) to (ei, ej), first to last, by the stated preference"""
    H, E, F, at = tabs
    go, ge = o["gap_open"], o["gap_ext"]
    cols = []
    i, j, state = ei, ej, "H"
    while i > 0 or j > 0:
        if state == "H":
            h = at(H, i, j)
            if i > 0 and j > 0 and at(H, i - 1, j - 1) > NONE // 2 and \
                    h == at(H, i - 1, j - 1) + (o["match"] if same(T[j - 1], Q[i - 1]) else -o["mismatch"]):
                cols.append("M")
                i, j = i - 1, j - 1
            elif h == at(E, i, j):
                state = "E"
            else:
                assert h == at(F, i, j)
                state = "F"
        elif state == "E":
            cols.append("D")
            if not at(E, i, j - 1) >= at(H, i, j - 1) - go:
                state = "H"
            j -= 1
        else:
            cols.append("I")
            if not at(F, i - 1, j) >= at(H, i - 1, j) - go:
                state = "H"
            i -= 1
    return cols[::-1]


def band_of(tl, ql, band, max_cells):
    d = tl - ql
    lo, W = min(0, d) - band, abs(d) + 2 * band + 1
    if W > MAX_W or (ql + 1) * W > max_cells:
        raise Overflow()
    return lo, W


def core_align(T, Q, o, cnt):
    """a core (both sides non-empty, not 1 x 1) -> its columns and score"""
    lo, W = band_of(len(T), len(Q), o["band"], o["max_cells"])
    cnt["cells"] += (len(Q) + 1) * W
    tabs = tables(T, Q, lo, W, o)
    return walk(T, Q, lo, W, o, tabs, len(Q), len(T)), tabs[3](tabs[0], len(Q), len(T))


def segment(T, Q, o, cnt):
    """the bases between two pins -> columns"""
    tl, ql = len(T), len(Q)
    if tl == ql and all(same(a, b) for a, b in zip(T, Q)):
        cnt["equal"] += 1
        return ["M"] * tl
    m = min(tl, ql)
    pre = 0
    while pre < m and same(T[pre], Q[pre]):
        pre += 1
    suf = 0
    while suf < m - pre and same(T[tl - 1 - suf], Q[ql - 1 - suf]):
        suf += 1
    Tc, Qc = T[pre:tl - suf], Q[pre:ql - suf]
    if not Tc or not Qc:
        cnt["pure_gap"] += 1
        mid = ["D"] * len(Tc) + ["I"] * len(Qc)
    elif len(Tc) == 1 and len(Qc) == 1:
        cnt["snv"] += 1
        mid = ["M"]
    else:
        cnt["cores"] += 1
        mid = core_align(Tc, Qc, o, cnt)[0]
    return ["M"] * pre + mid + ["M"] * suf


def extension(T_left, Q_rem, o, cnt):
    """T_left: the reference from the pin outwards (all that the contig has), Q_rem: the read's remainder outwards -> (columns
    outwards, read bases taken, reference bases taken)"""
    rem, ref_left, band = len(Q_rem), len(T_left), o["band"]
    n = min(rem, o["ext_max"], ref_left + band)
    if n == 0:
        return [], 0, 0
    T, Q = T_left[:min(ref_left, n + band)], Q_rem[:n]
    lo, W = -band, 2 * band + 1
    if W > MAX_W or (n + 1) * W > o["max_cells"]:
        raise Overflow()
    cnt["cells"] += (n + 1) * W
    tabs = tables(T, Q, lo, W, o)
    H, at = tabs[0], tabs[3]
    best = (0, 0, 0)  # (score, row, column)
    for i in range(n + 1):
        for j in range(max(0, i + lo), min(len(T), i + lo + W - 1) + 1):
            if at(H, i, j) > best[0]:
                best = (at(H, i, j), i, j)
    end = best
    if n == rem:
        row = [(at(H, n, j), j) for j in range(max(0, n + lo), min(len(T), n + lo + W - 1) + 1)]
        eh = max(h for h, _ in row)
        ej = min(j for h, j in row if h == eh)
        if eh + o["end_bonus"] >= best[0]:
            end = (eh, n, ej)
    return walk(T, Q, lo, W, o, tabs, end[1], end[2]), end[1], end[2]


def runs_of(cols):
    runs = []
    for c in cols:
        if runs and runs[-1][0] == c:
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    return runs


def left_align(runs, T, Q, t_start, q_start):
    """runs (no clips) of [op, len], in place"""
    i = 0
    while i < len(runs):
        op, L = runs[i]
        if op in "ID" and i > 0 and runs[i - 1][0] == "M" and not (i - 1 == 0 and runs[0][1] == 1):
            r = t_start + sum(l for c, l in runs[:i] if c in "MD")
            q = q_start + sum(l for c, l in runs[:i] if c in "MI")
            last = T[r + L - 1] if op == "D" else Q[q + L - 1]
            if same(T[r - 1], Q[q - 1]) and last == T[r - 1]:
                runs[i - 1][1] -= 1
                if i + 1 < len(runs) and runs[i + 1][0] == "M":
                    runs[i + 1][1] += 1
                else:
                    runs.insert(i + 1, ["M", 1])
                if runs[i - 1][1] == 0:
                    del runs[i - 1]
                    i -= 1
                    if i > 0 and runs[i - 1][0] == op:  # two gaps of one kind meet
                        runs[i - 1][1] += L
                        del runs[i]
                        i -= 1
                continue
        i += 1


def align_read(contig_codes, read, hit, chain, k, o, cnt):
    """-> (rec dict, cigar as a list of (op, len)) or (None, None) for an overflowed read"""
    T = contig_codes
    Q = codes(read)
    if hit["rev"]:
        Q = rc_codes(Q)
    pins = pins_of(chain, k)
    cnt["pins"] += len(pins)
    cnt["segments"] += len(pins) - 1
    try:
        r0, q0 = pins[0][0] - k + 1, pins[0][1] - k + 1
        # (the slots are classified head, segments, tail; an overflow anywhere leaves the read unaligned, the counts stand)
        over = None
        try:
            hcols, hq, ht = extension(T[:r0][::-1], Q[:q0][::-1], o, cnt)
        except Overflow as e:
            over, (hcols, hq, ht) = e, ([], 0, 0)
        cols = hcols[::-1] + ["M"] * k
        for (pr, pq), (r, q) in zip(pins[:-1], pins[1:]):
            try:
                cols += segment(T[pr + 1:r - k + 1], Q[pq + 1:q - k + 1], o, cnt)
            except Overflow as e:
                over = e
            cols += ["M"] * k
        r1, q1 = pins[-1][0] + 1, pins[-1][1] + 1
        try:
            tcols, tq, tt = extension(T[r1:], Q[q1:], o, cnt)
        except Overflow as e:
            over = e
        if over:
            raise over
    except Overflow:
        cnt["overflow"] += 1
        return None, None
    cols += tcols
    clip5, clip3, t_start = q0 - hq, len(Q) - q1 - tq, r0 - ht
    runs = runs_of(cols)
    while runs[0][0] != "M":
        op, L = runs.pop(0)
        if op == "I":
            clip5 += L
        else:
            t_start += L
    while runs[-1][0] != "M":
        op, L = runs.pop()
        if op == "I":
            clip3 += L
    left_align(runs, T, Q, t_start, clip5)
    nm = score = 0
    r, q = t_start, clip5
    for op, L in runs:
        if op == "M":
            for c in range(L):
                if same(T[r + c], Q[q + c]):
                    score += o["match"]
                else:
                    score -= o["mismatch"]
                    nm += 1
            r, q = r + L, q + L
        else:
            nm += L
            score -= o["gap_open"] + L * o["gap_ext"]
            if op == "D":
                r += L
            else:
                q += L
    cigar = ([("S", clip5)] if clip5 else []) + [(op, L) for op, L in runs] + ([("S", clip3)] if clip3 else [])
    cnt["clipped_bases"] += clip5 + clip3
    rec = dict(tid=hit["tid"], flag=16 if hit["rev"] else 0, pos=t_start, end=r, mapq=hit["mapq"], n_cigar=len(cigar), nm=nm)
    rec["as"] = score
    return rec, cigar


UNALIGNED = dict(tid=-1, flag=4, pos=0, end=0, mapq=0, n_cigar=0, nm=0)
UNALIGNED["as"] = 0


def align_reads(contigs, reads, map_kw=None, **kw):
    """-> (hits, recs: list of dicts, cigars: list of lists of (op, len), counts dict, map totals)"""
    map_kw = dict(map_kw or {})
    ix = mm.Index(contigs, map_kw.get("k", 19), map_kw.get("w", 19))
    mk = {f: v for f, v in map_kw.items() if f not in ("k", "w")}
    hits, chains, tot = mm.map_reads(ix, reads, **mk)
    return align_mapped(contigs, reads, hits, chains, ix.k, **kw) + (tot,)


def align_mapped(contigs, reads, hits, chains, k, **kw):
    o = opts(**kw)
    cc = [codes(c) for c in contigs]
    cnt = dict.fromkeys(COUNT_FIELDS, 0)
    recs, cigars = [], []
    for rd, h, ch in zip(reads, hits, chains):
        rec, cg = (None, None) if h is None else align_read(cc[h["tid"]], rd, h, ch, k, o, cnt)
        recs.append(rec if rec else dict(UNALIGNED))
        cigars.append(cg if rec else [])
    return hits, recs, cigars, cnt


def cigar_words(cigars):
    """the CIGARs as the C interface returns them: (uint32 words, offsets)"""
    words, off = [], [0]
    for cg in cigars:
        words += [L << 4 | OPS.index(op) for op, L in cg]
        off.append(len(words))
    return np.array(words, np.uint32), np.array(off, np.uint64)


def recs_array(recs):
    return np.array([[r[f] for f in REC_FIELDS] for r in recs], np.int64).reshape(len(recs), len(REC_FIELDS))


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def sam_header(tnames, tlens):
    return "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in zip(tnames, tlens)) + \
        "@PG\tID:nextpolish2_amd.map\tPN:nextpolish2_amd.map\n"


def sam_line(qname, read, hit, rec, cigar, tnames):
    read = bytes(read)
    if rec["tid"] < 0:
        return f"{qname}\t4\t*\t0\t0\t*\t*\t0\t0\t{read.decode() or '*'}\t*\n"
    seq = read.translate(_RC)[::-1] if rec["flag"] & 16 else read
    cg = "".join(f"{L}{op}" for op, L in cigar)
    return (f"{qname}\t{rec['flag']}\t{tnames[rec['tid']]}\t{rec['pos'] + 1}\t{rec['mapq']}\t{cg}\t*\t0\t0\t{seq.decode() or '*'}\t*\t"
            f"NM:i:{rec['nm']}\tAS:i:{rec['as']}\tcm:i:{hit['n']}\ts1:i:{hit['s1']}\ts2:i:{hit['s2']}\n")


def sam(names, reads, hits, recs, cigars, tnames, tlens):
    return sam_header(tnames, tlens) + "".join(sam_line(n, r, h, rc, cg, tnames) for n, r, h, rc, cg in zip(names, reads, hits, recs, cigars))
