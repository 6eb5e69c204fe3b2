"""The rule of the assembly-to-reference caller (include/np2_io.h, np2_asmcall), written from its text in plain Python: one
column at a time, no offsets carried between operations beyond the two running positions.  tests/test_asmcall_cpu.py holds the
host twin to it byte for byte, tests/test_gpu_asmcall.py the device.  Also here: the inputs the tests share (hand-built
alignments, seeded random ones, planted edits)."""
import random

import numpy as np

ALN_DTYPE = np.dtype([("tid", "<i4")] + [(f, "<u4") for f in ("pos", "flag", "mapq", "n_cigar", "q_len", "own_lo", "own_hi", "q_id", "q_base")] +
                     [("cigar_off", "<u8"), ("q_off", "<u8")])
RUN_DTYPE = np.dtype([("tid", "<u4"), ("start", "<u4"), ("end", "<u4")])
VAR_DTYPE = np.dtype([(f, "<u4") for f in ("tid", "pos", "aln", "len", "q_pos")] + [(f, "u1") for f in ("kind", "ref_code", "alt_code", "rev")])
SNV, DEL, INS = 0, 1, 2
OPS = "MIDNSHP=X"
STAT_KEYS = ("alns_seen", "alns_admitted", "alns_skipped", "alns_low_mapq", "alns_short", "alns_unaligned", "runs", "r_bases", "cov0_bases",
             "cov2_bases", "found_snv", "found_del", "found_ins", "kept_snv", "kept_del", "kept_ins", "ins_bases", "del_bases")
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def code(b):
    return "ACGT".find(chr(b).upper()) if chr(b).upper() in "ACGT" else 4


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def cigar_words(ops):
    """[(op letter, length)] -> BAM words"""
    return [(n << 4) | OPS.index(op) for op, n in ops]


def pack(alignments):
    """[dict(tid, pos, flag, mapq, ops=[(letter, n)], query=forward bytes, own=(lo, hi), q_id, q_base)] -> (query stream, alns
    array, cigar words); own defaults to the whole query"""
    alns, cigar, stream = np.zeros(len(alignments), ALN_DTYPE), [], b""
    for i, a in enumerate(alignments):
        w = cigar_words(a.get("ops", []))
        q = bytes(a.get("query", b""))
        lo, hi = a.get("own", (0, len(q)))
        alns[i] = (a.get("tid", 0), a.get("pos", 0), a.get("flag", 0), a.get("mapq", 60), len(w), a.get("q_len", len(q)), lo, hi, a.get("q_id", 0),
                   a.get("q_base", 0), len(cigar), len(stream))
        cigar += w
        stream += q
    return stream, alns, np.array(cigar, dtype=np.uint32)


def model(refs, query, alns, cigar, min_mapq=5, min_aln=5000):
    """-> dict(runs, vars, cov, stats) for arguments that np2_asmcall does not refuse"""
    refs = [bytes(r) for r in refs]
    ref_off = [0]
    for r in refs:
        ref_off.append(ref_off[-1] + len(r))
    G = ref_off[-1]
    diff = [0] * (G + 1)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["alns_seen"] = len(alns)
    events = []  # (tid, pos, kind, aln, order in the CIGAR, len, q_pos, ref_code, alt_code, rev)
    for ai, a in enumerate(alns):
        words = [int(w) for w in cigar[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]]
        ops = [(w & 15, w >> 4) for w in words]
        if int(a["flag"]) & 4 or not ops:
            st["alns_unaligned"] += 1
            continue
        if int(a["mapq"]) < min_mapq:
            st["alns_low_mapq"] += 1
            continue
        if any(op not in (0, 1, 2, 4, 7, 8) for op, _ in ops):
            st["alns_skipped"] += 1
            continue
        if sum(n for op, n in ops if op in (0, 2, 7, 8)) < min_aln:
            st["alns_short"] += 1
            continue
        st["alns_admitted"] += 1
        q_len, rev, tid = int(a["q_len"]), bool(int(a["flag"]) & 16), int(a["tid"])
        fwd = query[int(a["q_off"]):int(a["q_off"]) + q_len]
        sam = revcomp(fwd) if rev else bytes(fwd)  # the bases in SAM orientation (a non-ACGT byte is N either way)
        own = range(q_len - int(a["own_hi"]), q_len - int(a["own_lo"])) if rev else range(int(a["own_lo"]), int(a["own_hi"]))
        to_fwd = (lambda j: q_len - 1 - j) if rev else (lambda j: j)
        ref = refs[tid]
        p, j, anchor, covered = int(a["pos"]), 0, None, []
        for order, (op, n) in enumerate(ops):
            if op in (0, 7, 8):
                for _ in range(n):
                    if j in own:
                        covered.append(p)
                        rc, qc = code(ref[p]), code(sam[j])
                        if op != 7 and rc < 4 and qc < 4 and rc != qc:
                            events.append((tid, p, SNV, ai, order, 1, to_fwd(j), rc, qc, rev))
                    anchor = (j, p)
                    p, j = p + 1, j + 1
            elif op == 2:
                if n and anchor is not None and anchor[0] in own:
                    covered += range(p, p + n)
                    events.append((tid, anchor[1], DEL, ai, order, n, q_len - j if rev else j, 0, 0, rev))
                p += n
            elif op == 1:
                if n and anchor is not None and anchor[0] in own:
                    events.append((tid, anchor[1], INS, ai, order, n, min(to_fwd(j), to_fwd(j + n - 1)), 0, 0, rev))
                j += n
            else:
                j += n
        if covered:
            assert sorted(covered) == list(range(min(covered), max(covered) + 1))  # one interval
            diff[ref_off[tid] + min(covered)] += 1
            diff[ref_off[tid] + max(covered) + 1] -= 1
    cov = np.cumsum(diff[:G], dtype=np.int64).astype(np.uint32) if G else np.zeros(0, np.uint32)
    st["r_bases"], st["cov0_bases"], st["cov2_bases"] = int((cov == 1).sum()), int((cov == 0).sum()), int((cov >= 2).sum())
    runs = []
    for t in range(len(refs)):
        c, s = cov[ref_off[t]:ref_off[t + 1]], None
        for i in range(len(c) + 1):
            one = i < len(c) and c[i] == 1
            if one and s is None:
                s = i
            if not one and s is not None:
                runs.append((t, s, i))
                s = None
    st["runs"] = len(runs)
    kept = []
    for e in events:
        tid, pos, kind, n = e[0], e[1], e[2], e[5]
        st["found_" + ("snv", "del", "ins")[kind]] += 1
        c = cov[ref_off[tid]:ref_off[tid + 1]]
        foot = [pos] if kind == SNV else list(range(pos, pos + n + 1)) if kind == DEL else [pos] + ([pos + 1] if pos + 1 < len(c) else [])
        if all(c[x] == 1 for x in foot):
            kept.append(e)
            st["kept_" + ("snv", "del", "ins")[kind]] += 1
            st["ins_bases"] += n if kind == INS else 0
            st["del_bases"] += n if kind == DEL else 0
    kept.sort(key=lambda e: e[:5])  # (tid, pos, kind, alignment, CIGAR order)
    out = np.zeros(len(kept), VAR_DTYPE)
    for i, (tid, pos, kind, ai, _, n, q_pos, rc, qc, rev) in enumerate(kept):
        out[i] = (tid, pos, ai, n, q_pos, kind, rc, qc, int(rev))
    return dict(runs=np.array(runs, dtype=RUN_DTYPE) if runs else np.zeros(0, RUN_DTYPE), vars=out, cov=cov, stats=st)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def random_case(seed, n_refs=2, n_alns=12, max_ops=90):
    """seeded random references and alignments that the doors accept: random CIGARs (M I D S = X, some of length 0, leading and
    adjacent gaps), either strand, random owned intervals, queries with mismatches, N and lower case -> (refs, alignments)"""
    rng = random.Random(seed)
    refs = [random_seq(rng, rng.randint(1, 700), "ACGTacgtN") for _ in range(n_refs)]
    out = []
    for _ in range(n_alns):
        tid = rng.randrange(n_refs)
        L = len(refs[tid])
        ops, span, qn = [], 0, 0
        pos = rng.randrange(L)
        if rng.random() < 0.3:
            ops.append(("S", rng.randint(0, 5)))
        for _ in range(rng.randint(1, max_ops)):
            op = rng.choice("MMM=XIDID")
            n = rng.choice((0, 1, 1, 2, 3, 7, 40, 70)) if op in "M=X" else rng.choice((0, 1, 1, 2, 5))
            if op in "M=XD":
                n = min(n, L - pos - span)
                span += n
            ops.append((op, n))
        if rng.random() < 0.3:
            ops.append(("S", rng.randint(0, 5)))
        qn = sum(n for op, n in ops if op in "MIS=X")
        # the SAM-orientation query: the reference's bases on M = X columns, with mismatches, N and lower case sprinkled in
        sam, p = bytearray(), pos
        for op, n in ops:
            if op in "M=X":
                for i in range(n):
                    b = refs[tid][p + i:p + i + 1].upper()
                    r = rng.random()
                    sam += random_seq(rng, 1, "ACGT") if r < 0.1 else b"N" if r < 0.13 else b.lower() if r < 0.2 else b
                p += n
            elif op == "D":
                p += n
            else:
                sam += random_seq(rng, n, "ACGTN")
        rev = rng.random() < 0.5
        lo = rng.randint(0, qn)
        hi = rng.randint(lo, qn) if rng.random() < 0.8 else lo
        if rng.random() < 0.3:
            lo, hi = 0, qn
        out.append(dict(tid=tid, pos=pos, flag=16 if rev else 0, mapq=rng.choice((0, 4, 5, 60)), ops=ops, query=revcomp(sam) if rev else bytes(sam),
                        own=(lo, hi), q_id=rng.randrange(3), q_base=rng.randrange(1000)))
    return refs, out


def plant_edits(seed, L=60000, seams=()):
    """a seeded random truth of L bases and an edited copy -> (truth, edited, [(kind, start, end, ref allele, alt allele)] as the
    V lines report them against the truth).  SNVs, deletions of 1..4 and insertions of 1..5 bases, each placed so that no shift
    is possible (the allele's first base differs from the base after it, its last base from the base before it), at least 300
    bases apart; `seams`: positions of the edited copy on and beside which some are placed."""
    rng = random.Random(seed)
    truth = random_seq(rng, L)
    wanted = sorted(set([rng.randrange(2000, L - 2000) for _ in range(60)] + [s + d for s in seams for d in (-1, 0, 1)]))
    places, last = [], -1000
    for x in wanted:
        if x - last >= 300:
            places.append(x)
            last = x
    out, edits, prev, shift = bytearray(), [], 0, 0
    for i, x in enumerate(places):
        x -= shift  # (seams are positions of the edited copy: undo the length changes so far)
        kind = (SNV, DEL, INS)[i % 3]
        if kind == SNV:
            alt = rng.choice([b for b in b"ACGT" if b != truth[x]])
            out += truth[prev:x] + bytes([alt])
            edits.append((SNV, x, x + 1, chr(truth[x]).lower(), chr(alt).lower()))
            prev = x + 1
        elif kind == DEL:
            n = 1 + i % 4
            while truth[x] == truth[x + n] or truth[x + n - 1] == truth[x - 1]:
                x += 1
            out += truth[prev:x]
            edits.append((DEL, x, x + n, truth[x:x + n].decode().lower(), "-"))
            prev, shift = x + n, shift - n
        else:
            n = 1 + i % 5
            while True:
                ins = random_seq(rng, n)
                if ins[0] != truth[x] and ins[-1] != truth[x - 1]:
                    break
            out += truth[prev:x] + ins
            edits.append((INS, x, x, "-", ins.decode().lower()))
            prev, shift = x, shift + n
    out += truth[prev:]
    return truth, bytes(out), edits


def aln(ref, pos, ops, rev=False, mism=(), own=None, fill=b"GATTACA", **kw):
    """an alignment dict for pack(): the query follows `ref` on M = X columns except at the SAM indices `mism` (the next base in
    A C G T order), I and S bases come from `fill`; own: the owned forward interval (default: everything)"""
    sam, p = bytearray(), pos
    for op, n in ops:
        if op in "M=X":
            sam += bytes(ref[p:p + n]).upper()
            p += n
        elif op == "D":
            p += n
        elif op in "IS":
            sam += (fill * (n // len(fill) + 1))[:n]
    for j in mism:
        sam[j] = b"ACGTA"[b"ACGT".find(bytes([sam[j]])) + 1] if bytes([sam[j]]) in b"ACGT" else sam[j]
    q = revcomp(sam) if rev else bytes(sam)
    return dict(pos=pos, flag=16 if rev else 0, ops=ops, query=q, own=own if own is not None else (0, len(q)), **kw)


def hand_cases():
    """[(name, refs, alignments, opts)]: the edges the issue names, each on both strands where a strand can matter"""
    rng = random.Random(7)
    R = random_seq(rng, 400)
    cases, lo = [], dict(min_mapq=5, min_aln=1)
    for rev in (False, True):
        s = "-" if rev else "+"
        for n in (1, 63, 64, 65):
            cases.append((f"q_len {n} {s}", [R], [aln(R, 3, [("M", n)], rev, mism=range(0, n, 3))], lo))
        many = [("M", 3), ("I", 1), ("M", 2), ("D", 1)] * 40 + [("X", 4)]
        cases.append((f"161 words {s}", [R], [aln(R, 5, many, rev, mism=range(0, 200, 7))], lo))
        for own in ((0, 63), (0, 64), (0, 65), (63, 65), (64, 200), (65, 200), (64, 64), (0, 0), (200, 200)):
            cases.append((f"own {own} {s}", [R], [aln(R, 0, [("M", 200)], rev, mism=range(0, 200, 2), own=own)], lo))
        for gap in "DI":
            qn = 20 if gap == "D" else 22  # owned SAM intervals that end or start at the anchor, column 9, and one column beside it
            for s_lo, s_hi in ((0, 10), (0, 9), (10, qn), (9, qn)):
                own = (qn - s_hi, qn - s_lo) if rev else (s_lo, s_hi)
                cases.append((f"10M2{gap}10M own {own} {s}", [R], [aln(R, 20, [("M", 10), (gap, 2), ("M", 10)], rev, own=own)], lo))
        cases.append((f"leading gaps {s}", [R], [aln(R, 10, [("I", 2), ("M", 10)], rev), aln(R, 40, [("D", 2), ("M", 10)], rev),
                                                 aln(R, 70, [("S", 5), ("I", 2), ("D", 1), ("M", 10), ("S", 3)], rev)], lo))
        cases.append((f"gaps sharing an anchor {s}", [R], [aln(R, 10, [("M", 10), ("I", 2), ("D", 3), ("M", 10)], rev),
                                                           aln(R, 60, [("M", 10), ("I", 1), ("D", 1), ("I", 2), ("M", 0), ("D", 0), ("M", 10)], rev),
                                                           aln(R, 100, [("M", 10), ("D", 2), ("I", 3), ("=", 10)], rev)], lo))
        cases.append((f"overlap {s}", [R], [aln(R, 0, [("M", 100)], rev, mism=(10, 50, 90)), aln(R, 40, [("M", 100)], rev, mism=(10, 30, 80))], lo))
        cases.append((f"DEL across a coverage change {s}", [R], [aln(R, 0, [("M", 10), ("D", 3), ("M", 10)], rev, mism=(2,)), aln(R, 11, [("M", 30)], rev),
                                                                 aln(R, 100, [("M", 10), ("D", 3), ("M", 10)], rev), aln(R, 114, [("M", 30)], rev),
                                                                 aln(R, 200, [("M", 10), ("I", 3), ("M", 10)], rev), aln(R, 210, [("M", 30)], rev)], lo))
        cases.append((f"last base {s}", [R[:50], R[50:90], R[90:120]], [aln(R[:50], 40, [("M", 10)], rev, mism=(9,), tid=0),
                                                                        aln(R[50:90], 30, [("M", 10), ("I", 2)], rev, tid=1),
                                                                        aln(R[90:120], 18, [("M", 10), ("D", 2)], rev, tid=2)], lo))
        cases.append((f"two references {s}", [R[:100], R[100:250]], [aln(R[:100], 0, [("M", 100)], rev, tid=0), aln(R[100:250], 0, [("M", 150)], rev, tid=1, mism=(0, 149))], lo))
        N = R[:30] + b"NNnn" + R[34:60].lower()
        qn = aln(N, 0, [("M", 60)], rev, mism=(5, 31, 40))
        q = bytearray(qn["query"])
        q[8 if not rev else 51] = ord("N")
        q[12 if not rev else 47] = ord("n")
        cases.append((f"N and lower case {s}", [N], [dict(qn, query=bytes(q))], lo))
    cases.append(("no alignments", [R[:70]], [], lo))
    cases.append(("no references", [], [], lo))
    cases.append(("an empty reference between two", [R[:20], b"", R[20:40]], [aln(R[:20], 0, [("M", 20)], tid=0), aln(R[20:40], 0, [("M", 20)], tid=2)], lo))
    cases.append(("a reference of one base", [b"A", b"c"], [aln(b"A", 0, [("M", 1)], mism=(0,), tid=0), aln(b"c", 0, [("M", 1)], True, tid=1)], lo))
    cases.append(("admission", [R], [dict(aln(R, 0, [("M", 30)]), flag=4), dict(aln(R, 0, [("M", 30)]), mapq=4), aln(R, 0, [("M", 29)]),
                                     dict(aln(R, 0, [("M", 10), ("N", 5), ("M", 10)]), mapq=4), aln(R, 50, [("M", 10), ("N", 5), ("M", 20)]),
                                     aln(R, 50, [("H", 3), ("M", 30)]), aln(R, 50, [("M", 30), ("P", 1)]), dict(tid=0, pos=0, ops=[], query=b""),
                                     aln(R, 100, [("M", 30)], mism=(4,)), aln(R, 140, [("M", 20), ("D", 10)])], dict(min_mapq=5, min_aln=30)))
    return cases
