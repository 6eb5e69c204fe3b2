"""Caller-built chains for the aligner's doors np2_align_chains_host and np2_align_chains_device (include/np2_io.h), shared by
tests/test_alignchain_cpu.py and tests/test_gpu_map_alignchain.py.  A case is (contigs, reads, hits, chains, k, align options);
its expected answer is align_model.align_mapped's, computed once per process, together with what the model's tables say about
every matrix: the traceback bits by the stated preference (matrices under 20 000 cells) and where the equal best cells lie.

A core of arbitrary content is a read P1 + Q + P2 against a contig holding P1 + T + P2: P1 and P2 are k-mers, the two-anchor chain
sits at their last bases, T and Q differ in their first and last base, so nothing is trimmed and every such pair with both sides
>= 2 is a core.  An extension of arbitrary content is a read with one anchor at its first or last k-mer.  The mapper cannot be
steered into these shapes; each is the smallest that still has the edge its name says.

CELLS at the end of the file notes every case's matrix cells (the model's count); the largest stay near 150 000."""
import numpy as np

import align_model as am
import map_model as mm

K = 11
P1, P2 = b"GATTACAGCTC", b"CTGGAATCGTA"
# match, mismatch, gap_open, gap_ext: the extremes of the limits, the free-gap-open corner where the device's prefix maximum
# equals the sequential recurrence exactly, and the defaults
OPTSETS = {"m15": (15, 0, 0, 1), "x31": (1, 31, 255, 15), "m1x0": (1, 0, 0, 1), "m1x1": (1, 1, 0, 1), "x4o0": (1, 4, 0, 2), "dflt": (1, 4, 6, 2)}


def scoring(name):
    return dict(zip(("match", "mismatch", "gap_open", "gap_ext"), OPTSETS[name]))


def rand(rng, n, letters=b"ACGT"):
    return bytes(letters[i] for i in rng.integers(0, len(letters), n))


def differ(rng, ch, letters=b"ACGT"):
    """a letter that does not match ch (N matches nothing, itself included)"""
    pick = [c for c in letters if c != ch or c == ord("N")]
    return pick[int(rng.integers(0, len(pick)))]


def ends_differ(rng, T, Q, letters=b"ACGT"):
    Q = bytearray(Q)
    Q[0] = differ(rng, T[0], letters)
    Q[-1] = differ(rng, T[-1], letters)
    return bytes(Q)


class Case:
    """contig 0 is a pool the cores' blocks are appended to (their heads and tails are empty, so what surrounds a block does not
    matter); every other contig is exactly what the caller gives"""

    def __init__(self, **ao):
        self.ao = ao
        self.pool, self.extra = bytearray(), []
        self.reads, self.hits, self.chains = [], [], []

    def contig(self, seq):
        self.extra.append(bytes(seq))
        return len(self.extra)

    def read(self, tid, fwd, anchors, rev=False, mapq=60):
        """fwd: the read on the chain's strand; anchors: (r, q) end positions"""
        fwd = bytes(fwd)
        self.reads.append(mm.revcomp(fwd) if rev else fwd)
        hit = dict.fromkeys(mm.HIT_FIELDS, 0)
        hit.update(tid=tid, rev=int(rev), qlen=len(fwd), n=len(anchors), mapq=mapq)
        self.hits.append(hit)
        self.chains.append(np.array(anchors, np.uint32).reshape(-1, 2))

    def unmapped(self, read):
        self.reads.append(bytes(read))
        self.hits.append(None)
        self.chains.append(np.zeros((0, 2), np.uint32))

    def core(self, T, Q, rev=False):
        off = len(self.pool)
        self.pool += P1 + T + P2
        self.read(0, P1 + Q + P2, [(off + K - 1, K - 1), (off + 2 * K + len(T) - 1, 2 * K + len(Q) - 1)], rev)

    def tail(self, ref, rem, rev=False):
        """one anchor at the read's first k-mer; ref: all the contig has beyond the pin"""
        self.read(self.contig(P1 + ref), P1 + rem, [(K - 1, K - 1)], rev)

    def head(self, ref, rem, rev=False):
        """one anchor at the read's last k-mer; ref: all the contig has before the pin (given outwards, as rem is)"""
        ref, rem = bytes(ref)[::-1], bytes(rem)[::-1]
        self.read(self.contig(ref + P2), rem + P2, [(len(ref) + K - 1, len(rem) + K - 1)], rev)

    def done(self):
        return [bytes(self.pool) or b"A"] + self.extra, self.reads, self.hits, self.chains, K, self.ao


def mutate(rng, T, d, n_sub=3):
    """a read side d shorter than T (d < 0: longer): |d| single-base indels at seeded places and a few substitutions"""
    Q = bytearray(T)
    for _ in range(abs(d)):
        at = int(rng.integers(1, len(Q) - 1))
        if d > 0:
            del Q[at]
        else:
            Q.insert(at, b"ACGT"[int(rng.integers(0, 4))])
    for _ in range(n_sub):
        at = int(rng.integers(1, len(Q) - 1))
        Q[at] = differ(rng, Q[at])
    return ends_differ(rng, T, bytes(Q))


# W = |d| + 2 band + 1 per band: 1, 2 and the exact diagonals 0 .. d under band 0; 63, 64 | 65 | 127, 128 | 129, 130 around the lane
# blocks; 2047, 2048 and the overflowing 2049 under the widest band
BAND_SHAPES = {0: (0, 1, 3, -3, -1), 31: (0, 1, -1), 32: (0, -2), 63: (0, 1), 64: (0, 1), 1023: (1, 2, 0)}


def band_case(sc, band):
    rng = np.random.default_rng(1000 + band)
    c = Case(band=band, **scoring(sc))
    ql = 8 if band == 0 else 29 if band == 1023 else 70  # (rows beyond the band's half: every slot of the band holds a cell)
    for n, d in enumerate(BAND_SHAPES[band]):
        T = rand(rng, ql + d)
        c.core(T, mutate(rng, T, d), rev=bool(n & 1))
    return c.done()


def lane_case(sc):
    """one deletion run of 70 and of 140 columns inside one row, from slot 33 on (over the lane blocks' edges at 64 and 128); the
    run beginning exactly at slots 63, 64 and 65 behind an earlier deletion; the mirror image, one insertion down 70 rows"""
    rng = np.random.default_rng(77)
    c = Case(band=32, **scoring(sc))
    a, b, m = rand(rng, 10), rand(rng, 10), b"GGGGGGGG"  # (the runs hold no G: m matches m alone, and left-alignment leaves the runs apart)
    a2, b2 = ends_differ(rng, a, a)[:1] + a[1:], b[:-1] + ends_differ(rng, b, b)[-1:]
    for run in (70, 140):
        c.core(a + rand(rng, run, b"AC") + b, a2 + b2, rev=run == 140)
    for first in (30, 31, 32):  # the second run's first slot is first + 1 + band
        c.core(a + rand(rng, first, b"CT") + m + rand(rng, 70, b"AC") + b, a2 + m + b2)
    c.core(a + b, a2 + rand(rng, 70, b"AC") + b2)
    return c.done()


def random_case(sc, band, n=60):
    rng = np.random.default_rng(31 * band + list(OPTSETS).index(sc))
    c = Case(band=band, **scoring(sc))
    for i in range(n):
        letters = (b"AC", b"ACGT", b"ACGTN")[i % 3]
        T = rand(rng, int(rng.integers(2, 61)), letters)
        Q = rand(rng, int(rng.integers(2, 61)), letters)
        c.core(T, ends_differ(rng, T, Q, letters), rev=bool((i // 3) & 1))
    return c.done()


def near(rng, ref, n, n_sub=2):
    """the first n bases of ref with a few substitutions"""
    q = bytearray(ref[:n])
    for _ in range(n_sub):
        at = int(rng.integers(0, len(q)))
        q[at] = differ(rng, q[at])
    return bytes(q)


def ext_limits_case():
    """ext_max = 40, band = 8.  rem = 39, 40, 41 (the end cell exists, exists, does not); ref_left + band = rem - 1, rem, rem + 1
    with rem = 20; ref_left = 0 (a matrix of column 0 only); each as a tail and as a head on both strands, the other side empty"""
    rng = np.random.default_rng(5)
    c = Case(band=8, ext_max=40)
    for rev in (False, True):
        for side in (c.tail, c.head):
            for rem in (39, 40, 41):
                ref = rand(rng, 80)
                side(ref, near(rng, ref, rem), rev)
            for ref_left in (11, 12, 13):
                ref = rand(rng, ref_left)
                side(ref, near(rng, ref + rand(rng, 20), 20), rev)
            side(b"", rand(rng, 5), rev)
            side(b"", rand(rng, 30), rev)
    # N bases and lower case in the remainder, on the reverse strand
    ref = rand(rng, 60)
    c.tail(ref, ref[:10] + b"N" + ref[11:20].lower() + b"n" + ref[21:30], True)
    c.head(ref, ref[:7].lower() + b"NN" + ref[9:25], True)
    return c.done()


def ext_band0_case():
    """band = 0: the extension's band is the main diagonal alone; with ref_left = 0 there is no matrix (K_EMPTY) beside a
    non-empty other side"""
    rng = np.random.default_rng(6)
    c = Case(band=0)
    for rev in (False, True):
        for side in (c.tail, c.head):
            ref = rand(rng, 30)
            side(ref, near(rng, ref, 25), rev)
            side(b"", rand(rng, 9), rev)
            side(ref[:4], near(rng, ref, 25), rev)
    # K_EMPTY head (no reference before the pin) beside a non-empty tail, and the mirror
    ref = rand(rng, 30)
    c.read(c.contig(P1 + ref), b"ACGTA" + P1 + near(rng, ref, 20), [(K - 1, 5 + K - 1)])
    c.read(c.contig(ref + P2), near(rng, ref, 30) + P2 + b"TTGCA", [(30 + K - 1, 30 + K - 1)], True)
    return c.done()


TIE_SCORING = {"x0": dict(match=1, mismatch=0, gap_open=0, gap_ext=1), "m1x1": dict(match=1, mismatch=1, gap_open=0, gap_ext=1)}
# "best": ext_max = 12 is below every remainder, so no end cell exists and the best cell's order (smallest row, then smallest
# column) decides the answer; "end": the bonus is the largest, so the last row's smallest column always does
TIE_KINDS = {"best": dict(ext_max=12), "end": dict(end_bonus=1 << 16)}


def tie_facts(H):
    """where a matrix's largest H lies: the number of distinct rows and of distinct band slots that hold it, and the number of
    cells of the last row that hold that row's largest"""
    H = np.asarray(H, np.int64)
    rows, slots = np.nonzero(H == H.max())  # (the origin holds 0: the largest H is never a cell outside the band)
    return dict(best_rows=len(set(rows.tolist())), best_slots=len(set(slots.tolist())), last_best=int(np.count_nonzero(H[-1] == H[-1].max())))


def tie_case(sc, kind):
    """periodic and two-letter remainders, kept when the model's table holds the tie the kind is about: equal best cells in
    different lanes and in different rows, or equal cells in the last row"""
    rng = np.random.default_rng(8)
    band = 12
    o = am.opts(band=band, **TIE_SCORING[sc], **TIE_KINDS[kind])
    c = Case(band=band, **TIE_SCORING[sc], **TIE_KINDS[kind])
    units = (b"A", b"AC", b"AAC", b"ACC", b"AACC", b"ACAAC")
    n = 0
    while n < 16:
        if rng.random() < 0.5:
            u, v = units[int(rng.integers(0, len(units)))], units[int(rng.integers(0, len(units)))]
            ref, rem = (u * 40)[int(rng.integers(0, 4)):][:36], (v * 40)[:int(rng.integers(14, 30))]
        else:
            ref, rem = rand(rng, 36, b"AC"), rand(rng, int(rng.integers(14, 30)), b"AC")
        rows = min(len(rem), o["ext_max"])
        f = tie_facts(am.tables(am.codes(ref[:rows + band]), am.codes(rem[:rows]), -band, 2 * band + 1, o)[0])
        if (f["best_rows"] > 1 and f["best_slots"] > 1) if kind == "best" else f["last_best"] > 1:
            (c.tail if n & 1 else c.head)(ref, rem, bool(n & 2))
            n += 1
    return c.done()


def bonus_reads():
    """20 matching bases, two that match nothing, three matching.  Under the defaults the best cell is (20, 20) with 20 and the
    last row's best is (25, 25) with 20 - 8 + 3: BONUS_DIFF = 5"""
    rng = np.random.default_rng(9)
    ref = rand(rng, 40)
    return ref, ref[:20] + b"NN" + ref[22:25]


BONUS_DIFF = 5


def bonus_case(end_bonus):
    c = Case(band=8, end_bonus=end_bonus)
    ref, rem = bonus_reads()
    for rev in (False, True):
        c.tail(ref, rem, rev)
        c.head(ref, rem, rev)
    return c.done()


def ext_wide_case():
    """band = 1023, W = 2047: a tail of 70 rows and a head of 3 on the reverse strand"""
    rng = np.random.default_rng(10)
    c = Case(band=1023)
    ref = rand(rng, 1200)
    c.tail(ref, near(rng, ref[:30] + ref[33:], 70, 4))
    c.head(ref[:1100], near(rng, ref, 3, 1), True)
    return c.done()


def many_pins(rng, n_pins):
    """a read of n_pins pins, k-mers 4 .. 7 bases apart, the bases between them in turn equal, one mismatch, a gap, a core"""
    ref, read, anchors = bytearray(), bytearray(), []
    for p in range(n_pins):
        pin = rand(rng, K)
        ref += pin
        read += pin
        anchors.append((len(ref) - 1, len(read) - 1))
        if p + 1 == n_pins:
            break
        seg = rand(rng, 4 + p % 4)
        kind = p % 5
        if kind == 0:
            q = seg
        elif kind == 1:
            q = seg[:2] + bytes([differ(rng, seg[2])]) + seg[3:]
        elif kind == 2:
            q = seg[:2] + seg[3:]
        elif kind == 3:
            q = seg[:2] + b"T" + seg[2:]
        else:
            q = ends_differ(rng, seg, seg)
        ref += seg
        read += q
    return bytes(ref), bytes(read), anchors


def slots_case():
    """reads of 255, 256 and 257 slots between reads of one pin (two slots, the fewest a mapped read has): k_align_classify's
    blocks of 256 slots and its per-wavefront counters, slot_read and the slots' offsets across them"""
    rng = np.random.default_rng(11)
    c = Case(band=4)
    small = rand(rng, 40)
    c.tail(small, near(rng, small, 12))
    for i, n_slots in enumerate((255, 256, 257)):
        ref, read, anchors = many_pins(rng, n_slots - 1)
        c.read(c.contig(ref), read, anchors, rev=i == 1)
        c.head(small, near(rng, small, 9), rev=i == 2)
    return c.done()


def jobs_case(unmapped_at):
    """65 jobs around a wavefront of reads, one of them unmapped"""
    rng = np.random.default_rng(12)
    c = Case(band=4)
    for i in range(65):
        if i == unmapped_at:
            c.unmapped(rand(rng, 17))
            continue
        T = rand(rng, 5 + i % 4)
        c.core(T, mutate(rng, T, (i % 3) - 1, 1), rev=bool(i & 1))
    return c.done()


def plans_case():
    rng = np.random.default_rng(13)
    c = Case(band=6)
    X, Y = rand(rng, 7), rand(rng, 12)
    P3 = rand(rng, K)
    # 0: adjacent pins, an empty K_EQUAL segment
    t = c.contig(P1 + P2)
    c.read(t, P1 + P2, [(K - 1, K - 1), (2 * K - 1, 2 * K - 1)])
    # 1, 2: tl = 0 with ql > 0, and the mirror
    c.read(t, P1 + X + P2, [(K - 1, K - 1), (2 * K - 1, 2 * K + 6)], True)
    t = c.contig(P1 + X + P2)
    c.read(t, P1 + P2, [(K - 1, K - 1), (2 * K + 6, 2 * K - 1)])
    # 3, 4: an anchor that is k beyond the last pin in r but not in q, and the reverse, before one that is a pin
    t = c.contig(P1 + Y + P3 + Y + P2)
    full = P1 + Y + P3 + Y + P2
    last = (len(full) - 1, len(full) - 1)
    c.read(t, full, [(K - 1, K - 1), (2 * K + 11, 2 * K - 3), last])
    c.read(t, full, [(K - 1, K - 1), (2 * K - 3, 2 * K + 11), last], True)
    # 5, 6: anchors out of order
    mid = (2 * K + 11, 2 * K + 11)
    c.read(t, full, [(K - 1, K - 1), last, mid])
    c.read(t, full, [mid, (K - 1, K - 1), last], True)
    # 7, 8: one anchor at r = q = k - 1, and at the last base of both
    t = c.contig(P1 + Y)
    c.read(t, P1 + near(rng, Y, 12, 1), [(K - 1, K - 1)])
    t = c.contig(Y + P2)
    c.read(t, near(rng, Y, 12, 1) + P2, [(12 + K - 1, 12 + K - 1)])
    # 9, 10: a pin k-mer that does not match the reference beside the same read with the pin intact
    t = c.contig(P1 + Y + P2 + X)
    bad = bytearray(P2)
    bad[4] = differ(rng, bad[4])
    for pin in (P2, bytes(bad)):
        c.read(t, P1 + near(rng, Y, 12, 0) + pin + X, [(K - 1, K - 1), (2 * K + 11, 2 * K + 11)])
    # 11, 12: the last contig of the index, the chain touching its first and its last base
    t = c.contig(P1 + Y + P2)
    q = ends_differ(rng, Y, Y)
    c.read(t, P1 + q + P2, [(K - 1, K - 1), (2 * K + 11, 2 * K + 11)])
    c.read(t, P1 + q + P2, [(K - 1, K - 1), (2 * K + 11, 2 * K + 11)], True)
    return c.done()


def _build():
    cases = {}
    for sc in OPTSETS:
        for band in BAND_SHAPES:
            cases[f"band{band}_{sc}"] = band_case(sc, band)
        cases[f"lane_{sc}"] = lane_case(sc)
        for band in (0, 1, 5, 40):
            cases[f"rand{band}_{sc}"] = random_case(sc, band, 45 if band == 40 else 60)  # (225 pairs per option set)
    cases["ext_limits"] = ext_limits_case()
    cases["ext_band0"] = ext_band0_case()
    cases["ext_wide"] = ext_wide_case()
    for sc in TIE_SCORING:
        for kind in TIE_KINDS:
            cases[f"tie_{sc}_{kind}"] = tie_case(sc, kind)
    for name, bonus in (("eq", BONUS_DIFF), ("less", BONUS_DIFF - 1), ("0", 0), ("max", 1 << 16)):
        cases[f"bonus_{name}"] = bonus_case(bonus)
    cases["plans"] = plans_case()
    cases["slots"] = slots_case()
    for at in (0, 63, 64):
        cases[f"jobs_unmapped{at}"] = jobs_case(at)
    return cases


CASES = _build()
BAND_CASES = [n for n in CASES if n.startswith("band")]
LANE_CASES = [n for n in CASES if n.startswith("lane_")]
RANDOM_CASES = [n for n in CASES if n.startswith("rand")]
TIE_CASES = [n for n in CASES if n.startswith("tie_")]
SMALL_MATRIX = 20000

_EXPECTED = {}


def bits_of(T, Q, lo, W, o, tabs):
    """the traceback bits the model's tables imply, by the stated preference: H's source (diagonal, then E, then F), E continues,
    F continues (an open gap is continued rather than another opened, of equal values); row 0 is one deletion; a slot outside
    the matrix holds 0"""
    H, E, F, at = tabs
    go = o["gap_open"]
    out = np.zeros((len(Q) + 1, W), np.uint8)
    for i in range(len(Q) + 1):
        for L in range(W):
            j = i + lo + L
            if j < 0 or j > len(T) or (i == 0 and j == 0):
                continue
            if i == 0:
                out[i, L] = 1 | (4 if j > 1 else 0)
                continue
            h = at(H, i, j)
            if j > 0 and at(H, i - 1, j - 1) > am.NONE // 2 and \
                    h == at(H, i - 1, j - 1) + (o["match"] if am.same(T[j - 1], Q[i - 1]) else -o["mismatch"]):
                src = 0
            elif h == at(E, i, j):
                src = 1
            else:
                assert h == at(F, i, j)
                src = 2
            ce = at(E, i, j - 1) >= at(H, i, j - 1) - go
            cf = at(F, i - 1, j) >= at(H, i - 1, j) - go
            out[i, L] = src | (4 if ce else 0) | (8 if cf else 0)
    return out.reshape(-1)


def matrix_facts(T, Q, lo, W, o, tabs):
    """of one matrix: its bits (small matrices), the cells that hold the largest H as (rows, slots), the last row's columns that
    hold its largest H"""
    H = np.array(tabs[0], np.int64)
    return dict(H=H, lo=lo, shape=(len(Q) + 1, W), bits=bits_of(T, Q, lo, W, o, tabs) if (len(Q) + 1) * W < SMALL_MATRIX else None,
                **tie_facts(H))


def expected(name):
    """-> (recs, cigars, counts, matrices): align_model.align_mapped's answer, and matrix_facts of every matrix in the order the
    model fills them: read by read, head, segments, tail, which is the order of the slots that have cells"""
    if name not in _EXPECTED:
        contigs, reads, hits, chains, k, ao = CASES[name]
        seen, plain = [], am.tables

        def spy(T, Q, lo, W, o):
            tabs = plain(T, Q, lo, W, o)
            seen.append(matrix_facts(T, Q, lo, W, o, tabs))
            return tabs
        # the cell a matrix's walk starts from and its score, as extension and core_align of the model choose it
        plain_ext, plain_core = am.extension, am.core_align

        def ext_spy(T_left, Q_rem, o, cnt):
            n = len(seen)
            cols, ei, ej = plain_ext(T_left, Q_rem, o, cnt)
            if len(seen) > n:
                m = seen[-1]
                m["res"] = (int(m.pop("H")[ei, ej - ei - m["lo"]]), ei, ej)
            return cols, ei, ej

        def core_spy(T, Q, o, cnt):
            cols, score = plain_core(T, Q, o, cnt)
            seen[-1].pop("H")
            seen[-1]["res"] = (score, len(Q), len(T))
            return cols, score
        am.tables, am.extension, am.core_align = spy, ext_spy, core_spy
        try:
            _, recs, cigars, cnt = am.align_mapped(contigs, reads, hits, chains, k, **ao)
        finally:
            am.tables, am.extension, am.core_align = plain, plain_ext, plain_core
        _EXPECTED[name] = (recs, cigars, cnt, seen)
    return _EXPECTED[name]


def check(got, name):
    """(recs, cigar, cigar_off) of a door against the model, field for field"""
    gr, gc, go = got[:3]
    recs, cigars, _, _ = expected(name)
    want = am.recs_array(recs)
    have = np.array([[int(r[f]) for f in am.REC_FIELDS] for r in gr], np.int64).reshape(len(recs), len(am.REC_FIELDS))
    assert np.array_equal(have, want), (name, have.tolist(), want.tolist())
    words, off = am.cigar_words(cigars)
    text = lambda w, o: ["".join(f"{int(x) >> 4}{am.OPS[int(x) & 15]}" for x in w[int(a):int(b)]) for a, b in zip(o[:-1], o[1:])]
    assert np.array_equal(go, off) and np.array_equal(gc, words), (name, text(gc, go), text(words, off))


def cigar_str(cg):
    return "".join(f"{L}{op}" for op, L in cg)


# a slot's kind (np2_io.h, np2_align_slot_t)
K_EQUAL, K_GAP, K_SNV, K_CORE, K_HEAD, K_TAIL, K_EMPTY = range(7)
SLOT_FIELDS = ("t0", "q0", "tl", "ql", "pre", "suf", "kind", "W", "lo", "over")


def model_slots(name):
    """the slots of every read from the rule's text (pins; head, segments, tail; the trim and the class; band_of and the
    extension's n and band): per read a list of dicts of SLOT_FIELDS, none for an unmapped read"""
    contigs, reads, hits, chains, k, ao = CASES[name]
    o = am.opts(**ao)
    band = o["band"]
    out = []
    for rd, h, ch in zip(reads, hits, chains):
        if h is None:
            out.append([])
            continue
        T, Q = am.codes(contigs[h["tid"]]), am.codes(rd)
        if h["rev"]:
            Q = am.rc_codes(Q)
        pins = am.pins_of(ch, k)
        slots = []

        def ext(kind, t_at, q_at, rem, ref_left):
            n = min(rem, o["ext_max"], ref_left + band)
            W = 2 * band + 1
            over = int(n > 0 and (W > am.MAX_W or (n + 1) * W > o["max_cells"]))
            slots.append(dict(t0=t_at, q0=q_at, tl=min(ref_left, n + band), ql=n, pre=0, suf=0, kind=kind if n else K_EMPTY, W=W, lo=-band, over=over))
        r0, q0 = pins[0][0] - k + 1, pins[0][1] - k + 1
        ext(K_HEAD, r0, q0, q0, r0)
        for (pr, pq), (r, q) in zip(pins[:-1], pins[1:]):
            t0, s0, tl, ql = pr + 1, pq + 1, r - k - pr, q - k - pq
            st, sq = T[t0:t0 + tl], Q[s0:s0 + ql]
            x = dict(t0=t0, q0=s0, tl=tl, ql=ql, pre=0, suf=0, kind=K_EQUAL, W=0, lo=0, over=0)
            if tl == ql and all(am.same(a, b) for a, b in zip(st, sq)):
                x["pre"] = tl
                slots.append(x)
                continue
            m = min(tl, ql)
            pre = 0
            while pre < m and am.same(st[pre], sq[pre]):
                pre += 1
            suf = 0
            while suf < m - pre and am.same(st[tl - 1 - suf], sq[ql - 1 - suf]):
                suf += 1
            x.update(t0=t0 + pre, q0=s0 + pre, tl=tl - pre - suf, ql=ql - pre - suf, pre=pre, suf=suf)
            if x["tl"] == 0 or x["ql"] == 0:
                x["kind"] = K_GAP
            elif x["tl"] == 1 and x["ql"] == 1:
                x["kind"] = K_SNV
            else:
                x["kind"] = K_CORE
                d = x["tl"] - x["ql"]
                x["lo"], x["W"] = min(0, d) - band, abs(d) + 2 * band + 1
                try:
                    assert am.band_of(x["tl"], x["ql"], band, o["max_cells"]) == (x["lo"], x["W"])
                except am.Overflow:
                    x["over"] = 1
            slots.append(x)
        r1, q1 = pins[-1][0] + 1, pins[-1][1] + 1
        ext(K_TAIL, r1, q1, len(Q) - q1, len(T) - r1)
        out.append(slots)
    return out


def case_text(name):
    """the case as tests/tools/align_core_test.cpp's `chains` mode reads it"""
    contigs, reads, hits, chains, k, ao = CASES[name]
    o = am.opts(**ao)
    lines = [" ".join([str(k)] + [str(o[f]) for f in am.DEFAULTS]), str(len(contigs))] + [c.decode() for c in contigs] + [str(len(reads))]
    for rd, h, ch in zip(reads, hits, chains):
        if h is None:
            lines.append(f"{rd.decode()} -1 0 0 0")
        else:
            lines.append(" ".join([rd.decode(), str(h["tid"]), str(h["rev"]), str(h["mapq"]), str(h["n"])] + [str(int(x)) for x in ch.reshape(-1)]))
    return "\n".join(lines) + "\n"


def refusal_call():
    """a small good call, three reads of which the middle one is unmapped, as (contigs, reads, hits array, chain, chain_off)"""
    contigs, reads, hits, chains, k, _ = jobs_case(1)
    contigs, reads, hits, chains = contigs, reads[:3], hits[:3], chains[:3]
    h = np.zeros(3, [("tid", "<i4")] + [(f, "<u4") for f in ("qlen", "qs", "qe", "rev", "ts", "te", "matches", "block", "mapq", "n", "s1", "s2")])
    for i, (x, rd) in enumerate(zip(hits, reads)):
        h[i]["tid"], h[i]["qlen"] = -1, len(rd)
        if x is not None:
            for f in ("tid", "rev", "mapq", "n"):
                h[i][f] = x[f]
    off = np.zeros(4, np.uint64)
    off[1:] = np.cumsum([len(c) for c in chains])
    return contigs, reads, h, np.concatenate(chains).astype(np.uint32).reshape(-1), off


def _set(what, i, field, value):
    def change(hits, chain, off, k):
        {"hits": hits, "chain": chain, "off": off}[what][i][field] = value
        return k
    return change


def _set_flat(what, i, value):
    def change(hits, chain, off, k):
        {"chain": chain, "off": off}[what][i] = value
        return k
    return change


# one violation of each validation rule of the two doors: (label, the change to refusal_call()'s arrays, words of the message).
# Read 2's chain is pairs 2 and 3 of `chain`: its second anchor is the flat entries 6 (r) and 7 (q).
REFUSALS = [
    ("tid", _set("hits", 2, "tid", 1), ("read 2", "tid 1", "contig")),
    ("qlen", _set("hits", 0, "qlen", 7), ("read 0", "qlen is 7")),
    ("n_zero", lambda hits, chain, off, k: (hits[2].__setitem__("n", 0), off.__setitem__(3, off[2]), k)[2], ("read 2", "n = 0")),
    ("r_low", _set_flat("chain", 6, K - 2), ("read 2, anchor 1", "r = 9")),
    ("r_high", _set_flat("chain", 6, 10 ** 6), ("read 2, anchor 1", "r = 1000000")),
    ("q_low", _set_flat("chain", 7, K - 2), ("read 2, anchor 1", "q = 9")),
    ("q_high", _set_flat("chain", 1, 10 ** 6), ("read 0, anchor 0", "q = 1000000")),
    ("off_descends", _set_flat("off", 2, 1), ("read 1", "chain_off descends")),
    ("off_and_n", _set("hits", 2, "n", 1), ("read 2", "n is 1", "2 anchors")),
    ("off_unmapped", lambda hits, chain, off, k: (off.__setitem__(2, 3), k)[1], ("read 1", "unmapped", "1 anchors")),
    # (the device door has the index's k to compare with; the host door has the mapper's range, and is given k - 1)
    ("k", lambda hits, chain, off, k: k + 1, ("k = 11", "k = 12")),
]


# every case's matrix cells, cores and extensions within the limits (the model's count; test_alignchain_cpu.py holds the model to it)
CELLS = {
    "band0_m15": 117, "band31_m15": 13561, "band32_m15": 9372, "band63_m15": 18105, "band64_m15": 18389, "band1023_m15": 122850,
    "lane_m15": 33867, "rand0_m15": 33104, "rand1_m15": 46843, "rand5_m15": 51767, "rand40_m15": 145320, "band0_x31": 117,
    "band31_x31": 13561, "band32_x31": 9372, "band63_x31": 18105, "band64_x31": 18389, "band1023_x31": 122850, "lane_x31": 33867,
    "rand0_x31": 41814, "rand1_x31": 41404, "rand5_x31": 62257, "rand40_x31": 147472, "band0_m1x0": 117, "band31_m1x0": 13561,
    "band32_m1x0": 9372, "band63_m1x0": 18105, "band64_m1x0": 18389, "band1023_m1x0": 122850, "lane_m1x0": 33867,
    "rand0_m1x0": 35567, "rand1_m1x0": 44220, "rand5_m1x0": 71696, "rand40_m1x0": 157390, "band0_m1x1": 117, "band31_m1x1": 13561,
    "band32_m1x1": 9372, "band63_m1x1": 18105, "band64_m1x1": 18389, "band1023_m1x1": 122850, "lane_m1x1": 33867,
    "rand0_m1x1": 40091, "rand1_m1x1": 39560, "rand5_m1x1": 67943, "rand40_m1x1": 131368, "band0_x4o0": 117, "band31_x4o0": 13561,
    "band32_x4o0": 9372, "band63_x4o0": 18105, "band64_x4o0": 18389, "band1023_x4o0": 122850, "lane_x4o0": 33867,
    "rand0_x4o0": 46526, "rand1_x4o0": 41691, "rand5_x4o0": 60538, "rand40_x4o0": 131992, "band0_dflt": 117, "band31_dflt": 13561,
    "band32_dflt": 9372, "band63_dflt": 18105, "band64_dflt": 18389, "band1023_dflt": 122850, "lane_dflt": 33867,
    "rand0_dflt": 47319, "rand1_dflt": 38082, "rand5_dflt": 63038, "rand40_dflt": 140224, "ext_limits": 14501, "ext_band0": 176,
    "ext_wide": 153525, "tie_x0_best": 5200, "tie_x0_end": 9250, "tie_m1x1_best": 5200, "tie_m1x1_end": 9025, "bonus_eq": 1768,
    "bonus_less": 1768, "bonus_0": 1768, "bonus_max": 1768, "plans": 1196, "slots": 9171, "jobs_unmapped0": 4637,
    "jobs_unmapped63": 4607, "jobs_unmapped64": 4653,
}
