"""Records for the tests of the read front end (test_front_cases_cpu.py, test_gpu_front_edges.py): hand-built records with
the values the rule of front_model.py gives them written out, and a seeded generator that fills a ledger of the shapes it
produced.  They are built for the edges of the columnariser (csrc/np2_front.hip), which takes 32 columns a lane and 2048 a
pass: anchors (runs of 8 equal columns) that straddle a lane or a pass, anchors a whole pass away from either end, records without
any, and stream lengths on either side of every such boundary.

Junk: a stretch of 1-column X, I and D ops (in that order, over and over).  None of its columns is an equal one, so an
unbroken stretch never holds an anchor.  A junk stretch of n columns has (n + 1) // 3 insertions and so moves on by
tc(n) = n - (n + 1) // 3 contig positions."""
import functools

import numpy as np

import front_model as fm

REFS = [("edgeE", 20000), ("edgeO", 20011)]  # an even and an odd length
LOWER = (300, 500)     # a soft-masked stretch: never byte-equal to a read
N_RUN = (9000, 9020)   # N over N is byte-equal: it counts
R_AT = 12000


def front_opts():
    """only the trim decides what is kept: a record is dropped exactly when it has no anchor"""
    from nextpolish2_amd import io as np2io
    return np2io.FrontOpts(min_read_len=0, min_map_len=0, min_map_fra=0.0, max_clip_len=100000)


@functools.lru_cache(None)
def contig(tid):
    rng = np.random.default_rng(100 + tid)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, REFS[tid][1])].tobytes().decode()
    s = s[:LOWER[0]] + s[LOWER[0]:LOWER[1]].lower() + s[LOWER[1]:]
    s = s[:N_RUN[0]] + "N" * (N_RUN[1] - N_RUN[0]) + s[N_RUN[1]:]
    return s[:R_AT] + "R" + s[R_AT + 1:]


def tc(n, phase=0):
    """contig positions a junk stretch of n columns consumes (its X and D columns)"""
    return sum(1 for k in range(n) if "XID"[(k + phase) % 3] != "I")


def build(ref, pos, pieces, rng, tid=0, name=b"r"):
    """-> a record dict.  pieces, each (kind, n[, extra]):
      M = X  n columns under that op; the read carries what a BAM can of the contig's letter (M, =) or another letter (X)
      I D    one op of n columns; S H  a clip of n
      J      n junk columns (extra: the phase the X, I, D cycle starts at)
      XI     n times 1X 1I
      Q      (op, letters): one M, X or I op that carries exactly these read letters
      0      a zero-length op (n is the op letter)"""
    cigar, seq = [], []
    ts = pos
    acgt = "ACGT"

    def other(c):
        return "A" if c != "A" else "C"

    def ins(n):
        return [acgt[i] for i in rng.integers(0, 4, n)]
    for pc in pieces:
        kind, n = pc[0], pc[1]
        if kind in ("M", "="):
            cigar.append((kind, n))
            seq += [fm.bam_letter(c) for c in ref[ts:ts + n]]
            ts += n
        elif kind == "X":
            cigar.append(("X", n))
            seq += [other(c) for c in ref[ts:ts + n]]
            ts += n
        elif kind == "I":
            cigar.append(("I", n))
            seq += ins(n)
        elif kind == "D":
            cigar.append(("D", n))
            ts += n
        elif kind == "S":
            cigar.append(("S", n))
            seq += ins(n)
        elif kind == "H":
            cigar.append(("H", n))
        elif kind == "J":
            phase = pc[2] if len(pc) > 2 else 0
            for k in range(n):
                op = "XID"[(k + phase) % 3]
                cigar.append((op, 1))
                if op == "X":
                    seq.append(other(ref[ts]))
                elif op == "I":
                    seq += ins(1)
                if op != "I":
                    ts += 1
        elif kind == "XI":
            for _ in range(n):
                cigar += [("X", 1), ("I", 1)]
                seq.append(other(ref[ts]))
                seq += ins(1)
                ts += 1
        elif kind == "Q":
            op, letters = n, pc[2]
            cigar.append((op, len(letters)))
            seq += list(letters)
            if op != "I":
                ts += len(letters)
        elif kind == "0":
            cigar.append((n, 0))
        else:
            raise ValueError(kind)
    assert ts <= len(ref), (name, pos, ts)
    return dict(tid=tid, pos=pos, mapq=60, flag=0, cigar=cigar, seq="".join(seq), name=name)


M, J = "M", "J"
ALL16 = "=ACMGRSVTWYHKDBN"
# name -> (pos, pieces, expected (shift, new_len, aln_t_s, aln_t_e inclusive, n_cols) or None, contig or None for both).
# Every expectation is derived by hand: shift = the columns before the first anchor, new_len = the columns up to the end of
# the last one, aln_t_s = pos + the contig positions the dropped head consumes, aln_t_e = aln_t_s + the kept columns that
# are no insertion - 1.
NAMED = {
    "pos_zero": (0, [(M, 50)], (0, 50, 0, 49, 50), None),
    # [488, 500) is lower case: the first 12 columns never match, the anchor moves past them
    "lower_case_head": (488, [(M, 60)], (12, 60, 500, 547, 48), None),
    # head junk h, then 100 equal columns: the first anchor is columns h .. h + 7; tc(24) = 16, tc(25) = 17, tc(31) = 21,
    # tc(32) = 21, tc(33) = 22: it ends on the last column of lane 0, on column 0 and 6 of lane 1, or lies wholly in lane 1
    "head_junk_24": (600, [(J, 24), (M, 100)], (24, 124, 616, 715, 100), None),
    "head_junk_25": (610, [(J, 25), (M, 100)], (25, 125, 627, 726, 100), None),
    "head_junk_31": (620, [(J, 31), (M, 100)], (31, 131, 641, 740, 100), None),
    "head_junk_32": (630, [(J, 32), (M, 100)], (32, 132, 651, 750, 100), None),
    "head_junk_33": (640, [(J, 33), (M, 100)], (33, 133, 662, 761, 100), None),
    # tc(2041) = 1361, tc(2047) = tc(2048) = 1365: the anchor straddles the first two passes, or opens the second
    "head_junk_2041": (650, [(J, 2041), (M, 100)], (2041, 2141, 2011, 2110, 100), None),
    "head_junk_2047": (660, [(J, 2047), (M, 100)], (2047, 2147, 2025, 2124, 100), None),
    "head_junk_2048": (670, [(J, 2048), (M, 100)], (2048, 2148, 2035, 2134, 100), None),
    # the mirror images: 128 columns, the last t of them junk, so the last anchor is columns 120 - t .. 127 - t
    "tail_junk_1": (680, [(M, 127), (J, 1)], (0, 127, 680, 806, 127), None),
    "tail_junk_7": (690, [(M, 121), (J, 7)], (0, 121, 690, 810, 121), None),
    "tail_junk_25": (700, [(M, 103), (J, 25)], (0, 103, 700, 802, 103), None),   # columns 95 .. 102: over the lane edge at 96
    "tail_junk_31": (710, [(M, 97), (J, 31)], (0, 97, 710, 806, 97), None),      # ends on column 0 of lane 3
    "tail_junk_32": (720, [(M, 96), (J, 32)], (0, 96, 720, 815, 96), None),      # ends on the last column of lane 2
    "tail_junk_33": (730, [(M, 95), (J, 33)], (0, 95, 730, 824, 95), None),
    # 4096 columns: the last anchor is columns 2041 .. 2048, over the edge of the second pass
    "tail_junk_2047": (740, [(M, 2049), (J, 2047)], (0, 2049, 740, 2788, 2049), None),
    # 4196 columns in three passes: the last two hold junk alone
    "last_anchor_two_passes_early": (750, [(M, 1000), (J, 3196)], (0, 1000, 750, 1749, 1000), None),
    # one run of exactly 8 serves as both anchors; tc(28) = 19, tc(2044) = 1363
    "one_run_over_a_lane_edge": (760, [(J, 28), (M, 8), (J, 20)], (28, 36, 779, 786, 8), None),
    "one_run_over_a_pass_edge": (770, [(J, 2044), (M, 8), (J, 100)], (2044, 2052, 2133, 2140, 8), None),
    # no anchor
    "clips_only": (780, [("S", 50)], None, None),
    "seven_equal": (790, [(M, 7)], None, None),
    "junk_40": (800, [(J, 40)], None, None),
    "junk_4100": (810, [(J, 4100)], None, None),           # both searches run through all three passes
    "seven_junk_seven": (820, [(M, 7), (J, 1), (M, 7)], None, None),
    # stream lengths: 5 junk columns (tc = 3), n equal ones, 2 junk columns
    "n_cols_8": (830, [(J, 5), (M, 8), (J, 2)], (5, 13, 833, 840, 8), None),
    "n_cols_9": (840, [(J, 5), (M, 9), (J, 2)], (5, 14, 843, 851, 9), None),
    "n_cols_15": (850, [(J, 5), (M, 15), (J, 2)], (5, 20, 853, 867, 15), None),
    "n_cols_16": (860, [(J, 5), (M, 16), (J, 2)], (5, 21, 863, 878, 16), None),
    "n_cols_17": (870, [(J, 5), (M, 17), (J, 2)], (5, 22, 873, 889, 17), None),
    "n_cols_31": (880, [(J, 5), (M, 31), (J, 2)], (5, 36, 883, 913, 31), None),
    "n_cols_32": (890, [(J, 5), (M, 32), (J, 2)], (5, 37, 893, 924, 32), None),
    "n_cols_33": (900, [(J, 5), (M, 33), (J, 2)], (5, 38, 903, 935, 33), None),
    "n_cols_2047": (910, [(J, 5), (M, 2047), (J, 2)], (5, 2052, 913, 2959, 2047), None),
    "n_cols_2048": (920, [(J, 5), (M, 2048), (J, 2)], (5, 2053, 923, 2970, 2048), None),
    "n_cols_2049": (930, [(J, 5), (M, 2049), (J, 2)], (5, 2054, 933, 2981, 2049), None),
    "n_cols_4096": (940, [(J, 5), (M, 4096), (J, 2)], (5, 4101, 943, 5038, 4096), None),
    # ... and with an even shift (tc(4) = 3), and none
    "n_cols_16_even_shift": (950, [(J, 4), (M, 16), (J, 2)], (4, 20, 953, 968, 16), None),
    "n_cols_2048_even_shift": (960, [(J, 4), (M, 2048), (J, 2)], (4, 2052, 963, 3010, 2048), None),
    "n_cols_2048_no_shift": (970, [(M, 2048)], (0, 2048, 970, 3017, 2048), None),
    "n_cols_4096_no_shift": (980, [(M, 4096)], (0, 4096, 980, 5075, 4096), None),
    # 3202 ops: 20 equal columns, 1600 times 1X 1I, 20 equal columns; 1640 of the 3240 columns consume the contig
    "alternating_x_i": (990, [(M, 20), ("XI", 1600), (M, 20)], (0, 3240, 990, 2629, 3240), None),
    "zero_length_ops": (1000, [(M, 30), ("0", "I"), ("0", "M"), (M, 30)], (0, 60, 1000, 1059, 60), None),
    # op boundaries on columns 32, 64 and 2048; 2153 columns, 32 of them insertions
    "op_edges_32_64_2048": (1010, [(M, 32), ("I", 32), (M, 1984), ("D", 5), (M, 100)], (0, 2153, 1010, 3130, 2153), None),
    "eq_x_and_clips": (1020, [("H", 5), ("S", 10), ("=", 50), ("X", 1), ("=", 50), ("S", 7), ("H", 3)], (0, 101, 1020, 1120, 101), None),
    "h_s_m": (1030, [("H", 5), ("S", 10), (M, 100)], (0, 100, 1030, 1129, 100), None),  # aln_q_e stays 0 until the end
    # all 16 codes in X columns, lower case and bytes outside the table in an insertion; 67 columns, 11 of them insertions
    "all_codes": (1040, [(M, 20), ("Q", "X", ALL16), ("Q", "I", "acgtnrykm.z"), (M, 20)], (0, 67, 1040, 1095, 67), None),
    "d_before_the_tail_anchor": (1050, [(M, 30), ("D", 3), (M, 8)], (0, 41, 1050, 1090, 41), None),
    # 5 junk columns (tc = 3) up to the N run, an anchor of 8 N over N, 6 junk columns (tc = 4), 30 equal columns:
    # were N over N no match, shift would be 19
    "anchor_of_n": (8997, [(J, 5), (M, 8), (J, 6), (M, 30)], (5, 49, 9000, 9041, 44), None),
    "ends_at_the_contig_end_even": (19950, [(M, 50)], (0, 50, 19950, 19999, 50), 0),
    "ends_at_the_contig_end_odd": (19961, [(M, 50)], (0, 50, 19961, 20010, 50), 1),
}
# columns 20 .. 46 of all_codes: = 4, A 0, C 1, M 6, G 2, R S V 4, T 3, W Y H K D B 4, N 5; then | 8: a 8, c 9, g a, t b,
# n d, r y k c, m e, and . z -> N d
ALL_CODES_NIBBLES = (20, "4016244434444445" + "89abdcccedd")

PANIC_POS = 1100  # records the reference panics on ("Unknown cigar") start here: never part of the pileups above

HEAD_JUNK = (0, 0, 0, 1, 5, 7, 24, 25, 31, 32, 33, 2041, 2047, 2048)
TAIL_JUNK = (0, 0, 0, 1, 7, 25, 31, 32, 33, 2047)
BODY = (8, 9, 15, 16, 17, 31, 32, 33, 40, 100, 333, 1000, 2047, 2048, 2049, 4096)
NO_ANCHOR = ([("S", 30)], [(M, 7)], [(J, 40)], [(J, 2100)], [(J, 4100)])


def panic_record(tid, op):
    """80 equal columns with a 3N or 3P op in their middle"""
    rec = build(contig(tid), PANIC_POS, [(M, 80)], np.random.default_rng(1), tid, b"panic_" + op.encode())
    rec["cigar"] = [(M, 40), (op, 3), (M, 40)]
    return rec


def _body(rng, n):
    """n kept columns: M / = pieces of 8 .. 400 columns with 1 .. 3 junk columns between them; both ends are pieces"""
    out = []
    left = n
    while left:
        p = min(left, int(rng.integers(8, 401)))
        if left - p < 9:
            p = left
        out.append(("M" if rng.random() < 0.5 else "=", p))
        left -= p
        if left:
            j = min(int(rng.integers(1, 4)), left - 8)
            out.append((J, j, int(rng.integers(0, 3))))
            left -= j
    return out


@functools.lru_cache(None)
def records(tid, seed=20, n=400):
    """-> (records of contig tid in ascending order of POS, every POS its own; {name: front_model.front's result};
    ledger of the generated records alone)"""
    ref = contig(tid)
    L = len(ref)
    rng = np.random.default_rng(seed + tid)
    recs = []
    for name, (pos, pieces, _, only) in NAMED.items():
        if only is None or only == tid:
            recs.append(build(ref, pos, pieces, rng, tid, name.encode()))
    used = {r["pos"] for r in recs} | {PANIC_POS}
    built_without = 0
    gen = []
    for i in range(n):
        if rng.random() < 0.04:
            pieces = list(NO_ANCHOR[int(rng.integers(0, len(NO_ANCHOR)))])
            built_without += 1
        else:
            pieces = [(J, int(rng.choice(HEAD_JUNK)))] + _body(rng, int(rng.choice(BODY))) + [(J, int(rng.choice(TAIL_JUNK)))]
            pieces = [p for p in pieces if p[1]]
            if rng.random() < 0.2:
                pieces = [("S", int(rng.integers(1, 40)))] + pieces
            if rng.random() < 0.2:
                pieces = pieces + [("S", int(rng.integers(1, 40)))]
        span = sum(tc(p[1], p[2] if len(p) > 2 else 0) if p[0] == J else p[1] for p in pieces if p[0] in (M, "=", J))
        while True:  # behind the hand-built records and the soft-masked stretch
            pos = int(rng.integers(1300, L - span + 1))
            if pos not in used:
                break
        used.add(pos)
        name = b"g%d_%d" % (tid, i)
        gen.append(name)
        recs.append(build(ref, pos, pieces, rng, tid, name))
    recs.sort(key=lambda r: r["pos"])
    model = {r["name"].decode(): fm.front(ref, r) for r in recs}
    ledger = dict(first_lane=set(), first_chunk=set(), last_chunk=set(), last_chunk_from_end=set(), first_over_lane=set(), first_over_chunk=set(),
                  last_over_lane=set(), last_over_chunk=set(), n_cols_mod32=set(), n_cols=set(), n_cols_mod2048_is_0=set(),
                  shift_parity_at=set(), built_without_anchor=built_without, without_anchor=0, kept=0)
    n_cols_all = {r["name"].decode(): sum(l for op, l in r["cigar"] if op in "M=XID") for r in recs}
    for nm in gen:
        m = model[nm.decode()]
        if m is None:
            ledger["without_anchor"] += 1
            continue
        shift, new_len, _, _, n_cols, _ = m
        ledger["kept"] += 1
        e1, e2 = shift + 7, new_len - 1  # the last column of the first and of the last anchor
        ledger["first_lane"].add((e1 % 2048) // 32)
        ledger["first_chunk"].add(e1 // 2048)
        ledger["last_chunk"].add(e2 // 2048)
        ledger["last_chunk_from_end"].add((n_cols_all[nm.decode()] - 1) // 2048 - e2 // 2048)
        ledger["first_over_lane"].add(e1 % 32 < 7)
        ledger["first_over_chunk"].add(e1 % 2048 < 7)
        ledger["last_over_lane"].add(e2 % 32 < 7)
        ledger["last_over_chunk"].add(e2 % 2048 < 7)
        ledger["n_cols_mod32"].add(n_cols % 32)
        ledger["n_cols"].add(n_cols)
        ledger["n_cols_mod2048_is_0"].add(n_cols % 2048 == 0)
        ledger["shift_parity_at"].add((n_cols, shift & 1))
    return recs, model, ledger
