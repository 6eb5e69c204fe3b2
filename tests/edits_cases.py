"""Inputs for the edit tests (test_edits_cpu.py, test_gpu_edits.py): hand-derived cases with their expected records
written out, and a seeded generator of outputs the way a polish writes them (clean bases, substitutions, bases dropped,
bases added, and regions replaced whole with every base stamped with the region's start)."""
import numpy as np


def out_of(*pieces):
    """pieces of (bases, first position | list of positions) -> (bases, pos): a str piece with one position is stamped
    base by base from it on (an identical copy of the contig there), with a list as given"""
    b, p = b"", []
    for s, at in pieces:
        s = s.encode() if isinstance(s, str) else s
        b += s
        p += list(at) if isinstance(at, (list, tuple, range)) else list(range(at, at + len(s)))
    assert len(b) == len(p)
    return b, np.array(p, dtype=np.uint32)


def rec(ref_pos, out_off, ref, alt, kind):
    return dict(ref_pos=ref_pos, out_off=out_off, ref=ref.encode(), alt=alt.encode(), kind=kind)


# name -> (ref, (bases, pos), expected records, expected totals that matter, expected VCF (POS, REF, ALT) per record)
HAND = {}


def _case(name, ref, out, recs, vcf, **totals):
    HAND[name] = (ref.encode(), out, recs, totals, vcf)


R10 = "ACGTACGTAC"
_case("snv", R10, out_of(("ACGT", 0), ("G", 4), ("CGTAC", 5)), [rec(4, 4, "A", "G", "SNV")], [(5, b"A", b"G")], raw_runs=1, same_runs=0)
# region [3, 6] = TACG replaced by TTGG, every base stamped 3: suffix G, then prefix T
_case("mnv_in_a_region", R10, out_of(("ACG", 0), ("TTGG", [3] * 4), ("TAC", 7)), [rec(4, 4, "AC", "TG", "MNV")], [(5, b"AC", b"TG")],
      raw_runs=1, same_runs=0)
# region [3, 6] = TACG replaced by TGG: suffix G, prefix T, what is left has two lengths
_case("cpx", R10, out_of(("ACG", 0), ("TGG", [3] * 3), ("TAC", 7)), [rec(4, 4, "AC", "G", "CPX")], [(5, b"AC", b"G")], raw_runs=1)
# region [2, 7] = GTACGT replaced by GAACCT: the substitutions at 3 and 6 are ONE record, the equal bases between them inside it
_case("two_substitutions_one_region", R10, out_of(("AC", 0), ("GAACCT", [2] * 6), ("AC", 8)), [rec(3, 3, "TACG", "AACC", "MNV")],
      [(4, b"TACG", b"AACC")], raw_runs=1)
# GC AAAAA TCG: region [4, 6] = AAA replaced by AAAA; the suffix takes three, the A left moves to the homopolymer's left end
_case("ins_homopolymer", "GCAAAAATCG", out_of(("GCAA", 0), ("AAAA", [4] * 4), ("TCG", 7)), [rec(2, 2, "", "A", "INS")], [(2, b"C", b"CA")],
      raw_runs=1, bases_inserted=1, bases_deleted=0)
# GG CACACACA TT: positions 6, 7 (CA) have no output; CA rotates AC, CA, AC, CA down to position 2
_case("del_dinucleotide", "GGCACACACATT", out_of(("GGCACA", 0), ("CATT", 8)), [rec(2, 2, "CA", "", "DEL")], [(2, b"GCA", b"G")],
      raw_runs=1, bases_deleted=2)
# GC AAAAAA TC: an SNV at 3, then an A added at 6: it moves left to one past the SNV and no further
_case("shift_stopped_by_the_previous_edit", "GCAAAAAATC", out_of(("GCA", 0), ("G", 3), ("AA", 4), ("AA", [6, 6]), ("ATC", 7)),
      [rec(3, 3, "A", "G", "SNV"), rec(4, 4, "", "A", "INS")], [(4, b"A", b"G"), (4, b"A", b"AA")], raw_runs=2)
# the output covers positions 2 .. 8 of AAAAAATCGG: an A added at 4 moves left to `first` = 2 and no further; 0, 1, 9 lie outside
_case("shift_stopped_at_first", "AAAAAATCGG", out_of(("AA", 2), ("AA", [4, 4]), ("ATCG", 5)), [rec(2, 0, "", "A", "INS")],
      [(2, b"A", b"AA")], first=2, last=8, outside=3)
# position 0 holds TA: the T is an insertion before the contig's first base, anchored by the base after it
_case("ins_at_zero", "ACGTACGT", out_of(("TA", [0, 0]), ("CGTACGT", 1)), [rec(0, 0, "", "T", "INS")], [(1, b"A", b"TA")])
# region [0, 2] = ACG replaced by G: the suffix leaves a deletion of AC at 0, anchored by the G after it
_case("del_at_zero", "ACGTACGT", out_of(("G", [0]), ("TACGT", 3)), [rec(0, 0, "AC", "", "DEL")], [(1, b"ACG", b"G")])
_case("rewritten_the_same", R10, out_of(("ACG", 0), ("TACG", [3] * 4), ("TAC", 7)), [], [], raw_runs=1, same_runs=1, outside=0)
_case("first_and_last_inside", R10, out_of(("GTTCG", 2)), [rec(4, 2, "A", "T", "SNV")], [(5, b"A", b"T")], first=2, last=6, outside=5)
# case does not matter, N equals N; the records keep the bytes as they stand
_case("lower_case_and_n", "acgtNacgtn", out_of(("ATGTNACGTA", 0)), [rec(1, 1, "c", "T", "SNV"), rec(9, 9, "n", "A", "SNV")],
      [(2, b"c", b"T"), (10, b"n", b"A")], raw_runs=2, same_runs=0)
_case("lower_case_shift", "gcaaaaatcg", out_of(("GCAAAA", 0), ("AA", [6, 6]), ("TCG", 7)), [rec(2, 2, "", "A", "INS")], [(2, b"c", b"cA")])
_case("nothing_written", R10, out_of(), [], [], has_span=0, raw_runs=0, outside=10)


def random_case(seed, L, rate=0.02, span=None, alphabet=b"ACGT", ref=None):
    """a contig of L bases (drawn from `alphabet`, or `ref` as given) and a polish's output of it: (ref, bases, pos).
    rate: events per position; span: (first, last) or None for the whole contig."""
    rng = np.random.default_rng(seed)
    if ref is None:
        ref = bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=L).astype(np.uint8))
    assert len(ref) == L
    if L == 0:
        return ref, b"", np.zeros(0, dtype=np.uint32)
    first, last = span if span is not None else (0, L - 1)
    b, p = bytearray(), []
    q = first
    while q <= last:
        if rng.random() >= rate:
            b.append(ref[q])
            p.append(q)
            q += 1
            continue
        ev = int(rng.integers(0, 6))
        ln = int(min(last - q + 1, rng.integers(1, 12)))
        if ev == 0:  # substitution
            b.append(b"ACGT"[(b"ACGT".find(bytes([ref[q]]).upper()) + 1 + int(rng.integers(0, 3))) % 4])
            p.append(q)
            q += 1
        elif ev == 1:  # bases dropped
            q += ln
        elif ev == 2:  # bases added at q (a copy of the bases before them, often: something to shift)
            add = bytes(b[-ln:]) if len(b) >= ln and rng.random() < 0.7 else bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ln).astype(np.uint8))
            b += bytes([ref[q]]) + add
            p += [q] * (1 + len(add))
            q += 1
        elif ev == 3:  # a region rewritten the same, stamped with its start
            b += ref[q:q + ln]
            p += [q] * ln
            q += ln
        else:  # a region replaced: the contig's text with a base changed, dropped or doubled
            t = bytearray(ref[q:q + ln])
            at = int(rng.integers(0, ln))
            how = int(rng.integers(0, 3))
            if how == 0:
                t[at] = b"ACGT"[int(rng.integers(0, 4))]
            elif how == 1:
                del t[at]
            else:
                t.insert(at, t[at])
            b += t
            p += [q] * len(t)
            q += ln
    return ref, bytes(b), np.array(p, dtype=np.uint32)
