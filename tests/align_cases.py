"""The aligner's edge cases (include/np2_io.h: np2_map_align_*), shared by the CPU and the GPU tests: each is the smallest shape at
which one kernel or one branch of the rule's text can go wrong.  case(name) -> (contigs, reads, map options, align options, env);
expected(name) -> the model's (hits, recs, cigars, counts, map totals), computed once."""
import numpy as np

import align_model as am
import map_cases as mc
import map_model as mm

_B = np.frombuffer(b"ACGT", np.uint8)


def rand(n, seed):
    return bytearray(bytes(_B[np.random.default_rng(seed).integers(0, 4, n)]))


def other(ch, step=1):
    return b"ACGT"[(b"ACGT".index(bytes([ch]).upper()) + step) % 4]


def sub(read, at):
    read[at] = other(read[at])


CONTIG = bytes(rand(3000, 11))


def cut(a=500, n=600):
    return bytearray(CONTIG[a:a + n])


def two_subs(gap=5, at=300):
    r = cut()
    sub(r, at), sub(r, at + gap)
    return r


def _first_kmer_is_minimizer():
    for seed in range(100, 400):
        c = bytes(rand(1500, seed))
        if mm.sketch(c, 19, 19)[1][0] == 18:
            return c
    raise AssertionError("no seed puts a minimizer on a contig's first k-mer")


def _build():
    C = {}
    plain = [bytes(cut()), mm.revcomp(cut(900, 500)), bytes(cut(0, 400)), bytes(cut(2600, 400))]
    C["all_equal"] = ([CONTIG], plain, {}, {}, {})
    r_ins, r_del, r_snv = cut(), cut(), cut()
    r_ins[300:300] = b"GAT"
    del r_del[300:304]
    sub(r_snv, 300)
    C["pure_gaps_snv"] = ([CONTIG], [bytes(r_ins), bytes(r_del), bytes(r_snv), mm.revcomp(r_ins), mm.revcomp(r_del)], {}, {}, {})
    # a core of 6 x 6 (d = 0) and of 7 x 6 (d = 1): the band is 2 band + 1 + |d| diagonals wide
    d1 = two_subs(6)
    del d1[303]
    C["band_63"] = ([CONTIG], [bytes(two_subs())], {}, dict(band=31), {})
    C["band_64"] = ([CONTIG], [bytes(d1)], {}, dict(band=31), {})
    C["band_65"] = ([CONTIG], [bytes(two_subs()), mm.revcomp(d1)], {}, dict(band=32), {})
    C["band_129"] = ([CONTIG], [bytes(two_subs()), bytes(d1)], {}, dict(band=64), {})
    # an insertion of 2 and, 12 bases on, a deletion of 2 between two substitutions, no pin between them: one core with d = 0
    # whose best path lies on diagonal -2 for 12 columns
    z = cut()
    sub(z, 294), sub(z, 316)
    del z[310:312]
    z[298:298] = bytes([other(z[298], 2), other(z[297], 2)])
    C["band_touch"] = ([CONTIG], [bytes(z)], {}, dict(band=2), {})
    C["band_short"] = ([CONTIG], [bytes(z)], {}, dict(band=1), {})
    C["band_wide"] = ([CONTIG], [bytes(z)], {}, dict(band=40), {})
    # one and two read bases against three reference bases, none matching at either end
    c2 = bytearray(CONTIG)
    c2[800:803] = b"CGC"
    c2[799], c2[803] = ord("T"), ord("T")
    r1, r2 = bytearray(c2[500:1100]), bytearray(c2[500:1100])
    r1[300:303] = b"A"
    r2[300:303] = b"AA"
    C["core_rows_1_2"] = ([bytes(c2)], [bytes(r1), bytes(r2), mm.revcomp(r1)], {}, {}, {})
    contigs, reads, o = mc.case("read_length")
    C["one_pin"] = (contigs, reads, o, {}, {})
    e = cut()
    sub(e, len(e) - 3)
    C["end_bonus_equal"] = ([CONTIG], [bytes(e), mm.revcomp(e)], {}, dict(end_bonus=2), {})
    C["end_bonus_less"] = ([CONTIG], [bytes(e), mm.revcomp(e)], {}, dict(end_bonus=1), {})
    C["ext_max"] = ([CONTIG], plain, {}, dict(ext_max=3), {})
    c0 = _first_kmer_is_minimizer()
    C["head_no_reference"] = ([c0], [bytes(rand(40, 5)) + c0[:500], mm.revcomp(bytes(rand(40, 6)) + c0[:500]), c0[:300]], {}, {}, {})
    over = bytes(rand(300, 7)) + CONTIG[:400], CONTIG[2500:] + bytes(rand(300, 8))
    C["overhang"] = ([CONTIG], [over[0], over[1], mm.revcomp(over[0]), mm.revcomp(over[1])], {}, {}, {})
    # a base deleted from / inserted into an 8-base homopolymer
    c3 = bytearray(CONTIG)
    c3[800:808] = b"AAAAAAAA"
    c3[799], c3[808] = ord("C"), ord("G")
    hd, hi = bytearray(c3[500:1100]), bytearray(c3[500:1100])
    del hd[307]
    hi[307:307] = b"A"
    C["homopolymer"] = ([bytes(c3)], [bytes(hd), bytes(hi), mm.revcomp(hd), mm.revcomp(hi)], {}, {}, {})
    # a tandem repeat (unit 7, 8 copies) with one unit deleted / inserted: anchors inside it lie on two diagonals less than k apart
    c4 = bytearray(CONTIG)
    c4[800:856] = bytes(rand(7, 84)) * 8
    td, ti = bytearray(c4[500:1100]), bytearray(c4[500:1100])
    del td[342:349]
    ti[321:321] = c4[800:807]
    C["tandem"] = ([bytes(c4)], [bytes(td), bytes(ti), mm.revcomp(td), mm.revcomp(ti)], {}, {}, {})
    # a long tandem repeat (unit 7, 30 copies) with a unit deleted / inserted near either end of it, and a bandwidth that admits
    # a diagonal shift of 7 but not of 14: the chain shifts twice, pins lie between the two gaps, and left-alignment carries the
    # second gap through them to the first, where they merge and move on as one
    c5 = bytearray(CONTIG)
    c5[800:1010] = bytes(rand(7, 207)) * 30
    md, mi = bytearray(c5[500:1310]), bytearray(c5[500:1310])
    del md[475:482]
    del md[328:335]
    mi[475:475] = c5[800:807]
    mi[328:328] = c5[800:807]
    C["gaps_merge"] = ([bytes(c5)], [bytes(md), bytes(mi), mm.revcomp(md), mm.revcomp(mi)], dict(bandwidth=10), {}, {})
    # a contig that begins with a tandem repeat, reads with one and two units more, and an end bonus that pays for the insertion:
    # the head extension reaches the read's end, its insertion is left-aligned until one M column is left at the start
    u6 = bytes(rand(7, 408))
    c6 = u6 * 5 + bytes(rand(1200, 51))
    f1, f2 = u6 * 6 + c6[35:335], u6 * 7 + c6[35:335]
    C["first_column"] = ([c6], [f1, f2, mm.revcomp(f1)], {}, dict(end_bonus=60), {})
    n1, n2 = cut(), cut()
    n1[300] = ord("N")
    n2[3], n2[len(n2) - 4] = ord("N"), ord("n")
    C["n_bases"] = ([CONTIG], [bytes(n1), bytes(n2), mm.revcomp(n2)], {}, {}, {})
    low = bytes(two_subs()).lower()
    C["lower_case"] = ([CONTIG.lower()[:1500] + CONTIG[1500:]], [low, bytes(cut(1300, 500)), mm.revcomp(low)], {}, {}, {})
    big = cut()
    big[300:360] = rand(55, 9)
    C["cells_overflow"] = ([CONTIG], [bytes(cut(100, 500)), bytes(big), bytes(cut(1500, 500))], {}, dict(max_cells=3000),
                           dict(NP2_ALIGN_TEST_CELLS="3000"))
    C["unmapped_between"] = ([CONTIG], [bytes(cut()), bytes(rand(500, 10)), bytes(two_subs(9))], {}, {}, {})
    return C


CASES = _build()
_EXPECTED = {}


def case(name):
    return CASES[name]


def expected(name):
    if name not in _EXPECTED:
        contigs, reads, o, ao, _ = CASES[name]
        _EXPECTED[name] = am.align_reads(contigs, reads, map_kw=o, **ao)
    return _EXPECTED[name]


def call_kw(name):
    """the options of a case as the library takes them; max_cells stays at its default where the case lowers it by the hook"""
    _, _, o, ao, env = CASES[name]
    kw = dict(o)
    kw.update({f: v for f, v in ao.items() if not (f == "max_cells" and env)})
    return kw


def check(got, name):
    """(hits, recs, cigar, cigar_off) of the library against the model, field for field"""
    gh, gr, gc, go = got
    hits, recs, cigars, cnt, tot = expected(name)
    assert np.array_equal(mm.hits_array(hits)[:, [0] + list(range(2, 13))],
                          np.array([[int(h[f]) for f in mm.HIT_FIELDS if f != "qlen"] for h in gh], np.int64).reshape(len(hits), 12)), name
    want = am.recs_array(recs)
    have = np.array([[int(r[f]) for f in am.REC_FIELDS] for r in gr], np.int64).reshape(len(recs), len(am.REC_FIELDS))
    assert np.array_equal(have, want), (name, have.tolist(), want.tolist())
    words, off = am.cigar_words(cigars)
    assert np.array_equal(go, off) and np.array_equal(gc, words), (name, cigar_text(gc, go), [cigar_str(c) for c in cigars])


def cigar_str(cg):
    return "".join(f"{L}{op}" for op, L in cg)


def cigar_text(words, off):
    return ["".join(f"{int(w) >> 4}{am.OPS[int(w) & 15]}" for w in words[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
