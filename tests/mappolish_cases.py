"""Edge cases of the reads door of the resident SAM (include/np2_io.h: np2_sam_from_reads), shared by the CPU and the GPU tests,
in the form of align_cases (which stays as it is): name -> (contigs, reads, map options, align options, env).  Each is the smallest
shape at which the pack kernel or a branch of the rule's text (csrc/np2_alnpack_core.hpp) can go wrong; all against the 3 kb contig
of align_cases.  all_cases(): these and align_cases.CASES.  expected(name): the model's answers, computed once; text(name): the
SAM `map -a` would write; want(name, tie): what the text door holds of it (sam_model)."""
import numpy as np

import align_cases as ac
import align_model as am
import map_model as mm
import sam_model

CONTIG = ac.CONTIG
CONTIG2 = bytes(ac.rand(2000, 21))


def _build():
    C = {}
    # odd and even lengths on both strands: an odd read's last byte has a zero low nibble, and the reverse strand reaches it from
    # the read's first base
    fwd = [bytes(ac.cut(500, n)) for n in (599, 600, 601)]
    C["odd_even_both_strands"] = ([CONTIG], fwd + [mm.revcomp(r) for r in fwd], {}, {}, {})
    # four front reads of 201 packed bytes each (402 and 401 bases) between reads of 300 bytes: the long reads' SEQ begins at
    # byte offsets 1, 2, 3 and 0 modulo 4, forward and reverse
    x, xr = bytes(ac.cut(700, 600)), mm.revcomp(ac.cut(1400, 600))
    front = [bytes(ac.cut(0, 402)), bytes(ac.cut(2599, 401)), mm.revcomp(ac.cut(900, 402)), bytes(ac.cut(1200, 401))]
    C["seq_offsets"] = ([CONTIG], [front[0], x, front[1], xr, front[2], x, front[3], xr, x], {}, {}, {})
    # IUPAC and stray bytes: the complement leaves them alone, the nibble table does not
    z = ac.cut()
    for at, ch in ((100, "R"), (200, "y"), (300, "n"), (400, "*"), (450, "="), (598, "K"), (1, "w")):
        z[at] = ord(ch)
    C["iupac_stray"] = ([CONTIG], [bytes(z), mm.revcomp(z)], {}, {}, {})
    # the same start on opposite strands, the reverse one first: the tie settings order them differently
    s = bytes(ac.cut(800, 600))
    C["same_start"] = ([CONTIG], [mm.revcomp(s), s, mm.revcomp(s), bytes(ac.cut(100, 500))], {}, {}, {})
    # two contigs, the reads of the second first
    C["two_contigs"] = ([CONTIG, CONTIG2], [CONTIG2[300:900], bytes(ac.cut()), mm.revcomp(CONTIG2[1000:1601]), bytes(ac.cut(5, 601))], {}, {}, {})
    # no read maps: an empty handle
    C["none_maps"] = ([CONTIG], [bytes(ac.rand(500, 31)), bytes(ac.rand(401, 32))], {}, {}, {})
    return C


CASES = _build()
_EXPECTED, _WANT = {}, {}


def all_cases():
    return {**ac.CASES, **CASES}


def case(name):
    return all_cases()[name]


def expected(name):
    if name in ac.CASES:
        return ac.expected(name)
    if name not in _EXPECTED:
        contigs, reads, o, ao, _ = CASES[name]
        _EXPECTED[name] = am.align_reads(contigs, reads, map_kw=o, **ao)
    return _EXPECTED[name]


def call_kw(name):
    """the options of a case as the library takes them (align_cases.call_kw for every case)"""
    _, _, o, ao, env = case(name)
    kw = dict(o)
    kw.update({f: v for f, v in ao.items() if not (f == "max_cells" and env)})
    return kw


def names_of(name):
    return ["r%d" % i for i in range(len(case(name)[1]))]


def text(name, names=None):
    """the SAM text np2_map_align_files writes for the case (sequences are numbered from 1)"""
    contigs, reads = case(name)[:2]
    hits, recs, cigars = expected(name)[:3]
    tnames = [str(i + 1) for i in range(len(contigs))]
    return am.sam(names or names_of(name), reads, hits, recs, cigars, tnames, [len(c) for c in contigs]).encode()


def want(name, tie):
    """(recs, tids, cigar, seq4, stats) the text door holds of text(name): the rule's defining sentence"""
    if (name, tie) not in _WANT:
        res = sam_model.model(text(name), tie)
        _WANT[name, tie] = res.arrays() + (res.stats,)
    return _WANT[name, tie]


def align_arrays(name):
    """the model's records and CIGAR words as np2_map_align_bytes returns them: (recs ALIGN_REC_DTYPE, cigar, cigar_off)"""
    from nextpolish2_amd import io as np2io
    recs, cigars = expected(name)[1:3]
    arr = np.zeros(len(recs), np2io.ALIGN_REC_DTYPE)
    for i, r in enumerate(recs):
        for f in am.REC_FIELDS:
            arr[i][f] = r[f]
    words, off = am.cigar_words(cigars)
    return arr, words, off


def same_arrays(got, exp):
    """recs (every byte of every record, pad words included), tids, cigar, seq4"""
    return (got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]) and
            np.array_equal(got[3], exp[3]))
