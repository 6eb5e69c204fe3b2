"""SAM lines for the tests of the SAM reader (test_sam_cpu.py, test_gpu_sam.py): hand-derived lines with the values the rule of
include/np2_io.h gives them written out, malformed lines with the reason, and a seeded generator that covers the shapes at
which the kernels take another path."""
import numpy as np

import sam_model as sm

HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:500\n@PG\tID:x\n"  # 4 header lines: the first record is line 5


def line(flag=b"0", rname=b"c1", pos=b"1", mapq=b"60", cigar=b"*", seq=b"*", qname=b"q", rest=b"*"):
    """an alignment line of exactly 11 fields (rest = QUAL, or QUAL and optional fields)"""
    return b"\t".join([qname, flag, rname, pos, mapq, cigar, b"*", b"0", b"0", seq, rest])


# name -> (line, expected), every expected value derived by hand:
#   CIGAR word = len << 4 | op with M 0, I 1, D 2, N 3, S 4, H 5, P 6, = 7, X 8
#   SEQ codes of "=ACMGRSVTWYHKDBN" are 0 .. 15, two a byte, high nibble first, an odd tail padded with 0
GOOD = {
    # POS 0 is pos -1; 2M = 2 << 4 | 0 = 32; AC = 1, 2 -> 0x12
    "pos_zero": (line(pos=b"0", cigar=b"2M", seq=b"AC"),
                 dict(tid=0, pos=-1, flag=0, mapq=60, cigar=[32], l_seq=2, seq4="12", kept=True)),
    # flag 65535 has bit 0x4: not kept
    "flag_max": (line(flag=b"65535", pos=b"5", mapq=b"0"),
                 dict(tid=0, pos=4, flag=65535, mapq=0, cigar=[], l_seq=0, seq4="", kept=False)),
    # * CIGAR on a kept record; odd l_seq: ACG = 1, 2, 4 -> 0x12 0x40
    "star_cigar_odd_seq": (line(flag=b"16", rname=b"c2", pos=b"7", mapq=b"255", seq=b"ACG"),
                           dict(tid=1, pos=6, flag=16, mapq=255, cigar=[], l_seq=3, seq4="1240", kept=True)),
    # * SEQ with a CIGAR: 3S 4, 10M 0, 1I 1, 2D 2, 4N 3, 5H 5, 6P 6, 7= 7, 8X 8
    "star_seq_all_ops": (line(cigar=b"3S10M1I2D4N5H6P7=8X"),
                         dict(tid=0, pos=0, flag=0, mapq=60, cigar=[52, 160, 17, 34, 67, 85, 102, 119, 136], l_seq=0, seq4="", kept=True)),
    # lower case, IUPAC letters, and bytes outside the table (. z and 0xE9) -> 15:
    # a 1 c 2 | g 4 t 8 | n 15 R 5 | Y 10 K 12 | M 3 = 0 | . 15 z 15 | 0xE9 15 W 9 | s 6 v 7 | H 11 d 13 | B 14
    "letters": (line(seq=b"acgtnRYKM=.z\xe9WsvHdB"),
                dict(tid=0, pos=0, flag=0, mapq=60, cigar=[], l_seq=19, seq4="1248f5ac30fff967bde0", kept=True)),
    # the largest values: POS 2^31 - 1 -> pos 2^31 - 2; a length of 2^28 - 1 -> 0xFFFFFFF0
    "largest": (line(pos=b"2147483647", cigar=b"268435455M", seq=b"T"),
                dict(tid=0, pos=2147483646, flag=0, mapq=60, cigar=[0xFFFFFFF0], l_seq=1, seq4="80", kept=True)),
    # RNAME * is tid -1: not kept; leading zeros are digits like any other
    "rname_star": (line(flag=b"004", rname=b"*", pos=b"0", mapq=b"000", cigar=b"01M", seq=b"N"),
                   dict(tid=-1, pos=-1, flag=4, mapq=0, cigar=[16], l_seq=1, seq4="f0", kept=False)),
    # optional fields behind QUAL (13 fields), a QNAME with spaces
    "optional_fields": (line(qname=b"a b", cigar=b"1M", seq=b"G", rest=b"I\tNM:i:0\tXX:Z:a\tb"),
                        dict(tid=0, pos=0, flag=0, mapq=60, cigar=[16], l_seq=1, seq4="40", kept=True)),
}

# name -> (line, why): all NP2_E_ARG
BAD = {
    "header_after_record": (b"@CO\tlate", sm.HEADER_LATE),
    "ten_fields": (b"\t".join([b"q", b"0", b"c1", b"1", b"60", b"*", b"*", b"0", b"0", b"ACGT"]), sm.FIELDS),
    "unknown_rname": (line(rname=b"c3"), sm.RNAME),
    "rname_prefix_of_a_name": (line(rname=b"c"), sm.RNAME),
    "trailing_digits": (line(cigar=b"12M3"), sm.CIGAR),
    "no_length": (line(cigar=b"M"), sm.CIGAR),
    "two_letters": (line(cigar=b"3MM"), sm.CIGAR),
    "length_2_28": (line(cigar=b"268435456M"), sm.CIGAR),
    "bad_op": (line(cigar=b"3M2Z"), sm.CIGAR),
    "empty_cigar": (line(cigar=b""), sm.CIGAR),
    "flag_65536": (line(flag=b"65536"), sm.FLAG),
    "flag_letter": (line(flag=b"1x"), sm.FLAG),
    "flag_empty": (line(flag=b""), sm.FLAG),
    "flag_negative": (line(flag=b"-1"), sm.FLAG),
    "pos_2_31": (line(pos=b"2147483648"), sm.POS),
    "pos_overflow": (line(pos=b"99999999999999999999999"), sm.POS),
    "mapq_256": (line(mapq=b"256"), sm.MAPQ),
}


def good_text(crlf=False, final_newline=True, empty_lines=False):
    """the header and every GOOD line, in the dict's order"""
    nl = b"\r\n" if crlf else b"\n"
    body = []
    for i, (ln, _) in enumerate(GOOD.values()):
        body.append(ln)
        if empty_lines and i % 2 == 0:
            body.append(b"")
    text = HEADER.replace(b"\n", nl) + nl.join(body) + nl
    return text if final_newline else text[:-len(nl)]


def check_good(records_in_input_order):
    """the model's or the device's records (dicts with cigar as words, seq4 as hex) against the expectations"""
    for (name, (_, exp)), got in zip(GOOD.items(), records_in_input_order):
        assert got == exp, (name, got, exp)


def model_record_view(r):
    """a model record as GOOD writes its expectations"""
    from nextpolish2_amd import bamio
    arr, cig, seq4, _, _ = bamio.records_to_arrays([r])
    return dict(tid=r["tid"], pos=r["pos"], flag=r["flag"], mapq=r["mapq"], cigar=[int(w) for w in cig], l_seq=len(r["seq"]),
                seq4=seq4[:(len(r["seq"]) + 1) // 2].tobytes().hex(), kept=r["kept"])


TIE_TEXT = HEADER + line(flag=b"16", pos=b"10", qname=b"a") + b"\n" + line(flag=b"0", pos=b"10", qname=b"b") + b"\n" + \
    line(flag=b"16", pos=b"10", qname=b"c") + b"\n"

SEQ_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 257, 700)
CIGAR_OPS = (1, 63, 64, 65, 129, 300)
FLAGS = (0, 16, 4, 0x100, 0x800, 0x110, 20)
REFS = [("chrA", 50000), ("chrB_long_name.1", 30000), ("c", 20000)]


def generated(seed=7, n=400, bad=0.0):
    """-> SAM text of about n records on 3 references, lines in shuffled order, covering every shape of the GPU test's list
    (asserted here).  bad: the share of lines made malformed (for the per-line comparison of the host program only)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTacgtNnRYKMSWBDHV=.", dtype=np.uint8)
    ops = b"MIDNSHP=X"
    seen = dict(seq=set(), ops=set(), qname=set(), flags=set(), rname_star=0, pos0=0, opt_none=0, opt_long=0, straddle=set())
    lines = []

    def one(i, tid=None, pos=None, flag=None):
        l_seq = int(rng.choice(SEQ_LENS)) if i >= len(SEQ_LENS) else SEQ_LENS[i]
        n_ops = int(rng.choice(CIGAR_OPS)) if i >= len(CIGAR_OPS) else CIGAR_OPS[i]
        qlen = 1 + (i % 90)
        flag = int(rng.choice(FLAGS)) if flag is None else flag
        tid = int(rng.integers(-1, len(REFS))) if tid is None else tid
        pos = (0 if rng.random() < 0.05 else int(rng.integers(0, 20000))) if pos is None else pos
        seq = bytes(rng.choice(letters, l_seq)) if l_seq else b"*"
        cigar = b"".join(b"%d%c" % (int(rng.integers(1, 3000)) if rng.random() < 0.2 else int(rng.integers(1, 10)), ops[int(rng.integers(0, 9))])
                         for _ in range(n_ops)) if rng.random() > 0.03 else b"*"
        qname = bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789/_", dtype=np.uint8), qlen))
        opt = int(rng.integers(0, 3))
        rest = (b"*", bytes(rng.integers(33, 74, max(1, l_seq), dtype=np.uint8)) + b"\tNM:i:3",
                b"*\tXA:Z:" + bytes(rng.choice(letters[:4], 300)) + b"\tRG:Z:g")[opt]
        ln = line(b"%d" % flag, REFS[tid][0].encode() if tid >= 0 else b"*", b"%d" % pos, b"%d" % int(rng.integers(0, 256)), cigar, seq,
                  qname, rest)
        if rng.random() < bad:
            which = int(rng.integers(0, 6))
            f = ln.split(b"\t")
            if which == 0:
                f = f[:int(rng.integers(1, 11))]
            elif which == 1:
                f[1] = (b"70000", b"1 ", b"", b"0x4")[int(rng.integers(0, 4))]
            elif which == 2:
                f[2] = (b"chrZ", b"chr", b"")[int(rng.integers(0, 3))]
            elif which == 3:
                f[3] = (b"2147483648", b"-5", b"1e3")[int(rng.integers(0, 3))]
            elif which == 4:
                f[4] = (b"256", b"q")[int(rng.integers(0, 2))]
            else:
                f[5] = (b"10", b"M10", b"5M5", b"300000000M", b"4m", b"**")[int(rng.integers(0, 6))]
            ln = b"\t".join(f)
        elif tid >= -1:
            seen["seq"].add(l_seq), seen["flags"].add(flag), seen["qname"].add(qlen)
            if cigar != b"*":
                seen["ops"].add(n_ops)
            seen["rname_star"] += tid == -1
            seen["pos0"] += pos == 0
            seen["opt_none"] += opt == 0
            seen["opt_long"] += opt == 2
            tabs = [k for k, c in enumerate(ln) if c == 9][:10]
            seen["straddle"].update((t // 64) for t in tabs)  # the 64-byte chunk of the line a field tab falls into
        lines.append(ln)

    for i in range(n - 40):
        one(i)
    for j in range(40):  # one cluster at one (tid, pos), both strands
        one(n - 40 + j, tid=1, pos=1234, flag=16 if rng.random() < 0.5 else 0)
    if not bad:
        assert seen["seq"] == set(SEQ_LENS) and seen["ops"] == set(CIGAR_OPS) and seen["qname"] == set(range(1, 91))
        assert seen["flags"] >= {4, 16, 0x100, 0x800} and seen["rname_star"] and seen["pos0"] and seen["opt_none"] and seen["opt_long"]
        assert len(seen["straddle"]) > 3  # tabs of the first ten fields in several chunks: QNAMEs push them over the edges
    order = rng.permutation(len(lines))
    head = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm.encode(), ln_) for nm, ln_ in REFS)
    return head + b"\n".join(lines[k] for k in order) + b"\n"
