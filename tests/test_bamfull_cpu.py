"""The full BAM's rule on the CPU (include/np2_io.h: NP2_SAM_KEEP_ALL): np2_sam_tails_host, which walks SAM text with the
one-lane text of the rule the kernels' lanes run, and np2_bamout_host_full, the encoder's host twin, against the plain-Python
model (tests/bamfull_model.py), byte for byte.  No device."""
import random
import struct

import numpy as np
import pytest

import bamfull_model as fm
import bamout_model as bm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error

E_ARG, E_UNSUPPORTED = -1, -4
REFS = [("c1", 1 << 29), ("c2", 5000)]
SYMBOLS = ["np2_sam_export_tails", "np2_sam_header_text", "np2_sam_tail_stats", "np2_bamout_host_full", "np2_sam_tails_host"]
F_RNEXT, F_PNEXT, F_TLEN, F_QUAL, F_OPT = range(5)


def rec(pos=5, l_seq=8, **kw):
    r = bm.rec(kw.pop("tid", 0), pos, [("M", l_seq)] if l_seq else [], l_seq=l_seq, name=kw.pop("name", b"q"), seed=pos)
    r.update(kw)
    return r


def walk(recs, **kw):
    return np2io.sam_tails_host(fm.sam_text(REFS, recs, **kw))


def tail_of(out, i):
    a = int(out["tail_ref"][i]) >> 1
    n = 16 + int.from_bytes(out["tails"][a + 12:a + 16].tobytes(), "little")
    return out["tails"][a:].tobytes(), n


def accepted(recs, **kw):
    """every record is taken, and its tail is the model's"""
    out = walk(recs, **kw)
    assert out["code"] == 0 and list(out["status"]) == [0] * len(recs), (out["code"], out["message"])
    want, ref = fm.tails(REFS, recs, range(len(recs)))
    assert out["tails"].tobytes() == want.tobytes() and list(out["tail_ref"]) == list(ref)
    return out


def refused(recs, code, field, line=None, **kw):
    """exactly one record is refused, with `code`, in `field`; the message names its line"""
    out = walk(recs, **kw)
    bad = [i for i, s in enumerate(out["status"]) if s < 0]
    assert len(bad) == 1 and out["status"][bad[0]] == code == out["code"], (out["status"], out["message"])
    assert (int(out["where"][bad[0]]) >> 8) - 1 == field, (hex(out["where"][bad[0]]), out["message"])
    assert "line %d:" % (len(REFS) + 2 + bad[0] if line is None else line) in out["message"], out["message"]
    return out


def tagged(*tags, **kw):
    return rec(tags=list(tags), **kw)


# ---- the optional fields ---------------------------------------------------------------------------------------------------
def test_every_type_once():
    r = tagged(b"XA:A:!", b"NM:i:-7", b"de:f:0.0012", b"MD:Z:10A5^AC6", b"XH:H:1AE301", b"XB:B:c,-1,2", b"ZB:B:f,1.5,-2e3", b"Z9:Z:")
    out = accepted([r])
    t, n = tail_of(out, 0)
    assert t[16:n] == (b"XAA!" + b"NMc\xf9" + b"def" + struct.pack("<f", 0.0012) + b"MDZ10A5^AC6\0" + b"XHH1AE301\0" +
                       b"XBBc\2\0\0\0\xff\2" + b"ZBBf\2\0\0\0" + struct.pack("<ff", 1.5, -2000.0) + b"Z9Z\0")


@pytest.mark.parametrize("v,t", [(-2 ** 31, "i"), (-32769, "i"), (-32768, "s"), (-129, "s"), (-128, "c"), (-1, "c"), (0, "C"), (255, "C"),
                                 (256, "S"), (65535, "S"), (65536, "I"), (2 ** 32 - 1, "I")])
def test_integer_type_choice(v, t):
    out = accepted([tagged(b"XI:i:%d" % v)])
    tl, n = tail_of(out, 0)
    assert tl[16:n] == b"XI" + t.encode() + struct.pack(fm.INT_TYPES[t][0], v)


@pytest.mark.parametrize("text", [b"4294967296", b"-2147483649", b"+", b"1x", b"", b"-"])
def test_integers_refused(text):
    out = refused([rec(), tagged(b"NM:i:1", b"XI:i:" + text, pos=9)], E_ARG, F_OPT + 1)
    if text:
        assert "(XI)" in out["message"]


def test_signed_integers_accepted():
    accepted([tagged(b"XI:i:+5", b"XJ:i:-0", b"XK:i:007")])


@pytest.mark.parametrize("text", [b"0.0012", b"1", b"-3.5E+2", b"1e-5", b"0.1", b"16777217", b"9007199254740991", b"+0.5e1", b"1e22", b"1e-22",
                                  b"123456789.123456e-16"])
def test_floats_accepted(text):
    out = accepted([tagged(b"XF:f:" + text)])
    tl, n = tail_of(out, 0)
    assert tl[16:n] == b"XFf" + struct.pack("<f", float(text))


@pytest.mark.parametrize("text", [b"nan", b"inf", b"-inf", b"NaN", b"Infinity", b"9007199254740993", b"9007199254740992", b"1e23", b"1e-23",
                                  b"0.00000000000000000000001"])
def test_floats_outside_the_window_are_unsupported(text):
    refused([tagged(b"XF:f:" + text)], E_UNSUPPORTED, F_OPT)


@pytest.mark.parametrize("text", [b"", b".5", b"5.", b"1e", b"1e+", b"1.5x", b"--1", b"0x10"])
def test_malformed_floats(text):
    refused([tagged(b"XF:f:" + text)], E_ARG, F_OPT)


def test_random_decimals_equal_strtod():
    """2 000 decimals inside the window (digits below 2^53, |exponent - fraction digits| <= 22), bit for bit"""
    rng = random.Random(20260)
    texts = []
    while len(texts) < 2000:
        nd = rng.randint(1, 16)
        digits = "".join(rng.choice("0123456789") for _ in range(nd))
        if int(digits) >= 2 ** 53:
            continue
        cut = rng.randint(1, nd)  # digits before the point
        frac = nd - cut
        ex = rng.randint(-22 + frac, 22 + frac) if rng.random() < 0.7 else None
        if ex is None and frac > 22:
            continue
        s = rng.choice(["", "-", "+"]) + digits[:cut] + ("." + digits[cut:] if frac else "")
        if ex is not None:
            s += rng.choice("eE") + rng.choice(["", "+"] if ex >= 0 else ["-"]) + str(abs(ex))
        texts.append(s.encode())
    recs = [tagged(*[b"X%d:f:" % (j % 10) + t for j, t in enumerate(texts[k:k + 50])], pos=5 + k) for k in range(0, 2000, 50)]
    out = accepted(recs)
    got = []
    for i in range(len(recs)):
        tl, n = tail_of(out, i)
        got += [tl[16 + 7 * j + 3:16 + 7 * j + 7] for j in range(50)]
    assert got == [struct.pack("<f", float(t)) for t in texts]


@pytest.mark.parametrize("sub,vals", [("c", [-128, 127]), ("C", [0, 255]), ("s", [-32768, 32767]), ("S", [0, 65535]),
                                      ("i", [-2 ** 31, 2 ** 31 - 1]), ("I", [0, 2 ** 32 - 1]), ("f", ["0.5", "-1e3"])])
def test_arrays(sub, vals):
    text = lambda v: b"XB:B:" + sub.encode() + b"".join(b",%s" % str(x).encode() for x in v)
    accepted([tagged(text([]), pos=5), tagged(text(vals[:1]), pos=6), tagged(text(vals), pos=7), tagged(text(vals * 40), pos=8)])
    if sub != "f":
        lo, hi = fm.INT_TYPES[sub][1:]
        for v in (lo - 1, hi + 1):
            refused([tagged(text([vals[0], v]))], E_ARG, F_OPT)
    else:
        refused([tagged(text(["1", "1e23"]))], E_UNSUPPORTED, F_OPT)
        refused([tagged(text(["1", "x"]))], E_ARG, F_OPT)


@pytest.mark.parametrize("text", [b"", b"x,1", b"c1", b"c,", b"c,1,,2", b"c,1,", b",1"])
def test_malformed_arrays(text):
    refused([tagged(b"XB:B:" + text)], E_ARG, F_OPT)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 5000])
def test_z_lengths(n):
    val = bytes(32 + (i * 7) % 95 for i in range(n))
    out = accepted([tagged(b"NM:i:1", b"XZ:Z:" + val, b"XT:A:x")])
    tl, m = tail_of(out, 0)
    assert tl[16:m] == b"NMC\1" + b"XZZ" + val + b"\0" + b"XTAx"
    if n:
        for bad in (b"\x1f", b"\x7f", b"\x80"):
            for at in {0, n // 2, n - 1}:
                refused([tagged(b"NM:i:1", b"XZ:Z:" + val[:at] + bad + val[at + 1:])], E_ARG, F_OPT + 1)


@pytest.mark.parametrize("n", [0, 2, 64, 66, 200])
def test_h_values(n):
    val = bytes(b"0123456789abcdefABCDEF"[(i * 5) % 22] for i in range(n))
    accepted([tagged(b"XH:H:" + val)])
    refused([tagged(b"XH:H:" + val + b"0")], E_ARG, F_OPT)                # an odd number of digits
    refused([tagged(b"XH:H:" + val + b"0g")], E_ARG, F_OPT)               # not a hex digit
    if n:
        refused([tagged(b"XH:H:" + b"G" + val[1:])], E_ARG, F_OPT)


@pytest.mark.parametrize("field", [b"NM:i", b"NM:Z", b"N:i:1", b"1M:i:1", b"N_:i:1", b"NM;i:1", b"NM:i;1", b"NM:q:1", b"NM:I:1", b"NM:a:x", b""])
def test_field_form_refused(field):
    refused([tagged(b"XA:A:a", field, b"XB:A:b")], E_ARG, F_OPT + 1)


def test_a_values():
    accepted([tagged(b"XA:A:!", b"XB:A:~", b"X1:A::")])
    for bad in (b"XA:A: ", b"XA:A:\x7f", b"XA:A:ab", b"XA:A:"):
        refused([tagged(bad)], E_ARG, F_OPT)


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_many_fields_on_one_line(n):
    tags = [b"%s%d:i:%d" % (b"XYZ"[j % 3:j % 3 + 1], j % 10, j * 311 - 20000) for j in range(n)]
    accepted([tagged(*tags), tagged(*tags[::-1], pos=9)])
    for at in {0, n - 1, n // 2, min(63, n - 1), min(64, n - 1)}:
        bad = list(tags)
        bad[at] = b"XX:i:1x"
        refused([tagged(*bad)], E_ARG, F_OPT + at)


# ---- line ends, QUAL, mates ----------------------------------------------------------------------------------------------------
def test_line_ends():
    recs = [rec(qual=fm.qual_of(8)), tagged(b"NM:i:3", pos=9, qual=fm.qual_of(8, 3))]
    want = accepted(recs)
    for end in (b"\r\n",):
        out = walk(recs, end=end)
        assert out["code"] == 0 and out["tails"].tobytes() == want["tails"].tobytes()
    text = fm.sam_text(REFS, recs)
    out = np2io.sam_tails_host(text[:-1])  # the last line needs no newline
    assert out["code"] == 0 and out["tails"].tobytes() == want["tails"].tobytes()
    out = np2io.sam_tails_host(text[:-1] + b"\t\n")  # a tab behind the last field opens an empty field
    assert out["code"] == E_ARG and int(out["where"][1]) >> 8 == F_OPT + 2


@pytest.mark.parametrize("l_seq", [1, 2, 63, 64, 65, 15001])
def test_qual_lengths(l_seq):
    q = fm.qual_of(l_seq, l_seq)
    out = accepted([rec(l_seq=l_seq, qual=q), rec(l_seq=l_seq, pos=9), tagged(b"NM:i:1", l_seq=l_seq, qual=q, pos=11)])
    assert [int(x) & 1 for x in out["tail_ref"]] == [1, 0, 1]
    refused([rec(l_seq=l_seq, qual=q[:-1])], E_ARG, F_QUAL)
    refused([rec(l_seq=l_seq, qual=q + b"I")], E_ARG, F_QUAL)
    for bad in (b" ", b"\x7f"):
        for at in {0, l_seq - 1, l_seq // 2}:
            refused([tagged(b"NM:i:1", l_seq=l_seq, qual=q[:at] + bad + q[at + 1:])], E_ARG, F_QUAL)


def test_qual_star_and_seq_star():
    accepted([rec(l_seq=0), rec(l_seq=1, pos=7), tagged(b"NM:i:0", l_seq=0, pos=9)])
    refused([rec(l_seq=0, qual=b"II")], E_ARG, F_QUAL)
    refused([rec(l_seq=4, qual=b"")], E_ARG, F_QUAL)


def test_mates():
    ok = [rec(rnext=b"=", pnext=1, tlen=-1), rec(pos=6, rnext=b"*", pnext=0, tlen=0), rec(pos=7, rnext=b"c2", pnext=2 ** 31 - 1, tlen=-(2 ** 31 - 1)),
          rec(pos=8, rnext=b"c1", pnext=12, tlen=2 ** 31 - 1), rec(pos=9, tid=1, rnext=b"=", tlen=b"+17")]
    out = accepted(ok)
    heads = [struct.unpack_from("<iii", tail_of(out, i)[0]) for i in range(len(ok))]
    assert heads == [(0, 0, -1), (-1, -1, 0), (1, 2 ** 31 - 2, -(2 ** 31 - 1)), (0, 11, 2 ** 31 - 1), (1, -1, 17)]
    refused([rec(rnext=b"nope")], E_ARG, F_RNEXT)
    refused([rec(rnext=b"")], E_ARG, F_RNEXT)
    for bad in (2 ** 31, b"-1", b"", b"1x"):
        refused([rec(pnext=bad)], E_ARG, F_PNEXT)
    for bad in (2 ** 31, -(2 ** 31), b"", b"-", b"1.0"):
        refused([rec(tlen=bad)], E_ARG, F_TLEN)


def test_unmapped_records_are_not_looked_at():
    recs = [rec(), rec(pos=6, flag=4, tags=[b"bad"], qual=b"x"), rec(pos=7, tid=-1, rnext=b"nope"), rec(pos=8)]
    out = walk(recs)
    assert out["code"] == 0 and list(out["status"]) == [0, 1, 1, 0]


# ---- which line speaks ---------------------------------------------------------------------------------------------------------
def test_which_line_and_which_field_speak():
    good = rec()
    two_fields = rec(pos=6, pnext=b"x", tags=[b"NM:i:1", b"XX:i:z"], qual=b"short")  # PNEXT comes first in the line
    later = rec(pos=7, tags=[b"XF:f:nan"])
    out = walk([good, two_fields, later])
    assert list(out["status"]) == [0, E_ARG, E_UNSUPPORTED] and out["code"] == E_ARG
    assert (int(out["where"][1]) >> 8) - 1 == F_PNEXT and "line 5: PNEXT" in out["message"]
    out = walk([good, later, two_fields])
    assert out["code"] == E_UNSUPPORTED and "line 5: optional field 1 (XF)" in out["message"]
    # QUAL before the optional fields, the first optional field before the second
    out = walk([rec(qual=b"short", tags=[b"XX:i:z"])])
    assert (int(out["where"][0]) >> 8) - 1 == F_QUAL
    out = walk([rec(tags=[b"NM:i:1", b"XX:i:z", b"XY:Z:\x01"])])
    assert (int(out["where"][0]) >> 8) - 1 == F_OPT + 1 and "(XX)" in out["message"]
    # a bad name ranks with a bad tail: the first line speaks; what the lean parse refuses speaks before both
    out = walk([good, rec(pos=6, name=b"n" * 255), later])
    assert out["code"] == E_ARG and "line 5: QNAME" in out["message"]
    out = walk([good, later, rec(pos=6, name=b"n" * 255)])
    assert out["code"] == E_UNSUPPORTED and "line 5:" in out["message"]
    out = walk([good, later, rec(pos=6, flag=70000)])
    assert out["code"] == E_ARG and "line 6: FLAG" in out["message"] and list(out["status"]) == [0, E_UNSUPPORTED, E_ARG]


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_header_text():
    extra = [b"@RG\tID:a\tSM:s", b"@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a x y", b"@CO\tfree text", b"@RG\tID:a\tSM:s", b"@CO\tsecond",
             b"@HD\tVN:1.3", b"@XY"]
    out = walk([rec()], extra=extra)
    want = fm.header_text(REFS, [[b"@HD\tVN:1.0\tSO:unsorted"] + extra])
    assert out["header_text"] == want
    assert want == fm.HD + b"@SQ\tSN:c1\tLN:536870912\n@SQ\tSN:c2\tLN:5000\n" + b"".join(l + b"\n" for l in extra[:3] + [extra[4], extra[6]])
    assert walk([rec()], extra=extra, end=b"\r\n")["header_text"] == want  # '\r' is dropped
    assert walk([rec()])["header_text"] == fm.header_text(REFS, [])
    with pytest.raises(Np2Error):
        np2io.sam_tails_host(b"@SQ\tSN:c1\n")


# ---- the encoder's host twin -------------------------------------------------------------------------------------------------------
def full_twin(refs, given, extras=(), path=None, tie="strand"):
    """records in input order -> np2_bamout_host_full over the model's arrays and tails"""
    order = sorted(range(len(given)), key=lambda i: (given[i]["tid"], given[i]["pos"] + 1, (given[i].get("flag", 0) >> 4) & 1 if tie == "strand" else 0))
    recs = [given[i] for i in order]
    tails, tail_ref = fm.tails(refs, given, order)
    return recs, np2io.bamout_host(*bm.arrays(recs), refs, path=path, tails=tails, tail_ref=tail_ref, header_text=fm.header_text(refs, extras))


def decorated_case(case):
    refs, recs = bm.CASES[case]()
    recs = [r for r in recs if len(r["cigar"]) < 1000]
    given = [recs[k] for k in np.random.default_rng(4).permutation(len(recs))]
    return refs, fm.decorate(given, refs, seed=len(case))


@pytest.mark.parametrize("case", ["bins", "small", "cuts", "long"])
def test_host_twin_full_equals_the_model(case, tmp_path):
    refs, given = decorated_case(case)
    extras = [[b"@RG\tID:x", b"@PG\tID:p"]]
    path = str(tmp_path / "f.bam")
    recs, (S, st) = full_twin(refs, given, extras, path)
    want, off = fm.stream(refs, recs, extras)
    assert S == want, (len(S), len(want), next((i for i, (a, b) in enumerate(zip(S, want)) if a != b), None))
    bam, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
    assert bam == np2io.bgzf_deflate_host(want)
    assert fm.check_files(refs, recs, bam, bai, extras, case) == want
    assert st["records"] == len(recs) and st["stream_bytes"] == len(want) and st["file_bytes"] == len(bam)
    # the tails the text gives are the ones the twin was handed
    out = np2io.sam_tails_host(fm.sam_text(refs, given, extra=extras[0]))
    assert out["code"] == 0 and out["tails"].tobytes() == fm.tails(refs, given, range(len(given)))[0].tobytes()
    assert out["header_text"] == fm.header_text(refs, extras)


@pytest.mark.parametrize("case", sorted(bm.CASES))
def test_host_twin_full_without_tails_is_the_lean_twin(case, tmp_path):
    refs, recs = bm.CASES[case]()
    recs = bm.sort_records(recs)
    a = bm.arrays(recs)
    lean_S, _ = np2io.bamout_host(*a, refs, path=str(tmp_path / "lean.bam"))
    L = np2io._bind()
    import ctypes as C
    p, n, st = C.c_void_p(), C.c_uint64(), np2io.np2_bamout_stats_t()
    rn = (C.c_char_p * max(len(refs), 1))(*[x.encode() for x, _ in refs])
    rl = np.ascontiguousarray([l for _, l in refs], dtype=np.uint32)
    ptr = lambda x: x.ctypes.data if len(x) else None
    full = str(tmp_path / "full.bam").encode()
    assert L.np2_bamout_host_full(ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), len(a[0]), len(a[2]), len(a[3]), ptr(a[4]), len(a[4]), ptr(a[5]),
                                  None, 0, None, None, 0, rn, ptr(rl), len(refs), full, None, C.byref(p), C.byref(n), C.byref(st)) == 0
    got = C.string_at(p.value, n.value)
    L.np2_free(p)
    assert got == lean_S == bm.stream(refs, recs)[0]
    for ext in ("", ".bai"):
        assert open(str(tmp_path / "full.bam") + ext, "rb").read() == open(str(tmp_path / "lean.bam") + ext, "rb").read()


def test_host_twin_full_checks_its_arrays():
    refs, given = decorated_case("small")
    order = sorted(range(len(given)), key=lambda i: (given[i]["tid"], given[i]["pos"] + 1, (given[i].get("flag", 0) >> 4) & 1))
    recs = [given[i] for i in order]
    tails, tail_ref = fm.tails(refs, given, order)
    a = bm.arrays(recs)
    for bad in (int(tail_ref[1]) + 2, len(tails) << 1, (len(tails) - 4) << 1):  # not at a word, behind the bytes, no room for the head
        ref = tail_ref.copy()
        ref[1] = bad
        with pytest.raises(Np2Error) as e:
            np2io.bamout_host(*a, refs, tails=tails, tail_ref=ref)
        assert e.value.code == E_ARG and "record 1" in str(e.value)
    t = tails.copy()
    at = int(tail_ref[2]) >> 1
    t[at + 12:at + 16] = np.frombuffer(struct.pack("<I", len(tails)), dtype=np.uint8)  # an aux_len that leaves the bytes
    with pytest.raises(Np2Error) as e:
        np2io.bamout_host(*a, refs, tails=t, tail_ref=tail_ref)
    assert e.value.code == E_ARG and "record 2" in str(e.value)
    with pytest.raises(ValueError):
        np2io.bamout_host(*a, refs, tails=tails, tail_ref=tail_ref[:-1])


# ---- the per-lane core as a host program, plain and under the address and undefined-behaviour sanitizers ----------------------------
def build_core(tmp, extra=()):
    import os
    import subprocess
    exe = str(tmp / ("samtail_core_test" + ("_san" if extra else "")))
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "samtail_core_test.cpp")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_core_program_equals_the_library_also_under_sanitizers(tmp_path):
    import subprocess
    good = [tagged(b"XA:A:!", b"NM:i:-7", b"de:f:0.0012", b"XH:H:1AE301", b"XB:B:c,-1,2", b"ZB:B:f,1.5,-2e3", b"Z9:Z:", qual=fm.qual_of(8, 1)),
            tagged(b"XZ:Z:" + b"z" * 5000, pos=6, l_seq=65, qual=fm.qual_of(65, 2)), rec(pos=7, l_seq=0), rec(pos=8, l_seq=15001, qual=fm.qual_of(15001)),
            tagged(*[b"X%d:i:%d" % (j % 10, j * 977 - 40000) for j in range(130)], pos=9, rnext=b"c2", pnext=77, tlen=-5),
            tagged(b"XB:B:I" + b",4294967295" * 300, pos=10), rec(pos=11, flag=4, tags=[b"bad"]), rec(pos=12, tags=[b"XH:H:" + b"ab" * 100])]
    bad = [tagged(b"NM:i:1", b"XI:i:1x"), tagged(b"XF:f:1e23"), tagged(b"XF:f:"), tagged(b"XZ:Z:" + b"z" * 400 + b"\x7f"), tagged(b"NM:i"), tagged(b""),
           tagged(b"XB:B:c,1,"), tagged(b"XB:B:"), tagged(b"XH:H:abc"), rec(qual=b"short"), rec(qual=b""), rec(l_seq=0, qual=b"I"), rec(rnext=b""),
           rec(pnext=b""), rec(tlen=b"-"), rec(flag=70000), tagged(b"XA:A:"), tagged(b"XF:f:1e"), tagged(b"XF:f:-"), tagged(b"XI:i:-")]
    recs = good + [dict(r, pos=20 + i) for i, r in enumerate(bad)]
    exes = build_core(tmp_path), build_core(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for k, text in enumerate((fm.sam_text(REFS, recs), fm.sam_text(REFS, recs, end=b"\r\n")[:-2], fm.sam_text(REFS, recs[:3]) + b"\n\n")):
        path = tmp_path / ("t%d.sam" % k)
        path.write_bytes(text)
        lib = np2io.sam_tails_host(text)
        want = []
        for i in range(len(lib["status"])):
            st, wh = int(lib["status"][i]), int(lib["where"][i])
            if st == 0:
                a = int(lib["tail_ref"][i]) >> 1
                aux = int.from_bytes(lib["tails"][a + 12:a + 16].tobytes(), "little")
                hq = int(lib["tail_ref"][i]) & 1
                size = 16 + aux + (hq and len(recs[i]["seq"]))
                want.append("T\t%d\t%d\t%s" % (hq, aux, lib["tails"][a:a + size + (-size % 4)].tobytes().hex()))
            else:
                want.append("U" if st == 1 else "E\t%d" % wh if wh else "L")
        for exe in exes:
            r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            got = [ln.split("\t")[0] if ln.startswith("L") else ln for ln in r.stdout.split("\n")[:-1] if ln != "S"]
            assert got == want, (k, exe, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w) if len(got) == len(want) else (len(got), len(want)))
        assert sum(w.startswith("E") for w in want) >= (19 if k < 2 else 0)


def test_abi_symbols_and_null_arguments():
    import ctypes as C
    L = api.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in api.IO_ABI_SYMBOLS and s in np2io.IO_SYMBOLS
    assert np2io.NP2_SAM_KEEP_ALL == 2
    L = np2io._bind()
    p, n = C.c_void_p(), C.c_uint64()
    fake_ctx, fake_sam = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 12)
    assert L.np2_sam_tails_host(None, 0, None, None, None, None, None, None, None, None) == E_ARG
    assert L.np2_sam_export_tails(None, fake_sam, C.byref(p), C.byref(n), C.byref(p), C.byref(n)) == E_ARG
    assert L.np2_sam_export_tails(fake_ctx, fake_sam, C.byref(p), C.byref(n), C.byref(p), C.byref(n)) == E_ARG
    assert b"NP2_SAM_KEEP_ALL" in L.np2_io_last_error()
    assert L.np2_sam_header_text(fake_sam, C.byref(p), C.byref(n)) == E_ARG and L.np2_sam_header_text(None, C.byref(p), C.byref(n)) == E_ARG
    assert L.np2_sam_tail_stats(None, None, None, None) == E_ARG
    o, h = np2io.np2_sam_opts_t(1), C.c_void_p()
    missing = (C.c_char_p * 1)(b"/nonexistent/nope.sam")
    assert L.np2_sam_open_ex(fake_ctx, missing, 1, C.byref(o), 4, C.byref(h)) == E_ARG and b"unknown flag" in L.np2_io_last_error()
    assert L.np2_sam_open_ex(fake_ctx, missing, 1, C.byref(o), 3, C.byref(h)) == E_ARG and b"cannot open" in L.np2_io_last_error()
    out = np2io.sam_tails_host(b"")
    assert out["code"] == 0 and len(out["status"]) == 0 and out["header_text"] == fm.HD
