"""The SAM reader without a GPU: the plain-Python model of the rule (tests/sam_model.py) on hand-derived lines, the per-lane
core as a one-lane host program (csrc/np2_sam_core.hpp through tests/tools/sam_core_test.cpp, also under the address and
undefined-behaviour sanitizers) against the model, the new symbols, the argument checks that come before any device call,
io.mapping_kind, the command line's refusals, and the order of the committed bundle's records."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import sam_cases as sc
import sam_model as sm
from nextpolish2_amd import bamio
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
E_ARG, E_UNSUPPORTED = -1, -4


# ---- 1. the model on hand-derived lines -------------------------------------------------------------------------------------
@pytest.mark.parametrize("crlf,final_newline,empty_lines", [(False, True, False), (True, True, False), (False, False, False),
                                                            (True, False, True), (False, True, True)])
def test_model_gives_the_hand_derived_values(crlf, final_newline, empty_lines):
    m = sm.model(sc.good_text(crlf, final_newline, empty_lines))
    assert m.refs == [("c1", 1000), ("c2", 500)]
    sc.check_good([sc.model_record_view(r) for r in m.lines_out if r is not None])
    n_empty = sum(1 for r in m.lines_out if r is None)
    assert n_empty == (4 if empty_lines else 0)
    assert m.stats == dict(lines=4 + 8 + n_empty, records=8, unmapped=2, kept=6, cigar_words=1 + 0 + 9 + 0 + 1 + 1, seq_bytes=1 + 2 + 0 + 10 + 1 + 1)
    # sorted: (tid, pos + 1): pos_zero (0, 0), star_seq_all_ops / letters / optional_fields (0, 1) in input order, largest, then c2
    assert [r["name"] for r in m.records] == [b"q", b"q", b"q", b"a b", b"q", b"q"]
    assert [(r["tid"], r["pos"]) for r in m.records] == [(0, -1), (0, 0), (0, 0), (0, 0), (0, 2147483646), (1, 6)]
    arr, tids, cig, seq4 = m.arrays()
    assert list(tids) == [0, 0, 0, 0, 0, 1]
    assert list(cig) == [32, 52, 160, 17, 34, 67, 85, 102, 119, 136, 16, 0xFFFFFFF0]
    assert list(arr["cigar_off"]) == [0, 1, 10, 10, 11, 12] and list(arr["n_cigar"]) == [1, 9, 0, 1, 1, 0]
    # SEQ bytes lie as the kept records were met: pos_zero 1 byte, star_cigar_odd_seq 2, letters 10, largest 1, optional_fields 1
    assert list(arr["seq_off"]) == [0, 3, 3, 14, 13, 1] and seq4.tobytes().hex() == "12" "1240" "1248f5ac30fff967bde0" "80" "40"


@pytest.mark.parametrize("name", list(sc.BAD))
def test_model_refuses_the_malformed_lines_with_their_line_number(name):
    ln, why = sc.BAD[name]
    good = sc.GOOD["pos_zero"][0]
    with pytest.raises(sm.SamError) as e:
        sm.model(sc.HEADER + good + b"\n\n" + ln + b"\n" + good + b"\n")
    assert (e.value.code, e.value.line, e.value.what) == (E_ARG, 7, why)  # 4 header lines, a record, an empty line


def test_model_header_rules():
    for bad in (b"@SQ\tSN:c1\n", b"@SQ\tLN:5\n", b"@SQ\tSN:c1\tLN:5\n@SQ\tSN:c1\tLN:6\n", b"@SQ\tSN:c1\tLN:x\n"):
        with pytest.raises(sm.SamError) as e:
            sm.model(b"@HD\tVN:1.6\n" + bad)
        assert e.value.code == E_ARG and e.value.line == 1 + bad.count(b"\n")
    with pytest.raises(sm.SamError):
        sm.model([sc.HEADER, sc.HEADER.replace(b"LN:500", b"LN:501")])
    m = sm.model([sc.HEADER + sc.GOOD["pos_zero"][0], sc.HEADER])  # several files, one of them without a record
    assert m.stats["lines"] == 9 and m.stats["kept"] == 1


def test_tie_rule():
    assert sm.model(sc.TIE_TEXT, "strand").order == [1, 0, 2]
    assert sm.model(sc.TIE_TEXT, "input").order == [0, 1, 2]


# ---- 2. the per-lane core as a host program -----------------------------------------------------------------------------------
def build_core(tmp, extra=()):
    exe = str(tmp / ("sam_core_test" + ("_san" if extra else "")))
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, os.path.join(HERE, "tools", "sam_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def core_exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam")
    return build_core(tmp), build_core(tmp, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def model_lines(text, tie):
    """what tools/sam_core_test.cpp prints for `text`, from the model"""
    lines = sm.split_lines(text)
    try:
        refs, n_head = sm.parse_header(lines)
    except sm.SamError as e:
        return ["HERR\t%d" % e.line]
    out = ["REFS\t" + ",".join(f"{n}:{l}" for n, l in refs)]
    tid_of = {n.encode("latin-1"): i for i, (n, _) in enumerate(refs)}
    for ln in lines[n_head:]:
        r = sm.parse_line(ln, tid_of)
        if r is None:
            out.append("S")
        elif isinstance(r, int):
            out.append(f"E\t{r}")
        else:
            v = sc.model_record_view(r)
            key = sm.sort_key_int(r, tie) if r["kept"] else 0
            out.append("\t".join(str(x) for x in ("R", int(r["kept"]), v["tid"], v["pos"], v["flag"], v["mapq"], len(v["cigar"]), v["l_seq"], key,
                                                  ",".join(str(w) for w in v["cigar"]), v["seq4"])))
    return out


def core_lines(exe, path, tie):
    r = subprocess.run([exe, path, "1" if tie == "strand" else "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.split("\n")[:-1]
    return ["\t".join(ln.split("\t")[:2]) if ln.startswith("HERR") else ln for ln in out]


def test_core_program_equals_the_model(core_exes, tmp_path):
    texts = {"good": sc.good_text(), "good_crlf_no_final_newline": sc.good_text(True, False, True),
             "bad": sc.HEADER + sc.GOOD["pos_zero"][0] + b"\n" + b"".join(ln + b"\n" for ln, _ in sc.BAD.values()),
             "tie": sc.TIE_TEXT, "empty": b"", "header_only": sc.HEADER, "bad_header": b"@HD\n@SQ\tSN:x\n",
             "random": sc.generated(seed=11, n=2000, bad=0.15), "random_clean": sc.generated(seed=12, n=400)}
    for name, text in texts.items():
        p = str(tmp_path / (name + ".sam"))
        with open(p, "wb") as f:
            f.write(text)
        for tie in ("strand", "input"):
            want = model_lines(text, tie)
            for exe in core_exes:  # the plain build, and the one under the sanitizers run stand-alone on the same input
                assert core_lines(exe, p, tie) == want, (name, tie, exe)
    assert sum(1 for ln in model_lines(texts["random"], "strand") if ln.startswith("E")) > 100


# ---- 3. symbols and the argument checks that come before any device call -----------------------------------------------------------
SYMBOLS = ["np2_sam_open", "np2_sam_close", "np2_sam_n_refs", "np2_sam_ref_name", "np2_sam_stats", "np2_contig_from_sam", "np2_sam_parse_bytes", "np2_sam_export"]


def test_symbols_exist():
    L = np2io._bind()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in np2io.IO_SYMBOLS


def test_argument_checks_come_before_the_device(tmp_path):
    L = np2io._bind()
    o = np2io.np2_sam_opts_t(1)
    h, n = C.c_void_p(), C.c_uint64()
    pr, pt, pc, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    buf = np.frombuffer(sc.good_text(), dtype=np.uint8)
    assert L.np2_sam_parse_bytes(0, None, 5, C.byref(o), C.byref(pr), C.byref(pt), C.byref(pc), C.byref(ps), C.byref(n), None) == E_ARG
    assert b"NULL" in L.np2_io_last_error()
    assert L.np2_sam_parse_bytes(0, buf.ctypes.data, len(buf), C.byref(o), None, C.byref(pt), C.byref(pc), C.byref(ps), C.byref(n), None) == E_ARG
    assert L.np2_sam_parse_bytes(0, buf.ctypes.data, len(buf), C.byref(o), C.byref(pr), C.byref(pt), C.byref(pc), C.byref(ps), None, None) == E_ARG
    # np2_sam_open and np2_contig_from_sam look at their arguments and at the files before they look into the context or
    # the handle: a block of zero bytes stands in for both here
    fake_ctx, fake_sam = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 12)
    missing = (C.c_char_p * 1)(str(tmp_path / "nope.sam").encode())
    assert L.np2_sam_open(None, missing, 1, C.byref(o), C.byref(h)) == E_ARG
    assert L.np2_sam_open(fake_ctx, None, 1, C.byref(o), C.byref(h)) == E_ARG
    assert L.np2_sam_open(fake_ctx, missing, 0, C.byref(o), C.byref(h)) == E_ARG
    assert L.np2_sam_open(fake_ctx, missing, 1, C.byref(o), None) == E_ARG
    assert L.np2_sam_open(fake_ctx, missing, 1, C.byref(o), C.byref(h)) == E_ARG
    assert b"cannot open" in L.np2_io_last_error() and b"nope.sam" in L.np2_io_last_error() and not h.value
    ref = np.frombuffer(b"ACGT" * 10, dtype=np.uint8)
    fo = np2io.FrontOpts().c()
    assert L.np2_contig_from_sam(None, fake_sam, b"c1", ref.ctypes.data, 40, C.byref(fo), C.byref(h)) == E_ARG
    assert L.np2_contig_from_sam(fake_ctx, None, b"c1", ref.ctypes.data, 40, C.byref(fo), C.byref(h)) == E_ARG
    assert L.np2_contig_from_sam(fake_ctx, fake_sam, None, ref.ctypes.data, 40, C.byref(fo), C.byref(h)) == E_ARG
    assert L.np2_contig_from_sam(fake_ctx, fake_sam, b"c1", None, 40, C.byref(fo), C.byref(h)) == E_ARG
    assert L.np2_contig_from_sam(fake_ctx, fake_sam, b"c1", ref.ctypes.data, 40, None, C.byref(h)) == E_ARG
    assert L.np2_contig_from_sam(fake_ctx, fake_sam, b"c1", ref.ctypes.data, 40, C.byref(fo), None) == E_ARG
    fs = np2io.FrontOpts(use_secondary=True).c()
    assert L.np2_contig_from_sam(fake_ctx, fake_sam, b"c1", ref.ctypes.data, 40, C.byref(fs), C.byref(h)) == E_UNSUPPORTED
    assert b"BAM" in L.np2_io_last_error() and not h.value
    assert L.np2_sam_stats(None, None) == E_ARG and L.np2_sam_n_refs(None) == 0 and L.np2_sam_ref_name(None, 0, None) is None
    L.np2_sam_close(None)
    with pytest.raises(ValueError):
        np2io._sam_opts("coordinate")
    # the thread's next call works
    assert len(np2io.seqfile_stream(ASM)) == 100001


# ---- 4. io.mapping_kind, bamio.write_sam and the command line's refusals ----------------------------------------------------------------
@pytest.fixture(scope="module")
def bundle_sam(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bundle")
    refs, recs = bamio.read_bam(BAM)
    plain, gz = str(tmp / "bundle.sam"), str(tmp / "any_name.gz")
    bamio.write_sam(plain, refs, recs)
    bamio.write_sam(gz, refs, recs, gz=True)
    return refs, recs, plain, gz


def test_mapping_kind(bundle_sam, tmp_path):
    _, _, plain, gz = bundle_sam
    assert np2io.mapping_kind(BAM) == "bam"
    assert np2io.mapping_kind(plain) == "sam" and np2io.mapping_kind(gz) == "sam"
    assert gzip.open(gz, "rb").read() == open(plain, "rb").read()
    headless = str(tmp_path / "headless.sam")
    with open(headless, "wb") as f:
        f.write(sc.GOOD["pos_zero"][0] + b"\n")
    assert np2io.mapping_kind(headless) == "sam"
    with pytest.raises(ValueError, match="ref_test_asm.fa.gz"):
        np2io.mapping_kind(ASM)


def test_write_sam_is_the_text_twin_of_write_bam(bundle_sam):
    refs, recs, plain, _ = bundle_sam
    m = sm.model(open(plain, "rb").read(), "input")
    assert m.refs == refs and m.stats["records"] == len(recs) == 574
    for r, got in zip(recs, (x for x in m.lines_out if x is not None)):
        assert all(got[k] == r[k] for k in ("tid", "pos", "mapq", "flag", "cigar", "seq", "name"))


def run_cli(args, env_extra=None, stdin=None):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", **(env_extra or {}))  # no device: a refusal must not need one
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli"] + args, capture_output=True, env=env, timeout=600, stdin=stdin)


def test_cli_refuses_what_sam_input_cannot_do_before_any_work(bundle_sam, tmp_path):
    _, _, plain, gz = bundle_sam
    yaks = [os.path.join(BUNDLE, "k21.yak"), os.path.join(BUNDLE, "k31.yak")]
    out = str(tmp_path / "out.fa")
    for sam in (plain, gz):
        r = run_cli(["-S", "-L", "1000", "-o", out, sam, ASM] + yaks)
        assert r.returncode != 0 and b"-S" in r.stderr and b"BAM" in r.stderr and not os.path.exists(out)
    r = run_cli(["-S", "-o", out, "-", ASM] + yaks, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and b"-S" in r.stderr and not os.path.exists(out)
    r = run_cli(["-o", out, plain, ASM] + yaks, env_extra=dict(WORLD_SIZE="2", RANK="0"))
    assert r.returncode != 0 and b".bai" in r.stderr and not os.path.exists(out)
    r = run_cli(["-o", out, ASM, ASM] + yaks)  # neither a BAM nor SAM text
    assert r.returncode != 0 and b"ref_test_asm.fa.gz" in r.stderr and not os.path.exists(out)
    r = run_cli(["--sam_tie", "name", "-o", out, plain, ASM] + yaks)
    assert r.returncode == 2 and not os.path.exists(out)


# ---- 5. the committed bundle: sorted by (tid, pos), ties in an order of their own ----------------------------------------------------
def test_bundle_records_are_in_input_tie_order_and_not_in_strand_order(bundle_sam):
    _, recs, plain, _ = bundle_sam
    text = open(plain, "rb").read()
    by_input, by_strand = sm.model(text, "input"), sm.model(text, "strand")
    n = len(recs)
    assert by_input.stats["kept"] == n  # every record of the bundle is mapped
    assert by_input.order == list(range(n))  # the file is sorted by (tid, pos): tie = input is the identity
    assert by_strand.order != list(range(n)) and sorted(by_strand.order) == list(range(n))
    # where they differ: records at one position whose strands are not ascending in the file
    at0 = [r for r in recs if r["pos"] == 0]
    assert len(at0) == 69
    assert sum(1 for a, b in zip(at0, at0[1:]) if (a["flag"] >> 4) & 1 > (b["flag"] >> 4) & 1) == 17
