"""BAM input without a device (include/np2_io.h: "BAM input"): the host twin np2_bamin_host, which runs the one-lane text of
the rule (csrc/np2_bamin_core.hpp), against the plain-Python model (tests/bamin_model.py) on hand-built records, every refusal
with its code, record number and message, and tests/tools/bamin_test.cpp under the address and undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bamin_model as im
from bamin_model import E_ARG, E_UNSUPPORTED, raw_record
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import IO_ABI_SYMBOLS, Np2Error

HERE = os.path.dirname(os.path.abspath(__file__))
REFS = [("c1", 100000), ("c2", 5000)]
MODES = [dict(), dict(keep_names=True), dict(keep_all=True)]


def three_way(recs, what=""):
    """the twin equals the model in all three modes -> the twin's full result"""
    s = im.inflated(REFS, recs)
    for mode in MODES:
        host, model = np2io.bamin_host(s, **mode), im.decode(s, **mode)
        im.same(host, model, (what, mode))
        bad = model["first_bad"]
        assert host["code"] == (0 if bad is None else int(model["status"][bad])), (what, mode, host["message"])
    return host


def seq_of(l_seq, seed=3):
    b = bytes((seed * 31 + 17 * i) & 255 for i in range((l_seq + 1) // 2))
    return b[:-1] + bytes([b[-1] | 0x05]) if l_seq & 1 else b  # (an odd last byte comes with a low nibble that must go)


ALL_TYPES = (b"XAAq" + b"Xcc\x80" + b"XCC\xff" + b"Xss" + struct.pack("<h", -300) + b"XSS" + struct.pack("<H", 65535) + b"Xii" +
             struct.pack("<i", -2 ** 31) + b"XII" + struct.pack("<I", 2 ** 32 - 1) + b"Xff" + struct.pack("<f", 1.5) + b"XnfAAAA" +
             b"XzZ\0" + b"XZZtext with spaces\0" + b"XHH1AE3\0" + b"XbBc" + struct.pack("<I", 0) + b"XBBs" + struct.pack("<Ihh", 2, -1, 7) +
             b"XFBf" + struct.pack("<If", 1, float("inf")) + b"XiI" + struct.pack("<I", 7))


@pytest.mark.parametrize("l_seq", [0, 1, 2, 63, 64, 65])
def test_seq_lengths_with_and_without_qualities(l_seq):
    q = bytes((7 * i) % 94 for i in range(l_seq))
    host = three_way([raw_record(seq=seq_of(l_seq), l_seq=l_seq, cigar=((0, max(l_seq, 1)),)),
                      raw_record(seq=seq_of(l_seq, 5), l_seq=l_seq, qual=q, pos=11, aux=b"NMC\x01")], l_seq)
    assert list(host["tail_ref"] & 1) == [0, 1 if l_seq else 0]
    if l_seq & 1:
        assert host["seq4"][len(host["seq4"]) // 2 - 1] & 15 == 0 and host["seq4"][-1] & 15 == 0


def test_no_cigar_and_name_lengths():
    three_way([raw_record(cigar=()), raw_record(name=b"a\0"), raw_record(name=b"n" * 254 + b"\0", aux=ALL_TYPES)])


@pytest.mark.parametrize("n", range(1, 9))
def test_every_alignment_of_seq_qualities_and_tags(n):
    name = bytes(65 + i for i in range(n)) + b"\0"
    recs = [raw_record(name=name, seq=seq_of(l), l_seq=l, qual=bytes(i % 90 for i in range(l)), aux=ALL_TYPES, cigar=((0, 5), (1, 2), (4, 9)))
            for l in (5, 6, 7, 8, 21)]
    host = three_way(recs, n)
    assert host["code"] == 0 and list(host["status"]) == [0] * 5


def test_every_optional_type_is_copied_verbatim():
    host = three_way([raw_record(aux=ALL_TYPES)])
    assert ALL_TYPES in host["tails"].tobytes()  # inf included, integers in the types the file gave them


def test_mates_at_their_limits():
    three_way([raw_record(ntid=-1, npos=-1, tlen=-2 ** 31), raw_record(ntid=1, npos=2 ** 31 - 1, tlen=2 ** 31 - 1), raw_record(ntid=0, npos=0, pos=-1)])


def test_unmapped_records_are_counted_and_not_looked_at():
    junk = dict(aux=b"zz", qual=b"\xfe" * 4, ntid=77)
    host = three_way([raw_record(tid=-1, **junk), raw_record(flag=4, **junk), raw_record(flag=4 | 16), raw_record()])
    assert list(host["status"]) == [1, 1, 1, 0] and len(host["recs"]) == 1


REFUSALS = [
    ("block_size_below_32", struct.pack("<I", 31) + b"\0" * 31, E_ARG, im.W_SHORT, "block_size is below 32"),
    ("name_overruns", raw_record(l_name=200), E_ARG, im.W_OVERRUN, "overrun block_size"),
    ("cigar_overruns", raw_record(n_cigar=9), E_ARG, im.W_OVERRUN, "overrun block_size"),
    ("seq_overruns", raw_record(l_seq=2 ** 31, qual=b""), E_ARG, im.W_OVERRUN, "overrun block_size"),
    ("refid_beyond", raw_record(tid=2), E_ARG, im.W_REFID, "refID"),
    ("refid_negative", raw_record(tid=-2), E_ARG, im.W_REFID, "refID"),
    ("pos_negative", raw_record(pos=-2), E_ARG, im.W_POS, "pos is below -1"),
    ("cigar_operation", raw_record(cigar=((9, 4),)), E_ARG, im.W_CIGAR, "CIGAR operation"),
    ("cg_placeholder", raw_record(cigar=((4, 4), (3, 100))), E_UNSUPPORTED, im.W_CG, "CG tag"),
    ("name_empty", raw_record(name=b"\0"), E_ARG, im.W_NAME, "read name"),
    ("name_without_nul", raw_record(name=b"abc"), E_ARG, im.W_NAME, "read name"),
    ("next_refid", raw_record(ntid=2), E_ARG, im.W_NEXT_REFID, "next_refID"),
    ("next_pos", raw_record(npos=-2), E_ARG, im.W_NEXT_POS, "next_pos"),
    ("quality_above_93", raw_record(qual=b"\x00\x5d\x5e\x00"), E_ARG, im.W_QUAL, "quality byte"),
    ("quality_partly_ff", raw_record(qual=b"\xff\xff\xff\x00"), E_ARG, im.W_QUAL, "quality byte"),
    ("aux_short", raw_record(aux=b"NM"), E_ARG, im.W_AUX, "optional fields"),
    ("aux_type", raw_record(aux=b"NMx\0"), E_ARG, im.W_AUX, "optional fields"),
    ("aux_int_cut", raw_record(aux=b"NMi\0\0"), E_ARG, im.W_AUX, "optional fields"),
    ("aux_z_without_nul", raw_record(aux=b"NMZabc"), E_ARG, im.W_AUX, "optional fields"),
    ("aux_b_count_beyond", raw_record(aux=b"XBBc" + struct.pack("<I", 2 ** 32 - 1) + b"\1"), E_ARG, im.W_AUX, "optional fields"),
    ("aux_b_subtype", raw_record(aux=b"XBBZ" + struct.pack("<I", 0)), E_ARG, im.W_AUX, "optional fields"),
]


@pytest.mark.parametrize("name,bad,code,where,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_record(name, bad, code, where, words):
    s = im.inflated(REFS, [raw_record(), raw_record(tid=-1), bad, raw_record(pos=99)])
    host, model = np2io.bamin_host(s, keep_all=True), im.decode(s, keep_all=True)
    im.same(host, model, name)
    assert host["code"] == code and int(host["where"][2]) == where and int(host["status"][2]) == code
    assert host["message"].startswith("the stream: record 2: ") and words in host["message"], host["message"]
    if where != im.W_SHORT:  # (behind a block_size that is no record's nothing can be found)
        assert list(host["status"]) == [0, 1, code, 0] and len(host["recs"]) == 2  # the arrays are filled all the same


def test_lean_handles_do_not_look_at_names_tails_or_tags():
    s = im.inflated(REFS, [raw_record(name=b"abc", ntid=9, npos=-5, qual=b"\xfe" * 4, aux=b"zz")])
    assert np2io.bamin_host(s)["code"] == 0
    assert np2io.bamin_host(s, keep_names=True)["where"][0] == im.W_NAME
    assert np2io.bamin_host(s, keep_all=True)["where"][0] == im.W_NAME  # the first check in the rule's order speaks


def test_stream_ends():
    good = im.inflated(REFS, [raw_record(), raw_record(pos=12)])
    last = len(raw_record(pos=12))
    for cut, where, words in ((1, im.W_TRUNC, "truncated BAM"), (last - 4, im.W_TRUNC, "truncated BAM"), (last - 3, im.W_GARBAGE, "not a record"),
                              (last - 1, im.W_GARBAGE, "not a record")):
        s = good[:len(good) - cut]
        host = np2io.bamin_host(s, keep_all=True)
        im.same(host, im.decode(s, keep_all=True), cut)
        assert host["code"] == E_ARG and int(host["where"][-1]) == where and "record 1: " in host["message"] and words in host["message"]
    host = np2io.bamin_host(good + b"\0" * 8, keep_all=True)  # bytes behind the last record that are not a record
    assert host["code"] == E_ARG and list(host["where"]) == [0, 0, im.W_SHORT] and "record 2: " in host["message"]


def test_header_refusals_and_an_empty_file():
    empty = np2io.bamin_host(im.inflated(REFS, []))
    assert empty["code"] == 0 and len(empty["status"]) == 0
    for bad in (b"BAM\2" + b"\0" * 8, im.inflated(REFS, [])[:-3], b"", im.inflated([("c1", 5), ("c1", 6)], [])):
        with pytest.raises(Np2Error) as e:
            np2io.bamin_host(bad)
        assert e.value.code == E_ARG


def test_abi_symbols():
    assert "np2_bamin_host" in IO_ABI_SYMBOLS and "np2_sam_bamin_stats" in IO_ABI_SYMBOLS


def test_core_program_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "bamin_test")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(HERE, "tools", "bamin_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for scenario in ("refusals", "prefixes"):
        r = subprocess.run([exe, scenario], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (scenario, r.returncode, r.stdout, r.stderr[-3000:])
