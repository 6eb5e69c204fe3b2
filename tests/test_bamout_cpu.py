"""The BAM writer's host twin (np2_bamout_host: the kernels' per-record code run on the CPU, no device) against the plain-Python
model of the rule (tests/bamout_model.py), byte for byte: the stream, the .bam and the .bai on the hand-built shapes; the
refusals and argument checks, each before a file exists; the file read back by bamio.read_bam; the ABI symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import bamout_model as bm
from nextpolish2_amd import api, bamio
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error

SYMBOLS = ["np2_sam_open_ex", "np2_sam_write_bam", "np2_sam_bam_stream", "np2_bamout_host", "np2_sam_export_names"]
E_ARG, E_UNSUPPORTED = -1, -4


def twin(refs, recs, path=None):
    return np2io.bamout_host(*bm.arrays(recs), refs, path=path)


@pytest.mark.parametrize("case", sorted(bm.CASES))
@pytest.mark.parametrize("tie", ["strand", "input"])
def test_host_twin_equals_the_model(case, tie, tmp_path):
    refs, recs = bm.CASES[case]()
    recs = bm.sort_records(recs, tie)
    path = str(tmp_path / "out.bam")
    S, st = twin(refs, recs, path)
    want, off = bm.stream(refs, recs)
    assert S == want, (case, len(S), len(want), next((i for i, (a, b) in enumerate(zip(S, want)) if a != b), None))
    bam, bai = open(path, "rb").read(), open(path + ".bai", "rb").read()
    assert bam == np2io.bgzf_deflate_host(want)  # blocks cut every 65280 bytes wherever records fall, and the EOF block
    assert bm.check_files(refs, recs, bam, bai, case) == want
    assert st["records"] == len(recs) and st["stream_bytes"] == len(want) and st["file_bytes"] == len(bam)
    assert st["blocks"] == (len(want) + bm.BLOCK - 1) // bm.BLOCK


def test_the_shapes_are_what_their_names_say():
    refs, recs = bm.case_cuts()
    S, off = bm.stream(refs, recs)
    targets = [i for i, r in enumerate(recs) if r["name"].startswith(b"target_")]
    starts = (0, 4, 36, 57, 177, 277, 477)
    for k, i in enumerate(targets):  # block boundary k + 1 lies strictly inside part k of target k
        cut = bm.BLOCK * (k + 1) - off[i]
        assert starts[k] < cut < starts[k + 1], (k, cut)
    assert (bm.BLOCK * 4 - off[targets[3]] - 57) % 4 != 0  # ... and inside a CIGAR word
    for blocks in (1, 2):
        assert len(bm.stream(*bm.case_exact(blocks))[0]) == blocks * bm.BLOCK
    assert 2 * bm.BLOCK < len(bm.stream(*bm.case_long())[0]) <= 3 * bm.BLOCK


def test_index_entries_of_the_bins_case(tmp_path):
    """what the rule says of bins and windows, read off the written index without the model"""
    import struct
    refs, recs = bm.case_bins()
    recs = bm.sort_records(recs, "strand")
    path = str(tmp_path / "b.bam")
    _, st = twin(refs, recs, path)
    data = open(path + ".bai", "rb").read()
    assert data[:4] == b"BAI\1" and struct.unpack_from("<I", data, 4)[0] == 3
    at, per_ref = 8, []
    for _ in refs:
        n_bin, = struct.unpack_from("<I", data, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", data, at)
            bins[b] = [struct.unpack_from("<QQ", data, at + 8 + 16 * j) for j in range(n_chunk)]
            at += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<I", data, at)
        lin = list(struct.unpack_from("<%dQ" % n_intv, data, at + 4))
        at += 4 + 8 * n_intv
        per_ref.append((bins, lin))
    assert at == len(data)
    b0, l0 = per_ref[0]
    # bin 4681 is met again after bin 585: two chunks; then the three records around 16384 (4681, 585, 585)
    assert len(b0[4681]) == 2 and list(b0) == sorted(b0)
    assert 4681 + 5 in b0 and 585 in b0 and 73 in b0 and 9 in b0 and 1 in b0 and 0 in b0  # one bin of each level
    assert 4681 + (bm.BIG - 1 >> 14) in b0 and len(l0) == bm.BIG >> 14
    assert l0[2] == l0[3] == l0[4] == l0[1] and l0[5] > l0[4]  # an empty window takes the previous one's value
    assert per_ref[1] == ({}, [])                                # the middle reference has no record
    b2, l2 = per_ref[2]
    assert l2[:6] == [0] * 6 and l2[6] > 0 and len(l2) == ((100000 + 40000 - 1) >> 14) + 1  # leading empty windows are 0
    assert st["bins"] == sum(len(b) for b, _ in per_ref) and st["chunks"] == sum(len(c) for b, _ in per_ref for c in b.values())


def test_read_bam_reads_the_records_and_names_back(tmp_path):
    for case in ("small", "bins", "cuts"):
        refs, recs = bm.CASES[case]()
        recs = bm.sort_records(recs)
        path = str(tmp_path / (case + ".bam"))
        twin(refs, recs, path)
        got_refs, got = bamio.read_bam(path)
        assert got_refs == refs and len(got) == len(recs)
        for g, w in zip(got, recs):
            assert {k: g[k] for k in ("tid", "pos", "mapq", "flag", "name", "cigar", "seq")} == \
                   {k: w[k] for k in ("tid", "pos", "mapq", "flag", "name", "cigar", "seq")}, w["name"]


@pytest.mark.parametrize("case", sorted(bm.REFUSED))
def test_refusals_come_before_any_file(case, tmp_path):
    refs, recs, status = bm.REFUSED[case]
    path = str(tmp_path / "refused.bam")
    with pytest.raises(Np2Error) as e:
        twin(refs, bm.sort_records(recs) if case != "pos_zero" else recs, path)
    assert e.value.code == status, (case, str(e.value))
    assert ("c1" in str(e.value)) if case == "ln_too_large" else ("record" in str(e.value))
    assert os.listdir(tmp_path) == []
    if case == "pos_zero":
        assert "record 1 " in str(e.value) and "c2" in str(e.value) and "POS 0" in str(e.value)


def test_argument_checks(tmp_path):
    L = np2io._bind()
    refs, recs = bm.case_small()
    a = list(bm.arrays(recs))
    path = str(tmp_path / "x.bam")
    # arrays that do not hold what the records point at
    for i, (field, value) in enumerate((("cigar_off", 1 << 40), ("seq_off", 1 << 40), ("l_seq", 0x7FFFFFF0))):
        b = [x.copy() for x in a]
        b[0][field][1] = value
        with pytest.raises(Np2Error) as e:
            np2io.bamout_host(*b, refs, path=path)
        assert e.value.code == E_ARG and "record 1" in str(e.value)
    for bad_ref in (5 << 8 | 0, 5 << 8 | 255, (len(a[4]) - 1) << 8 | 2):  # empty, 255 bytes, past the end
        b = [x.copy() for x in a]
        b[5][2] = bad_ref
        with pytest.raises(Np2Error) as e:
            np2io.bamout_host(*b, refs, path=path)
        assert e.value.code == E_ARG and "record 2" in str(e.value)
    b = [x.copy() for x in a]
    b[1][3] = 7  # a tid the list lacks
    with pytest.raises(Np2Error):
        np2io.bamout_host(*b, refs, path=path)
    with pytest.raises(Np2Error) as e:  # not in coordinate order
        np2io.bamout_host(*bm.arrays(recs[::-1]), refs, path=path)
    assert "coordinate order" in str(e.value)
    with pytest.raises(ValueError):
        np2io.bamout_host(a[0], a[1][:-1], a[2], a[3], a[4], a[5], refs)
    assert os.listdir(tmp_path) == []
    # NULL arguments, and fake handles: the device entry points look at their arguments before the context or the handle
    st = np2io.np2_bamout_stats_t()
    p, n = C.c_void_p(), C.c_uint64()
    fake_ctx, fake_sam = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 12)
    assert L.np2_bamout_host(None, None, None, None, 1, 0, 0, None, 0, None, None, None, 0, None, None, None, None, None) == E_ARG
    assert L.np2_bamout_host(None, None, None, None, 0, 0, 0, None, 0, None, None, None, 0, None, path.encode(), None, None, None) == E_ARG
    assert L.np2_sam_write_bam(None, fake_sam, path.encode(), None, C.byref(st)) == E_ARG
    assert L.np2_sam_write_bam(fake_ctx, None, path.encode(), None, C.byref(st)) == E_ARG
    assert L.np2_sam_write_bam(fake_ctx, fake_sam, None, None, C.byref(st)) == E_ARG
    assert b"NULL" in L.np2_io_last_error()
    assert L.np2_sam_write_bam(fake_ctx, fake_sam, path.encode(), None, C.byref(st)) == E_ARG  # a handle without names
    assert b"NP2_SAM_KEEP_NAMES" in L.np2_io_last_error()
    assert L.np2_sam_bam_stream(None, fake_sam, C.byref(p), C.byref(n)) == E_ARG
    assert L.np2_sam_bam_stream(fake_ctx, fake_sam, None, C.byref(n)) == E_ARG
    assert L.np2_sam_bam_stream(fake_ctx, fake_sam, C.byref(p), C.byref(n)) == E_ARG and not p.value
    assert L.np2_sam_export_names(fake_ctx, fake_sam, C.byref(p), C.byref(n), C.byref(p), C.byref(n)) == E_ARG
    o, h = np2io.np2_sam_opts_t(1), C.c_void_p()
    missing = (C.c_char_p * 1)(str(tmp_path / "nope.sam").encode())
    assert L.np2_sam_open_ex(fake_ctx, missing, 1, C.byref(o), 2, C.byref(h)) == E_ARG and b"flag" in L.np2_io_last_error()
    assert L.np2_sam_open_ex(fake_ctx, missing, 1, C.byref(o), 1, C.byref(h)) == E_ARG and b"cannot open" in L.np2_io_last_error()
    assert os.listdir(tmp_path) == []
    # no record and no reference at all is still a BAM
    S, _ = np2io.bamout_host(*bm.arrays([]), [], path=path)
    assert S == bm.header([]) and bm.check_files([], [], open(path, "rb").read(), open(path + ".bai", "rb").read()) == S


def test_abi_symbols():
    L = api.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in api.IO_ABI_SYMBOLS and s in np2io.IO_SYMBOLS
