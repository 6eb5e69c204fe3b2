"""More chains per read without a GPU (include/np2_io.h, "More chains"): the plain-Python model of the rule
(tests/mapmulti_model.py) shows what each hand-built case of tests/mapmulti_cases.py is for; the host twin np2_map_host_m,
which runs the rule's one text (csrc/np2_map_core.hpp), equals the model unit for unit on the cases, on the seeded generator of
map_model.synthetic and on every sixth read of the committed bundle; the same text as a stand-alone program under the host sanitizers,
which also aligns and settles the units and writes their SAM lines, the model's line for line; the
argument checks with their statuses; the ABI list and the command line's device-free helpers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_model as am
import map_model as mm
import mapmulti_cases as xc
import mapmulti_model as xm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map
from test_map_cpu import bundle, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1
SUPP_SEC = xm.multi(max_chains=10, supplementary=1, secondary_n=5)  # the command line's --supp --secondary 5


# ---- shared, computed once: the model on the synthetic generator and on the bundle ----------------------------------------------
_SHARED = {}


def synthetic_units():
    if "synthetic" not in _SHARED:
        s = synthetic()
        _SHARED["synthetic"] = xm.map_reads(s.index, s.reads, SUPP_SEC)
    return _SHARED["synthetic"]


BUNDLE_STEP = 6  # the model runs on every sixth read of the bundle (96 of 574): it is slow, and the whole bundle is the GPU test's


def bundle_units():
    if "bundle" not in _SHARED:
        b = bundle()
        _SHARED["bundle"] = xm.map_reads(b.index, b.reads[::BUNDLE_STEP], SUPP_SEC)
    return _SHARED["bundle"]


def single(name):
    """the single-chain model (map_model) on a case"""
    contigs, reads, o, _ = xc.case(name)
    kw = {f: v for f, v in o.items() if f not in ("k", "w")}
    return mm.map_reads(mm.Index(contigs, o["k"], o["w"]), reads, **kw)


def spans(units):
    return [[(u["cls"], u["parent"]) for u in us] for us in units]


# ---- 1. the model alone shows what each case is for ------------------------------------------------------------------------------
def test_model_chimera_is_a_primary_and_one_supplementary():
    units, tot, info = xc.expected("chimera", 0)
    for us in units:
        assert [(u["cls"], u["parent"]) for u in us] == [(xm.PRIMARY, 0), (xm.SUPPLEMENTARY, 1)]
        p, s = us[0]["hit"], us[1]["hit"]
        assert {p["tid"], s["tid"]} == {0, 1} and p["rev"] != s["rev"]
        assert min(p["qe"], s["qe"]) - max(p["qs"], s["qs"]) <= 0  # side by side on the read
        assert s["s2"] == 0 and s["mapq"] == 60 and s["s1"] == p["s2"]
    assert all(i["anchors"] > 4 * 64 for i in info)  # several 64-anchor blocks
    # without --supp the second half is a parent that is not reported, and one selection is all max_chains = 2 allows
    assert spans(xc.expected("chimera", 1)[0]) == [[(0, 0)]] * 2 and xc.expected("chimera", 1)[1]["selections"] == 2
    assert spans(xc.expected("chimera", 2)[0]) == spans(units)


def test_model_two_copies_is_a_primary_and_one_secondary():
    units, tot, info = xc.expected("two_copies", 0)
    hits1 = single("two_copies")[0]
    for us, h1 in zip(units[:2], hits1[:2]):
        assert [(u["cls"], u["parent"]) for u in us] == [(xm.PRIMARY, 0), (xm.SECONDARY, 0)]
        p, s = us[0]["hit"], us[1]["hit"]
        assert p == h1 and p["mapq"] == 0  # the primary is the single-chain run's in every field
        assert (s["qs"], s["qe"]) == (p["qs"], p["qe"])  # the overlap is 100 %
        assert s["s1"] == p["s2"] and s["s2"] == 0 and s["mapq"] == 0 and s["ts"] > p["te"]
    # the read that starts in unique sequence: its second chain scores under pri_pm of the primary and is dropped, but counted
    assert spans(units[2:]) == [[(0, 0)]] and units[2][0]["hit"]["s2"] == info[2]["scores"][0] and tot["dropped_secondary"] == 1
    assert tot["kept_secondary"] == 2
    # secondary_n = 0 keeps none
    assert spans(xc.expected("two_copies", 2)[0]) == [[(0, 0)]] * 3


def test_model_first_further_score_is_the_primarys_s2():
    for name, mi in xc.all_runs():
        units, _, info = xc.expected(name, mi)
        o = mm.opts(**xc.case(name)[2])
        for us, i in zip(units, info):
            h = us[0]["hit"]
            if h is None or xc.case(name)[3][mi]["max_chains"] < 2:
                continue
            if h["s2"] >= o["min_score"]:
                assert i["scores"] and i["scores"][0] == h["s2"], (name, mi)
            else:
                assert i["scores"] == [], (name, mi)


def test_model_pri_pm_edge_is_exact():
    ms = xc.case("pri_edge")[3]
    kept = [[len(us) == 2 for us in xc.expected("pri_edge", mi)[0]] for mi in range(len(ms))]
    ratios = [us[1]["hit"]["s1"] * 1000 // us[0]["hit"]["s1"] for us in xc.expected("pri_edge", 0)[0]]
    for m, k in zip(ms, kept):
        assert k == [m["pri_pm"] <= r for r in ratios], (m, ratios)
    assert kept[0] == [True, True] and kept[-1] == [False, False] and any(k in ([True, False], [False, True]) for k in kept)


def test_model_mask_pm_edge_is_exact():
    (at, above), (under, _) = (xc.expected("mask_edge", mi)[0] for mi in (0, 1))
    m = xc.case("mask_edge")[3][0]
    p, s = at[0]["hit"], at[1]["hit"]
    ov, mn = min(p["qe"], s["qe"]) - max(p["qs"], s["qs"]), min(p["qe"] - p["qs"], s["qe"] - s["qs"])
    assert ov * 1000 == m["mask_pm"] * mn  # on the edge: supplementary, because the comparison is strict
    assert at[1]["cls"] == xm.SUPPLEMENTARY and under[1]["cls"] == xm.SECONDARY  # ... and secondary one per mille lower
    assert above[1]["cls"] == xm.SECONDARY  # the neighbouring trim has the larger ratio
    assert at[1]["hit"]["tid"] != at[0]["hit"]["tid"]


def test_model_caps_and_the_dropped_chain_that_uses_a_selection():
    ms = xc.case("caps")[3]
    got = {(m["max_chains"], m["secondary_n"]): xc.expected("caps", mi) for mi, m in enumerate(ms)}
    n_sec = {key: [len(us) - 1 for us in v[0]] for key, v in got.items()}
    assert n_sec == {(2, 5): [1, 1], (3, 5): [2, 2], (4, 5): [2, 2], (5, 5): [3, 3], (5, 2): [2, 2], (5, 3): [3, 3], (16, 15): [3, 3]}
    # the third further selection outscores the fourth but has fewer than min_cnt anchors: dropped, marked, a selection used
    assert got[(4, 5)][1]["dropped_min_cnt"] == 2 and got[(4, 5)][1]["selections"] == 6 and got[(3, 5)][1]["dropped_min_cnt"] == 0
    for i in got[(5, 5)][2]:
        assert len(i["scores"]) == 4 and i["scores"][2] > i["scores"][3]
    for us in got[(5, 5)][0]:
        assert us[3]["hit"]["n"] >= xc.CAPS_MIN_CNT and us[3]["hit"]["s1"] < us[2]["hit"]["s1"]
    assert got[(5, 2)][1]["dropped_secondary"] == 2


def test_model_wave_block_counts_and_non_monotone_f():
    info = xc.expected("wave_blocks", 0)[2]
    assert tuple(i["anchors"] for i in info[:5]) == xc.BLOCK_COUNTS
    assert 1 <= info[5]["anchors"] < mm.DEFAULTS["min_cnt"] and info[6]["anchors"] == 0
    units = xc.expected("wave_blocks", 0)[0]
    assert [len(us) for us in units] == [2] * 5 + [1, 1] and units[5][0]["hit"] is None and units[6][0]["hit"] is None
    assert all(us[1]["cls"] == xm.SUPPLEMENTARY for us in xc.expected("wave_blocks", 1)[0][:5])  # mask_pm = 1000: nothing is secondary
    units, _, info = xc.expected("non_monotone", 0)
    assert all(i["non_monotone"] > 0 for i in info) and all(len(us) == 2 for us in units)


def test_model_options_on_leave_the_primary_as_it_is():
    for name, mi in xc.all_runs():
        hits1 = single(name)[0]
        assert [us[0]["hit"] for us in xc.expected(name, mi)[0]] == hits1, (name, mi)
    s = synthetic()
    assert [us[0]["hit"] for us in synthetic_units()[0]] == s.hits
    # the generator's reads inside the two-copy repeat gain their second copy; the clear ones gain nothing
    for c, us in zip(s.cases, synthetic_units()[0]):
        assert len(us) == (2 if c["kind"] == "inside" else 1), c["kind"]


# ---- 2. the host twin against the model ------------------------------------------------------------------------------------------
def host_equals_model(contigs, reads, m, units, tot, **o):
    got = np2io.map_host(contigs, reads, chains=True, multi=m, **o)
    xm.check(got, units, reads)
    st = np2io.map_last_multi_stats()
    assert {f: st[f] for f in tot} == tot and st["units"] == sum(len(us) for us in units) and st["more_ms"] == 0
    xm.check(np2io.map_host(contigs, reads, multi=m, **o), units, reads)  # (without the chains)


@pytest.mark.parametrize("name,mi", xc.all_runs())
def test_host_twin_equals_the_model(name, mi):
    contigs, reads, o, ms = xc.case(name)
    units, tot, _ = xc.expected(name, mi)
    host_equals_model(contigs, reads, ms[mi], units, tot, **o)


def test_host_twin_equals_the_model_on_the_generator_and_the_bundle():
    s, b = synthetic(), bundle()
    host_equals_model(s.contigs, s.reads, SUPP_SEC, *synthetic_units())
    host_equals_model(b.contigs, b.reads[::BUNDLE_STEP], SUPP_SEC, *bundle_units())


def test_options_off_through_the_new_door_are_the_plain_doors_arrays():
    for name in sorted(xc.CASES):
        contigs, reads, o, _ = xc.case(name)
        hits, chain, off = np2io.map_host(contigs, reads, chains=True, **o)
        unit_off, uh, cls, parent, uc, uco = np2io.map_host(contigs, reads, chains=True, multi={}, **o)
        assert np.array_equal(unit_off, np.arange(len(reads) + 1)) and not cls.any() and not parent.any()
        assert uh.tobytes() == hits.tobytes() and np.array_equal(uc, chain) and np.array_equal(uco, off)
        assert np2io.map_last_multi_stats()["selections"] == 0


def test_paf_lines_of_the_units():
    contigs, reads, o, ms = xc.case("two_copies")
    units = xc.expected("two_copies", 0)[0]
    lens = [len(c) for c in contigs]
    text = xm.paf(xc.names_of(reads), units, xc.tnames_of(contigs), lens)
    lines = text.splitlines(keepends=True)
    plain = mm.paf(xc.names_of(reads), single("two_copies")[0], xc.tnames_of(contigs), lens).splitlines(keepends=True)
    assert [ln for ln in lines if "tp:A:P" in ln] == plain and sum("tp:A:S" in ln for ln in lines) == 2
    assert lines[1].startswith("r1\t") and lines[1].split("\t")[11] == "0" and "\ts2:i:0\n" in lines[1]


# ---- 3. the rule's text as a stand-alone program under the sanitizers -----------------------------------------------------------
def core_output(name, mi):
    units, tot, _ = xc.expected(name, mi)
    lines = [" ".join(str(tot[f]) for f in xm.COUNTS)]
    for rd, us in zip(xc.case(name)[1], units):
        lines.append(str(len(us)))
        for u in us:
            h = u["hit"]
            fields = " ".join(str(h[f]) for f in mm.HIT_FIELDS) if h else "-1 %d 0 0 0 0 0 0 0 0 0 0 0" % len(rd)
            lines.append("%d %d %s" % (u["cls"], u["parent"], fields))
            lines.append(" ".join("%d:%d" % (r, q) for r, q in u["chain"]))
    return "\n".join(lines) + "\n"


def test_core_program_under_the_sanitizers_matches_the_model(tmp_path):
    exe = str(tmp_path / "mapmulti_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HERE, "tools", "mapmulti_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name, mi in xc.all_runs():
        contigs, reads, o, ms = xc.case(name)
        o, m = mm.opts(**o), ms[mi]
        (tmp_path / "asm").write_bytes(b"".join(c + b"\n" for c in contigs))
        (tmp_path / "reads").write_bytes(b"".join(c + b"\n" for c in reads))
        r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(o[f]) for f in mm.DEFAULTS] +
                           [str(m[f]) for f in xm.MULTI_DEFAULTS], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, mi, r.returncode, r.stderr[-3000:])
        assert r.stdout == core_output(name, mi), (name, mi)
        # the same units aligned, settled (Units::settle) and written as SAM (sa_entry, sam_line_x): the model's text line for line
        aligned, dropped = xc.aligned(name, mi)
        max_cells = xc.ALIGN_KW.get(name, {}).get("max_cells", am.DEFAULTS["max_cells"])
        r = subprocess.run(r.args + ["sam", str(max_cells)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, mi, r.returncode, r.stderr[-3000:])
        want = "".join("".join(xm.sam_lines(nm, rd, None, us, xc.tnames_of(contigs))) for nm, rd, us in zip(xc.names_of(reads), reads, aligned))
        assert r.stdout == f"{dropped}\n" + want, (name, mi)
    r = subprocess.run([exe, str(tmp_path / "asm"), str(tmp_path / "reads")] + [str(mm.DEFAULTS[f]) for f in mm.DEFAULTS] + ["17", "0", "0", "500", "800"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr.startswith("argument: max_chains")


# ---- 4. refusals, before any device call ------------------------------------------------------------------------------------------
def test_argument_checks_return_e_arg_without_a_device():
    asm, reads = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    for kw, word in ((dict(max_chains=0), "max_chains"), (dict(max_chains=17), "max_chains"), (dict(supplementary=2), "supplementary"),
                     (dict(secondary_n=16), "secondary_n"), (dict(mask_pm=0), "mask_pm"), (dict(mask_pm=1001), "mask_pm"),
                     (dict(pri_pm=1001), "pri_pm")):
        with pytest.raises(api.Np2Error) as e:
            np2io.map_host(asm, reads, multi=kw)
        assert e.value.code == E_ARG and word in str(e.value), kw
    with pytest.raises(TypeError):
        np2io.multi_opts(max_chain=3)
    L = np2io._bind()
    o, m = np2io.map_opts(), np2io.multi_opts()
    bad = np2io.multi_opts(max_chains=17)
    a, r = np.frombuffer(asm, np.uint8), np.frombuffer(reads, np.uint8)
    off = np.zeros(2, np.uint64)
    ph, pc, pp, pch, pco = (C.c_void_p() for _ in range(5))
    outs = (off.ctypes.data, C.byref(ph), C.byref(pc), C.byref(pp))
    host = lambda mo, *tail: L.np2_map_host_m(a.ctypes.data, len(a), r.ctypes.data, len(r), 1, C.byref(o), mo, None, *tail)
    assert host(None, *outs, None, None) == E_ARG and b"multi" in L.np2_io_last_error()
    assert host(C.byref(m), off.ctypes.data, None, C.byref(pc), C.byref(pp), None, None) == E_ARG
    assert host(C.byref(m), *outs, C.byref(pch), None) == E_ARG and b"chain" in L.np2_io_last_error()
    # the device doors check the multi-chain options before they look at the index, so no device is touched
    assert L.np2_map_bytes_m(None, r.ctypes.data, len(r), 1, C.byref(o), C.byref(bad), *outs, None, None) == E_ARG
    assert b"max_chains" in L.np2_io_last_error()
    assert L.np2_map_bytes_m(None, r.ctypes.data, len(r), 1, C.byref(o), C.byref(m), *outs, None, None) == E_ARG
    assert b"index" in L.np2_io_last_error()
    assert L.np2_map_files_m(None, None, 0, C.byref(o), C.byref(bad), b"x", None) == E_ARG and b"max_chains" in L.np2_io_last_error()
    assert L.np2_map_last_multi_stats(None) == E_ARG
    assert ph.value is None and pc.value is None and pp.value is None
    # the thread's next call works
    assert host(C.byref(m), *outs, None, None) == 0 and int(off[1]) == 1
    for p in (ph, pc, pp):
        L.np2_free(p)


def test_abi_symbols_are_listed():
    L = api.lib()
    for s in ("np2_map_bytes_m", "np2_map_files_m", "np2_map_host_m", "np2_map_last_multi_stats"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)


# ---- 5. the command line's device-free helpers ------------------------------------------------------------------------------------
def test_command_line_helpers():
    parse = lambda *a: np2map.multi_of(np2map.build_parser().parse_args(["asm.fa", "r.fa"] + list(a)))
    assert parse() is None  # the defaults: the plain doors
    assert parse("--supp") == dict(max_chains=5, supplementary=1, secondary_n=0, mask_pm=500, pri_pm=800)
    assert parse("--secondary", "5") == dict(max_chains=6, supplementary=0, secondary_n=5, mask_pm=500, pri_pm=800)
    assert parse("-N", "5", "--supp") == SUPP_SEC
    assert parse("-N", "15", "--supp")["max_chains"] == 16
    assert parse("--supp", "--max_chains", "3", "--mask_level", "0.3457", "--pri_ratio", "0.9")["max_chains"] == 3
    assert parse("--supp", "--mask_level", "0.3457", "--pri_ratio", "0.9996") == dict(max_chains=5, supplementary=1, secondary_n=0, mask_pm=346,
                                                                                      pri_pm=1000)
    assert parse("--max_chains", "4") == dict(max_chains=4, supplementary=0, secondary_n=0, mask_pm=500, pri_pm=800)
    st = dict(units=7, selections=4, dropped_min_cnt=1, dropped_secondary=1, kept_supplementary=1, kept_secondary=1, overflow_units=0, more_ms=0.25)
    head, row = np2map.multi_stats_row(st).splitlines()
    assert head.split("\t") == list(np2map.MULTI_STATS_HEADER) and row.split("\t") == ["7", "4", "1", "1", "1", "1", "0", "0.250"]


# ---- 6. the units aligned: records, CIGARs, MD and cs per unit, and the SAM lines ---------------------------------------------------
FLAG_SETS = [dict(md=m, cs=c, eqx=e) for m in (False, True) for c in (False, True) for e in (False, True)]


@pytest.mark.parametrize("name,mi", xc.all_runs())
def test_aligned_host_twin_equals_the_model(name, mi):
    contigs, reads, o, ms = xc.case(name)
    aligned, dropped = xc.aligned(name, mi)
    for flags in (FLAG_SETS[0], FLAG_SETS[-1]):
        got = np2io.map_align_host_m(contigs, reads, ms[mi], **flags, **xc.ALIGN_KW.get(name, {}), **o)
        xm.check_aligned(got, aligned, **flags)
        st = np2io.map_last_multi_stats()
        assert st["overflow_units"] == dropped and st["units"] == sum(len(us) for us in aligned)


def test_a_further_unit_that_overflows_is_dropped_and_counted():
    aligned, dropped = xc.aligned("overflow", 0)
    assert [len(us) for us in xc.expected("overflow", 0)[0]] == [2, 2, 2]
    assert [len(us) for us in aligned] == [1, 1, 2] and dropped == 2 and all(us[0]["rec"]["tid"] == 0 for us in aligned)


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "".join(k for k, v in f.items() if v) or "plain")
def test_aligned_options_off_are_the_plain_doors_arrays(flags):
    contigs, reads, o, _ = xc.case("chimera")
    hits, recs, cigar, cigar_off, md, cs = np2io.map_align_host_x(contigs, reads, **flags, **o)
    got = np2io.map_align_host_m(contigs, reads, {}, **flags, **o)
    assert np.array_equal(got["unit_off"], np.arange(len(reads) + 1)) and not got["cls"].any() and not got["parent"].any()
    assert got["hits"].tobytes() == hits.tobytes() and got["recs"].tobytes() == recs.tobytes()
    assert np.array_equal(got["cigar"], cigar) and np.array_equal(got["cigar_off"], cigar_off) and got["md"] == md and got["cs"] == cs


def test_model_sam_of_the_chimera_flags_and_reciprocal_sa():
    contigs, reads, o, ms = xc.case("chimera")
    aligned, _ = xc.aligned("chimera", 0)
    tn = xc.tnames_of(contigs)
    for nm, rd, us in zip(xc.names_of(reads), reads, aligned):
        p, s = (ln.rstrip("\n").split("\t") for ln in xm.sam_lines(nm, rd, None, us, tn, md=True, cs=True, eqx=True))
        assert {int(p[1]) & ~16, int(s[1]) & ~16} == {0, 2048} and (int(p[1]) ^ int(s[1])) & 16  # the halves lie on opposite strands
        assert p[9] == (mm.revcomp(rd) if int(p[1]) & 16 else rd).decode() and len(s[9]) == len(rd)  # full SEQ, soft clips
        assert "S" in p[5] and "H" not in p[5] and "=" in p[5] and p[-2].startswith("cs:Z:")
        # each names the other: rname,pos,strand,CIGAR in M/I/D/S form,mapq,NM;
        for me, other in ((p, s), (s, p)):
            rname, pos, strand, cg, mapq, nmv = me[-1][5:].rstrip(";").split(",")
            assert (rname, pos, mapq, nmv) == (other[2], other[3], other[4], other[11][5:]) and strand == ("-" if int(other[1]) & 16 else "+")
            assert "=" not in cg and "X" not in cg and cg == xm._cigar_text(__import__("aligntags_model").collapse(
                [(c[-1], int(c[:-1])) for c in __import__("re").findall(r"\d+[MIDS=X]", other[5])]))
    # the primary's line is the options-off line but for the appended SA:Z:
    import align_model as am
    hits, chains, _ = single("chimera")
    _, recs, cigars, _ = am.align_mapped(contigs, reads, hits, chains, o["k"])
    for nm, rd, h, rc, cg, us in zip(xc.names_of(reads), reads, hits, recs, cigars, aligned):
        line = xm.sam_lines(nm, rd, None, us, tn)[0]
        assert line.startswith(am.sam_line(nm, rd, h, rc, cg, tn).rstrip("\n") + "\tSA:Z:")
    # a secondary has no SA:Z:, flag 256, mapq 0, and its read's lone parent none either
    aligned, _ = xc.aligned("two_copies", 0)
    lines = xm.sam_lines("r1", xc.case("two_copies")[1][0], None, aligned[0], xc.tnames_of(xc.case("two_copies")[0]))
    assert len(lines) == 2 and "SA:Z:" not in "".join(lines) and lines[1].split("\t")[1] == "256" and lines[1].split("\t")[4] == "0"


def test_aligned_abi_and_argument_checks():
    L = api.lib()
    for s in ("np2_map_align_bytes_m", "np2_map_align_files_m", "np2_map_align_host_m"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)
    asm, reads = b"ACGT" * 30 + b"\n", b"ACGT" * 20 + b"\n"
    with pytest.raises(api.Np2Error) as e:
        np2io.map_align_host_m(asm, reads, dict(max_chains=17))
    assert e.value.code == E_ARG and "max_chains" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.map_align_host_m(asm, reads, {}, gap_ext=0)
    assert e.value.code == E_ARG and "gap_ext" in str(e.value)
    L = np2io._bind()
    o, m, ao = np2io.map_opts(), np2io.multi_opts(max_chains=17), np2io.align_opts()
    r = np.frombuffer(reads, np.uint8)
    off, out = np.zeros(2, np.uint64), np2io.np2_map_units_t()
    assert L.np2_map_align_bytes_m(None, r.ctypes.data, None, len(r), 1, C.byref(o), C.byref(m), C.byref(ao), 0, off.ctypes.data, C.byref(out)) == E_ARG
    assert b"max_chains" in L.np2_io_last_error() and out.hits is None
    assert L.np2_map_align_files_m(None, None, 0, C.byref(o), C.byref(m), C.byref(ao), 0, b"x", None) == E_ARG
    a = np2map.build_parser().parse_args(["asm.fa", "r.fq", "-a", "--supp", "-N", "5", "--qual"])
    assert a.sam and np2map.multi_of(a) == SUPP_SEC
