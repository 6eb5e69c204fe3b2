"""The aligner on caller-built chains without a GPU (include/np2_io.h: np2_align_chains_host): the cases of
tests/alignchain_cases.py through the host door against the Python model of tests/align_model.py, field for field: records,
CIGARs and counters; every read's slots and the cell each matrix's walk starts from against the model's band_of and extension;
the traceback bytes of dp_slot against the bits the model's tables imply, over every cell of every matrix under 20 000 cells;
the same rule text as a stand-alone program with and without the host sanitizers; and one refusal per validation rule.

The cases come first: that each reaches the edge it is built for is asserted on the model's answers and on the slots."""
import os
import subprocess

import numpy as np
import pytest

import align_model as am
import alignchain_cases as cc
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1


def host(name, probe=True):
    contigs, reads, hits, chains, k, ao = cc.CASES[name]
    got = np2io.align_chains_host(contigs, reads, hits, chains, k=k, probe=probe, **ao)
    return got, np2io.align_last_stats()


_HOST = {}


def host_once(name):
    if name not in _HOST:
        _HOST[name] = host(name)
    return _HOST[name]


def kinds(name):
    return [int(x) for x in host_once(name)[0][3]["slots"]["kind"]]


# ---- 1. the cases reach the edges they are built for ---------------------------------------------------------------------------
def test_random_pairs_are_cores_by_construction():
    for sc in cc.OPTSETS:
        n = 0
        for band in (0, 1, 5, 40):
            name = f"rand{band}_{sc}"
            cnt = cc.expected(name)[2]
            assert cnt["cores"] == cnt["segments"] == len(cc.CASES[name][1]) and cnt["overflow"] == 0, name
            n += cnt["cores"]
            assert {h["rev"] for h in cc.CASES[name][2]} == {0, 1}
        assert n >= 200, sc


def test_band_widths_and_the_overflow():
    widths = {}
    for band in cc.BAND_SHAPES:
        sl = cc.model_slots(f"band{band}_dflt")
        widths[band] = [s[1]["W"] for s in sl]
        assert all(s[0]["kind"] == s[2]["kind"] == cc.K_EMPTY and s[1]["kind"] == cc.K_CORE for s in sl)
    assert widths == {0: [1, 2, 4, 4, 2], 31: [63, 64, 64], 32: [65, 67], 63: [127, 128], 64: [129, 130], 1023: [2048, 2049, 2047]}
    assert [(s[1]["lo"], s[1]["tl"] - s[1]["ql"]) for s in cc.model_slots("band0_dflt")] == [(0, 0), (0, 1), (0, 3), (-3, -3), (-1, -1)]
    for sc in cc.OPTSETS:
        recs, _, cnt, _ = cc.expected(f"band1023_{sc}")
        assert [r["tid"] for r in recs] == [0, -1, 0] and cnt["overflow"] == 1 and cnt["cores"] == 3 and cnt["cells"] == 30 * 2048 + 30 * 2047


def test_lane_block_runs_are_single_gaps_under_the_defaults():
    cig = [cc.cigar_str(c) for c in cc.expected("lane_dflt")[1]]
    runs = [[(op, L) for op, L in c if op in "ID" and L >= 30] for c in cc.expected("lane_dflt")[1]]
    assert runs == [[("D", 70)], [("D", 140)], [("D", 30), ("D", 70)], [("D", 31), ("D", 70)], [("D", 32), ("D", 70)], [("I", 70)]], cig
    # the runs lie where the lane blocks meet: slot = column - row - lo
    assert [s[1]["lo"] for s in cc.model_slots("lane_dflt")] == [-32] * 5 + [-102]
    assert [s[1]["W"] for s in cc.model_slots("lane_dflt")] == [135, 205, 165, 166, 167, 135]


def test_tie_cases_hold_equal_best_cells_in_other_lanes_and_rows():
    for sc in cc.TIE_SCORING:
        best, end = cc.expected(f"tie_{sc}_best"), cc.expected(f"tie_{sc}_end")
        assert len(best[3]) == len(end[3]) == 16
        # no end cell: the walk starts at the best cell, which other rows and other lanes hold as well
        assert all(m["best_rows"] > 1 and m["best_slots"] > 1 and m["shape"][0] == 13 for m in best[3])
        assert all(s["ql"] == 12 and s["ql"] < h["qlen"] - cc.K for rd, h in zip(cc.model_slots(f"tie_{sc}_best"), cc.CASES[f"tie_{sc}_best"][2])
                   for s in rd if s["kind"] != cc.K_EMPTY)
        # the largest bonus: the walk starts in the last row, whose largest H more than one column holds
        assert all(m["last_best"] > 1 and m["res"][1] == m["shape"][0] - 1 for m in end[3])


def test_end_bonus_flips_at_the_difference():
    cig = lambda name: [cc.cigar_str(c) for c in cc.expected(name)[1]]
    whole, clipped = ["36M", "36M"] * 2, ["31M5S", "5S31M"] * 2
    assert cig("bonus_eq") == whole and cig("bonus_max") == whole and cig("bonus_less") == clipped and cig("bonus_0") == clipped
    assert [m["res"] for m in cc.expected("bonus_eq")[3]] == [(20 - 2 * 4 + 3, 25, 25)] * 4
    assert [m["res"] for m in cc.expected("bonus_less")[3]] == [(20, 20, 20)] * 4 and cc.BONUS_DIFF == 5 and cc.CASES["bonus_eq"][5]["end_bonus"] == 5


def test_extension_shapes():
    sl = cc.model_slots("ext_limits")
    per_side = []
    for i in range(0, 32, 8):  # tail forward, head forward, tail reverse, head reverse
        side = [s[1] if s[1]["kind"] != cc.K_EMPTY else s[0] for s in sl[i:i + 8]]
        assert all(s[0]["kind"] == cc.K_EMPTY or s[1]["kind"] == cc.K_EMPTY for s in sl[i:i + 8])
        per_side.append([(x["ql"], x["tl"]) for x in side])
    assert per_side == [[(39, 47), (40, 48), (40, 48), (19, 11), (20, 12), (20, 13), (5, 0), (8, 0)]] * 4
    k = kinds("ext_band0")
    assert k.count(cc.K_EMPTY) > len(cc.CASES["ext_band0"][1]) and k[-4:] == [cc.K_EMPTY, cc.K_TAIL, cc.K_HEAD, cc.K_EMPTY]
    assert [(s["ql"], s["W"]) for rd in cc.model_slots("ext_wide") for s in rd if s["kind"] != cc.K_EMPTY] == [(70, 2047), (3, 2047)]
    recs = cc.expected("ext_limits")[0]
    assert all(r["tid"] >= 0 for r in recs) and [r["flag"] for r in recs[-2:]] == [16, 16]


def test_plans():
    k = [[s["kind"] for s in rd] for rd in cc.model_slots("plans")]
    E, G, S, C, H, T, N = cc.K_EQUAL, cc.K_GAP, cc.K_SNV, cc.K_CORE, cc.K_HEAD, cc.K_TAIL, cc.K_EMPTY
    assert k[0] == [N, E, N] and k[1] == k[2] == [N, G, N]
    sl = cc.model_slots("plans")
    assert (sl[0][1]["tl"], sl[0][1]["ql"]) == (0, 0) and (sl[1][1]["tl"], sl[1][1]["ql"]) == (0, 7) and (sl[2][1]["tl"], sl[2][1]["ql"]) == (7, 0)
    assert k[3] == k[4] == k[5] == [N, E, N] and k[6] == [H, E, N]  # the anchors that are no pins leave two pins, or one less
    assert k[7] == [N, T] and k[8] == [H, N]
    recs, cigars = cc.expected("plans")[:2]
    assert cc.cigar_str(cigars[9]) == cc.cigar_str(cigars[10]) and recs[10]["nm"] == recs[9]["nm"] + 1 and recs[10]["as"] == recs[9]["as"] - 5
    assert {f: recs[9][f] for f in ("pos", "end", "flag")} == {f: recs[10][f] for f in ("pos", "end", "flag")}
    contigs = cc.CASES["plans"][0]
    assert recs[11]["tid"] == recs[12]["tid"] == len(contigs) - 1 and (recs[11]["pos"], recs[11]["end"]) == (0, len(contigs[-1]))
    assert [len(s) for s in cc.model_slots("slots")] == [2, 255, 2, 256, 2, 257, 2]
    for at in (0, 63, 64):
        recs = cc.expected(f"jobs_unmapped{at}")[0]
        assert [i for i, r in enumerate(recs) if r["tid"] < 0] == [at] and len(recs) == 65


# ---- 2. the host door against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_door_equals_the_model(name):
    (recs, cigar, off, pr), st = host_once(name)
    cc.check((recs, cigar, off), name)
    cnt, facts = cc.expected(name)[2:]
    assert {f: st[f] for f in cnt} == cnt
    assert cnt["cells"] == cc.CELLS[name]
    # the slots, from the rule's text
    want = cc.model_slots(name)
    assert pr["slot_off"].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    flat = [s for rd in want for s in rd]
    have = [{f: int(x[f]) for f in cc.SLOT_FIELDS} for x in pr["slots"]]
    assert have == flat, next((i, h, w) for i, (h, w) in enumerate(zip(have, flat)) if h != w)
    # the matrices: one per slot with cells, in slot order; the cell its walk starts from, and the bits
    cells = np.diff(pr["tb_off"].astype(np.int64))
    with_cells = [i for i, s in enumerate(flat) if s["kind"] >= cc.K_CORE and s["kind"] != cc.K_EMPTY and not s["over"]]
    assert np.flatnonzero(cells).tolist() == with_cells and len(facts) == len(with_cells)
    n_small = 0
    for i, m in zip(with_cells, facts):
        assert m["shape"] == (flat[i]["ql"] + 1, flat[i]["W"]) and cells[i] == m["shape"][0] * m["shape"][1]
        assert tuple(int(x) for x in pr["res"][i]) == m["res"], (name, i)
        if m["bits"] is None:
            continue
        n_small += 1
        got = pr["tb"][int(pr["tb_off"][i]):int(pr["tb_off"][i + 1])]
        if not np.array_equal(got, m["bits"]):
            at = int(np.flatnonzero(got != m["bits"])[0])
            raise AssertionError(f"{name}: slot {i}, row {at // m['shape'][1]}, band slot {at % m['shape'][1]}: dp_slot {got[at]}, the model {m['bits'][at]}")
    assert all(tuple(int(x) for x in pr["res"][i]) == (0, 0, 0) for i in range(len(flat)) if i not in set(with_cells))
    assert n_small or name in ("band1023_" + sc for sc in cc.OPTSETS) or name == "ext_wide"


def test_probe_is_optional_and_changes_nothing():
    contigs, reads, hits, chains, k, ao = cc.CASES["plans"]
    plain = np2io.align_chains_host(contigs, reads, hits, chains, k=k, **ao)
    assert len(plain) == 3
    cc.check(plain, "plans")
    slots_only = np2io.align_chains_host(contigs, reads, hits, chains, k=k, probe=np2io.PROBE_SLOTS, **ao)[3]
    tb_only = np2io.align_chains_host(contigs, reads, hits, chains, k=k, probe=np2io.PROBE_TB, **ao)[3]
    whole = host_once("plans")[0][3]
    assert sorted(slots_only) == ["res", "slot_off", "slots"] and sorted(tb_only) == ["tb", "tb_off"]
    assert all(np.array_equal(whole[f], x) for f, x in list(slots_only.items()) + list(tb_only.items()))


# ---- 3. the rule's text as a stand-alone program, plain and under the host sanitizers -----------------------------------------------
def program_output(name):
    recs, cigars, cnt, _ = cc.expected(name)
    lines = [" ".join(str(cnt[f]) for f in am.COUNT_FIELDS)]
    for rec, cg in zip(recs, cigars):
        lines.append(" ".join(str(rec[f]) for f in am.REC_FIELDS) + " " + (cc.cigar_str(cg) or "*"))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_chains_program_matches_the_model(tmp_path, flags):
    exe = str(tmp_path / "align_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "tools", "align_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in sorted(cc.CASES):
        (tmp_path / "case").write_text(cc.case_text(name))
        r = subprocess.run([exe, "chains", str(tmp_path / "case")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-3000:])
        assert r.stdout == program_output(name), name


# ---- 4. refusals: one per validation rule, before any walk -------------------------------------------------------------------------
def call_host(contigs, reads, hits, chain, off, k):
    return np2io.align_chains_host(contigs, reads, hits, (chain, off), k=k, band=4)


@pytest.mark.parametrize("label", [r[0] for r in cc.REFUSALS])
def test_host_door_refuses(label):
    change, words = next(r[1:] for r in cc.REFUSALS if r[0] == label)
    contigs, reads, hits, chain, off = cc.refusal_call()
    good = call_host(contigs, reads, hits, chain, off, cc.K)
    assert [int(t) for t in good[0]["tid"]] == [0, -1, 0]
    bad = (hits.copy(), chain.copy(), off.copy())
    k = change(*bad, cc.K)
    if label == "k":
        k, words = cc.K - 1, ("k = 10", "11 .. 28")
    with pytest.raises(api.Np2Error) as e:
        call_host(contigs, reads, *bad, k)
    assert e.value.code == E_ARG and all(w in str(e.value) for w in words) and "np2_align_chains_host" in str(e.value), str(e.value)
    again = call_host(contigs, reads, hits, chain, off, cc.K)
    assert all(np.array_equal(a, b) for a, b in zip(good, again))


def test_null_arguments_and_option_limits_are_statuses():
    import ctypes as C
    contigs, reads, hits, chain, off = cc.refusal_call()
    L = np2io._bind()
    a, s = np2io._stream_of(contigs)[0], np2io._stream_of(reads)[0]
    recs, coff, pc, ao = np.zeros(3, np2io.ALIGN_REC_DTYPE), np.zeros(4, np.uint64), C.c_void_p(), np2io.align_opts(band=4)
    call = lambda *x: L.np2_align_chains_host(a.ctypes.data, len(a), s.ctypes.data, len(s), *x)
    ok = (3, cc.K, hits.ctypes.data, chain.ctypes.data, off.ctypes.data, C.byref(ao), recs.ctypes.data, C.byref(pc), coff.ctypes.data, None)
    for at, word in ((2, b"hits"), (4, b"chain_off"), (5, b"align_opts"), (6, b"recs"), (7, b"cigar"), (8, b"cigar")):
        args = list(ok)
        args[at] = None
        assert call(*args) == E_ARG and word in L.np2_io_last_error(), word
    assert call(*((2,) + ok[1:])) == E_ARG and b"n_reads" in L.np2_io_last_error()
    pr = np2io.np2_align_probe_t(want=4)
    assert call(*(ok[:-1] + (C.byref(pr),))) == E_ARG and b"probe" in L.np2_io_last_error()
    assert L.np2_align_chains_device(None, s.ctypes.data, len(s), *ok) == E_ARG and b"index" in L.np2_io_last_error()
    with pytest.raises(api.Np2Error) as e:
        np2io.align_chains_host(contigs, reads, hits, (chain, off), k=cc.K, band=1024)
    assert e.value.code == E_ARG and "band" in str(e.value)
    assert call(*ok) == 0 and [int(t) for t in recs["tid"]] == [0, -1, 0]
    L.np2_free(pc)


def test_abi_symbols_are_listed():
    L = api.lib()
    for s in ("np2_align_chains_device", "np2_align_chains_host"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)
