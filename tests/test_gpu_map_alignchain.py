"""The aligner's kernels on caller-built chains (np2_align_chains_device; include/np2_io.h): the cases of
tests/alignchain_cases.py, which the mapper cannot be steered into.  k_align_dp's matrix loop is its own text (a prefix maximum
over 64 lanes for E, carries between the lane blocks of a band, the previous row in LDS, the best cell reduced over the lanes), so
it is held here to the Python model (records, CIGAR words, offsets, counters) and to the host door's sequential dp_slot, which
tests/test_alignchain_cpu.py holds to the model: slots, the cell every walk starts from, and the traceback bytes of every matrix,
byte for byte over every cell.  Again with traceback-budget boundaries between the reads, on recycled memory, and around calls
of the ordinary door on the same index; and one refusal per validation rule.

(The file's name sorts it behind test_gpu_map.py, as tests/test_gpu_map_align.py's docstring explains it must.)"""
import contextlib

import numpy as np
import pytest

import alignchain_cases as cc
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io

pytestmark = pytest.mark.gpu

E_ARG = -1
W = 5  # (the index is there for its assembly; its minimizers are never looked up)


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


_HOST = {}


def host(name):
    """the host door's answer and probe, once per case"""
    if name not in _HOST:
        contigs, reads, hits, chains, k, ao = cc.CASES[name]
        _HOST[name] = np2io.align_chains_host(contigs, reads, hits, chains, k=k, probe=True, **ao)
    return _HOST[name]


def index(name):
    return np2io.MapIndex(cc.CASES[name][0], k=cc.K, w=W, stream=True)


def device_equals_model_and_host(name, ix=None, **hooks):
    """-> the mapper's stats of the call (groups: the sub-groups of the traceback budget)"""
    contigs, reads, hits, chains, k, ao = cc.CASES[name]
    with env(**hooks), (index(name) if ix is None else contextlib.nullcontext(ix)) as ix:
        recs, cigar, off, pr = np2io.align_chains_device(ix, reads, hits, chains, probe=True, **ao)
        st, mst = np2io.align_last_stats(), np2io.map_last_stats()
    cc.check((recs, cigar, off), name)
    cnt = cc.expected(name)[2]
    assert {f: st[f] for f in cnt} == cnt, name
    assert (mst["reads"], mst["unmapped"]) == (len(reads), sum(h is None for h in hits))
    h_recs, h_cigar, h_off, hp = host(name)
    assert np.array_equal(recs, h_recs) and np.array_equal(cigar, h_cigar) and np.array_equal(off, h_off), name
    assert np.array_equal(pr["slot_off"], hp["slot_off"]) and np.array_equal(pr["tb_off"], hp["tb_off"]), name
    for i, (a, b) in enumerate(zip(pr["slots"], hp["slots"])):
        assert a == b, f"{name}: slot {i}: the device {a}, the host {b}"
    for i, (a, b) in enumerate(zip(pr["res"], hp["res"])):
        assert a == b, f"{name}: slot {i} ({pr['slots'][i]}): the device's cell {a}, the host's {b}"
    if not np.array_equal(pr["tb"], hp["tb"]):
        assert len(pr["tb"]) == len(hp["tb"]), name
        at = int(np.flatnonzero(pr["tb"] != hp["tb"])[0])
        slot = int(np.searchsorted(hp["tb_off"], at, side="right")) - 1
        cell, width = at - int(hp["tb_off"][slot]), int(hp["slots"][slot]["W"])
        raise AssertionError(f"{name}: slot {slot} ({hp['slots'][slot]}), row {cell // width}, band slot {cell % width}: "
                             f"the device wrote {pr['tb'][at]}, dp_slot {hp['tb'][at]}")
    return mst


# ---- 1. every case: the device equals the model, and the host cell by cell ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_device_equals_the_model_and_the_host(name):
    mst = device_equals_model_and_host(name)
    assert mst["groups"] == 1


# ---- 2. traceback-budget boundaries between the reads ------------------------------------------------------------------------------
def read_cells(name):
    hp = host(name)[3]
    at = hp["tb_off"][hp["slot_off"].astype(np.int64)].astype(np.int64)
    return np.diff(at)


@pytest.mark.parametrize("name", sorted(cc.BAND_CASES + cc.LANE_CASES + ["slots"]))
def test_budget_boundaries_change_nothing(name):
    n_reads = len(cc.CASES[name][1])
    cells = read_cells(name)
    first = int(np.flatnonzero(cells)[0])
    assert np.count_nonzero(cells[first + 1:])  # (a later read has a matrix: the cut falls between two reads that have one)
    with index(name) as ix:
        one = device_equals_model_and_host(name, ix, NP2_ALIGN_TEST_BUDGET="1")
        cut = device_equals_model_and_host(name, ix, NP2_ALIGN_TEST_BUDGET=str(int(cells[:first + 1].sum())))
    assert one["groups"] == n_reads and 1 < cut["groups"] <= n_reads


# ---- 3. recycled memory: sH[W], the unwritten tail of a traceback row, the slack behind the traceback buffer -------------------------
@pytest.mark.parametrize("byte", [0xFF, 0x00])
@pytest.mark.parametrize("sc", ["ties"] + list(cc.OPTSETS))
def test_recycled_memory_changes_nothing(sc, byte):
    names = cc.TIE_CASES if sc == "ties" else [n for n in cc.BAND_CASES if n.endswith("_" + sc)]
    assert len(names) == (4 if sc == "ties" else len(cc.BAND_SHAPES))
    with api.alloc_poison(byte):
        for name in names:
            with index(name) as ix:  # (made inside the block: a handle keeps its buffers)
                device_equals_model_and_host(name, ix)
                device_equals_model_and_host(name, ix, NP2_ALIGN_TEST_BUDGET="1")


# ---- 4. the order of calls: the ordinary door before and after a chains call on one index ---------------------------------------
def test_the_ordinary_door_is_unchanged_around_a_chains_call():
    contigs, reads, hits, chains, k, ao = cc.CASES["slots"]
    with index("slots") as ix:
        before = ix.align(reads, band=4)
        device_equals_model_and_host("slots", ix)
        after = ix.align(reads, band=4)
        device_equals_model_and_host("slots", ix)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # (the mapper finds the long reads on its own: the comparison is of records, not of flag 4 with flag 4)
    assert [int(r["tid"]) for r in before[1]][1::2] == [h["tid"] for h in hits][1::2] and len(before[2]) > 300


# ---- 5. refusals: one per validation rule, before anything is uploaded ----------------------------------------------------------
@pytest.mark.parametrize("label", [r[0] for r in cc.REFUSALS])
def test_device_door_refuses_and_the_handle_goes_on(label):
    change, words = next(r[1:] for r in cc.REFUSALS if r[0] == label)
    contigs, reads, hits, chain, off = cc.refusal_call()
    with np2io.MapIndex(contigs, k=cc.K, w=W, stream=True) as ix:
        bad = (hits.copy(), chain.copy(), off.copy())
        k = change(*bad, cc.K)
        with pytest.raises(api.Np2Error) as e:
            np2io.align_chains_device(ix, reads, bad[0], (bad[1], bad[2]), k=k, band=4)
        assert e.value.code == E_ARG and all(w in str(e.value) for w in words) and "np2_align_chains_device" in str(e.value), str(e.value)
        good = np2io.align_chains_device(ix, reads, hits, (chain, off), band=4)
    want = np2io.align_chains_host(contigs, reads, hits, (chain, off), k=cc.K, band=4)
    assert all(np.array_equal(a, b) for a, b in zip(good, want)) and [int(t) for t in good[0]["tid"]] == [0, -1, 0]
