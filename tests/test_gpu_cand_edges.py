"""The candidate kernels (csrc/np2_cand.hip: k_region_measure, k_region_write) at the edges of the clean-read shortcut: the
hand-built pileups of cand_cases.py, each straddling one condition of the shortcut, against the CPU oracle — every stage
traced, the default (untraced) path, the same inputs with the shortcut off (NP2_TILE_CAP=1: every record spills, every pair
is decoded), all of them through one batch, and the cases about slots and lanes on poisoned memory.  Every comparison is
exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cand_cases as cc
from nextpolish2_amd import BatchPolisher, Polisher, api
from nextpolish2_amd.api import Np2Error
from test_gpu_parity import check_all_stages

pytestmark = pytest.mark.gpu
E_DEVICE = -2  # NP2_E_DEVICE
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = sorted(cc.CASES)


def guarded(what, fn, *a, **kw):
    """Nothing more may run on a device that has reported an error: the session ends here."""
    try:
        return fn(*a, **kw)
    except Np2Error as e:
        if e.code == E_DEVICE:
            pytest.exit(f"device error in {what}: {e}", returncode=3)
        raise


def untraced(what, pu, yaks, opts, ref):
    """Polisher.polish without set_trace (trace mode changes allocation and pass reuse in np2_polish.cpp) against the oracle's answer"""
    gb, gp = guarded(what, lambda: Polisher(yaks).polish(pu, opts))
    assert np.array_equal(gb, ref[1]) and np.array_equal(gp, ref[2]), what


def run_case(name, what, traced=True, plain=True):
    pu, yaks, opts = cc.CASES[name]
    ref = cc.expected(name)
    if ref is None:  # the same refusal on both sides
        with pytest.raises(Np2Error):
            guarded(what, lambda: Polisher(yaks).polish(pu, opts))
        return
    if traced:
        guarded(what, check_all_stages, pu, yaks, opts, ref)
    if plain:
        untraced(what, pu, yaks, opts, ref)


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_matches_the_oracle(name):
    run_case(name, name, plain=False)


@pytest.mark.parametrize("name", NAMES)
def test_default_path_matches_the_oracle(name):
    run_case(name, f"{name} untraced", traced=False)


@pytest.mark.parametrize("name", NAMES)
def test_shortcut_off_gives_the_same_answer(monkeypatch, name):
    """one-record buckets: the tile's records spill, tn > bucket_cap, every pair is decoded — the general path next to the shortcut"""
    monkeypatch.setenv("NP2_TILE_CAP", "1")  # (read when a context is made)
    run_case(name, f"{name} NP2_TILE_CAP=1")


@pytest.mark.parametrize("cap", cc.BUCKET_CAPS)
def test_bucket_holds_its_tile_exactly_or_one_record_less(monkeypatch, cap):
    """tn <= bucket_cap: case `bucket` has tiles of 12 and 13 records; cap 13 is the last that keeps the record index (and the
    shortcut), 12 the first under which a tile spills and the contig takes the device-wide sort"""
    monkeypatch.setenv("NP2_TILE_CAP", str(cap))
    run_case("bucket", f"bucket NP2_TILE_CAP={cap}")


def test_all_cases_through_a_two_slot_batch():
    groups = {}
    for name in NAMES:
        pu, yaks, opts = cc.CASES[name]
        if cc.expected(name) is not None:
            groups.setdefault((id(yaks[0]), tuple(sorted(vars(opts).items()))), []).append(name)
    for names in groups.values():
        _, yaks, opts = cc.CASES[names[0]]
        names = names * 2 if len(names) == 1 else names  # (a lone contig twice: both slots busy)
        g = Polisher(yaks)
        contigs = [guarded(f"upload {n}", g.upload, cc.CASES[n][0]) for n in names]
        bp = BatchPolisher(g, 2)
        out = guarded(f"batch of {names}", bp.polish, contigs, opts, want_pos=True)
        for n, (bb, pp) in zip(names, out):
            _, ob, op = cc.expected(n)
            assert np.array_equal(bb, ob) and np.array_equal(pp, op), n
        bp.close()


def poisoned_run():
    d0 = api.alloc_poison_stats()[0]
    with api.alloc_poison(0xFF):  # (the contexts are made inside the block)
        for name in cc.POISONED:
            run_case(name, f"{name} on 0xFF memory")
    assert api.alloc_poison_stats()[0] > d0


_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import pytest\n"
                "import test_gpu_cand_edges as t\n"
                "try:\n"
                "    t.poisoned_run()\n"
                "except pytest.exit.Exception as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3)\n" % (ROOT, HERE))


def test_kept_slots_and_list_lanes_on_poisoned_memory():
    """kept_* slots beyond reg_ncand and lanes beyond nlist must never be read as data: the cases about the 60 kept candidates
    and the 64-read list, traced and untraced, with every block the pools hand out filled with 0xFF first.  In a process
    of its own: the hook's counters are the process's (test_gpu_dirty_memory.py reads them from zero)."""
    r = subprocess.run([sys.executable, "-c", _POISON_CODE], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        pytest.exit(f"device error under poison 0xff: {r.stderr.decode(errors='replace')[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
