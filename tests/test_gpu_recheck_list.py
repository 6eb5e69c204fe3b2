"""The final pass's recheck rounds from the list of its RECH regions (np2_regions.hip: k_rech_prepare, k_rech_finish)
against the CPU oracle: bases and positions of every input, three ways —
    list     the default: k_seed lists the regions it labels RECH, five launches per table, nothing read back;
    general  NP2_RECH_GENERAL=1: the kernels over all regions, with their read-backs;
    capped   NP2_TEST_RECH_CAP one below the input's RECH regions: the list overflows, the round splices nothing, the
             error word says so at the end of the pass and the pass is repeated on the general kernels
— each through Polisher.polish and through a two-slot BatchPolisher.  Which path ran is read from the timings
("rech_list": rounds that went by the list, "rech_redo": passes repeated after an overflow).

The RECH counts below are the oracle's (its seed / rech<i> label traces), written out so that a capacity can be set to
"exactly full" and "one past full".  An input without RECH regions cannot overflow: its capped run (capacity 0, exactly
full) must stay on the list path."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_oracle_pinning as tp
from nextpolish2_amd import BatchPolisher, Np2Error, Opts, Polisher
from nextpolish2_amd.api import lib
from nextpolish2_amd.synth import Synth, pileup_from_alignments
from oracle.np2_oracle import Oracle, RefPanic

pytestmark = pytest.mark.gpu


def _chain(n_sites, k=31):
    """n_sites SNP sites 14 bases apart (tests/test_oracle_pinning.py's construction: every 31-mer over a site also covers a
    neighbour, the regions chain), two haplotypes — the contig's (6 reads, count 50) and the one with every site changed
    (4 reads, count 20): every region keeps two candidates and is labelled RECH."""
    bb = tp.backbone(100 + 14 * n_sites + 130, 21)
    h1 = bb
    for p in (100 + 14 * i for i in range(n_sites)):
        h1 = tp.put(h1, p, tp.other(bb[p], skip=(bb[p - 1], bb[p + 1])))
    yak = tp.yak_counted([(h1, 20), (bb, 50)], k)
    return pileup_from_alignments(bb, [(0, bb, bb)] * 6 + [(0, bb, h1)] * 4), [yak], Opts(iter_count=1)


def _three_chained():
    """the pileup of test_three_chained_regions_cartesian_order_and_last_writer_wins: three haplotypes over three sites"""
    bb = tp.backbone(260, 21)
    alt = {p: tp.other(bb[p], skip=(bb[p - 1], bb[p + 1])) for p in (100, 114, 128)}

    def hap(*on):
        s = bb
        for p, o in zip((100, 114, 128), on):
            if o:
                s = tp.put(s, p, alt[p])
        return s
    h0, hy, hx = hap(0, 0, 0), hap(0, 1, 1), hap(1, 1, 0)
    yak = tp.yak_counted([(hx, 10), (hy, 20), (h0, 50)], 31)
    alns = [(0, h0, h0)] * 6 + [(0, h0, hy)] * 3 + [(0, h0, hx)] * 3
    return pileup_from_alignments(h0, alns), [yak], Opts(iter_count=1)


def _contig_ends():
    """two single-region groups: one 5 bases behind the contig's start (its left flank is cut at index 0 under both
    tables), one 28 bases before its end (the closest to the end that still keeps two candidates; its right flank is cut
    at M under the k = 31 table)"""
    L = 300
    bb = tp.backbone(L, 9)
    h1 = bb
    for p in (5, L - 1 - 28):
        h1 = tp.put(h1, p, tp.other(bb[p], skip=(bb[p - 1], bb[p + 1])))
    yaks = [tp.yak_counted([(h1, 20), (bb, 50)], k) for k in (21, 31)]
    return pileup_from_alignments(bb, [(0, bb, bb)] * 6 + [(0, bb, h1)] * 4), yaks, Opts(iter_count=1)


def _synth(seed, read_err, asm_err, snp, indel):
    s = Synth(60000, depth=30, seed=seed, diploid=True, read_err_rate=read_err, asm_err_rate=asm_err, snp_rate=snp,
              hap_indel_rate=indel, read_len_mean=9000.0, read_len_sd=1500.0)
    return s.pileup, [s.yak(21), s.yak(31)], Opts()


def _small_diploid():  # (the recipe of conftest's small_diploid fixture)
    s = Synth(60000, depth=30, seed=22, diploid=True, read_len_mean=9000.0, read_len_sd=1500.0)
    return s.pileup, [s.yak(21), s.yak(31)], Opts()


# name -> (builder, RECH regions after the seed, still RECH after each table): the oracle's counts
CASES = {
    "synth_x10": (lambda: _synth(3, .02, 1e-3, .1, .02), 23, (13, 13)),      # a chain of two; the TEMP / relabel path
    "synth_x6": (lambda: _synth(6, .012, 6e-4, .08, .012), 6, (6, 6)),       # a chain of two that survives both tables
    "small_diploid": (_small_diploid, 0, (0, 0)),                            # the empty list: no job, n_ap == 0
    "three_chained": (_three_chained, 3, (3,)),
    "seven_chained": (lambda: _chain(7), 7, (0,)),                           # the cut at six: 64 + 2 jobs
    "contig_ends": (_contig_ends, 2, (2, 2)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pileup, yaks, opts, the oracle's answer): computed once, shared by every run of the input, never changed"""
    pile, yaks, opts = CASES[name][0]()
    o = Oracle(yaks)
    o.set_trace(True)
    try:
        b, p = o.polish(pile, opts)
        want = ("ok", b, p)
        last = opts.iter_count - 1
        rech = [int(((o.trace(last, tag + ".lable") & 0x20) != 0).sum()) for tag in ["seed"] + [f"rech{i}" for i in range(len(yaks))]]
        assert rech == [CASES[name][1], *CASES[name][2]], rech  # the counts the capacities below are set by
    except RefPanic as e:
        want = ("panic", str(e))
    return pile, yaks, opts, want


def _timings_of(ctx_handle):
    names, ms, n = C.c_void_p(), C.c_void_p(), C.c_int()
    lib().np2_last_timings(ctx_handle, C.byref(names), C.byref(ms), C.byref(n))
    out, addr = {}, names.value
    vals = np.ctypeslib.as_array(C.cast(ms, C.POINTER(C.c_float)), shape=(max(n.value, 1),))
    for i in range(n.value):
        nm = C.string_at(addr)
        addr += len(nm) + 1
        out[nm.decode()] = float(vals[i])
    return out


def _check_result(got, want):
    if want[0] == "ok":
        assert got[0] == "ok", got
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    else:  # the product raises the reference's panic, on every path
        assert got[0] == "panic", got


def _run_both_drivers(name, expect_list, expect_redo):
    pile, yaks, opts, want = _case(name)
    n_tab = len(yaks)

    def check_path(t):
        print(name, {k: v for k, v in t.items() if k.startswith("rech_")})
        if want[0] != "ok":
            return
        assert t.get("rech_list", 0) == (n_tab if expect_list else 0)
        assert t.get("rech_redo", 0) == (1 if expect_redo else 0)
    pol = Polisher(yaks)
    try:
        b, p = pol.polish(pile, opts)
        got = ("ok", b, p)
    except Np2Error as e:
        got = ("panic", str(e)) if "reference would panic" in str(e) else ("error", str(e))
    _check_result(got, want)
    check_path(pol.timings())
    if want[0] != "ok":
        return
    c = pol.upload(pile)
    bp = BatchPolisher(pol, 2)
    try:
        for bb, pp in bp.polish([c, c], opts, want_pos=True):
            _check_result(("ok", bb, pp), want)
        for slot in range(2):
            check_path(_timings_of(lib().np2_batch_slot_ctx(bp._h, slot)))
    finally:
        bp.close()


@pytest.mark.parametrize("name", list(CASES))
def test_list_path_equals_the_oracle(monkeypatch, name):
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    monkeypatch.delenv("NP2_TEST_RECH_CAP", raising=False)
    _run_both_drivers(name, expect_list=True, expect_redo=False)


@pytest.mark.parametrize("name", list(CASES))
def test_general_path_equals_the_oracle(monkeypatch, name):
    monkeypatch.delenv("NP2_TEST_RECH_CAP", raising=False)
    monkeypatch.setenv("NP2_RECH_GENERAL", "1")
    _run_both_drivers(name, expect_list=False, expect_redo=False)


@pytest.mark.parametrize("name", list(CASES))
def test_overflowing_list_is_redone_on_the_general_path(monkeypatch, name):
    """one past full: a capacity one below the regions the seed labels RECH (none: capacity 0 is exactly full, no redo)"""
    n_rech = CASES[name][1]
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    monkeypatch.setenv("NP2_TEST_RECH_CAP", str(max(n_rech, 1) - 1))
    _run_both_drivers(name, expect_list=True, expect_redo=n_rech > 0)


@pytest.mark.parametrize("name", ["synth_x10", "three_chained", "seven_chained"])
def test_exactly_full_list_stays_on_the_list_path(monkeypatch, name):
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    monkeypatch.setenv("NP2_TEST_RECH_CAP", str(CASES[name][1]))
    _run_both_drivers(name, expect_list=True, expect_redo=False)


def test_one_element_list(monkeypatch):
    """a list of one region, exactly full (capacity 1) and one past full (capacity 0): the contig's site of
    test_oracle_pinning's lone-winner case, [contig, winner] kept, the winner taken by the recheck"""
    truth = tp.backbone(220, 5)
    t = truth[100]
    _, ref, wrong, _ = tp._site_case([t])
    x, y = [b for b in "ACGT" if b not in (t, wrong)]
    ins = t + tp.other(t, skip=(truth[101],))
    _, ref, _, alns = tp._site_case([t, x, y, "", ins])
    pile, yaks, opts = pileup_from_alignments(ref, alns), [tp.yak_counted([(truth, 50)], 21)], Opts(iter_count=1)
    ob, op = Oracle(yaks).polish(pile, opts)
    assert ob.tobytes().decode() == truth
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    for cap, redo in ((1, 0), (0, 1)):
        monkeypatch.setenv("NP2_TEST_RECH_CAP", str(cap))
        pol = Polisher(yaks)
        gb, gp = pol.polish(pile, opts)
        assert np.array_equal(gb, ob) and np.array_equal(gp, op)
        t = pol.timings()
        assert t.get("rech_list", 0) == 1 and t.get("rech_redo", 0) == redo


@pytest.mark.parametrize("cap,redo", [("3,8", 0), ("3,7", 1), ("3,8,100000", 0), ("3,8,300", 1)])
def test_job_and_byte_capacities(monkeypatch, cap, redo):
    """the three chained regions make 2 x 2 x 2 = 8 jobs of about 100 bytes each (two flanks of 30, three candidates, two
    stretches of 13): 8 jobs are exactly full, 7 one short; 300 bytes hold no three of the strings"""
    pile, yaks, opts, want = _case("three_chained")
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    monkeypatch.setenv("NP2_TEST_RECH_CAP", cap)
    pol = Polisher(yaks)
    gb, gp = pol.polish(pile, opts)
    assert np.array_equal(gb, want[1]) and np.array_equal(gp, want[2])
    t = pol.timings()
    assert t.get("rech_list", 0) == 1 and t.get("rech_redo", 0) == redo


def test_overflow_redo_composes_with_the_growth_guess_redo(monkeypatch):
    """NP2_TEST_GROW_GUESS=0 makes the first attempt outgrow its guessed allowance, the capacity makes the list overflow:
    the pass ends on the exact allowance and the general kernels, whichever error the first attempt met first"""
    pile, yaks, opts, want = _case("synth_x10")
    monkeypatch.delenv("NP2_RECH_GENERAL", raising=False)
    monkeypatch.setenv("NP2_TEST_GROW_GUESS", "0")
    monkeypatch.setenv("NP2_TEST_RECH_CAP", "22")
    pol = Polisher(yaks)
    gb, gp = pol.polish(pile, opts)
    assert np.array_equal(gb, want[1]) and np.array_equal(gp, want[2])
    assert pol.timings().get("rech_redo", 0) == 1
