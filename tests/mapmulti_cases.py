"""Hand-built cases of the mapper's further chains (test_mapmulti_cpu.py, test_gpu_mapmulti.py; the rule: include/np2_io.h,
"More chains"): contigs of 2-6 kb and reads of up to 2 kb at k = 15, w = 5, a few hundred anchors a read, so that a read
spans several of the selection kernel's 64-anchor blocks.  A case is (contigs, reads, mapper options, a list of multi-chain
options); the values that sit on an edge (pri_pm, mask_pm, the trims) are derived from the model's own scores and intervals
(mapmulti_model.py), so every edge is exact."""
import functools

import numpy as np

import map_model as mm
import mapmulti_model as xm
from map_cases import rand

KW = dict(k=15, w=5)


def _index(contigs):
    return mm.Index(contigs, KW["k"], KW["w"])


def _units(contigs, reads, m, o=None, info=None):
    kw = {f: v for f, v in (o or KW).items() if f not in ("k", "w")}
    return xm.map_reads(_index(contigs), reads, m, info, **kw)


def mutate(rng, s, every):
    """a substitution at every `every`-th base"""
    s = bytearray(s)
    for at in range(every // 2, len(s), every):
        s[at] = b"ACGT"[(b"ACGT".index(bytes([s[at]])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


# ---- 1. a chimera: the read's left half from contig A forward, its right half from contig B reverse ---------------------------
def _chimera():
    rng = np.random.default_rng(201)
    a, b = rand(rng, 2500), rand(rng, 2000)
    read = a[600:1400] + mm.revcomp(b[500:1200])
    return [a, b], [read, mm.revcomp(read)], dict(KW), [xm.multi(max_chains=5, supplementary=1), xm.multi(max_chains=5, secondary_n=5),
                                                       xm.multi(max_chains=2, supplementary=1, secondary_n=3)]


# ---- 2. two exact repeat copies -------------------------------------------------------------------------------------------------
def _two_copy_contig(rng, rep_n=1200):
    rep = rand(rng, rep_n)
    c = rand(rng, 400) + rep + rand(rng, 500) + rep + rand(rng, 400)
    return c, 400, 400 + rep_n + 500  # the copies' starts


def _two_copies():
    rng = np.random.default_rng(202)
    c, r0, r1 = _two_copy_contig(rng)
    reads = [c[r0 + 100:r0 + 1100], mm.revcomp(c[r1 + 50:r1 + 1150]), c[r0 - 300:r0 + 700]]  # the last: 300 unique bases first
    return [c], reads, dict(KW), [xm.multi(max_chains=6, secondary_n=5), xm.multi(max_chains=6, supplementary=1, secondary_n=5),
                                  xm.multi(max_chains=16, supplementary=1)]


# ---- 3. pri_pm on its edge: one copy carries substitutions ----------------------------------------------------------------------
def _pri_edge():
    rng = np.random.default_rng(203)
    rep = rand(rng, 1200)
    c = rand(rng, 400) + rep + rand(rng, 500) + mutate(rng, rep, 97) + rand(rng, 400)
    reads = [rep[100:1100], mm.revcomp(rep[:900])]
    units, _ = _units([c], reads, xm.multi(max_chains=4, secondary_n=5, pri_pm=0))
    assert all(len(us) == 2 and us[1]["cls"] == xm.SECONDARY for us in units)
    edge = min(us[1]["hit"]["s1"] * 1000 // us[0]["hit"]["s1"] for us in units)  # the smaller ratio: both kept at it
    edge_hi = max(us[1]["hit"]["s1"] * 1000 // us[0]["hit"]["s1"] for us in units)
    assert 0 < edge <= edge_hi < 1000
    return [c], reads, dict(KW), [xm.multi(max_chains=4, secondary_n=5, pri_pm=pm) for pm in sorted({edge, edge + 1, edge_hi, edge_hi + 1})]


# ---- 4. mask_pm on its edge: a chimera whose pieces overlap on the read ---------------------------------------------------------
def _mask_edge():
    """A holds X M, B holds M Y, the read is X M Y: the two chains overlap by about M on the read.  The read's end is trimmed
    until ov * 1000 == mask_pm * min(len) for a whole mask_pm: supplementary there (the comparison is strict) and secondary at
    mask_pm - 1; and a second trim, the nearest one with a larger ratio, is secondary at that same mask_pm."""
    rng = np.random.default_rng(204)
    x, mid, y = rand(rng, 700), rand(rng, 300), rand(rng, 600)
    a, b = rand(rng, 500) + x + mid + rand(rng, 500), rand(rng, 300) + mid + y + rand(rng, 400)
    full = x + mid + y
    ix = _index([a, b])
    o = mm.opts(**KW)
    ratios = {}
    for trim in range(0, 48):
        us, _ = xm.map_read(ix, full[:len(full) - trim], o, xm.multi(max_chains=3, supplementary=1, mask_pm=1000))
        if len(us) != 2:
            continue
        h0, h1 = us[0]["hit"], us[1]["hit"]
        ov = max(0, min(h0["qe"], h1["qe"]) - max(h0["qs"], h1["qs"]))
        mn = min(h0["qe"] - h0["qs"], h1["qe"] - h1["qs"])
        ratios[trim] = (ov, mn)
    exact = [(t, ov * 1000 // mn) for t, (ov, mn) in sorted(ratios.items()) if ov and ov * 1000 % mn == 0 and 1 < ov * 1000 // mn <= 1000]
    assert exact, "no trim puts the overlap on a whole per-mille value"
    t0, pm = exact[0]
    above = [t for t, (ov, mn) in sorted(ratios.items()) if ov * 1000 > pm * mn]
    assert above
    t1 = min(above, key=lambda t: abs(t - t0))
    reads = [full[:len(full) - t0], full[:len(full) - t1]]
    return [a, b], reads, dict(KW), [xm.multi(max_chains=3, supplementary=1, secondary_n=2, mask_pm=pm, pri_pm=0),
                                     xm.multi(max_chains=3, supplementary=1, secondary_n=2, mask_pm=pm - 1, pri_pm=0)]


# ---- 5. the caps: three full copies, a mutated one with few anchors and a high score, a short exact one ------------------------
CAPS_MIN_CNT = 80


def _caps():
    """The mutated copy (a substitution every 18 bases: few, far-apart anchors, each worth up to k) outscores the short exact
    copy (dense anchors, each worth little) but has fewer than min_cnt anchors: it is selected first, dropped, stays marked and
    has used up a selection."""
    rng = np.random.default_rng(205)
    rep = rand(rng, 1000)
    gap = lambda: rand(rng, 300)
    c = gap() + rep + gap() + rep + gap() + rep + gap() + rep[700:1000] + gap() + mutate(rng, rep[:700], 18) + gap()
    reads = [rep, mm.revcomp(rep)]
    o = dict(KW, min_cnt=CAPS_MIN_CNT)
    ms = [xm.multi(max_chains=mc, secondary_n=sn, pri_pm=0) for mc, sn in ((2, 5), (3, 5), (4, 5), (5, 5), (5, 2), (5, 3), (16, 15))]
    return [c], reads, o, ms


# ---- 6. anchor counts around the selection kernel's 64-anchor blocks ------------------------------------------------------------
BLOCK_COUNTS = (63, 64, 65, 128, 129)


def _wave_blocks():
    """reads of case 2's contig that start in the unique flank (one anchor a minimizer) and run into the repeat (two), cut so
    that their anchors number exactly 63 .. 129; then a read with fewer than min_cnt anchors and one with none"""
    rng = np.random.default_rng(202)
    c, r0, _ = _two_copy_contig(rng)
    ix = _index([c])
    o = mm.opts(**KW)
    reads = []
    for want in BLOCK_COUNTS:
        found = None
        for lead in (20, 21, 22, 23, 30, 40, 55, 70):
            for n in range(60, 400):
                rd = c[r0 - lead:r0 - lead + n]
                cnt = len(mm.anchors(ix, rd, o)[2])
                if cnt == want:
                    found = rd
                if cnt >= want:
                    break
            if found:
                break
        assert found is not None, want
        reads.append(found)
    few = [c[r0 + 200:r0 + 200 + n] for n in range(15, 40)]
    few = [rd for rd in few if 1 <= len(mm.anchors(ix, rd, o)[2]) < mm.DEFAULTS["min_cnt"]]
    reads += [few[0], rand(rng, 300)]
    return [c], reads, dict(KW), [xm.multi(max_chains=4, secondary_n=3, pri_pm=0), xm.multi(max_chains=4, supplementary=1, secondary_n=3, pri_pm=0,
                                                                                       mask_pm=1000)]


# ---- 7. f is not monotone along p: a large diagonal shift inside the chains -----------------------------------------------------
def _non_monotone():
    rng = np.random.default_rng(207)
    x, y = rand(rng, 500), rand(rng, 500)
    a = rand(rng, 300) + x + rand(rng, 480) + y + rand(rng, 300)
    b = rand(rng, 200) + x + rand(rng, 470) + y + rand(rng, 200)
    reads = [x + y, mm.revcomp(x + y), x[200:] + y[:300]]
    return [a, b], reads, dict(KW), [xm.multi(max_chains=6, secondary_n=5, pri_pm=0), xm.multi(max_chains=6, supplementary=1, secondary_n=5)]


CASES = {
    "chimera": _chimera,
    "two_copies": _two_copies,
    "pri_edge": _pri_edge,
    "mask_edge": _mask_edge,
    "caps": _caps,
    "wave_blocks": _wave_blocks,
    "non_monotone": _non_monotone,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, mi):
    """the model's (units per read, counts, info per read) of a case under its mi-th multi-chain options, computed once"""
    contigs, reads, o, ms = case(name)
    info = []
    units, tot = _units(contigs, reads, ms[mi], o, info)
    return units, tot, info


def all_runs():
    """(name, mi) of every case and options"""
    return [(name, mi) for name in sorted(CASES) for mi in range(len(case(name)[3]))]


def names_of(reads):
    return [f"r{i + 1}" for i in range(len(reads))]


def tnames_of(contigs):
    return [f"ctg{i + 1}" for i in range(len(contigs))]


# ---- 8. a further unit that overflows the aligner: the second copy has 40 bases replaced by 60 others, and max_cells is too small for that core ---
def _overflow():
    rng = np.random.default_rng(208)
    rep = rand(rng, 1200)
    c = rand(rng, 400) + rep + rand(rng, 500) + rep[:600] + rand(rng, 60) + rep[640:] + rand(rng, 400)
    reads = [rep[100:1100], mm.revcomp(rep[200:1000]), rep[700:1150]]  # the last lies beyond the replaced block: both units align
    return [c], reads, dict(KW), [xm.multi(max_chains=4, secondary_n=5, pri_pm=0)]


CASES["overflow"] = _overflow
ALIGN_KW = {"overflow": dict(max_cells=1024)}  # aligner options of a case (np2_align_opts_t); the others take the defaults


@functools.lru_cache(maxsize=None)
def aligned(name, mi):
    """the model's (aligned and settled units per read, further units dropped) of a case"""
    contigs, reads, o, ms = case(name)
    return xm.align_units(contigs, reads, expected(name, mi)[0], o["k"], **ALIGN_KW.get(name, {}))
