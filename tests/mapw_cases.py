"""Cases of the weighted mapper's tests (test_mapw_cpu.py, test_gpu_mapw.py): small assemblies, reads and weight sets, each
built to reach one edge of the weighted window order (include/np2_io.h: np2_map_*, "Weights"), with the function that shows
the edge is reached (EDGES; run by test_mapw_cpu.py on the model alone).  A case is a dict: contigs, reads, o (the mapper's
options, k and w among them) and L (the listed canonical indices).  The sketch kernel's tile is 3968 owned positions."""
import functools

import numpy as np

import map_model as mm
import mapw_model as wm
from map_cases import cuts, rand

MAP_TILE = 3968
PAL12 = b"ACGTACGTACGT"  # its own reverse complement


def canon(seq, k):
    """the canonical indices of a sequence's k-mers (those of whole k-mers only), by end position"""
    ok, v, h, _ = wm.kmers_v(seq, k)
    return ok, v, h


def listed_of(contigs, k, min_count):
    """canonical k-mers that occur more than min_count times in the contigs (repkmers' rule with --min_count)"""
    vs = []
    for c in contigs:
        ok, v, _ = canon(c, k)
        vs.append(v[ok])
    u, n = np.unique(np.concatenate(vs), return_counts=True)
    return [int(x) for x in u[n > min_count]]


def windows(seq, k, w, L):
    """every window of the sequence: (start, v[w], h[w], key[w], listed[w]) as arrays over windows; runs without a break only"""
    ok, v, h, _ = wm.kmers_v(seq, k)
    assert ok[k - 1:].all() and not (h == mm._INF).any(), "built for one run of bases without palindromes"
    v, h = v[k - 1:], h[k - 1:]
    listed = np.isin(v, wm.weight_array(L))
    key = wm.key_of(h, listed, k)
    sw = lambda a: np.lib.stride_tricks.sliding_window_view(a, w)
    return sw(v), sw(h), sw(key), sw(listed)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _all_listed(k, w):
    """a tandem array (its unit shorter than w, so a window holds equal k-mers) between random flanks; every k-mer of the array
    and of its junctions is listed: windows of listed k-mers only, decided by key, then (the same k-mer twice) by leftmost"""
    rng = np.random.default_rng(201 + k + w)
    unit = rand(rng, 7 if w > 7 else 3)
    mid = rand(rng, 150)  # a listed random stretch: distinct listed k-mers in one window
    c = rand(rng, 700) + unit * 30 + mid + unit * 12 + rand(rng, 700)
    ok, v, _ = canon(c, k)
    L = sorted({int(x) for x in v[700:700 + len(unit) * 42 + 150 + k]})
    reads = cuts(rng, [c], 8, 300, 900) + [c[600:1300], mm.revcomp(c[650:1250]), c[:]]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w, min_cnt=1, min_score=1), L=L)


def _edge_all_listed(case):
    k, w = case["o"]["k"], case["o"]["w"]
    v, h, key, listed = windows(case["contigs"][0], k, w, case["L"])
    full = listed.all(axis=1)
    assert full.sum() > 100
    kmin = key.min(axis=1)
    at_min = key == kmin[:, None]
    tied_key = full & (at_min.sum(axis=1) > 1)
    # equal (key, h): the leftmost decides (equal keys of different hashes: the key_collapse case)
    h_lo = np.where(at_min, h, mm._INF).min(axis=1)
    assert (tied_key & ((at_min & (h == h_lo[:, None])).sum(axis=1) > 1)).any(), "the same listed k-mer twice in a window"
    assert (full & (at_min.sum(axis=1) == 1)).any(), "distinct listed k-mers: the key alone decides"


def _one_unlisted(k, w):
    """windows whose k-mers are all listed but one, and that one has the window's largest hash: in one window it still wins
    (every listed key passes it), in another it loses (a listed key stays below it), as the integers say"""
    rng = np.random.default_rng(202 + k)
    c = rand(rng, 6000)
    v, h, _, _ = windows(c, k, w, [])
    M = np.uint64((1 << (2 * k)) - 1)
    keys = wm.key_of(h, np.ones_like(h, bool), k)  # were every k-mer listed
    top = h.argmax(axis=1)
    rows = np.arange(len(h))
    keys_others = keys.copy()
    keys_others[rows, top] = M + np.uint64(1)
    wins = np.flatnonzero(keys_others.min(axis=1) > h[rows, top])
    loses = np.flatnonzero(keys_others.min(axis=1) < h[rows, top])
    a = int(wins[0])
    b = int(loses[loses > a + 4 * (w + k)][0])
    L = set()
    for s in (a, b):
        L |= {int(v[s, j]) for j in range(w) if j != top[s]}
    reads = cuts(rng, [c], 6, 400, 1500) + [c[max(0, a - 300):a + 400], mm.revcomp(c[max(0, b - 300):b + 400])]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w), L=sorted(L))


def _edge_one_unlisted(case):
    k, w = case["o"]["k"], case["o"]["w"]
    v, h, key, listed = windows(case["contigs"][0], k, w, case["L"])
    rows = np.arange(len(h))
    one = (~listed).sum(axis=1) == 1
    u = (~listed).argmax(axis=1)
    largest = one & (h.argmax(axis=1) == u) & (w > 1)
    order = (key << np.uint64(2 * k)) | h
    won = largest & (order.argmin(axis=1) == u)
    lost = largest & (order.argmin(axis=1) != u)
    assert won.any() and lost.any(), (int(won.sum()), int(lost.sum()))
    assert (key[won][np.arange(int(won.sum())), u[won]] == h[rows[won], u[won]]).all()


def _key_collapse():
    """k = 11, w = 5: a window of listed k-mers whose y8 is 0, every key == M: h, then leftmost, decide among them.  The window
    is found in a seeded random text and embedded between random flanks"""
    k, w = 11, 5
    rng = np.random.default_rng(203)
    text = rand(rng, 400000)
    v, h, key, _ = windows(text, k, w, [])
    M = np.uint64((1 << (2 * k)) - 1)
    keys = wm.key_of(h, np.ones_like(h, bool), k)
    at = np.flatnonzero((keys == M).all(axis=1))
    assert len(at) >= 2
    pieces = [text[int(s):int(s) + k + w - 1] for s in at[:3]]
    c = rand(rng, 500) + pieces[0] + rand(rng, 400) + pieces[1] + rand(rng, 300) + pieces[-1] + rand(rng, 500)
    L = set()
    for p in pieces:
        ok, pv, _ = canon(p, k)
        L |= {int(x) for x in pv[ok]}
    reads = cuts(rng, [c], 6, 300, 1000) + [c[400:1100], mm.revcomp(c[300:1700])]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w, min_cnt=1, min_score=1), L=sorted(L))


def _edge_key_collapse(case):
    k, w = case["o"]["k"], case["o"]["w"]
    v, h, key, listed = windows(case["contigs"][0], k, w, case["L"])
    M = np.uint64((1 << (2 * k)) - 1)
    tied = listed.all(axis=1) & (key == M).all(axis=1)
    assert tied.sum() >= 2
    assert all(len(set(row.tolist())) == w for row in h[tied]), "equal keys of different hashes: h decides"


def _palindrome():
    """k = 12: a listed palindrome (fw == rv) inside windows of listed and unlisted k-mers: never chosen"""
    k, w = 12, 5
    rng = np.random.default_rng(204)
    c = rand(rng, 800) + PAL12 + rand(rng, 600) + PAL12 * 3 + rand(rng, 800)
    ok, v, h = canon(c, k)
    L = {wm.index_of(PAL12.decode())} | {int(x) for x in v[805:830]}
    reads = cuts(rng, [c], 6, 300, 900) + [c[600:1100], mm.revcomp(c[1200:1700])]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w), L=sorted(L))


def _edge_palindrome(case):
    k = case["o"]["k"]
    c = case["contigs"][0]
    ok, v, h = canon(c, k)
    pal = ok & (h == mm._INF)
    assert pal.sum() >= 4 and wm.index_of(PAL12.decode()) in case["L"] and np.isin(v[pal], wm.weight_array(case["L"])).all()
    hh, pos, _ = wm.sketch(c, k, case["o"]["w"], wm.weight_array(case["L"]))
    assert not pal[pos].any() and (hh != mm._INF).all()
    for kk in (11, 15):  # an odd k has no palindrome: the guard is met at k = 12 only
        assert not (canon(c, kk)[2] == mm._INF).any()


def largest_canonical(k):
    """odd k = 2m + 1: T^m C A^m (its reverse complement T^m G A^m is larger; any larger word's is smaller)"""
    m = k // 2
    return wm.index_of("T" * m + "C" + "A" * m)


def _extremes(k, w):
    """the listed indices 0 (poly-A, met as A.. and as T..) and the largest canonical index"""
    rng = np.random.default_rng(205 + k)
    m = k // 2
    top = b"T" * m + b"C" + b"A" * m
    c = rand(rng, 600) + b"A" * 60 + rand(rng, 500) + top + rand(rng, 400) + b"T" * 50 + rand(rng, 300) + mm.revcomp(top) + rand(rng, 600)
    L = [0, largest_canonical(k)]
    reads = cuts(rng, [c], 6, 300, 900) + [c[500:1300], mm.revcomp(c[1000:2200])]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w, min_cnt=1, min_score=1), L=L)


def _edge_extremes(case):
    k = case["o"]["k"]
    ok, v, _ = canon(case["contigs"][0], k)
    assert (v[ok] == 0).sum() > 60 and (v[ok] == np.uint64(largest_canonical(k))).sum() == 2
    if k == 11:  # by exhaustion: no larger canonical index
        x = np.arange(1 << 22, dtype=np.uint64)
        r = np.zeros_like(x)
        for j in range(k):
            r = (r << np.uint64(2)) | (np.uint64(3) - ((x >> np.uint64(2 * j)) & np.uint64(3)))
        assert int(x[x <= r].max()) == largest_canonical(k)


def _word_edges(k, w):
    """listed indices at the edges of the bitmap's 64-bit words (v & 63 in {0, 63}) and of a 64-word group ((v >> 6) & 63 in
    {0, 63}); their neighbours v +- 1 and v +- 64 are not listed"""
    rng = np.random.default_rng(206 + k)
    # (a canonical index that ends in TTT begins with AAA: v & 63 == 63 is rare in random text, so such k-mers are put in)
    c = b"".join(rand(rng, 500) + b"AAA" + rand(rng, k - 6) + b"TTT" for _ in range(10)) + rand(rng, 300)
    ok, v, _ = canon(c, k)
    vv = v[ok]
    lo, hi = vv & np.uint64(63), (vv >> np.uint64(6)) & np.uint64(63)
    pick = (lo == 0) | (lo == 63) | (hi == 0) | (hi == 63)
    L = sorted({int(x) for x in vv[pick]})
    reads = cuts(rng, [c], 8, 300, 1500)
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w), L=L)


def _edge_word_edges(case):
    L = np.asarray(case["L"], np.uint64)
    for f in (L & np.uint64(63), (L >> np.uint64(6)) & np.uint64(63)):
        assert (f == 0).sum() > 5 and (f == 63).sum() > 5
    assert 100 < len(L) < 1000


def _tile_edges():
    """listed k-mers that end exactly at the owned positions MAP_TILE - 1 and MAP_TILE of a two-tile sequence (the assembly's
    one contig, and the batch's first read), and around the piece boundaries of NP2_MAP_TEST_PIECE = 1024"""
    k, w = 15, 19
    rng = np.random.default_rng(207)
    c = rand(rng, 6500)
    ok, v, _ = canon(c, k)
    ends = list(range(MAP_TILE - 8, MAP_TILE + 8)) + list(range(1016, 1024 + k + 4)) + list(range(2040, 2048 + k + 4))
    L = sorted({int(v[e]) for e in ends})
    reads = [c[:5200], mm.revcomp(c[1000:6500]), c[3000:4500]] + cuts(rng, [c], 5, 300, 1200)
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w), L=L)


def _edge_tile_edges(case):
    k = case["o"]["k"]
    c = case["contigs"][0]
    ok, v, _ = canon(c, k)
    L = wm.weight_array(case["L"])
    assert len(c) > MAP_TILE + 64 and np.isin(v[[MAP_TILE - 1, MAP_TILE]], L).all()
    assert case["reads"][0] == c[:5200]  # the batch's stream begins with it: the same two positions
    assert np.isin(v[1023:1024 + k], L).all()
    # the weights move minimizers there
    plain = set(mm.sketch(c, k, case["o"]["w"])[1].tolist())
    assert plain != set(wm.sketch(c, k, case["o"]["w"], L)[1].tolist())


def _w1():
    """w = 1: every k-mer is its window's minimum, weighted or not"""
    rng = np.random.default_rng(208)
    c = rand(rng, 1500)
    return dict(contigs=[c], reads=cuts(rng, [c], 5, 100, 600), o=dict(k=15, w=1), L=listed_of([c[:700]], 15, 0))


def _edge_w1(case):
    c, o = case["contigs"][0], case["o"]
    a, b = mm.sketch(c, o["k"], 1), wm.sketch(c, o["k"], 1, wm.weight_array(case["L"]))
    assert len(case["L"]) > 600 and all(np.array_equal(x, y) for x, y in zip(a, b))


def _strands():
    """reads and their reverse complements, in a random assembly without a repeated k-mer in any window"""
    k, w = 15, 19
    rng = np.random.default_rng(209)
    c = rand(rng, 5000)
    fw = cuts(rng, [c], 10, 300, 1500)
    ok, v, _ = canon(c, k)
    L = sorted({int(x) for x in v[ok][::3]})  # a third of the assembly's k-mers
    return dict(contigs=[c], reads=fw + [mm.revcomp(r) for r in fw], o=dict(k=k, w=w), L=L)


def _edge_strands(case):
    hits = expected("strands")[0]
    n = len(hits) // 2
    assert n == 10
    for a, b in zip(hits[:n], hits[n:]):
        assert a is not None and b is not None and a["rev"] == 1 - b["rev"]
        flip = dict(b, rev=a["rev"], qs=b["qlen"] - b["qe"], qe=b["qlen"] - b["qs"])
        assert flip == a


# the model's counts for the tandem case below, of its 40 reads, as (unweighted, weighted): reads at mapq >= 30, and at mapq 60
TANDEM_MAPQ30 = (39, 40)
TANDEM_MAPQ60 = (4, 24)


def _tandem():
    """6 kb random + 240 copies of a 171-base monomer (every 4th copy with one substitution) + 6 kb random; 40 reads of 3 kb
    inside the array; the list: canonical 15-mers counted more than 10 times"""
    k, w = 15, 19
    rng = np.random.default_rng(210)
    unit = rand(rng, 171)
    copies = []
    for i in range(240):
        u = bytearray(unit)
        if i % 4 == 3:
            at = int(rng.integers(0, 171))
            u[at] = b"ACGT"[(b"ACGT".index(bytes([u[at]])) + 1 + int(rng.integers(0, 3))) % 4]
        copies.append(bytes(u))
    c = rand(rng, 6000) + b"".join(copies) + rand(rng, 6000)
    origins = [6000 + int(rng.integers(0, 240 * 171 - 3000)) for _ in range(40)]
    reads = [c[a:a + 3000] if i % 2 == 0 else mm.revcomp(c[a:a + 3000]) for i, a in enumerate(origins)]
    return dict(contigs=[c], reads=reads, o=dict(k=k, w=w), L=listed_of([c], k, 10), origins=origins)


def _edge_tandem(case):
    assert 150 <= len(case["L"]) <= 200


CASES = {
    "all_listed_k11_w19": lambda: _all_listed(11, 19),
    "all_listed_k15_w5": lambda: _all_listed(15, 5),
    "one_unlisted_k11_w5": lambda: _one_unlisted(11, 5),
    "one_unlisted_k15_w19": lambda: _one_unlisted(15, 19),
    "key_collapse": _key_collapse,
    "palindrome_k12": _palindrome,
    "extremes_k11": lambda: _extremes(11, 5),
    "extremes_k15": lambda: _extremes(15, 19),
    "word_edges_k11": lambda: _word_edges(11, 5),
    "word_edges_k15": lambda: _word_edges(15, 19),
    "tile_edges": _tile_edges,
    "w1": _w1,
    "strands": _strands,
    "tandem": _tandem,
}
EDGES = {
    "all_listed_k11_w19": _edge_all_listed, "all_listed_k15_w5": _edge_all_listed, "one_unlisted_k11_w5": _edge_one_unlisted,
    "one_unlisted_k15_w19": _edge_one_unlisted, "key_collapse": _edge_key_collapse, "palindrome_k12": _edge_palindrome,
    "extremes_k11": _edge_extremes, "extremes_k15": _edge_extremes, "word_edges_k11": _edge_word_edges,
    "word_edges_k15": _edge_word_edges, "tile_edges": _edge_tile_edges, "w1": _edge_w1, "strands": _edge_strands, "tandem": _edge_tandem,
}
# device runs of a case under test hooks: pieces that end inside reads, and an anchor budget that splits a batch into groups
HOOKS = {
    "tile_edges": [dict(NP2_MAP_TEST_PIECE="1024"), dict(NP2_MAP_TEST_PIECE="64", NP2_MAP_TEST_BUDGET="600")],
    "all_listed_k11_w19": [dict(NP2_MAP_TEST_PIECE="80", NP2_MAP_TEST_BUDGET="2000")],
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, weighted=True):
    """the model's (hits, chains, totals, index minimizers) of a case, computed once; weighted=False: under the empty set"""
    c = case(name)
    kw = dict(c["o"])
    k, w = kw.pop("k"), kw.pop("w")
    L = c["L"] if weighted else []
    ix = wm.Index(c["contigs"], k, w, L)
    hits, chains, tot = wm.map_reads(ix, c["reads"], L, **kw)
    return hits, chains, tot, ix.n_minimizers


def list_text(name, form="fw"):
    """the case's list as a list file's text: every k-mer in its canonical form ("fw"), as the reverse complement ("rc"), or
    both on consecutive lines ("both")"""
    c = case(name)
    k = c["o"]["k"]
    out = []
    for v in c["L"]:
        f, r = wm.text_of(v, k), wm.text_of(wm.revcomp_index(v, k), k)
        out += {"fw": [f], "rc": [r], "both": [f, r]}[form]
    return "".join(x + "\n" for x in out)
