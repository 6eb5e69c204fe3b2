"""Cases of the mapper's tests (test_map_cpu.py, test_gpu_map.py): small assemblies and reads, each the smallest shape at which
one step of the rule (include/np2_io.h: np2_map_*) can go wrong, and the comparison of an implementation's hits and chains
with the numpy model (map_model.py).  A case is (contigs, reads, options); env: test hooks the device run takes."""
import functools

import numpy as np

import map_model as mm

PAL20 = b"ACGTACGTACGTACGTACGT"  # its own reverse complement: k = 20 meets fw == rv here


def rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)])


def cuts(rng, contigs, n, lo, hi):
    """n reads cut from the contigs, lengths in [lo, hi], either strand"""
    out = []
    for i in range(n):
        c = contigs[i % len(contigs)]
        ln = min(int(rng.integers(lo, hi + 1)), len(c))
        at = int(rng.integers(0, len(c) - ln + 1))
        s = c[at:at + ln]
        out.append(mm.revcomp(s) if rng.integers(0, 2) else s)
    return out


def _read_length():
    rng = np.random.default_rng(101)
    c = rand(rng, 3000)
    k, w = 19, 19
    reads = []
    for at in (0, 700, 2963):  # k + w - 1 bases: one window; k + w - 2: none
        reads += [c[at:at + k + w - 1], c[at:at + k + w - 2], mm.revcomp(c[at:at + k + w - 1])]
    return [c], reads, dict(min_cnt=1, min_score=1)


def _broken_runs():
    rng = np.random.default_rng(102)
    c = bytearray(rand(rng, 6000))
    for at in (500, 1000, 1036, 1500, 1537, 2000, 2038, 2500, 2501, 3000, 3003, 4097, 5999):  # runs of 35, 36 and 37 bases among them
        c[at] = ord("N")
    c[3500:3510] = b"nnnnnNNNNN"
    c[3600:3700] = bytes(c[3600:3700]).lower()
    c = bytes(c)
    return [c], cuts(rng, [c], 24, 200, 1500) + [c[900:1700], c[1400:2600], mm.revcomp(c[1900:3100])], {}


def _strand_edges(k, w):
    rng = np.random.default_rng(103 + k + 7 * w)
    c = rand(rng, 1500) + PAL20 + rand(rng, 700) + PAL20 + PAL20 + rand(rng, 1500)
    c2 = rand(rng, 2500)
    reads = cuts(rng, [c, c2], 14, 150, 1200) + [c[1300:1800], mm.revcomp(c[1400:2400]), c[2100:2400]]
    return [c, c2], reads, dict(k=k, w=w)


def _equal_hashes():
    rng = np.random.default_rng(104)
    c = rand(rng, 1200) + b"AT" * 40 + rand(rng, 800) + b"A" * 60 + rand(rng, 900) + b"ta" * 25 + rand(rng, 500)
    reads = [c[1000:1500], c[1150:1330], mm.revcomp(c[1100:1400]), c[1900:2300], mm.revcomp(c[2000:2200]), c[2080:2140], c[2900:3300],
             c[:], mm.revcomp(c)]
    return [c], reads, dict(min_cnt=1, min_score=1)


def _boundaries():
    rng = np.random.default_rng(105)
    contigs = [rand(rng, 9000), rand(rng, 4200)]  # the first spans three of the sketch kernel's tiles
    reads = cuts(rng, contigs, 10, 2500, 4100) + cuts(rng, contigs, 20, 100, 600)  # 40 kb of reads: tile boundaries fall inside reads
    return contigs, reads, {}


def _occ_cut():
    rng = np.random.default_rng(106)
    u, v = rand(rng, 300), rand(rng, 300)
    c = b"".join(rand(rng, 200) + u for _ in range(5)) + b"".join(rand(rng, 200) + v for _ in range(6)) + rand(rng, 300)
    reads = [u, v, c[150:600], c[2600:3200], mm.revcomp(u), mm.revcomp(c[2700:3300])]
    return [c], reads, dict(max_occ=5)  # u occurs max_occ times: kept; v once more: dropped


def _gap_pair(rng, gap):
    """(contig, read): the read lacks the contig's middle `gap` bases; no k-mer of the read's junction is the contig's"""
    x, z, y = rand(rng, 300), bytearray(rand(rng, gap)), rand(rng, 300)
    other = lambda b: b"ACGT"[(b"ACGT".index(bytes([b])) + 1) % 4]
    z[0], z[-1] = other(y[0]), other(x[-1])
    return x + bytes(z) + y, x + y


def _bandwidth():
    """w = 1: every k-mer is a minimizer, so the anchors on either side of a deletion of G bases are G off the diagonal and
    nothing else: G == bandwidth chains across, G + 1 does not"""
    rng = np.random.default_rng(107)
    (c0, r0), (c1, r1) = _gap_pair(rng, 120), _gap_pair(rng, 121)
    return [c0, c1], [r0, r1, mm.revcomp(r0), mm.revcomp(r1)], dict(k=15, w=1, bandwidth=120, max_gap=5000)


def _max_gap():
    """the same shape: the first anchor after the deletion is dr = G + k from the last before it"""
    rng = np.random.default_rng(108)
    k = 15
    (c0, r0), (c1, r1) = _gap_pair(rng, 400 - k), _gap_pair(rng, 401 - k)
    return [c0, c1], [r0, r1, mm.revcomp(r0), mm.revcomp(r1)], dict(k=k, w=1, bandwidth=1000, max_gap=400)


def _lookback(lb):
    """a tandem repeat: a read's anchors on neighbouring diagonals interleave in r order, so the predecessor on an anchor's own
    diagonal lies several places back"""
    rng = np.random.default_rng(109)
    unit = rand(rng, 40)
    c = rand(rng, 300) + unit * 8 + rand(rng, 300)
    reads = [c[250:700], unit * 3, mm.revcomp(c[200:650]), c[100:500]]
    return [c], reads, dict(k=15, w=5, lookback=lb, min_cnt=1, min_score=1)


def _unmapped():
    rng = np.random.default_rng(110)
    c = rand(rng, 4000)
    reads = [rand(rng, 800), c[100:160], c[1000:1900], b"N" * 100, b"", c[2000:2037], b"ACGT", mm.revcomp(c[3000:3900])]
    return [c], reads, {}


CASES = {
    "read_length": _read_length,
    "broken_runs": _broken_runs,
    "k20_palindrome": lambda: _strand_edges(20, 10),
    "k11": lambda: _strand_edges(11, 5),
    "k28": lambda: _strand_edges(28, 19),
    "w1": lambda: _strand_edges(20, 1),
    "w64": lambda: _strand_edges(19, 64),
    "equal_hashes": _equal_hashes,
    "boundaries": _boundaries,
    "occ_cut": _occ_cut,
    "bandwidth": _bandwidth,
    "max_gap": _max_gap,
    "lookback_2": lambda: _lookback(2),
    "lookback_3": lambda: _lookback(3),
    "lookback_64": lambda: _lookback(64),
    "unmapped": _unmapped,
}
# device runs of a case under test hooks: pieces that end inside reads (and batches of eight of them), and an anchor budget
# that splits a batch into groups of reads
HOOKS = {
    "boundaries": [dict(NP2_MAP_TEST_PIECE="1024"), dict(NP2_MAP_TEST_PIECE="64", NP2_MAP_TEST_BUDGET="600"), dict(NP2_MAP_TEST_BUDGET="1000")],
    "equal_hashes": [dict(NP2_MAP_TEST_PIECE="80")],
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's (hits, chains, totals, info) of a case, computed once"""
    contigs, reads, o = case(name)
    kw = dict(o)
    ix = mm.Index(contigs, kw.pop("k", 19), kw.pop("w", 19))
    info = {}
    hits, chains, tot = mm.map_reads(ix, reads, info=info, **kw)
    return hits, chains, tot, info


def check(got_hits, got_chain, got_off, hits, chains, reads):
    """an implementation's hit array, chain rows and offsets against the model's lists"""
    assert len(got_hits) == len(hits)
    for i, h in enumerate(hits):
        g = got_hits[i]
        assert int(g["qlen"]) == len(reads[i]), i
        if h is None:
            assert int(g["tid"]) == -1, (i, g)
        else:
            assert {f: int(g[f]) for f in mm.HIT_FIELDS} == h, (i, g)
    if got_chain is None:
        return
    want_off = np.concatenate(([0], np.cumsum([len(c) for c in chains]))).astype(np.uint64)
    assert np.array_equal(got_off, want_off)
    want = np.concatenate(chains) if chains else np.zeros((0, 2), np.int64)
    assert np.array_equal(got_chain.astype(np.int64), want.reshape(-1, 2))
