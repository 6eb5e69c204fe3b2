"""Mapping depth on the device (np2_depth_from_records, np2_depth_from_bam, the nextpolish2_amd.lowdepth module) against the
numpy model of tests/depth_model.py, which tests/test_depth_cpu.py pins to known answers.  The scan and the two compactions
work on tiles of 8192 positions (np2::DEPTH_TILE): the lengths below straddle it as well as the 64 lanes of a wavefront and
the 4096 of the older tile scans."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_model as dm
from nextpolish2_amd import Polisher, api
from nextpolish2_amd import io as np2io
from nextpolish2_amd.bamio import write_bam

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE_BAM = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
E_ARG = -1
TILE = 8192
STAT_KEYS = ("records_seen", "records_counted", "sum_depth", "max_depth", "bases_ok", "runs", "runs_kept", "bases_kept")


@pytest.fixture(scope="module")
def pol():
    p = Polisher([])  # (no k-mer table: the depth needs the device only)
    yield p
    p.close()


def check(pol, L, recs, cigar, **opts):
    m = dm.model(L, recs, cigar, **opts)
    runs, st, depth = api.depth_from_records(pol, L, recs, cigar, want_depth=True, **opts)
    assert depth.dtype == np.uint32 and np.array_equal(depth, m["depth"]), (L, opts)
    assert runs.dtype == np.uint32 and runs.shape == m["runs"].shape and np.array_equal(runs, m["runs"]), (L, opts)
    assert {k: st[k] for k in STAT_KEYS} == m["stats"], (L, opts)
    assert st["kernel_ms"] > 0 or L == 0
    return m


def long_cigar(n_ops):
    """n_ops operations M I M D M I ... of 1 to 3 bases: the wavefront's lanes stride over them"""
    return [("MIMD"[k % 4], 1 + k % 3) for k in range(n_ops)]


BOUNDARY = [  # (flag, mapq, CIGAR): the admission cases of tests/tools/depth_core_test.cpp
    (0, 60, [("M", 80), ("S", 20)]), (0, 60, [("M", 799), ("S", 201)]), (0, 60, [("M", 80), ("H", 20)]), (0, 60, [("M", 80), ("H", 21)]),
    (0, 60, [("I", 10)]), (0, 60, [("M", 10), ("I", 3), ("M", 10), ("D", 4), ("N", 5), ("P", 6), ("M", 1)]), (0, 60, [("=", 7), ("X", 1), ("=", 7)]),
    (0, 60, [("S", 10), ("D", 3)]), (0, 60, [("D", 3)]), (0, 60, []), (4, 60, [("M", 30)]), (0x100, 60, [("M", 30)]), (0x800, 60, [("M", 30)]),
    (0x400, 60, [("M", 30)]), (0x200 | 0x10, 60, [("M", 30)]), (0, 0, [("M", 30)]), (0, 19, [("M", 30)]), (0, 20, [("M", 30)]),
    (0, 60, [("H", 5), ("S", 5), ("M", 40), ("S", 5)]), (0, 60, [("H", 5), ("S", 5), ("M", 39), ("S", 5)]),
]


def edge_records(L, seed):
    rng = np.random.default_rng(seed)
    recs = [(0, 0, 60, [("M", min(L, 50))]),                       # starts at 0
            (max(0, L - 37), 0, 60, [("M", L - max(0, L - 37))]),  # ends exactly at L
            (max(0, L - 10), 0, 60, [("M", 100)]),                 # overhangs L: clamped
            (L - 1, 0, 60, [("M", 1)]), (L - 1, 0, 60, [("I", 4)]),
            (-1, 0, 60, [("M", 10)]), (L, 0, 60, [("M", 10)])]     # outside: ignored
    for n_ops in (1, 63, 64, 65, 129, 1000):
        recs.append((int(rng.integers(0, L)), 0, 60, long_cigar(n_ops)))
        recs.append((int(rng.integers(0, L)), 0, 60, long_cigar(n_ops)[::-1]))
    for flag, mapq, ops in BOUNDARY:
        recs.append((int(rng.integers(0, L)), flag, mapq, ops))
        recs.append((0, flag, mapq, ops))
    if L > 100000:  # enough coverage for runs in every block of the scan
        for p in rng.integers(0, L, 4000):
            recs.append((int(p), 0, int(rng.integers(0, 61)), [("M", int(rng.integers(200, 1500)))]))
    return dm.records(recs)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1, TILE - 1, TILE, TILE + 1, 1000003])
def test_records_against_the_model(pol, L):
    recs, cigar = edge_records(L, L)
    m = check(pol, L, recs, cigar, min_depth=1, min_len=1)
    assert m["stats"]["records_counted"] > 20 and m["stats"]["runs"] >= 1
    check(pol, L, recs, cigar, min_depth=2, min_len=3)
    check(pol, L, recs, cigar, min_depth=1, min_len=1, min_mapq=20, exclude_flags=0x904)
    check(pol, L, recs, cigar, min_depth=3, min_len=40, min_aligned_fra=1.0)
    check(pol, L, recs, cigar, min_depth=1, min_len=1, min_aligned_fra=0.0, exclude_flags=0)
    runs, _, depth = api.depth_from_records(pol, L, recs, cigar, min_depth=1, min_len=1)  # the per-base array stays on the device
    assert depth is None and np.array_equal(runs, m["runs"])


def test_run_edges(pol):
    L = 2 * TILE + 100
    one = lambda pos, n: (pos, 0, 60, [("M", n)])
    # runs of 10 and of 9 positions, one touching position 0, one position L - 1, one across the tile boundary
    recs, cigar = dm.records([one(0, 10), one(100, 9), one(200, 10), one(TILE - 5, 10), one(TILE + 20, 9), one(L - 10, 10), one(L - 30, 9)])
    m = check(pol, L, recs, cigar, min_depth=1, min_len=10)
    assert m["runs"].tolist() == [[0, 9], [200, 209], [TILE - 5, TILE + 4], [L - 10, L - 1]] and m["stats"]["runs"] == 7
    assert check(pol, L, recs, cigar, min_depth=1, min_len=9)["stats"]["runs_kept"] == 7
    assert check(pol, L, recs, cigar, min_depth=1, min_len=11)["stats"]["runs_kept"] == 0
    # depth exactly min_depth against min_depth - 1
    recs, cigar = dm.records([one(50, 100)] * 3 + [one(60, 20)] + [one(TILE - 1, 2)] * 4)
    m = check(pol, L, recs, cigar, min_depth=4, min_len=1)
    assert m["runs"].tolist() == [[60, 79], [TILE - 1, TILE]]
    assert check(pol, L, recs, cigar, min_depth=3, min_len=1)["runs"].tolist() == [[50, 149], [TILE - 1, TILE]]
    # a threshold above the maximum gives no run
    m = check(pol, L, recs, cigar, min_depth=5, min_len=1)
    assert len(m["runs"]) == 0 and m["stats"]["bases_ok"] == 0
    # min_depth = 0 without a record: the whole contig; min_len beyond it: nothing
    none = dm.records([])
    for n in (1, 64, TILE, L):
        assert check(pol, n, *none, min_depth=0, min_len=1)["runs"].tolist() == [[0, n - 1]]
        assert check(pol, n, *none, min_depth=0, min_len=n)["runs"].tolist() == [[0, n - 1]]
        assert check(pol, n, *none, min_depth=0, min_len=n + 1)["runs"].tolist() == []
        assert check(pol, n, *none, min_depth=1, min_len=1)["runs"].tolist() == []
    runs, st, depth = api.depth_from_records(pol, 0, *none, min_depth=0, min_len=0, want_depth=True)  # L = 0 gives nothing
    assert len(runs) == 0 and len(depth) == 0 and st["runs"] == 0


def test_alternating_depth_gives_the_most_runs_there_can_be(pol):
    L = 8193
    recs, cigar = dm.records([(p, 0, 60, [("M", 1)]) for p in range(0, L, 2)])
    m = check(pol, L, recs, cigar, min_depth=1, min_len=1)
    assert m["stats"]["runs"] == 4097 == m["stats"]["runs_kept"] and m["runs"][-1].tolist() == [8192, 8192]
    assert check(pol, L, recs, cigar, min_depth=1, min_len=2)["stats"]["runs_kept"] == 0
    # and the other phase: 4096 runs, none at either end
    recs, cigar = dm.records([(p, 0, 60, [("M", 1)]) for p in range(1, L, 2)])
    assert check(pol, L, recs, cigar, min_depth=1, min_len=1)["stats"]["runs"] == 4096


def test_depth_above_65535(pol):
    recs, cigar = dm.records([(20, 0, 60, [("M", 10)])] * 70000)
    m = check(pol, 100, recs, cigar, min_depth=65536, min_len=10)
    assert m["stats"]["max_depth"] == 70000 and m["runs"].tolist() == [[20, 29]] and m["stats"]["sum_depth"] == 700000


def test_random_records(pol):
    rng = np.random.default_rng(20261017)
    L, n = 200003, 20000
    recs = []
    for p in np.sort(rng.integers(-50, L + 50, n)):
        ops = []
        for _ in range(int(rng.integers(0, 12))):
            ops.append(("MIDNSHP=X"[int(rng.integers(0, 9))], int(rng.integers(1, 120))))
        if rng.random() < 0.7:
            ops = [("S", int(rng.integers(1, 40)))] * int(rng.random() < 0.3) + [("M", int(rng.integers(50, 400)))] + ops
        recs.append((int(p), int(rng.choice([0, 0, 0, 16, 4, 0x100, 0x800, 0x400])), int(rng.integers(0, 61)), ops))
    recs, cigar = dm.records(recs)
    seen = set()
    for min_depth, min_len in ((1, 1), (3, 1000), (20, 50), (40, 1), (60, 200), (0, 1)):
        m = check(pol, L, recs, cigar, min_depth=min_depth, min_len=min_len)
        seen.add((m["stats"]["runs"] > 10, m["stats"]["runs_kept"] < m["stats"]["runs"]))
    assert (True, True) in seen  # (the length filter had something to drop)
    check(pol, L, recs, cigar, min_depth=10, min_len=20, min_mapq=30, exclude_flags=0x904, min_aligned_fra=0.5)


# ---- from an indexed BAM, on both fetch paths ---------------------------------------------------------------------------------
BUNDLE_OPTS = ((3, 1000), (60, 1000), (65, 100), (70, 1))
_CHILD = ("import json, sys\n"
          "sys.path.insert(0, %r)\n"
          "import numpy as np\n"
          "from nextpolish2_amd import Polisher, io as np2io\n"
          "pol = Polisher([])\n"
          "bam = np2io.Bam(sys.argv[1])\n"
          "out = []\n"
          "for d, l in json.loads(sys.argv[2]):\n"
          "    runs, st, depth = np2io.depth_from_bam(pol, bam, bam.refs()[0][0], bam.refs()[0][1], min_depth=d, min_len=l, want_depth=True)\n"
          "    out.append(dict(runs=runs.tolist(), stats=st, depth_sum=int(depth.astype(np.int64).sum()), depth_min=int(depth.min()),\n"
          "                    depth_max=int(depth.max())))\n"
          "    np.save(sys.argv[3], depth)\n"
          "print('RESULT ' + json.dumps(out))\n" % ROOT)


@pytest.mark.parametrize("mode", ["gpu", "libdeflate"])
def test_bundle_bam_known_answers_on_both_fetch_paths(tmp_path, mode):
    npy = str(tmp_path / "depth.npy")
    r = subprocess.run([sys.executable, "-c", _CHILD, BUNDLE_BAM, json.dumps(BUNDLE_OPTS), npy], capture_output=True, text=True,
                       env=dict(os.environ, NP2_INFLATE=mode, NP2_IO_PROFILE="1"), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert ("fetch_records_gpu" in r.stderr) == (mode == "gpu"), r.stderr[-2000:]  # (the path asked for really ran)
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    by = {o: x for o, x in zip(BUNDLE_OPTS, res)}
    for x in res:
        assert (x["stats"]["records_seen"], x["stats"]["records_counted"]) == (574, 478)
        assert x["stats"]["sum_depth"] == 6168697 == x["depth_sum"] and (x["depth_min"], x["depth_max"], x["stats"]["max_depth"]) == (17, 80, 80)
    assert by[(3, 1000)]["runs"] == [[0, 99999]]
    x = by[(60, 1000)]
    assert (x["stats"]["runs"], x["stats"]["runs_kept"], x["stats"]["bases_kept"]) == (8, 4, 64096)
    assert x["runs"][:3] == [[7514, 38258], [46875, 49174], [51414, 78473]]
    x = by[(65, 100)]
    assert (x["stats"]["runs"], x["stats"]["runs_kept"], x["stats"]["bases_kept"]) == (13, 8, 53899)
    x = by[(70, 1)]
    assert (x["stats"]["runs"], x["stats"]["runs_kept"], x["stats"]["bases_kept"]) == (44, 44, 29198)
    # and the whole per-base array is the model's
    _, per = dm.read_bam(BUNDLE_BAM)
    assert np.array_equal(np.load(npy), dm.model(100000, *per[0])["depth"])


@pytest.mark.parametrize("mode", ["gpu", "libdeflate"])
def test_three_references_the_middle_one_without_a_record(pol, tmp_path, monkeypatch, mode):
    monkeypatch.setenv("NP2_INFLATE", mode)  # (read at every fetch)
    rng = np.random.default_rng(7)
    refs = [("ctgA", 30011), ("ctgB", 9001), ("ctgC", 20003)]
    records, per = [], {0: [], 2: []}
    for tid in (0, 2):
        L = refs[tid][1]
        for p in np.sort(rng.integers(0, L, 300)):
            n = int(rng.integers(100, 3000))
            s = int(rng.integers(0, 400)) if rng.random() < 0.4 else 0
            ops = ([("S", s)] if s else []) + [("M", n)]
            records.append(dict(tid=tid, pos=int(p), mapq=int(rng.integers(0, 61)), flag=int(rng.choice([0, 16, 0x100, 0x800])), cigar=ops,
                                seq="A" * (n + s)))
            per[tid].append((int(p), records[-1]["flag"], records[-1]["mapq"], ops))
    path = str(tmp_path / "three.bam")
    write_bam(path, refs, records)
    bam = np2io.Bam(path)
    assert bam.refs() == refs
    for opts in (dict(min_depth=1, min_len=1), dict(min_depth=8, min_len=200, min_mapq=10, exclude_flags=0x104)):
        for tid in (0, 2):  # each reference sees its own records only
            runs, st, depth = np2io.depth_from_bam(pol, bam, refs[tid][0], refs[tid][1], want_depth=True, **opts)
            m = dm.model(refs[tid][1], *dm.records(per[tid]), **opts)
            assert np.array_equal(depth, m["depth"]) and np.array_equal(runs, m["runs"]) and {k: st[k] for k in STAT_KEYS} == m["stats"], (tid, opts)
        runs, st, depth = np2io.depth_from_bam(pol, bam, "ctgB", 9001, want_depth=True, **opts)
        assert not depth.any() and len(depth) == 9001 and len(runs) == 0
        assert (st["records_seen"], st["records_counted"], st["sum_depth"], st["runs"]) == (0, 0, 0, 0)
    runs, _, _ = np2io.depth_from_bam(pol, bam, "ctgB", 9001, min_depth=0, min_len=1)
    assert runs.tolist() == [[0, 9000]]
    bam.close()


def test_module_end_to_end_on_the_bundle(tmp_path):
    refs, per = dm.read_bam(BUNDLE_BAM)
    name, L = refs[0]
    rng = np.random.default_rng(3)
    seq = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)[rng.integers(0, 10, L)].tobytes()
    fa = tmp_path / "genome.fa"
    fa.write_bytes(b">" + name.encode() + b" a description\n" + b"\n".join(seq[i:i + 70] for i in range(0, L, 70)) + b"\n")
    paths = {k: str(tmp_path / k) for k in ("bed", "low_bed", "bedgraph")}
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.lowdepth", BUNDLE_BAM, str(fa), "-d", "60", "-t", "8", "--bed", paths["bed"],
                        "--low_bed", paths["low_bed"], "--bedgraph", paths["bedgraph"]], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT),
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    m = dm.model(L, *per[0], min_depth=60, min_len=1000)
    assert len(m["runs"]) == 4
    assert r.stdout == dm.fasta_of(name, seq, m["runs"])
    assert ("output rate in %s: %.3f%%\n" % (name, 100 * 64096 / L)) in r.stderr.decode()
    low = dm.low_of(m["runs"], L)
    assert open(paths["bed"]).read() == dm.bed_of(name, m["runs"])
    assert open(paths["low_bed"]).read() == dm.bed_of(name, low)
    assert open(paths["bedgraph"]).read() == dm.bedgraph_of(name, m["depth"])
    # the kept runs and the low runs tile [0, L)
    both = sorted([tuple(x) for x in m["runs"].tolist()] + [tuple(x) for x in low.tolist()])
    assert both[0][0] == 0 and both[-1][1] == L - 1 and all(a[1] + 1 == b[0] for a, b in zip(both, both[1:]))
    # the bedGraph's lengths times depths sum to sum_depth
    rows = [ln.split("\t") for ln in open(paths["bedgraph"]).read().splitlines()]
    assert sum((int(e) - int(s)) * int(d) for _, s, e, d in rows) == 6168697 and int(rows[-1][2]) == L
    # -o: written there, nothing on standard output; and not overwritten by a second run
    out = tmp_path / "filter.fa"
    cmd = [sys.executable, "-m", "nextpolish2_amd.lowdepth", BUNDLE_BAM, str(fa), "-d", "60", "-o", str(out)]
    r2 = subprocess.run(cmd, capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r2.returncode == 0 and r2.stdout == b"" and out.read_bytes() == r.stdout
    r3 = subprocess.run(cmd, capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    assert r3.returncode != 0 and b"already exists" in r3.stderr and out.read_bytes() == r.stdout


def test_argument_errors_leave_the_context_usable(pol, tmp_path):
    L = api.lib()
    np2io._bind()
    recs, cigar = dm.records([(5, 0, 60, [("M", 10)]), (8, 0, 60, [("M", 10)])])
    bam = np2io.Bam(BUNDLE_BAM)
    bundle_name = bam.refs()[0][0].encode()

    def from_records(fra=0.8, opts=True, starts=True, recs_p=recs.ctypes.data, cigar_p=cigar.ctypes.data):
        o = api.np2_depth_opts_t(1, 1, fra, 4, 0)
        ps, pe, n, st = C.c_void_p(), C.c_void_p(), C.c_uint32(), api.np2_depth_stats_t()
        rc = L.np2_depth_from_records(pol._h, 30, recs_p, len(recs), cigar_p, C.byref(o) if opts else None, C.byref(ps) if starts else None, C.byref(pe),
                                      C.byref(n), None, C.byref(st))
        assert rc != 0 and not ps.value and not pe.value and n.value == 0
        return rc

    def from_bam(fra=0.8, name=bundle_name, bam_h=bam._h):
        o = api.np2_depth_opts_t(1, 1, fra, 4, 0)
        ps, pe, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        rc = L.np2_depth_from_bam(pol._h, bam_h, name, 100000, C.byref(o), C.byref(ps), C.byref(pe), C.byref(n), None, None)
        assert rc != 0 and not ps.value and n.value == 0
        return rc

    cases = [
        (lambda: from_records(fra=1.5), "min_aligned_fra"), (lambda: from_records(fra=-0.001), "min_aligned_fra"),
        (lambda: from_records(fra=float("nan")), "min_aligned_fra"), (lambda: from_records(fra=float("inf")), "min_aligned_fra"),
        (lambda: from_records(opts=False), "opts is NULL"), (lambda: from_records(starts=False), "is NULL"),
        (lambda: from_records(recs_p=None), "recs is NULL"), (lambda: from_records(cigar_p=None), "cigar is NULL"),
        (lambda: from_bam(fra=2.0), "min_aligned_fra"), (lambda: from_bam(fra=float("nan")), "min_aligned_fra"),
        (lambda: from_bam(name=b"no_such_contig"), "contig not in the BAM header"), (lambda: from_bam(bam_h=None), "is NULL"),
    ]
    for fn, text in cases:
        assert fn() == E_ARG
        assert text in L.np2_last_error(pol._h).decode(), text
        runs, st, depth = api.depth_from_records(pol, 30, recs, cigar, min_depth=2, min_len=1, want_depth=True)  # the context still answers
        assert runs.tolist() == [[8, 14]] and st["sum_depth"] == 20 and depth[7:16].tolist() == [1, 2, 2, 2, 2, 2, 2, 2, 1]
    with pytest.raises(api.Np2Error) as e:
        api.depth_from_records(pol, 30, recs, cigar, min_aligned_fra=1.01)
    assert e.value.code == E_ARG and "min_aligned_fra" in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        np2io.depth_from_bam(pol, bam, "no_such_contig", 100)
    assert e.value.code == E_ARG
    o = api.np2_depth_opts_t(1, 1, 0.8, 4, 0)
    assert L.np2_depth_from_records(None, 30, None, 0, None, C.byref(o), None, None, None, None, None) == E_ARG
    assert L.np2_depth_from_bam(None, None, None, 0, None, None, None, None, None, None) == E_ARG
    bam.close()
