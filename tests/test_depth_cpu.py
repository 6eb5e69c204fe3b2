"""Mapping depth without a device: the per-record core (csrc/np2_depth_core.hpp) as a stand-alone host program under the
address and undefined-behaviour sanitizers, the argument handling of the nextpolish2_amd.lowdepth module, and the numpy
model of tests/depth_model.py pinned to known answers on the reference's test bundle.  tests/test_gpu_depth.py compares the
device against that model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_model as dm
from nextpolish2_amd import lowdepth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUNDLE_BAM = os.path.join(HERE, "golden", "ref_bundle", "hifi.map.sort.bam")
ENV = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))


# ---- 1. the core ----------------------------------------------------------------------------------------------------------------
def test_core_program_under_sanitizers(tmp_path):
    """every op code alone, the admission boundaries (80M20S, 799M201S, 80M20H, 80M21H), I / D / N / P, zero span, the empty
    CIGAR, flag & 4, a serial difference-array model on a hand-written contig, and the double predicate against 5a < 4b"""
    exe = str(tmp_path / "depth_core_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "depth_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stderr == ""  # (a sanitizer report goes there)


def test_double_predicate_equals_the_integer_test_in_numpy():
    """the model's float64 comparison is the same rule: 5a < 4b over operands up to 2^32 - 1, the boundary included"""
    rng = np.random.default_rng(5)
    b = rng.integers(1, 2 ** 32, 400000, dtype=np.int64)
    t = rng.integers(1, (2 ** 32 - 2) // 5, 200000, dtype=np.int64)
    a = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.int64), 4 * b[200000:] // 5 + rng.integers(-1, 2, 200000)])
    a, b = np.concatenate([a, 4 * t - 1, 4 * t, 4 * t + 1]), np.concatenate([b, 5 * t - 1, 5 * t, 5 * t + 1])
    a = np.clip(a, 0, 2 ** 32 - 1)
    d = 5 * a - 4 * b
    assert all(int((d == k).sum()) > 100000 for k in (-1, 0, 1))
    assert np.array_equal(a.astype(np.float64) / b.astype(np.float64) < 0.8, d < 0)


# ---- 2. the module's arguments --------------------------------------------------------------------------------------------------
@pytest.fixture()
def inputs(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">c\nACGT\n")
    return [BUNDLE_BAM, str(fa)]


def test_defaults_and_ignored_thread_option(inputs):
    a = lowdepth.parse_args(inputs)
    assert (a.min_depth, a.min_len, a.min_fra, a.min_mapq, a.exclude_flags, a.out) == (3, 1000, 0.8, 0, 4, None)
    b = lowdepth.parse_args(inputs + ["-t", "48", "-d", "60", "-l", "100", "--exclude_flags", "0x904", "--min_mapq", "20", "--min_fra", "1"])
    c = lowdepth.parse_args(inputs + ["--thread", "1", "-d", "60", "-l", "100", "--exclude_flags", "2308", "--min_mapq", "20", "--min_fra", "1.0"])
    for k in ("min_depth", "min_len", "min_fra", "min_mapq", "exclude_flags", "device", "bed", "low_bed", "bedgraph", "out"):
        assert getattr(b, k) == getattr(c, k), k  # -t changes nothing
    assert (b.min_depth, b.min_len, b.exclude_flags, b.min_mapq, b.min_fra) == (60, 100, 0x904, 20, 1.0)
    assert "ignored" in lowdepth.build_parser().format_help()


def test_argument_errors_stop_before_any_device_use(inputs, tmp_path):
    """run as a child: the process ends in the parser (exit 2, or the overwrite refusal) with the library never loaded —
    this machine has no device, so a call that reached one would fail differently"""
    mod = [sys.executable, "-m", "nextpolish2_amd.lowdepth"]
    for extra in (["--min_fra", "1.5"], ["--min_fra", "-0.1"], ["--min_fra", "nan"], ["-d", "-1"], ["-l", "4294967296"], ["--min_mapq", "256"],
                  ["--exclude_flags", "65536"]):
        r = subprocess.run(mod + inputs + extra, capture_output=True, text=True, timeout=600, env=ENV)
        assert r.returncode == 2 and r.stdout == "" and extra[0] in r.stderr, (extra, r.stderr[-500:])
        with pytest.raises(SystemExit):
            lowdepth.parse_args(inputs + extra)
    r = subprocess.run(mod + [inputs[0], str(tmp_path / "missing.fa")], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 2 and "cannot open" in r.stderr
    out = tmp_path / "there.fa"
    out.write_text("keep me\n")
    r = subprocess.run(mod + inputs + ["-o", str(out)], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode != 0 and "already exists" in r.stderr and r.stdout == ""
    assert out.read_text() == "keep me\n"
    with pytest.raises(SystemExit) as e:
        lowdepth.parse_args(inputs + ["-o", str(out)])
    assert "already exists" in str(e.value)


def test_module_helpers_format_runs():
    runs = np.array([[2, 4], [8, 9]], np.uint32)
    assert lowdepth.low_runs(runs, 12) == [(0, 1), (5, 7), (10, 11)]
    assert lowdepth.low_runs(np.array([[0, 11]]), 12) == [] and lowdepth.low_runs([], 3) == [(0, 2)] and lowdepth.low_runs([], 0) == []
    assert lowdepth.fasta_text("c", b"acgtnACGTNac", runs) == b">c_2_4\nGTN\n>c_8_9\nTN\n"
    assert lowdepth.bed_text("c", runs) == "c\t2\t5\nc\t8\t10\n"
    assert lowdepth.bedgraph_text("c", np.array([0, 0, 3, 3, 3, 1], np.uint32)) == "c\t0\t2\t0\nc\t2\t5\t3\nc\t5\t6\t1\n"
    assert lowdepth.bedgraph_text("c", np.zeros(0, np.uint32)) == ""
    assert lowdepth.rate_text("c", 1, 3) == "output rate in c: 33.333%\n"
    # and they agree with the model's formatters
    d = np.array([5, 5, 0, 7, 7, 7, 0, 0, 1], np.uint32)
    assert lowdepth.bedgraph_text("x", d) == dm.bedgraph_of("x", d)
    assert lowdepth.bed_text("x", lowdepth.low_runs(runs, 12)) == dm.bed_of("x", dm.low_of(runs, 12))
    assert lowdepth.fasta_text("x", b"acgtnACGTNac", runs) == dm.fasta_of("x", b"acgtnACGTNac", runs)


# ---- 3. the model, pinned -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundle():
    refs, per = dm.read_bam(BUNDLE_BAM)
    return refs, per[0]


def test_bundle_bam_as_the_reader_sees_it(bundle):
    refs, (recs, cigar) = bundle
    assert len(refs) == 1 and refs[0][1] == 100000
    assert len(recs) == 574
    first = cigar[recs["cigar_off"].astype(np.int64)] & 15
    last = cigar[(recs["cigar_off"] + recs["n_cigar"] - 1).astype(np.int64)] & 15
    assert int(((first == 4) | (last == 4)).sum()) == 131  # soft-clipped at either end
    ok, _ = dm.counted_mask(recs, cigar)
    assert int(ok.sum()) == 478


def test_model_known_answers_on_the_bundle(bundle):
    _, (recs, cigar) = bundle
    m = dm.model(100000, recs, cigar)
    assert m["stats"]["records_seen"] == 574 and m["stats"]["records_counted"] == 478
    assert m["stats"]["sum_depth"] == 6168697 == int(m["depth"].astype(np.int64).sum())
    assert int(m["depth"].min()) == 17 and m["stats"]["max_depth"] == 80
    assert m["runs"].tolist() == [[0, 99999]] and m["stats"]["runs"] == 1 and m["stats"]["bases_kept"] == 100000  # -d 3 -l 1000
    m = dm.model(100000, recs, cigar, min_depth=60, min_len=1000)
    assert (m["stats"]["runs"], m["stats"]["runs_kept"], m["stats"]["bases_kept"]) == (8, 4, 64096)
    assert m["runs"][:3].tolist() == [[7514, 38258], [46875, 49174], [51414, 78473]]
    m = dm.model(100000, recs, cigar, min_depth=65, min_len=100)
    assert (m["stats"]["runs"], m["stats"]["runs_kept"], m["stats"]["bases_kept"]) == (13, 8, 53899)
    m = dm.model(100000, recs, cigar, min_depth=70, min_len=1)
    assert (m["stats"]["runs"], m["stats"]["runs_kept"], m["stats"]["bases_kept"]) == (44, 44, 29198)
    assert m["stats"]["bases_ok"] == 29198


def test_model_edge_semantics():
    recs, cigar = dm.records([(0, 0, 0, [("M", 5)]), (3, 0, 0, [("M", 2), ("D", 3), ("M", 2)]), (5, 0, 0, [("I", 10)]), (15, 0, 0, [("M", 10)]),
                              (19, 0, 0, [("=", 1)]), (8, 4, 0, [("M", 10)]), (8, 0, 0, []), (8, 0, 0, [("M", 10), ("S", 10)]),
                              (-1, 0, 0, [("M", 10)]), (20, 0, 0, [("M", 10)])])
    m = dm.model(20, recs, cigar, min_depth=1, min_len=5)
    assert m["depth"].tolist() == [1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2]  # (the core program's contig)
    assert m["runs"].tolist() == [[0, 9], [15, 19]] and m["stats"]["records_counted"] == 5  # (the two outside [0, L) are ignored)
    assert dm.model(20, recs, cigar, min_depth=1, min_len=6)["runs"].tolist() == [[0, 9]]
    none = dm.records([])
    assert dm.model(7, *none, min_depth=0, min_len=1)["runs"].tolist() == [[0, 6]]
    assert dm.model(0, *none, min_depth=0, min_len=0)["runs"].tolist() == []
    assert dm.model(7, *none, min_depth=1, min_len=1)["runs"].tolist() == []
