"""The mapper on the device (np2_map_index_*, np2_map_bytes, np2_map_files, python -m nextpolish2_amd.map) against the numpy
model of tests/map_model.py: hits and exported primary chains equal, counts equal, PAF byte for byte.  The edge cases are
tests/map_cases.py's (each the smallest shape at which one kernel can go wrong); the sketch kernel's tile is 3968 positions and
its lane stretch 16, so the `boundaries` case puts reads across both, and the test hooks put piece, batch and group boundaries
inside and between reads."""
import contextlib
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases as mc
import map_model as mm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from test_map_cpu import ASM, bundle, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


def device_equals_model(contigs, reads, hits, chains, tot, n_index, **o):
    kw = dict(o)
    with np2io.MapIndex(contigs, k=kw.pop("k", 19), w=kw.pop("w", 19), stream=True) as ix:
        assert ix.n_minimizers == n_index and ix.lens == [len(c) for c in contigs]
        gh, gc, go = ix.map(reads, chains=True, **kw)
        st = np2io.map_last_stats()
        mc.check(gh, gc, go, hits, chains, reads)
        assert {f: st[f] for f in tot} == tot and st["reads"] == len(reads) and st["index_minimizers"] == n_index
        assert np.array_equal(ix.map(reads, **kw), gh)  # (without the export)
    return st


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_edge_case_equals_the_model(name):
    contigs, reads, o = mc.case(name)
    hits, chains, tot, _ = mc.expected(name)
    n_index = mm.Index(contigs, o.get("k", 19), o.get("w", 19)).n_minimizers
    device_equals_model(contigs, reads, hits, chains, tot, n_index, **o)


@pytest.mark.parametrize("name,hooks", [(n, i) for n in sorted(mc.HOOKS) for i in range(len(mc.HOOKS[n]))])
def test_piece_batch_and_group_boundaries_change_nothing(name, hooks):
    contigs, reads, o = mc.case(name)
    hits, chains, tot, _ = mc.expected(name)
    n_index = mm.Index(contigs, o.get("k", 19), o.get("w", 19)).n_minimizers
    h = mc.HOOKS[name][hooks]
    with env(**h):
        st = device_equals_model(contigs, reads, hits, chains, tot, n_index, **o)
    if "NP2_MAP_TEST_PIECE" in h:  # the boundaries were there: pieces inside reads, more than one batch
        assert st["pieces"] > len(reads) // 2
    if "NP2_MAP_TEST_BUDGET" in h:
        assert st["groups"] > 2


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65])
def test_read_counts_around_a_wavefront(n_reads):
    s = synthetic()
    reads = (s.reads * 2)[:n_reads]
    hits, chains = (s.hits * 2)[:n_reads], (s.chains * 2)[:n_reads]
    with np2io.MapIndex(s.contigs, stream=True) as ix:
        gh, gc, go = ix.map(reads, chains=True)
    mc.check(gh, gc, go, hits, chains, reads)


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_dirty_memory_changes_nothing(byte):
    s = synthetic()
    with api.alloc_poison(byte):
        device_equals_model(s.contigs, s.reads, s.hits, s.chains, s.tot, s.index.n_minimizers)
        with env(NP2_MAP_TEST_PIECE="2048", NP2_MAP_TEST_BUDGET="3000"):
            device_equals_model(s.contigs, s.reads, s.hits, s.chains, s.tot, s.index.n_minimizers)


def test_synthetic_known_answer():
    s = synthetic()
    device_equals_model(s.contigs, s.reads, s.hits, s.chains, s.tot, s.index.n_minimizers)


def test_bundle_known_answer_and_files_to_paf(tmp_path):
    b = bundle()
    fa = tmp_path / "hifi.fa"
    fa.write_text("".join(f">{n} some comment\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    fq = tmp_path / "hifi.fq.gz"  # the second half again, as gzip FASTQ: a second reader thread
    with gzip.open(fq, "wt") as f:
        f.write("".join(f"@{n}\n{r.decode()}\n+\n{'I' * len(r)}\n" for n, r in zip(b.names[287:], b.reads[287:])))
    with np2io.MapIndex(ASM) as ix:
        assert ix.n_minimizers == 10008 and ix.names == b.tnames and ix.lens == [100000]
        gh, gc, go = ix.map(b.reads, chains=True)
        mc.check(gh, gc, go, b.hits, b.chains, b.reads)
        assert int(np.count_nonzero(gh["tid"] >= 0)) == 574 and int(np.count_nonzero(gh["mapq"] == 60)) == 125
        st = np2io.map_files(ix, [fa, fq], tmp_path / "out.paf")
        assert (st["reads"], st["mapped"], st["unmapped"]) == (574 + 287, 574 + 287, 0)
        assert st["minimizers"] == b.tot["minimizers"] + sum(len(mm.sketch(r, 19, 19)[0]) for r in b.reads[287:])
        want = b.paf + "".join(b.paf.splitlines(keepends=True)[287:])
        assert (tmp_path / "out.paf").read_text() == want
        with env(NP2_MAP_TEST_PIECE="4096", NP2_MAP_TEST_BUDGET="20000"):  # pieces inside reads, many batches and groups
            st = np2io.map_files(ix, [fa, fq], tmp_path / "small.paf")
        assert st["groups"] > 20 and (tmp_path / "small.paf").read_text() == want


def run_cli(*args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.map"] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600)


def test_command_line_plain_and_gz_read_back_equal(tmp_path):
    b = bundle()
    fa = tmp_path / "hifi.fa.gz"
    with gzip.open(fa, "wt") as f:
        f.write("".join(f">{n}\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    r = run_cli(ASM, fa, "-o", tmp_path / "map.paf", "--stats", tmp_path / "stats.tsv")
    assert r.returncode == 0 and r.stdout == "", r.stderr[-3000:]
    assert (tmp_path / "map.paf").read_text() == b.paf
    head, row = (tmp_path / "stats.tsv").read_text().splitlines()
    assert dict(zip(head.split("\t"), row.split("\t")))["mapped"] == "574"
    r = run_cli(ASM, fa, "-o", tmp_path / "map.paf.gz")
    assert r.returncode == 0, r.stderr[-3000:]
    with gzip.open(tmp_path / "map.paf.gz", "rt") as f:
        assert f.read() == b.paf
    r = run_cli(ASM, fa)  # to standard output
    assert r.returncode == 0 and r.stdout == b.paf
    r = run_cli(ASM, fa, "-k", "29")
    assert r.returncode != 0 and "NP2_E_UNSUPPORTED" in r.stderr and "k" in r.stderr
    r = run_cli(ASM, tmp_path / "missing.fa")
    assert r.returncode != 0 and "cannot open" in r.stderr
