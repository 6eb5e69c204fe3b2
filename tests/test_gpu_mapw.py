"""The weighted mapper on the device (np2_map_index_*_w and every door that takes the index; python -m nextpolish2_amd.map -W /
--rep; cli --from_reads --map_weights) against the numpy model of tests/mapw_model.py and the host twin: hits and exported
primary chains equal, counts equal, PAF and FASTA byte for byte.  The cases are tests/mapw_cases.py's, each the smallest shape
at which the weighted sketch can go wrong: the bitmap's word edges, the sketch kernel's tile edge (3968 owned positions), piece
boundaries inside listed k-mers, and recycled device memory under the bitmap (which is zeroed, never assumed zero)."""
import contextlib
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases as mc
import map_model as mm
import mapw_cases as wc
import mapw_model as wm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import repkmers
from test_map_cpu import ASM, bundle, synthetic
from test_mapw_cpu import BUNDLE_K, BUNDLE_MIN_COUNT, YAKS, weighted_bundle, weights_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT)


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


def device_equals_model(name, host=False):
    c = wc.case(name)
    hits, chains, tot, n_index = wc.expected(name)
    kw = dict(c["o"])
    k, w = kw.pop("k"), kw.pop("w")
    with weights_of(name) as W:
        with np2io.MapIndex(c["contigs"], k=k, w=w, stream=True, weights=W) as ix:
            assert (ix.weights_k, ix.weights_listed) == (k, len(c["L"])) and ix.n_minimizers == n_index
            gh, gc, go = ix.map(c["reads"], chains=True, **kw)
            st = np2io.map_last_stats()
            mc.check(gh, gc, go, hits, chains, c["reads"])
            assert {f: st[f] for f in tot} == tot and st["reads"] == len(c["reads"]) and st["index_minimizers"] == n_index
            assert np.array_equal(ix.map(c["reads"], **kw), gh)  # (without the export)
        if host:
            hh, hc, ho = np2io.map_host(c["contigs"], c["reads"], chains=True, weights=W, **c["o"])
            assert np.array_equal(hh, gh) and np.array_equal(hc, gc) and np.array_equal(ho, go)
    return st


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_edge_case_equals_the_model_and_the_host_twin(name):
    device_equals_model(name, host=True)


@pytest.mark.parametrize("name,hooks", [(n, i) for n in sorted(wc.HOOKS) for i in range(len(wc.HOOKS[n]))])
def test_piece_batch_and_group_boundaries_change_nothing(name, hooks):
    h = wc.HOOKS[name][hooks]
    with env(**h):
        st = device_equals_model(name)
    if "NP2_MAP_TEST_PIECE" in h:
        assert st["pieces"] > len(wc.case(name)["reads"]) // 2
    if "NP2_MAP_TEST_BUDGET" in h:
        assert st["groups"] > 2


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_dirty_memory_changes_nothing(byte):
    """an uncleared bitmap would list everything (0xFF), nothing, or a pattern"""
    with api.alloc_poison(byte):
        for name in ("word_edges_k11", "tile_edges", "one_unlisted_k15_w19"):
            device_equals_model(name)
        with env(NP2_MAP_TEST_PIECE="1024", NP2_MAP_TEST_BUDGET="3000"):
            device_equals_model("tile_edges")


def test_tandem_array_known_answer_on_the_device():
    c = wc.case("tandem")
    with np2io.MapIndex(c["contigs"], k=15, w=19, stream=True) as ix:
        plain = ix.map(c["reads"])
    with weights_of("tandem") as W, np2io.MapIndex(c["contigs"], k=15, w=19, stream=True, weights=W) as ix:
        weighted = ix.map(c["reads"])
    q30 = tuple(int(np.count_nonzero(h["mapq"] >= 30)) for h in (plain, weighted))
    q60 = tuple(int(np.count_nonzero(h["mapq"] == 60)) for h in (plain, weighted))
    assert q30 == wc.TANDEM_MAPQ30 and q30[1] > q30[0] and q60 == wc.TANDEM_MAPQ60
    mc.check(plain, None, None, wc.expected("tandem", False)[0], None, c["reads"])
    mc.check(weighted, None, None, wc.expected("tandem")[0], None, c["reads"])


def test_an_index_with_the_empty_set_is_the_plain_index(tmp_path):
    s = synthetic()
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">r{i}\n{r.decode()}\n" for i, r in enumerate(s.reads)))
    with np2io.MapIndex(s.contigs, stream=True) as ix:
        assert (ix.weights_k, ix.weights_listed) == (0, 0)
        want = ix.map(s.reads, chains=True)
        np2io.map_files(ix, [fa], tmp_path / "plain.paf")
        want_al = ix.align(s.reads)
    with np2io.MapWeights([], k=15) as W, np2io.MapIndex(s.contigs, stream=True, weights=W) as ix:
        assert (ix.weights_k, ix.weights_listed) == (0, 0) and ix.n_minimizers == s.index.n_minimizers
        got = ix.map(s.reads, chains=True)
        np2io.map_files(ix, [fa], tmp_path / "empty.paf")
        got_al = ix.align(s.reads)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a, b) for a, b in zip(got_al, want_al))
    assert (tmp_path / "plain.paf").read_bytes() == (tmp_path / "empty.paf").read_bytes() != b""
    mc.check(got[0], got[1], got[2], s.hits, s.chains, s.reads)


def test_every_door_of_a_weighted_index_sketches_under_the_weights(tmp_path):
    """np2_map_bytes, np2_map_files, np2_map_align_bytes and the file-built index, on the bundle under its own list"""
    b = weighted_bundle()
    fa = tmp_path / "hifi.fa"
    fa.write_text("".join(f">{n}\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    with np2io.MapWeights(b.L, k=BUNDLE_K) as W, np2io.MapIndex(ASM, k=BUNDLE_K, weights=W) as ix:
        assert (ix.weights_k, ix.weights_listed, ix.n_minimizers) == (BUNDLE_K, len(b.L), b.index.n_minimizers)
        gh, gc, go = ix.map(b.reads, chains=True)
        mc.check(gh, gc, go, b.hits, b.chains, b.reads)
        st = np2io.map_files(ix, [fa], tmp_path / "out.paf")
        assert {f: st[f] for f in b.tot} == b.tot
        assert (tmp_path / "out.paf").read_text() == b.paf
        ah, ar, acg, aoff = ix.align(b.reads[:60])
        hh, hr, hcg, hoff = np2io.map_align_host(b.contigs, b.reads[:60], weights=W, k=BUNDLE_K)
    assert np.array_equal(ah, gh[:60]) and np.array_equal(ah, hh) and np.array_equal(ar, hr)
    assert np.array_equal(acg, hcg) and np.array_equal(aoff, hoff)


# ---- the command lines ---------------------------------------------------------------------------------------------------------
def run(module, *args, stdin=subprocess.DEVNULL):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600, stdin=stdin)


@pytest.fixture(scope="module")
def bundle_files(tmp_path_factory):
    """the bundle's reads as gzip FASTA, and the list `repkmers --min_count 1` writes of its assembly"""
    d = tmp_path_factory.mktemp("mapw")
    b = bundle()
    fa = d / "hifi.fa.gz"
    with gzip.open(fa, "wt") as f:
        f.write("".join(f">{n}\n{r.decode()}\n" for n, r in zip(b.names, b.reads)))
    lst = d / "rep_k15.txt"
    r = run("repkmers", ASM, "-k", BUNDLE_K, "--min_count", BUNDLE_MIN_COUNT, "-o", lst)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, fa, lst


def test_map_rep_equals_repkmers_then_map_W(bundle_files):
    d, fa, lst = bundle_files
    b = weighted_bundle()
    assert wm.parse_list(lst.read_bytes()) == (BUNDLE_K, b.L)
    r = run("map", ASM, fa, "-W", lst, "-o", d / "w.paf", "--stats", d / "w.tsv")
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("map", ASM, fa, "--rep", f"min_count={BUNDLE_MIN_COUNT}", "-o", d / "rep.paf", "--stats", d / "rep.tsv")
    assert r.returncode == 0, r.stderr[-3000:]
    assert (d / "w.paf").read_text() == (d / "rep.paf").read_text() == b.paf
    for f in ("w.tsv", "rep.tsv"):
        head, row = (d / f).read_text().splitlines()
        st = dict(zip(head.split("\t"), row.split("\t")))
        assert (st["weights_k"], st["weights_listed"], st["mapped"]) == (str(BUNDLE_K), str(len(b.L)), "574")
    r = run("map", ASM, fa, "--rep", "-o", d / "rep_default.paf", "--stats", d / "d.tsv")  # distinct=0.9998 at k = 15
    assert r.returncode == 0, r.stderr[-3000:]
    head, row = (d / "d.tsv").read_text().splitlines()
    st = dict(zip(head.split("\t"), row.split("\t")))
    with np2io.MapWeights.from_assembly(ASM) as W:
        assert (st["weights_k"], st["weights_listed"]) == (str(W.k), str(W.n_listed))
    r = run("map", ASM, fa, "--stats", d / "plain.tsv", "-o", d / "plain.paf")  # an unweighted run says 0, 0
    assert r.returncode == 0, r.stderr[-3000:]
    head, row = (d / "plain.tsv").read_text().splitlines()
    assert row.split("\t")[-2:] == ["0", "0"] and (d / "plain.paf").read_text() == bundle().paf


def test_map_a_W_piped_into_cli_equals_cli_from_reads_map_weights(bundle_files):
    d, fa, lst = bundle_files
    r = run("map", ASM, fa, "-a", "-W", lst, "-w", "19", "-o", d / "map.sam")
    assert r.returncode == 0, r.stderr[-3000:]
    with open(d / "map.sam", "rb") as f:
        r = run("cli", "-", ASM, *YAKS, "-L", "10000", "-o", d / "piped.fa", stdin=f)
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("cli", "--from_reads", fa, ASM, *YAKS, "-L", "10000", "--map_weights", lst, "-o", d / "reads.fa")
    assert r.returncode == 0, r.stderr[-3000:]
    out = (d / "reads.fa").read_bytes()
    assert out == (d / "piped.fa").read_bytes() and out.count(b">") == 1
    r = run("cli", "--from_reads", fa, ASM, *YAKS, "-L", "10000", "--map_weights", "auto", "-o", d / "auto.fa")
    assert r.returncode == 0, r.stderr[-3000:]
    assert (d / "auto.fa").read_bytes().count(b">") == 1
