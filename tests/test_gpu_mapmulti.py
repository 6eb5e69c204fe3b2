"""More chains per read on the device (np2_map_bytes_m, np2_map_files_m, np2_map_align_bytes_m, np2_map_align_files_m, python -m
nextpolish2_amd.map [-a] --supp / --secondary) against the host twins and the plain-Python model (tests/mapmulti_model.py): units,
classes, parents and exported chains equal, counts equal, PAF byte for byte; the units aligned: records, CIGARs, MD and cs equal,
SAM text line for line under every output flag, and the two end-to-end runs into the polisher.  The cases are tests/mapmulti_cases.py's: reads of several 64-anchor blocks of the
selection kernel, anchor counts on both sides of a block, the per-mille edges, the caps; the test hooks put piece, batch and
group boundaries inside and between reads, and one run is on recycled non-zero memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

import map_model as mm
import mapmulti_cases as xc
import mapmulti_model as xm
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io
from nextpolish2_amd import map as np2map
from test_gpu_map import ENV, env
from test_map_cpu import ASM, bundle, synthetic
from test_mapmulti_cpu import BUNDLE_STEP, SUPP_SEC, bundle_units, synthetic_units

pytestmark = pytest.mark.gpu


def same_arrays(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def device_equals_host_and_model(contigs, reads, m, units, tot, index=None, **o):
    kw = {f: v for f, v in o.items() if f not in ("k", "w")}
    ix = index or np2io.MapIndex(contigs, k=o.get("k", 19), w=o.get("w", 19), stream=True)
    try:
        got = ix.map(reads, chains=True, multi=m, **kw)
        st = np2io.map_last_multi_stats()
        same_arrays(got, np2io.map_host(contigs, reads, chains=True, multi=m, k=ix.k, w=ix.w, **kw))  # array for array
        xm.check(got, units, reads)
        assert {f: st[f] for f in tot} == tot and st["units"] == sum(len(us) for us in units)
        assert (st["more_ms"] > 0) == (m["max_chains"] > 1)
        same_arrays(ix.map(reads, multi=m, **kw), got[:4])  # (without the export)
    finally:
        if index is None:
            ix.close()
    return st


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_case_equals_the_host_twin_and_the_model(name):
    contigs, reads, o, ms = xc.case(name)
    with np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True) as ix:
        for mi, m in enumerate(ms):
            units, tot, _ = xc.expected(name, mi)
            device_equals_host_and_model(contigs, reads, m, units, tot, index=ix, **o)


def test_generator_and_bundle_with_supp_and_five_secondaries():
    s, b = synthetic(), bundle()
    device_equals_host_and_model(s.contigs, s.reads, SUPP_SEC, *synthetic_units())
    device_equals_host_and_model(b.contigs, b.reads[::BUNDLE_STEP], SUPP_SEC, *bundle_units())
    with np2io.MapIndex(ASM) as ix:  # all 574 reads: the device against the host twin, array for array
        got = ix.map(b.reads, chains=True, multi=SUPP_SEC)
        st = np2io.map_last_multi_stats()
    same_arrays(got, np2io.map_host(b.contigs, b.reads, chains=True, multi=SUPP_SEC))
    host = np2io.map_last_multi_stats()
    assert {f: st[f] for f in st if f != "more_ms"} == {f: host[f] for f in host if f != "more_ms"} and st["units"] >= 574
    assert got[1][got[0][:-1].astype(np.int64)].tobytes() == ix_plain_hits(b).tobytes()  # every primary is the plain door's hit


def ix_plain_hits(b):
    with np2io.MapIndex(ASM) as ix:
        return ix.map(b.reads)


# an anchor budget just above each case's largest read: groups of one or two reads
BUDGETS = dict(two_copies=800, caps=1200, wave_blocks=140)


@pytest.mark.parametrize("budget,piece", [(True, None), (False, "256"), (True, "64")], ids=["groups", "pieces", "both"])
def test_group_and_piece_boundaries_change_nothing(budget, piece):
    for name in ("two_copies", "caps", "wave_blocks"):
        contigs, reads, o, ms = xc.case(name)
        units, tot, _ = xc.expected(name, 0)
        hooks = {}
        if budget:
            hooks["NP2_MAP_TEST_BUDGET"] = BUDGETS[name]
        if piece:
            hooks["NP2_MAP_TEST_PIECE"] = piece
        with env(**hooks):
            device_equals_host_and_model(contigs, reads, ms[0], units, tot, **o)
            st = np2io.map_last_stats()
        if "NP2_MAP_TEST_BUDGET" in hooks:
            assert st["groups"] > 1  # groups split between reads
        if "NP2_MAP_TEST_PIECE" in hooks:
            assert st["pieces"] > len(reads) // 2  # pieces end inside reads
    s = synthetic()
    with env(NP2_MAP_TEST_PIECE="2048", NP2_MAP_TEST_BUDGET="3000"):
        device_equals_host_and_model(s.contigs, s.reads, SUPP_SEC, *synthetic_units())


@pytest.mark.parametrize("byte", [0xFF, 0xA5])
def test_recycled_non_zero_memory_changes_nothing(byte):
    """as tests/test_gpu_dirty_memory.py arranges it: every block the pools hand out is filled, a small input A, a larger
    input B and A again, each against the model; the two A results are identical (the second runs in buffers B dirtied)"""
    from test_gpu_dirty_memory import same
    s = synthetic()
    d0 = api.alloc_poison_stats()[0]
    with api.alloc_poison(byte):
        seen = []
        for name, mi in (("wave_blocks", 0), ("caps", 3), ("wave_blocks", 0)):
            contigs, reads, o, ms = xc.case(name)
            units, tot, _ = xc.expected(name, mi)
            device_equals_host_and_model(contigs, reads, ms[mi], units, tot, **o)
            with np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True) as ix:
                seen.append(ix.map(reads, chains=True, multi=ms[mi], **{f: v for f, v in o.items() if f not in ("k", "w")}))
        assert same(seen[0], seen[2])
        with env(NP2_MAP_TEST_BUDGET="3000"):
            device_equals_host_and_model(s.contigs, s.reads, SUPP_SEC, *synthetic_units())
    assert api.alloc_poison_stats()[0] > d0  # the hook was on: it filled device blocks


def test_options_off_are_the_plain_doors_arrays_and_bytes(tmp_path):
    contigs, reads, o, _ = xc.case("two_copies")
    kw = {f: v for f, v in o.items() if f not in ("k", "w")}
    fa = tmp_path / "reads.fa"
    fa.write_text("".join(f">{n}\n{r.decode()}\n" for n, r in zip(xc.names_of(reads), reads)))
    with np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True, names=xc.tnames_of(contigs)) as ix:
        hits, chain, off = ix.map(reads, chains=True, **kw)
        unit_off, uh, cls, parent, uc, uco = ix.map(reads, chains=True, multi={}, **kw)
        st = np2io.map_last_multi_stats()
        assert np.array_equal(unit_off, np.arange(len(reads) + 1)) and not cls.any() and not parent.any()
        assert uh.tobytes() == hits.tobytes() and np.array_equal(uc, chain) and np.array_equal(uco, off)
        assert st["more_ms"] == 0 and st["selections"] == 0 and st["units"] == len(reads)  # no further kernel was launched
        np2io.map_files(ix, [fa], tmp_path / "plain.paf", **kw)
        np2io.map_files(ix, [fa], tmp_path / "off.paf", multi={}, **kw)
        assert (tmp_path / "off.paf").read_bytes() == (tmp_path / "plain.paf").read_bytes()
        # options on: every read's primary line is the options-off line, the others follow it in selection order
        np2io.map_files(ix, [fa], tmp_path / "on.paf", multi=xc.case("two_copies")[3][0], **kw)
    units = xc.expected("two_copies", 0)[0]
    want = xm.paf(xc.names_of(reads), units, xc.tnames_of(contigs), [len(c) for c in contigs])
    on = (tmp_path / "on.paf").read_text()
    assert on == want
    assert [ln for ln in on.splitlines(keepends=True) if "tp:A:P" in ln] == (tmp_path / "plain.paf").read_text().splitlines(keepends=True)


def run_cli(*args):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.map"] + [str(a) for a in args], capture_output=True, text=True, env=ENV,
                          timeout=600)


def test_command_line_supp_and_secondary_to_paf(tmp_path):
    b = bundle()
    units, tot = bundle_units()
    fa = tmp_path / "hifi.fa"
    names, reads = b.names[::BUNDLE_STEP], b.reads[::BUNDLE_STEP]
    fa.write_text("".join(f">{n}\n{r.decode()}\n" for n, r in zip(names, reads)))
    want = xm.paf(names, units, b.tnames, [len(c) for c in b.contigs])
    r = run_cli(ASM, fa, "--supp", "--secondary", "5", "-o", tmp_path / "map.paf", "--stats", tmp_path / "stats.tsv")
    assert r.returncode == 0 and r.stdout == "", r.stderr[-3000:]
    assert (tmp_path / "map.paf").read_text() == want
    rows = (tmp_path / "stats.tsv").read_text().splitlines()
    assert rows[2].split("\t") == list(np2map.MULTI_STATS_HEADER)
    st = dict(zip(rows[2].split("\t"), rows[3].split("\t")))
    assert {f: int(st[f]) for f in tot} == tot and int(st["units"]) == sum(len(us) for us in units)
    with env(NP2_MAP_TEST_PIECE="4096", NP2_MAP_TEST_BUDGET="5000"):  # pieces inside reads, many batches and groups
        with np2io.MapIndex(ASM) as ix:
            st = np2io.map_files(ix, [fa], tmp_path / "small.paf", multi=SUPP_SEC)
    assert st["groups"] > 20 and (tmp_path / "small.paf").read_text() == want
    # the defaults are the parent's bytes
    r = run_cli(ASM, fa, "-o", tmp_path / "plain.paf")
    assert r.returncode == 0 and (tmp_path / "plain.paf").read_text() == "".join(b.paf.splitlines(keepends=True)[::BUNDLE_STEP])
    r = run_cli(ASM, fa, "-a", "--supp", "--secondary", "5", "--stats", tmp_path / "a.tsv")  # the same units as SAM records
    body = [ln.split("\t") for ln in r.stdout.splitlines() if ln[0] != "@"]
    assert r.returncode == 0 and sum(not int(f[1]) & (2048 | 256) for f in body) == len(reads) and len(body) == sum(len(us) for us in units)
    assert (tmp_path / "a.tsv").read_text().splitlines()[-2].split("\t") == list(np2map.MULTI_STATS_HEADER)
    r = run_cli(ASM, fa, "--supp", "--max_chains", "17")
    assert r.returncode != 0 and "NP2_E_ARG" in r.stderr and "max_chains" in r.stderr


# ---- the units aligned: records, CIGARs, MD, cs and the SAM text ---------------------------------------------------------------------
ALL = dict(md=True, cs=True, eqx=True)


def aligned_equals_host_and_model(name, mi, index=None, **flags):
    contigs, reads, o, ms = xc.case(name)
    kw = {f: v for f, v in o.items() if f not in ("k", "w")}
    akw = xc.ALIGN_KW.get(name, {})
    aligned, dropped = xc.aligned(name, mi)
    ix = index or np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True, names=xc.tnames_of(contigs))
    try:
        got = np2io.map_align_reads_m(ix, reads, ms[mi], **flags, **kw, **akw)
        st = np2io.map_last_multi_stats()
        got["map_stats"] = np2io.map_last_stats()  # (the device call's: the host twin below has its own)
        twin = np2io.map_align_host_m(contigs, reads, ms[mi], **flags, **akw, **o)
        for key in ("unit_off", "hits", "cls", "parent", "recs", "cigar", "cigar_off"):
            assert got[key].tobytes() == twin[key].tobytes(), key  # array for array
        assert got["md"] == twin["md"] and got["cs"] == twin["cs"]
        xm.check_aligned(got, aligned, **flags)
        assert st["overflow_units"] == dropped and st["units"] == sum(len(us) for us in aligned)
    finally:
        if index is None:
            ix.close()
    return got


def arrays_of(got):
    return {key: v for key, v in got.items() if key != "map_stats"}


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_aligned_case_equals_the_host_twin_and_the_model(name):
    contigs, reads, o, ms = xc.case(name)
    with np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True, names=xc.tnames_of(contigs)) as ix:
        for mi in range(len(ms)):
            aligned_equals_host_and_model(name, mi, index=ix)
            aligned_equals_host_and_model(name, mi, index=ix, **ALL)


@pytest.mark.parametrize("hooks", [dict(NP2_MAP_TEST_BUDGET="1200", NP2_ALIGN_TEST_BUDGET="2048"), dict(NP2_MAP_TEST_PIECE="64"),
                                   dict(NP2_MAP_TEST_PIECE="256", NP2_MAP_TEST_BUDGET="1200", NP2_ALIGN_TEST_BUDGET="1")], ids=["groups", "pieces", "both"])
def test_aligned_group_subgroup_and_piece_boundaries_change_nothing(hooks):
    for name, mi in (("chimera", 0), ("caps", 3), ("overflow", 0), ("non_monotone", 0)):
        with env(**hooks):
            st = aligned_equals_host_and_model(name, mi, **ALL)["map_stats"]
        if "NP2_MAP_TEST_BUDGET" in hooks:
            assert st["groups"] > 1  # groups between reads, sub-groups of the aligner between units
        if "NP2_MAP_TEST_PIECE" in hooks:
            assert st["pieces"] > 2


def test_aligned_on_recycled_non_zero_memory():
    from test_gpu_dirty_memory import same
    with api.alloc_poison(0xFF):
        seen = [arrays_of(aligned_equals_host_and_model(name, mi, **ALL)) for name, mi in (("overflow", 0), ("caps", 3), ("overflow", 0))]
        assert same(seen[0], seen[2])


def test_aligned_bundle_with_supp_and_five_secondaries():
    b = bundle()
    with np2io.MapIndex(ASM) as ix:
        got = np2io.map_align_reads_m(ix, b.reads, SUPP_SEC, **ALL)
        st = np2io.map_last_multi_stats()
        plain = ix.align_x(b.reads, **ALL)
    twin = np2io.map_align_host_m(b.contigs, b.reads, SUPP_SEC, **ALL)
    for key in ("unit_off", "hits", "cls", "parent", "recs", "cigar", "cigar_off"):
        assert got[key].tobytes() == twin[key].tobytes(), key
    assert got["md"] == twin["md"] and got["cs"] == twin["cs"] and st["units"] >= 574
    first = got["unit_off"][:-1].astype(np.int64)  # every primary is the plain door's record
    assert got["recs"][first].tobytes() == plain[1].tobytes() and [got["md"][i] for i in first] == plain[4]


def reads_file(path, names, reads, qual=False):
    path.write_text("".join(f"@{n}\n{r.decode()}\n+\n{'I' * (len(r) - 1)}5\n" if qual else f">{n}\n{r.decode()}\n" for n, r in zip(names, reads)))
    return path


OUT_FLAGS = [dict(qual=q, md=m, cs=c, eqx=e) for q in (False, True) for m in (False, True) for c in (False, True) for e in (False, True)]


def test_sam_text_options_off_and_on_under_every_out_flags_combination(tmp_path):
    contigs, reads, o, ms = xc.case("chimera")
    kw = {f: v for f, v in o.items() if f not in ("k", "w")}
    names, tn, lens = xc.names_of(reads), xc.tnames_of(contigs), [len(c) for c in contigs]
    fq = reads_file(tmp_path / "r.fq", names, reads, qual=True)
    quals = [b"I" * (len(r) - 1) + b"5" for r in reads]
    aligned, _ = xc.aligned("chimera", 0)
    with np2io.MapIndex(contigs, k=o["k"], w=o["w"], stream=True, names=tn) as ix:
        for flags in OUT_FLAGS:
            np2io.map_align_files(ix, [fq], tmp_path / "plain.sam", **flags, **kw)
            np2io.map_align_files(ix, [fq], tmp_path / "off.sam", multi={}, **flags, **kw)
            plain = (tmp_path / "plain.sam").read_bytes()
            assert (tmp_path / "off.sam").read_bytes() == plain, flags  # options off: the plain door's bytes
            np2io.map_align_files(ix, [fq], tmp_path / "on.sam", multi=ms[0], **flags, **kw)
            on = (tmp_path / "on.sam").read_text()
            tags = {f: v for f, v in flags.items() if f != "qual"}
            assert on == xm.sam(names, reads, quals if flags["qual"] else None, aligned, tn, lens, **tags), flags  # line for line the model's
            # options on: a read's records are adjacent, and its primary line is the options-off line up to an appended SA:Z:
            body = [ln for ln in on.splitlines() if ln[0] != "@"]
            prim = [ln for ln in body if not int(ln.split("\t")[1]) & (2048 | 256)]
            off_lines = [ln for ln in plain.decode().splitlines() if ln[0] != "@"]
            assert [ln.split("\tSA:Z:")[0] for ln in prim] == off_lines and all(ln.split("\t")[-1].startswith("SA:Z:") for ln in body)
            assert [ln.split("\t")[0] for ln in body] == ["r1", "r1", "r2", "r2"]


def run_tool(module, *args, stdin=None):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd." + module] + [str(a) for a in args], capture_output=True, env=ENV, timeout=600,
                          stdin=stdin)


def pileup_reads(pol, rc, ref):
    return len(np2io.export_contig(pol, rc, ref).reads["flags"])


def test_end_to_end_chimeras_with_supp_into_the_polisher(tmp_path):
    """case 1 as a pile of 30 reads over the two contigs: map -a --supp | cli - ... -s -c 100000 through the SAM text door, the
    same SAM through samsort --full and the BAM door: the same FASTA; and with -s the resident pileups hold more records than
    those of the run without --supp"""
    from nextpolish2_amd import Polisher
    from test_oracle import yak_from_seqs
    contigs, _, o, _ = xc.case("chimera")
    a, b = contigs
    reads = [a[600 + 7 * i:1400] + mm.revcomp(b[500:1200 - 5 * i]) for i in range(15)]
    reads += [mm.revcomp(r) for r in reads]
    names = [f"q{i}" for i in range(len(reads))]
    fa = reads_file(tmp_path / "reads.fa", names, reads)
    asm = tmp_path / "asm.fa"
    asm.write_text("".join(f">{n}\n{c.decode()}\n" for n, c in zip(xc.tnames_of(contigs), contigs)))
    for k in (21, 31):
        np2io.write_yak(str(tmp_path / f"k{k}.yak"), yak_from_seqs([c.decode() for c in contigs], k))
    # (-a 500.3: a half of a chimera is under the default half of its read)
    rest = [asm, tmp_path / "k21.yak", tmp_path / "k31.yak", "-L", "1000", "-s", "-c", "100000", "-a", "500.3"]
    mapped = {}
    for key, extra in (("supp", ["--supp"]), ("plain", [])):
        r = run_tool("map", asm, fa, "-a", "-k", o["k"], "-w", o["w"], "-o", tmp_path / f"{key}.sam", *extra)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        mapped[key] = (tmp_path / f"{key}.sam").read_text()
    body = [ln.split("\t") for ln in mapped["supp"].splitlines() if ln[0] != "@"]
    assert len(body) == 60 and sum(int(f[1]) & 2048 > 0 for f in body) == 30 and all(f[-1].startswith("SA:Z:") for f in body)
    feeder = subprocess.Popen([sys.executable, "-c", "import sys; sys.stdout.buffer.write(open(sys.argv[1], 'rb').read())", str(tmp_path / "supp.sam")],
                              stdout=subprocess.PIPE)
    r = run_tool("cli", "-", *rest, stdin=feeder.stdout)
    feeder.stdout.close()
    assert feeder.wait(timeout=60) == 0 and r.returncode == 0, r.stderr.decode()[-3000:]
    want = r.stdout
    assert want.count(b">") == 2
    r = run_tool("samsort", tmp_path / "supp.sam", "--full", "-o", tmp_path / "x.bam")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = run_tool("cli", tmp_path / "x.bam", *rest)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()[-3000:]
    pol = Polisher([])
    fo = np2io.FrontOpts(use_supplementary=True, max_clip_len=100000, min_map_fra=0.3)
    n = {}
    for key in ("supp", "plain"):
        sam = np2io.Sam(pol, [str(tmp_path / f"{key}.sam")])
        n[key] = [pileup_reads(pol, np2io.contig_from_sam(pol, sam, nm, c, fo), np.frombuffer(c, np.uint8)) for nm, c in zip(xc.tnames_of(contigs), contigs)]
        sam.close()
    pol.close()
    # the primaries lie on the first contig either way; the 30 supplementary records are the second contig's pileup
    assert n["supp"][0] == n["plain"][0] and n["supp"][1] - n["plain"][1] == 30 and n["plain"][0] - n["plain"][1] == 30


def test_end_to_end_secondaries_through_samsort_into_the_bam_door(tmp_path):
    """case 2: map -a --secondary 5 --qual -> samsort --full -> cli x.bam -S -q -1 runs, and the BAM front end with -S reads
    exactly the model's number of secondary records more than without it"""
    from nextpolish2_amd import Polisher
    from test_oracle import yak_from_seqs
    contigs, reads, o, ms = xc.case("two_copies")
    names = xc.names_of(reads)
    fq = reads_file(tmp_path / "reads.fq", names, reads, qual=True)
    asm = tmp_path / "asm.fa"
    asm.write_text(f">ctg1\n{contigs[0].decode()}\n")
    for k in (21, 31):
        np2io.write_yak(str(tmp_path / f"k{k}.yak"), yak_from_seqs([contigs[0].decode()], k))
    r = run_tool("map", asm, fq, "-a", "--secondary", "5", "--qual", "-k", o["k"], "-w", o["w"], "-o", tmp_path / "map.sam")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    aligned, _ = xc.aligned("two_copies", 0)
    n_sec = sum(u["cls"] == xm.SECONDARY for us in aligned for u in us)
    body = [ln.split("\t") for ln in (tmp_path / "map.sam").read_text().splitlines() if ln[0] != "@"]
    assert n_sec == 2 and sum(int(f[1]) & 256 > 0 for f in body) == n_sec and all(len(f[10]) == len(f[9]) for f in body)
    r = run_tool("samsort", tmp_path / "map.sam", "--full", "-o", tmp_path / "x.bam")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = run_tool("cli", tmp_path / "x.bam", asm, tmp_path / "k21.yak", tmp_path / "k31.yak", "-L", "1000", "-l", "500", "-S", "-q", "-1")
    assert r.returncode == 0 and r.stdout.count(b">") == 1, r.stderr.decode()[-3000:]
    pol = Polisher([])
    bam = np2io.Bam(str(tmp_path / "x.bam"))
    ref = np.frombuffer(contigs[0], np.uint8)
    n = [pileup_reads(pol, np2io.contig_from_bam(pol, bam, "ctg1", contigs[0], np2io.FrontOpts(min_read_len=500, min_map_qual=-1, use_secondary=s)), ref)
         for s in (True, False)]
    bam.close(), pol.close()
    assert n[0] - n[1] == n_sec and n[1] >= len(reads)
