"""The assembly-to-reference caller without a device: the rule (csrc/np2_asmcall_core.hpp) as a stand-alone host program under
the address and undefined-behaviour sanitizers, the host twin np2_asmcall_host held byte for byte to the model of
tests/asmcall_model.py on hand-built and seeded random alignments, its refusals, the ABI, the module's tiling, text and
--known arithmetic, and the known answers end to end through the host mapper (python -m nextpolish2_amd.asmcall --host).
tests/test_gpu_asmcall.py holds the device to the host twin."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import asmcall_model as am
from nextpolish2_amd import api, asmcall

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
EXPECTED = os.path.join(HERE, "golden", "ref_bundle", "expected.fa.gz")
E_ARG, E_UNSUPPORTED = -1, -4
CASES = am.hand_cases()


def test_core_program_under_sanitizers(tmp_path):
    """codes, the owned interval on both strands, admission, keys, footprints, every refusal, hand-written alignments"""
    exe = str(tmp_path / "asmcall_core_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "asmcall_core_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stderr == ""  # (a sanitizer report goes there)


def same(got, m):
    """what a door returned against the model, byte for byte"""
    runs, vars_, st, cov = got
    assert runs.dtype.itemsize == am.RUN_DTYPE.itemsize and vars_.dtype.itemsize == am.VAR_DTYPE.itemsize
    assert runs.tobytes() == m["runs"].tobytes(), (runs, m["runs"])
    assert vars_.tobytes() == m["vars"].tobytes(), (vars_, m["vars"])
    assert np.array_equal(cov, m["cov"])
    assert {k: st[k] for k in am.STAT_KEYS} == m["stats"]


def twin(refs, alignments, **opts):
    """model and np2_asmcall_host on one input: equal byte for byte -> the model"""
    query, alns, cigar = am.pack(alignments)
    m = am.model(refs, query, alns, cigar, **opts)
    got = api.asmcall_host(refs, query, alns, cigar, want_cov=True, **opts)
    same(got, m)
    assert got[2]["kernel_ms"] == 0
    return m


def events(m):
    return [(int(v["tid"]), int(v["pos"]), "SDI"[v["kind"]], int(v["len"]), int(v["q_pos"])) for v in m["vars"]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_equals_model_on_hand_built(case):
    _, refs, alignments, opts = case
    twin(refs, alignments, **opts)


@pytest.mark.parametrize("seed", range(12))
def test_host_twin_equals_model_on_random(seed):
    refs, alignments = am.random_case(seed, n_refs=1 + seed % 3, n_alns=6 + seed, max_ops=30 + 15 * seed)
    m = twin(refs, alignments, min_mapq=5, min_aln=20)
    if seed == 11:
        assert m["stats"]["alns_admitted"] > 3 and len(m["vars"]) > 0 and max(int(a["n_cigar"]) for a in am.pack(alignments)[1]) > 64


def by_name(prefix):
    return [c for c in CASES if c[0].startswith(prefix)]


def test_model_pinned_to_hand_derived_answers():
    """the model itself, against answers worked out by hand from the rule's text"""
    R = CASES[0][1][0]
    # 10M 2D 10M at 20: the D's anchor is SAM column 9 (reference 29); it deletes 30, 31
    for name, refs, alignments, opts in by_name("10M2D10M"):
        m = twin(refs, alignments, **opts)
        own, rev = eval(name.split("own ")[1][:-2]), name.endswith("-")
        s_lo, s_hi = (20 - own[1], 20 - own[0]) if rev else own
        if s_lo <= 9 < s_hi:
            assert events(m) == [(0, 29, "D", 2, 10)]  # (the base after the gap is forward index 10 on both strands: 20 - 10)
            assert m["runs"].tolist() == [(0, 20 + s_lo, 32 + max(0, s_hi - 10))]
        else:
            assert events(m) == []
            assert m["runs"].tolist() == ([(0, 20 + s_lo, 20 + s_hi)] if s_hi <= 10 else [(0, 32 + s_lo - 10, 32 + s_hi - 10)])
    for name, refs, alignments, opts in by_name("10M2I10M"):
        m = twin(refs, alignments, **opts)
        own, rev = eval(name.split("own ")[1][:-2]), name.endswith("-")
        s_lo, s_hi = (22 - own[1], 22 - own[0]) if rev else own
        assert m["stats"]["found_ins"] == (1 if s_lo <= 9 < s_hi else 0)
        # its footprint is 29 and 30: kept only when the column behind it (SAM 12, reference 30) is owned as well
        assert events(m) == ([(0, 29, "I", 2, 10)] if s_lo <= 9 and s_hi > 12 else [])
    # a leading I or D has no anchor; so has one behind a clip; I then D share the anchor, DEL sorts first
    for name, refs, alignments, opts in by_name("leading gaps"):
        m = twin(refs, alignments, **opts)
        assert events(m) == [] and m["runs"].tolist() == [(0, 10, 20), (0, 42, 52), (0, 71, 81)]
    for name, refs, alignments, opts in by_name("gaps sharing an anchor +"):
        m = twin(refs, alignments, **opts)
        assert events(m) == [(0, 19, "D", 3, 12), (0, 19, "I", 2, 10), (0, 69, "D", 1, 11), (0, 69, "I", 1, 10), (0, 69, "I", 2, 11),
                             (0, 109, "D", 2, 10), (0, 109, "I", 3, 10)]
    for name, refs, alignments, opts in by_name("overlap +"):
        m = twin(refs, alignments, **opts)
        assert events(m) == [(0, 10, "S", 1, 10), (0, 120, "S", 1, 80)] and m["runs"].tolist() == [(0, 0, 40), (0, 100, 140)]
        assert m["stats"]["found_snv"] == 6 and m["stats"]["cov2_bases"] == 60
    for name, refs, alignments, opts in by_name("DEL across a coverage change +"):
        m = twin(refs, alignments, **opts)  # footprint 9..12 meets coverage 2 at 11; 109..112 does not (the next starts at 114); INS 209, 210 does
        assert events(m) == [(0, 2, "S", 1, 2), (0, 109, "D", 3, 10)] and m["stats"]["found_del"] == 2 and m["stats"]["found_ins"] == 1
    for name, refs, alignments, opts in by_name("last base +"):
        m = twin(refs, alignments, **opts)
        assert events(m) == [(0, 49, "S", 1, 9), (1, 39, "I", 2, 10), (2, 27, "D", 2, 10)]
        assert m["runs"].tolist() == [(0, 40, 50), (1, 30, 40), (2, 18, 30)]
    for name, refs, alignments, opts in by_name("two references"):
        m = twin(refs, alignments, **opts)
        assert m["runs"].tolist() == [(0, 0, 100), (1, 0, 150)] and [e[:2] for e in events(m)] == [(1, 0), (1, 149)]
    for name, refs, alignments, opts in by_name("N and lower case +"):
        m = twin(refs, alignments, **opts)
        assert events(m) == [(0, 5, "S", 1, 5), (0, 40, "S", 1, 40)]  # (31 is a reference N; the query N at 8 and 12 are no SNV)
    for name, refs, alignments, opts in by_name("admission"):
        m = twin(refs, alignments, **opts)
        st = m["stats"]
        assert (st["alns_seen"], st["alns_unaligned"], st["alns_low_mapq"], st["alns_short"], st["alns_skipped"], st["alns_admitted"]) == (10, 2, 2, 1, 3, 2)
        # (the trailing D's first base after the gap is q_len)
        assert events(m) == [(0, 104, "S", 1, 4), (0, 159, "D", 10, 20)] and m["runs"].tolist() == [(0, 100, 130), (0, 140, 170)]
    for n in (63, 64, 65):
        m = twin([R], [am.aln(R, 0, [("M", 200)], mism=range(0, 200, 2), own=(0, n))], min_aln=1)
        assert len(m["vars"]) == (n + 1) // 2 and m["runs"].tolist() == [(0, 0, n)]


def raw_call(refs, query, alns, cigar, n_refs=None, ref_off=None, opts=(5, 1), nulls=()):
    """np2_asmcall_host with every argument in the caller's hand -> its status"""
    L = api.lib()
    cat = np.frombuffer(b"".join(refs), dtype=np.uint8)
    off = np.array(ref_off if ref_off is not None else np.concatenate(([0], np.cumsum([len(r) for r in refs]))), dtype=np.uint64)
    q = np.frombuffer(bytes(query), dtype=np.uint8)
    o, st = api.np2_asmcall_opts_t(*opts), api.np2_asmcall_stats_t()
    pr, pv, nr, nv = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    args = dict(refs=cat.ctypes.data if len(cat) else None, ref_off=off.ctypes.data, n_refs=len(refs) if n_refs is None else n_refs,
                query=q.ctypes.data if len(q) else None, query_bytes=len(q), alns=alns.ctypes.data if len(alns) else None, n_alns=len(alns),
                cigar=cigar.ctypes.data if len(cigar) else None, n_cigar=len(cigar), opts=C.byref(o), runs=C.byref(pr), n_runs=C.byref(nr),
                vars=C.byref(pv), n_vars=C.byref(nv), cov=None, stats=C.byref(st))
    for k in nulls:
        args[k] = None
    rc = L.np2_asmcall_host(*args.values())
    for p in (pr, pv):
        if p.value:
            L.np2_free(p)
    return rc


def refusal_inputs():
    """[(name, expected status, keyword arguments of raw_call)] shared with the device test"""
    R = b"ACGTTGCAAGGCTTAACCGT" * 3
    good = am.pack([am.aln(R, 5, [("M", 20), ("I", 2), ("M", 20)])])

    def changed(**fields):
        q, a, c = good[0], good[1].copy(), good[2].copy()
        for k, v in fields.items():
            a[k] = v
        return dict(refs=[R], query=q, alns=a, cigar=c)
    out = [("fine", 0, changed()),
           ("tid outside", E_ARG, changed(tid=1)), ("tid negative", E_ARG, changed(tid=-1)), ("beyond the end", E_ARG, changed(pos=21)),
           ("query length", E_ARG, changed(q_len=41, own_hi=41)), ("own_hi beyond", E_ARG, changed(own_hi=43)),
           ("own_lo above own_hi", E_ARG, changed(own_lo=9, own_hi=8)), ("CIGAR outside", E_ARG, changed(cigar_off=1)),
           ("CIGAR far outside", E_ARG, changed(cigar_off=2 ** 40)), ("query outside", E_ARG, changed(q_off=1)),
           ("ref_off not from 0", E_ARG, dict(changed(), ref_off=[1, 60])), ("ref_off descending", E_ARG, dict(changed(), ref_off=[0, 60, 59], n_refs=2)),
           ("too long", E_UNSUPPORTED, dict(changed(), ref_off=[0, 4294901761]))]
    out += [(f"NULL {k}", E_ARG, dict(changed(), nulls=(k,))) for k in ("refs", "ref_off", "query", "alns", "cigar", "opts", "runs", "n_runs", "vars", "n_vars")]
    return out


@pytest.mark.parametrize("case", refusal_inputs(), ids=[c[0] for c in refusal_inputs()])
def test_host_refusals(case):
    _, want, kw = case
    assert raw_call(**kw) == want
    if want:
        assert api.lib().np2_io_last_error()  # (a message is left)
    assert raw_call(**refusal_inputs()[0][2]) == 0  # (and the next call is served)


def test_abi_symbols_and_struct_sizes():
    L = api.lib()
    for s in ("np2_asmcall", "np2_asmcall_host"):
        assert s in api.IO_ABI_SYMBOLS and hasattr(L, s)
    assert C.sizeof(api.np2_asmcall_opts_t) == 8 and C.sizeof(api.np2_asmcall_stats_t) == 184
    assert api.np2_asmcall_stats_t.found.offset == 80 and api.np2_asmcall_stats_t.kernel_ms.offset == 144
    assert (api.ASMALN_DTYPE.itemsize, api.ASMRUN_DTYPE.itemsize, api.ASMVAR_DTYPE.itemsize) == (56, 12, 24)
    assert api.ASMALN_DTYPE == am.ALN_DTYPE and api.ASMVAR_DTYPE == am.VAR_DTYPE and api.ASMRUN_DTYPE == am.RUN_DTYPE
    assert api.ASMALN_DTYPE.fields["cigar_off"][1] == 40 and api.ASMVAR_DTYPE.fields["kind"][1] == 20
    text = open(os.path.join(ROOT, "include", "np2_io.h")).read()
    assert "THE RULE IS THIS PROJECT'S OWN: equality with\n * minimap2, paftools" in text


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_tiling():
    for Lc, seg, ov in [(0, 100, 20), (1, 100, 20), (99, 100, 20), (100, 100, 20), (101, 100, 20), (179, 100, 20), (180, 100, 20), (181, 100, 20),
                        (259, 100, 20), (260, 100, 20), (1000, 100, 20), (100000, 10000, 2000), (100004, 10000, 2000), (60007, 3000, 600), (500, 100, 0)]:
        t = asmcall.tile(Lc, seg, ov)
        step, m = seg - ov, ov // 2
        assert len(t) == (1 if Lc < seg else max(1, (Lc - ov) // step))
        assert t[0][0] == 0 and t[0][2] == 0 and t[-1][1] == Lc and t[-1][3] == Lc
        for i, (s, e, lo, hi) in enumerate(t):
            assert s == i * step and s <= lo <= hi <= e
            assert e == (Lc if i == len(t) - 1 else s + seg)
            if i:
                assert lo == t[i - 1][3] == s + m  # the owned intervals tile the contig
    assert asmcall.tile(100000, 10000, 2000)[1] == (8000, 18000, 9000, 17000) and len(asmcall.tile(100000, 10000, 2000)) == 12


def test_text_by_hand():
    """R and V lines of one event of each kind on each strand, written out by hand"""
    ref = b"ACGTACGTACGTTTGACC"
    sam = b"ACTTAC" + b"ACGT" + b"a" + b"TTGACC"  # 6M 2D 4M 1I 6M: SNV g > t at 2, gt deleted after 5, a inserted after 11
    for rev in (False, True):
        q = am.revcomp(sam) if rev else sam
        query, alns, cigar = am.pack([dict(pos=0, flag=16 if rev else 0, mapq=37, ops=[("M", 6), ("D", 2), ("M", 4), ("I", 1), ("M", 6)], query=q, q_id=1,
                                           q_base=5000)])
        runs, vars_, _, _ = api.asmcall_host([ref], query, alns, cigar, min_aln=1)
        assert asmcall.run_text("chr", runs) == "R\tchr\t0\t18\n"
        s = "-" if rev else "+"
        want = (f"V\tchr\t2\t3\t1\t37\tg\tt\tctgB\t{5014 if rev else 5002}\t{5015 if rev else 5003}\t{s}\n"
                f"V\tchr\t6\t8\t1\t37\tgt\t-\tctgB\t{5011 if rev else 5006}\t{5011 if rev else 5006}\t{s}\n"
                f"V\tchr\t12\t12\t1\t37\t-\ta\tctgB\t{5006 if rev else 5010}\t{5007 if rev else 5011}\t{s}\n")
        assert asmcall.var_text("chr", ref, vars_, alns, query, ["ctgA", "ctgB"]) == want


def test_known_arithmetic(tmp_path):
    vcf = tmp_path / "known.vcf"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\n\nchr1\t3\t.\tA\tC\nchr1\t8\t.\tA\tC\nchr1\t8\t.\tA\tG\nchr3\t12\t.\tA\tAT\n")
    with gzip.open(str(vcf) + ".gz", "wt") as f:
        f.write(vcf.read_text())
    known = asmcall.read_known(str(vcf))
    assert known == {"chr1": {3, 8}, "chr3": {12}} == asmcall.read_known(str(vcf) + ".gz")
    assert asmcall.known_counts(known, "chr1", 1000, [3, 4, 8, 8, 12]) == (3, 2, 1000)
    assert asmcall.known_counts(known, "chr2", 500, [3, 8]) == (0, 0, 0)  # (a reference the set does not name counts nowhere)
    row = lambda **kw: dict(dict.fromkeys(("r_bases", "snv", "del", "ins", "ins_bases", "del_bases", "segments", "unmapped", "not_admitted", "matched",
                                           "errors", "known_bases"), 0), **kw)
    rows = [("chr1", row(r_bases=1000, snv=3, ins=2, ins_bases=5, segments=2, matched=3, errors=2, known_bases=1000)),
            ("chr2", row(r_bases=500, **{"del": 2}, del_bases=4, segments=1, not_admitted=1)), (None, row(segments=1, unmapped=1))]
    text = asmcall.summary_text(rows, known).split("\n")
    assert text[0] == asmcall.SUMMARY_HEADER + asmcall.KNOWN_HEADER
    assert text[1] == "chr1\t1000\t3\t0\t2\t5\t0\t2\t0\t0\t5000.000\t3\t2\t0.200000"
    assert text[2] == "chr2\t500\t0\t2\t0\t0\t4\t1\t0\t1\t4000.000\t0\t0\t0.000000"
    assert text[3] == "total\t1500\t3\t2\t2\t5\t4\t4\t1\t1\t4666.667\t3\t2\t0.200000" and text[4:] == [""]
    assert asmcall.summary_text(rows).split("\n")[3] == "total\t1500\t3\t2\t2\t5\t4\t4\t1\t1\t4666.667"


def test_module_arguments(tmp_path):
    for bad in (["--overlap", "3"], ["--seg", "2000"], ["--overlap", "-2"], ["-q", "256"], ["--map_opts", "k=15"], ["--map_opts", "nonsense=1"],
                ["--min_aln", "-1"]):
        with pytest.raises(SystemExit) as e:
            asmcall.parse_args([ASM, EXPECTED, "-o", str(tmp_path / "o.txt")] + bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        asmcall.parse_args([ASM, str(tmp_path / "missing.fa"), "-o", str(tmp_path / "o.txt")])
    (tmp_path / "there.txt").write_text("x")
    with pytest.raises(SystemExit, match="already exists"):
        asmcall.parse_args([ASM, EXPECTED, "-o", str(tmp_path / "there.txt")])
    a = asmcall.parse_args([ASM, EXPECTED, "-o", str(tmp_path / "o.txt")])
    assert (a.seg, a.overlap, a.min_aln, a.min_mapq, a.host) == (10000, 2000, 5000, 5, False)


# ---- known answers, through the host mapper -------------------------------------------------------------------------------------
def read_fa(path):
    from nextpolish2_amd import io as np2io
    return list(np2io.read_fasta(path))


def lines(text, kind):
    return [l.split("\t") for l in text.split("\n") if l.startswith(kind + "\t")]


def check_bundle(text, rows, st, swapped):
    """the two bundle answers of the issue"""
    assert st["alns_seen"] == st["alns_admitted"] == 12  # (a segment that does not map fails the test)
    name = lines(text, "R")[0][1]
    v = lines(text, "V")
    if not swapped:
        assert lines(text, "R") == [["R", name, "0", "100000"]]
        assert [(l[2], l[3], l[6], l[7]) for l in v] == [(str(p), str(p), "-", b) for p, b in zip((63156, 76368, 79624, 81108), "ttat")]
    else:
        assert lines(text, "R") == [["R", name, "0", "100004"]]
        assert [(l[2], l[3], l[6], l[7]) for l in v] == [(str(p), str(p + 1), b, "-") for p, b in zip((63156, 76369, 79626, 81111), "ttat")]
    assert all(l[4] == "1" and l[11] == "+" for l in v)
    total = [r for n, r in rows if n is not None]
    assert len(total) == 1 and total[0]["segments"] == 12 and total[0]["not_admitted"] == 0


TILINGS = [(10000, 2000), (5000, 1000), (3000, 600)]
SEAMS = [9000, 17000, 4500, 8500, 2700, 5100]  # owned-interval ends of the three tilings


def planted():
    truth, edited, edits = am.plant_edits(20260101, 60000, SEAMS)
    want = [(str(s), str(e), r, a) for _, s, e, r, a in edits]
    return truth, edited, want


def check_planted(text, st, truth_len, want, rev):
    assert lines(text, "R") == [["R", "truth", "0", str(truth_len)]]
    v = lines(text, "V")
    assert [(l[2], l[3], l[6], l[7]) for l in v] == want
    assert all(l[11] == ("-" if rev else "+") for l in v) and st["alns_admitted"] == st["alns_seen"]


@pytest.mark.parametrize("swapped", [False, True])
def test_bundle_known_answer_host(swapped):
    a, b = read_fa(ASM), read_fa(EXPECTED)
    refs, contigs = (b, a) if swapped else (a, b)
    text, rows, st = asmcall.call(refs, contigs, host=True)
    check_bundle(text, rows, st, swapped)


@pytest.mark.parametrize("tiling", TILINGS)
def test_planted_edits_host(tiling):
    truth, edited, want = planted()
    assert len(want) == 49 and sum(w[2] == "-" for w in want) == 16 and sum(w[3] == "-" for w in want) == 16  # (17 SNV, 16 DEL, 16 INS)
    for rev in (False, True):
        q = am.revcomp(edited) if rev else edited
        text, _, st = asmcall.call([("truth", truth)], [("asm", q)], seg=tiling[0], overlap=tiling[1], min_aln=tiling[0] // 2, host=True)
        check_planted(text, st, len(truth), want, rev)


def test_segments_unmapped_and_not_admitted_host():
    """a contig of random bases (its segments do not map) and a 3 kb copy of a piece of the reference (it maps, and is too short
    to be admitted: it covers nothing) beside the real contig: the answer stays, the summary counts them"""
    a, b = read_fa(ASM), read_fa(EXPECTED)
    rng = am.random.Random(5)
    contigs = b + [("noise", am.random_seq(rng, 12000)), ("piece", a[0][1][40000:43000])]
    text, rows, st = asmcall.call(a, contigs, host=True)
    assert lines(text, "R") == [["R", a[0][0], "0", "100000"]] and len(lines(text, "V")) == 4
    assert (st["alns_seen"], st["alns_admitted"], st["alns_unaligned"], st["alns_short"]) == (14, 12, 1, 1) and st["cov2_bases"] == 0
    assert rows[0][1]["segments"] == 13 and rows[0][1]["not_admitted"] == 1 and rows[1][0] is None and rows[1][1]["unmapped"] == 1
    assert asmcall.summary_text(rows).split("\n")[2] == "total\t100000\t0\t0\t4\t4\t0\t14\t1\t1\t40.000"


def test_module_end_to_end_host(tmp_path):
    out, summary = tmp_path / "calls.txt", tmp_path / "s.tsv"
    vcf = tmp_path / "known.vcf"
    name = read_fa(ASM)[0][0]
    vcf.write_text(f"#CHROM\tPOS\n{name}\t63156\n{name}\t5\n")
    assert asmcall.main([ASM, EXPECTED, "-o", str(out), "--summary", str(summary), "--known", str(vcf), "--host"]) == 0
    text = out.read_text()
    assert len(lines(text, "R")) == 1 and len(lines(text, "V")) == 4
    rows = summary.read_text().split("\n")
    assert rows[0] == asmcall.SUMMARY_HEADER + asmcall.KNOWN_HEADER
    assert rows[1] == f"{name}\t100000\t0\t0\t4\t4\t0\t12\t0\t0\t40.000\t1\t3\t0.003000" and rows[2].split("\t")[1:] == rows[1].split("\t")[1:]
