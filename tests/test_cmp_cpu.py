"""K-mer completeness and copy-number spectra, the part that needs no GPU: the numpy brute force every device test is
held to (numpy_cmp), the known answer on the committed fixtures, the host helpers of nextpolish2_amd.completeness, and the
command line's argument checks.

Known answer (numpy_cmp on tests/golden/ref_test_asm.fa.gz as `in` and tests/golden/ref_bundle/expected.fa.gz as `out`
against ref_bundle/k21.yak and k31.yak; the dumps hold no singletons, so min_count 1 and 2 agree):

    k  side min_count  n_read  n_found  completeness  n_asm  n_asm_only  reliable read k-mers by class 0..5
    21 in   1, 2       118978  96089    80.7620       96121  32          22889, 92393, 3629, 38, 28, 1
    21 out  1, 2       118978  96125    80.7922       96125  0           22853, 92429, 3629, 38, 28, 1
    21 in   5          109744  96089    87.5574       96121  32          13655, then as above
    31 in   1, 2       127153  96795    76.1248       96877  82          30358, 93746, 3029, 18, 1, 1
    31 out  1, 2       127153  96871    76.1846       96881  10          30282, 93822, 3029, 18, 1, 1
    31 in   20         114822  96787    84.2931       96877  90          18035, 93738, 3029, 18, 1, 1

At k = 31 with min_count 20 eight assembly k-mers fall under the threshold and move to asm_only: the row that pins the
threshold rule on the probe side."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from nextpolish2_amd import completeness as cmpl
from test_qv_cpu import ASM_IN, BAM, BUNDLE, FASTA, fasta_records, kmer_hashes_at, read_dump, table_counts

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DUMPS = {21: os.path.join(BUNDLE, "k21.yak"), 31: os.path.join(BUNDLE, "k31.yak")}
KNOWN = {  # (k, side, min_count): (n_read, n_found, completeness text, n_asm, n_asm_only, reliable read k-mers by class)
    (21, "in", 1): (118978, 96089, "80.7620", 96121, 32, (22889, 92393, 3629, 38, 28, 1)),
    (21, "in", 2): (118978, 96089, "80.7620", 96121, 32, (22889, 92393, 3629, 38, 28, 1)),
    (21, "out", 1): (118978, 96125, "80.7922", 96125, 0, (22853, 92429, 3629, 38, 28, 1)),
    (21, "out", 2): (118978, 96125, "80.7922", 96125, 0, (22853, 92429, 3629, 38, 28, 1)),
    (21, "in", 5): (109744, 96089, "87.5574", 96121, 32, (13655, 92393, 3629, 38, 28, 1)),
    (31, "in", 1): (127153, 96795, "76.1248", 96877, 82, (30358, 93746, 3029, 18, 1, 1)),
    (31, "in", 2): (127153, 96795, "76.1248", 96877, 82, (30358, 93746, 3029, 18, 1, 1)),
    (31, "out", 1): (127153, 96871, "76.1846", 96881, 10, (30282, 93822, 3029, 18, 1, 1)),
    (31, "out", 2): (127153, 96871, "76.1846", 96881, 10, (30282, 93822, 3029, 18, 1, 1)),
    (31, "in", 20): (114822, 96787, "84.2931", 96877, 90, (18035, 93738, 3029, 18, 1, 1)),
}


# ---- the numpy brute force ---------------------------------------------------------------------------------------------
def numpy_cmp(seqs, k, table, min_count):
    """((n_read, n_found, n_asm, n_asm_only), spectra (6, 1024), asm_only (6,)) of the set `seqs` against the read table
    `table` = (sorted distinct hashes, their counts): np.unique over the set's valid hashes, then searchsorted both ways."""
    th, tc = table
    per = [kmer_hashes_at(s, k) for s in seqs]
    hs = [h[v] for v, h in per]
    ah, an = np.unique(np.concatenate(hs) if hs else np.zeros(0, np.uint64), return_counts=True)
    cn_asm = np.minimum(an, 1023).astype(np.int64)  # cn(x) of the set's distinct k-mers
    # reads -> set: cn of every reliable read k-mer
    rel = np.asarray(tc, dtype=np.int64) >= max(int(min_count), 1)
    rh, rc = np.asarray(th, dtype=np.uint64)[rel], np.asarray(tc, dtype=np.int64)[rel]
    cn = np.zeros(len(rh), np.int64)
    if len(ah) and len(rh):
        at = np.minimum(np.searchsorted(ah, rh), len(ah) - 1)
        cn = np.where(ah[at] == rh, cn_asm[at], 0)
    spectra = np.zeros((6, 1024), np.uint64)
    np.add.at(spectra, (np.minimum(cn, 5), rc), 1)
    # set -> reads: the read count with the threshold applied (np2_qv_*'s rule)
    miss = table_counts((np.asarray(th, dtype=np.uint64), np.asarray(tc)), ah, min_count) == 0
    asm_only = np.bincount(np.minimum(cn_asm[miss], 5), minlength=6).astype(np.uint64)
    stats = (int(len(rh)), int((cn > 0).sum()), int(len(ah)), int(miss.sum()))
    return stats, spectra, asm_only


def check_identities(stats, spectra, asm_only, min_count):
    """what include/np2.h promises about the arrays, whatever the numbers"""
    n_read, n_found, n_asm, n_asm_only = stats
    assert int(spectra.sum()) == n_read and int(spectra[1:].sum()) == n_found
    assert int(spectra[:, :max(int(min_count), 1)].sum()) == 0
    assert int(asm_only.sum()) == n_asm_only and int(asm_only[0]) == 0
    assert n_found <= min(n_read, n_asm) and n_asm_only <= n_asm


@pytest.fixture(scope="module")
def fixtures():
    seqs = {side: [s for _, s in fasta_records(FASTA[side])] for side in ("in", "out")}
    tables = {}
    for k, p in DUMPS.items():
        dk, th, tc = read_dump(p)
        assert dk == k and int(tc.min()) >= 2  # (no singletons: min_count 1 and 2 agree)
        tables[k] = (th, tc)
    return seqs, tables


# ---- 1. the known answer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(KNOWN))
def test_brute_force_reproduces_the_known_answer(fixtures, case):
    k, side, min_count = case
    seqs, tables = fixtures
    stats, spectra, asm_only = numpy_cmp(seqs[side], k, tables[k], min_count)
    n_read, n_found, text, n_asm, n_asm_only, classes = KNOWN[case]
    assert stats == (n_read, n_found, n_asm, n_asm_only)
    assert tuple(int(x) for x in spectra.sum(axis=1)) == classes
    assert cmpl.completeness_text(stats[1], stats[0]) == text
    check_identities(stats, spectra, asm_only, min_count)
    assert int(asm_only[1]) == n_asm_only  # (every k-mer the reads lack is single-copy on these fixtures)


def test_brute_force_on_hand_made_sets():
    k = 3
    # reads' table: AAA x7 (canonical of TTT too), ACG x2 (its own reverse complement is CGT), CCC x1
    from test_kcount_cpu import numpy_count
    from test_qv_cpu import kmer_hashes_at as at
    words, off = numpy_count(b"AAAAAAAAA\nACG\nACG\nCCC\n", k)
    b = np.repeat(np.arange(1024, dtype=np.uint64), np.diff(off.astype(np.int64)))
    h = ((words >> np.uint64(10)) << np.uint64(10)) | b
    order = np.argsort(h)
    table = (h[order], (words & np.uint64(1023)).astype(np.uint32)[order])
    assert sorted(int(c) for c in table[1]) == [1, 2, 7]
    # the set: TTT twice in one sequence and once more in another (cn 3 with AAA), CGT once, GGA (no read has it);
    # "AC" + "G" in two sequences spells no k-mer
    stats, spectra, asm_only = numpy_cmp([b"TTTT", b"AAA", b"CGT", b"GGA", b"AC", b"G", b"", b"NN"], k, table, 1)
    assert stats == (3, 2, 3, 1)
    assert int(spectra[3, 7]) == 1 and int(spectra[1, 2]) == 1 and int(spectra[0, 1]) == 1 and int(spectra.sum()) == 3
    assert [int(x) for x in asm_only] == [0, 1, 0, 0, 0, 0]
    # min_count 2: CCC is no longer reliable; min_count 3: ACG is not either, and the set's CGT becomes asm_only
    assert numpy_cmp([b"TTTT", b"AAA", b"CGT", b"GGA"], k, table, 2)[0] == (2, 2, 3, 1)
    stats, spectra, asm_only = numpy_cmp([b"TTTT", b"AAA", b"CGT", b"GGA"], k, table, 3)
    assert stats == (1, 1, 3, 2) and int(spectra[3, 7]) == 1 and [int(x) for x in asm_only] == [0, 2, 0, 0, 0, 0]
    # nothing in the set: everything is read-only
    stats, spectra, asm_only = numpy_cmp([], k, table, 0)
    assert stats == (3, 0, 0, 0) and int(spectra[0].sum()) == 3
    assert at(b"AC", k)[0].sum() == 0


# ---- 2. host helpers -------------------------------------------------------------------------------------------------------
def test_completeness_value_and_text():
    assert math.isnan(cmpl.completeness_value(0, 0)) and cmpl.completeness_text(0, 0) == "nan"
    assert cmpl.completeness_value(1, 4) == 25.0 and cmpl.completeness_text(1, 4) == "25.0000"
    assert cmpl.completeness_text(96089, 118978) == "80.7620" and cmpl.completeness_text(7, 7) == "100.0000"
    assert cmpl.completeness_text(0, 9) == "0.0000" and cmpl.completeness_text(2, 3) == "66.6667"


def test_spectra_rows_skip_zero_cells_and_name_the_classes():
    sp = np.zeros((6, 1024), np.uint64)
    sp[0, 2], sp[0, 1023], sp[1, 30], sp[2, 61], sp[4, 5], sp[5, 1023] = 11, 1, 900, 40, 2, 3
    ao = np.array([0, 4, 0, 0, 0, 1], np.uint64)
    assert cmpl.spectra_rows(sp, ao) == [("read-only", 2, 11), ("read-only", 1023, 1), ("1", 30, 900), ("2", 61, 40), ("4", 5, 2),
                                         (">4", 1023, 3), ("asm-only:1", 0, 4), ("asm-only:>4", 0, 1)]
    assert cmpl.spectra_rows(np.zeros((6, 1024), np.uint64), np.zeros(6, np.uint64)) == []
    assert cmpl.COPIES == ("read-only", "1", "2", "3", "4", ">4")


def test_report_lines_on_hand_made_numbers():
    rep = cmpl.CmpReport([21, 31], min_count=2, want_spectra=True)
    rep.rows = [("in", 21, (118978, 96089, 96121, 32)), ("in", 31, (0, 0, 5, 5)), ("out", 21, (4, 4, 4, 0))]
    assert rep.lines() == ["set\tk\tread_kmers\tfound\tcompleteness\tasm_kmers\tasm_only\n",
                           "in\t21\t118978\t96089\t80.7620\t96121\t32\n", "in\t31\t0\t0\tnan\t5\t5\n", "out\t21\t4\t4\t100.0000\t4\t0\n"]
    sp = np.zeros((6, 1024), np.uint64)
    sp[1, 9] = 5
    rep.spectra[("in", 21)] = (sp, np.array([0, 0, 2, 0, 0, 0], np.uint64))
    assert rep.spectra_text("in", 21) == "copies\tcount\tkmers\n1\t9\t5\nasm-only:2\t0\t2\n"


# ---- 3. arguments are checked before any device is touched -------------------------------------------------------------
def test_cli_rejects_bad_cmp_arguments_at_argument_parsing(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tsv, out = str(tmp_path / "c.tsv"), str(tmp_path / "o.fa")
    base = [sys.executable, "-m", "nextpolish2_amd.cli", BAM, ASM_IN, DUMPS[21], "-o", out]
    r = subprocess.run(base + ["--cmp", tsv, "--out_pos"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--out_pos" in r.stderr and "--cmp" in r.stderr and r.stdout == ""
    assert not os.path.exists(tsv) and not os.path.exists(out)
    r = subprocess.run(base + ["--cmp_spectra", str(tmp_path / "p")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--cmp_spectra" in r.stderr and "--cmp" in r.stderr.replace("--cmp_spectra", "") and r.stdout == ""
    assert not os.path.exists(out)
    for bad in ("1024", "-1"):
        r = subprocess.run(base + ["--cmp", tsv, "--cmp_min_count", bad], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 2 and "--cmp_min_count" in r.stderr and r.stdout == "" and not os.path.exists(out)


def test_module_wants_dumps_or_reads_not_both_and_not_neither(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    mod = [sys.executable, "-m", "nextpolish2_amd.completeness", ASM_IN]
    r = subprocess.run(mod, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--sr" in r.stderr and r.stdout == ""
    r = subprocess.run(mod + [DUMPS[21], "--sr", ASM_IN], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--sr" in r.stderr and r.stdout == ""
    r = subprocess.run(mod + [DUMPS[21], "--min_count", "1024"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 2 and "--min_count" in r.stderr and r.stdout == ""


def test_abi_declares_the_entry():
    from nextpolish2_amd import api
    assert "np2_cmp_strings" in api.ABI_SYMBOLS and hasattr(api.lib(), "np2_cmp_strings")
