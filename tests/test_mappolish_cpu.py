"""The reads door of the resident SAM without a device (include/np2_io.h: np2_sam_from_reads): the rule's host twin
(np2_align_pack_host, the text the kernels compile too) against the defining sentence, on every edge case of align_cases and
mappolish_cases; the rule's text stand-alone, plain and under the sanitizers; the command line's refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mappolish_cases as pc
from nextpolish2_amd import api
from nextpolish2_amd import io as np2io

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT)


# ---- 1. the host twin holds the defining sentence -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.all_cases()))
def test_host_twin_equals_the_text_door_model(name):
    """io.align_pack_host on the model's records == sam_model's parse of the SAM text align_model writes for the same reads"""
    reads = pc.case(name)[1]
    recs, words, off = pc.align_arrays(name)
    for tie in np2io.SAM_TIES:
        exp = pc.want(name, tie)
        got = np2io.align_pack_host(recs, words, off, reads, tie=tie)
        assert pc.same_arrays(got, exp), (name, tie)
        assert len(got[0]) == exp[4]["kept"] and exp[4]["records"] == len(reads)


def test_the_new_cases_reach_what_they_are_for():
    w = pc.want("seq_offsets", "input")
    assert w[4]["kept"] == 9
    long_ones = [r for r in w[0] if r["l_seq"] == 600]
    assert sorted(int(r["seq_off"]) % 4 for r in long_ones) == [0, 0, 1, 2, 3] and {int(r["flag"]) for r in long_ones} == {0, 16}
    w = pc.want("odd_even_both_strands", "strand")
    assert sorted((int(r["l_seq"]), int(r["flag"])) for r in w[0]) == [(n, f) for n in (599, 600, 601) for f in (0, 16)]
    assert pc.want("iupac_stray", "strand")[4]["kept"] == 2 and pc.want("none_maps", "strand")[4] == dict(
        lines=5, records=2, unmapped=2, kept=0, cigar_words=0, seq_bytes=0)
    # the nibble table sees what the complement left alone: R 5, Y 10, N 15, * 15, = 0, K 12, W 9 (the second read's SEQ is the
    # reverse complement of its bytes: the first read's again)
    seq4 = pc.want("iupac_stray", "input")[3]
    nib = lambda j: int(seq4[j // 2]) >> (0 if j & 1 else 4) & 15
    assert [nib(j) for j in (100, 200, 300, 400, 450, 598, 1)] == [5, 10, 15, 15, 0, 12, 9]
    assert [nib(600 + j) for j in (100, 200, 300, 400, 450, 598, 1)] == [5, 10, 15, 15, 0, 12, 9]
    a, b = pc.want("same_start", "strand"), pc.want("same_start", "input")
    assert [int(r["flag"]) for r in a[0]] == [0, 0, 16, 16] and [int(r["flag"]) for r in b[0]] == [0, 16, 0, 16]
    t = pc.want("two_contigs", "strand")
    assert t[1].tolist() == [0, 0, 1, 1] and [int(r["seq_off"]) for r in t[0]] == [901, 300, 0, 600]


def test_host_twin_refusals():
    recs, words, off = pc.align_arrays("all_equal")
    reads = pc.case("all_equal")[1]
    with pytest.raises(api.Np2Error) as e:
        np2io.align_pack_host(recs, words, off + np.arange(len(off), dtype=np.uint64), reads)
    assert e.value.code == -1 and "cigar_off" in str(e.value)
    with pytest.raises(ValueError):
        np2io.align_pack_host(recs[:-1], words, off, reads)
    with pytest.raises(ValueError):
        np2io.align_pack_host(recs, words, off, reads, tie="name")


# ---- 2. the rule's text stand-alone, plain and under the sanitizers -------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_core_program(flags, tmp_path):
    exe = str(tmp_path / "alnpack_core_test")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "tools", "alnpack_core_test.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), (r.stdout, r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 1000


# ---- 4. the command line's refusals: before any device work ---------------------------------------------------------------------
def run_cli(args, **env):
    return subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli"] + [str(a) for a in args], capture_output=True, text=True,
                          env=dict(ENV, **env), timeout=300, stdin=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mappolish_cli")
    (d / "hifi.fa").write_text(">r0\n" + bytes(pc.ac.cut()).decode() + "\n")
    (d / "asm.fa").write_text(">ctg\n" + pc.CONTIG.decode() + "\n")
    (d / "k21.yak").write_bytes(b"not a dump")  # (a refusal comes before the dumps are looked at)
    return d


@pytest.mark.parametrize("extra, env, message", [
    (["--sorted_bam", "x.bam", "--sorted_bam_full"], {}, "--sorted_bam_full needs the SAM text"),
    (["-S"], {}, "-S needs secondary records"),
    (["--bam_unsorted"], {}, "--bam_unsorted says how a BAM is read"),
    ([], dict(WORLD_SIZE="2", RANK="0"), "--from_reads runs on one rank"),
], ids=["sorted_bam_full", "secondary", "bam_unsorted", "world_size"])
def test_cli_refuses_what_the_reads_door_does_not_do(files, extra, env, message):
    r = run_cli(["--from_reads", files / "hifi.fa", files / "asm.fa", files / "k21.yak", "-o", files / "never.fa"] + extra, **env)
    assert r.returncode != 0 and message in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr[-2000:]
    assert not (files / "never.fa").exists()


def test_cli_refuses_standard_input_as_reads_and_bad_map_opts(files):
    r = run_cli(["--from_reads", "-", files / "asm.fa", files / "k21.yak"])
    assert r.returncode != 0 and "not standard input" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run_cli(["--from_reads", files / "hifi.fa", files / "asm.fa", files / "k21.yak", "--map_opts", "k=19,bandwith=3"])
    assert r.returncode == 2 and "unknown key 'bandwith'" in r.stderr
    r = run_cli(["--from_reads", files / "hifi.fa", files / "asm.fa", files / "k21.yak", "--map_opts", "band=x"])
    assert r.returncode == 2 and "band" in r.stderr
    r = run_cli([files / "hifi.fa", files / "asm.fa", files / "k21.yak", "--more_reads", files / "hifi.fa"])
    assert r.returncode == 2 and "--from_reads" in r.stderr
    assert np2io.map_opts_arg("k=21, band=64,") == dict(k=21, band=64)
