"""The BGZF deflater without a device: the host twin (np2_bgzf_deflate_host: csrc/np2_deflate_core.hpp stepped 64 lanes at
a time on the CPU — the statement of what k_bgzf_deflate must produce, tests/test_gpu_deflate.py holds the kernel to it byte
for byte) against zlib over the whole corpus of tests/deflate_cases.py, through the project's own readers, as a stand-alone
program under the address and undefined-behaviour sanitizers, its size against zlib level 1, and the command line's
argument handling."""
import os
import subprocess
import zlib

import pytest

import deflate_cases as dc
from nextpolish2_amd import io as np2io
from nextpolish2_amd import srqc
from nextpolish2_amd.api import Np2Error

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- 1. every field of every stream ---------------------------------------------------------------------------------------------
def test_twin_streams_check_out_against_zlib():
    stored = 0
    for name, b in dc.blocks():
        z = np2io.bgzf_deflate_host(b)
        dc.check_stream(z, b)
        assert np2io.bgzf_deflate_host(b) == z, name  # twice: the same bytes
        if name.startswith("random_") and len(b):
            assert len(z) == 18 + len(b) + 5 + 8 + 28 and z[18] == 1, name  # uniform bytes: a stored block, n + 5
            stored += 1
    assert stored == len(dc.LENGTHS) - 1
    for name, b, bb in dc.streams():
        z = np2io.bgzf_deflate_host(b, bb)
        dc.check_stream(z, b, bb)
        assert np2io.bgzf_deflate_host(b, bb) == z, name
    assert np2io.bgzf_deflate_host(b"") == dc.EOF_BLOCK


def test_matches_are_found_and_far_copies_are_not_used():
    """what the contents were built for, read off the streams' sizes"""
    blocks = dict(dc.blocks())
    size = lambda name: len(np2io.bgzf_deflate_host(blocks[name])) - 28 - 26
    # (a match ends at its 64-byte segment's end: 1020 segments of a few bits each, and a first stripe of 4096 literals
    # under a short code while the table fills: well under a sixteenth of the block)
    assert size("repeat_65280") < 4096 and size("alternate_65280") < 4096
    # (dist32768: the table has 4096 slots and keeps the latest position of a hash, so among random bytes few copies 32768
    # back are still remembered; those that are must be used: smaller than stored)
    assert size("dist32768_65280") < 65280
    assert size("dna_65280") < 65280 * 0.30                  # four symbols and newlines: a dynamic code, some 2.1 bits a base
    for name in ("far32769", "far40000"):                    # the word's copies are out of reach: nothing to gain, stored
        assert size(name) == 65280 + 5, name
    # the 15-bit limit costs little: within a tenth of the bytes' order-0 entropy (an unlimited code would need 21 bits)
    import numpy as np
    f = np.bincount(np.frombuffer(blocks["fibonacci"], np.uint8)).astype(float)
    f = f[f > 0]
    entropy_bytes = float(-(f * np.log2(f / f.sum())).sum()) / 8
    assert size("fibonacci") < 1.10 * entropy_bytes


def test_argument_errors():
    with pytest.raises(Np2Error) as e:
        np2io.bgzf_deflate_host(b"abc", 65281)
    assert e.value.code == -1 and "65280" in str(e.value)
    import ctypes as C
    import numpy as np
    L = np2io._bind()
    src, out, n = np.frombuffer(b"ACGT" * 100, np.uint8), np.empty(40, np.uint8), C.c_uint64()
    rc = L.np2_bgzf_deflate_host(src.ctypes.data, len(src), 0, out.ctypes.data, len(out), C.byref(n))
    want = len(np2io.bgzf_deflate_host(src))
    assert rc == -1 and n.value == want and str(want) in L.np2_io_last_error().decode()


# ---- 2. through the project's own readers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [dc.ASM_GZ, dc.FASTQ_GZ], ids=["fasta", "fastq"])
def test_the_projects_readers_take_the_twins_file(tmp_path, path):
    data = dc.fixture(path)
    ext = ".fa" if path == dc.ASM_GZ else ".fq"
    plain, packed = str(tmp_path / ("x" + ext)), str(tmp_path / ("x" + ext + ".gz"))
    open(plain, "wb").write(data)
    open(packed, "wb").write(np2io.bgzf_deflate_host(data))
    a, b = np2io.seqfile_stream(plain), np2io.seqfile_stream(packed)
    assert len(a) > 90000 and bytes(a) == bytes(b)


# ---- 3. the core as a stand-alone program under the sanitizers ---------------------------------------------------------------------------
def test_deflate_core_under_sanitizers(tmp_path):
    exe, corpus = str(tmp_path / "deflate_core_test"), str(tmp_path / "corpus.bin")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(HERE, "tools", "deflate_core_test.cpp"), "-lz"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n = dc.corpus_file(corpus)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout.strip()) == n and n >= 5 * len(dc.LENGTHS) + 6


# ---- 4. the command line's arguments --------------------------------------------------------------------------------------------------
def test_srqc_out_gz_names_and_refusal(tmp_path, capsys):
    with pytest.raises(SystemExit):
        srqc.parse_args([dc.FASTQ_GZ, "--out_gz"])
    assert "--out_gz needs --out_fq" in capsys.readouterr().err
    prefix = str(tmp_path / "clean")
    a = srqc.parse_args([dc.FASTQ_GZ, dc.FASTQ_GZ, "--out_fq", prefix, "--out_gz"])
    assert a.out_paths == [prefix + ".0.fq.gz", prefix + ".1.fq.gz"]
    assert srqc.parse_args([dc.FASTQ_GZ, "--out_fq", prefix]).out_paths == [prefix + ".0.fq"]
    open(prefix + ".0.fq.gz", "wb").close()
    with pytest.raises(SystemExit) as e:  # nothing is overwritten
        srqc.parse_args([dc.FASTQ_GZ, "--out_fq", prefix, "--out_gz"])
    assert "already exists" in str(e.value)
    assert np2io.is_bgzf_path("a.fa.gz") and np2io.is_bgzf_path("a.bgz") and not np2io.is_bgzf_path("a.fa") and not np2io.is_bgzf_path("a.gz.txt")


# ---- size ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [dc.ASM_GZ, dc.FASTQ_GZ], ids=["ref_test_asm", "sr.R1.2000"])
def test_size_against_zlib_level_1(path):
    """The twin's DEFLATE bytes over the fixture's 65280-byte blocks are at most 1.05 x zlib level 1's on the same blocks.
    Measured: ref_test_asm 26 811 B against zlib's 32 747 (0.819); sr.R1.2000 216 156 B against 229 614 (0.941)."""
    data = dc.fixture(path)
    ref = 0
    for at in range(0, len(data), dc.BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += len(c.compress(data[at:at + dc.BLOCK]) + c.flush())
    ours = dc.check_stream(np2io.bgzf_deflate_host(data), data)
    print(f"{os.path.basename(path)}: {len(data)} bytes, zlib level 1 {ref} B, the twin {ours} B, ratio {ours / ref:.3f}")
    assert ours <= 1.05 * ref
