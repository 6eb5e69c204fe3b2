"""The CRC-32 every BGZF block carries, on the paths that need no GPU: the arithmetic of the GPU kernel
(csrc/np2_crc32_core.hpp: 64 pieces of a right-aligned 64 KiB frame, slice-by-4 tables, the fixed-length mulmod and the
six-step fold) as a one-lane host program against zlib, and the host reader (Bgzf::read_block) refusing a BAM whose first
block does not carry the CRC of what it inflates to.  Also the helpers the GPU tests damage their BAMs with."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- damaging a BGZF file ------------------------------------------------------------------------------------------
def bgzf_blocks(data):
    """[(file offset, payload offset, payload length, block size, isize)] of the BGZF blocks of `data`"""
    out, p = [], 0
    while p < len(data):
        assert data[p] == 31 and data[p + 1] == 139, p
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        bsize = None
        q = p + 12
        while q < p + 12 + xlen:
            si1, si2, slen = data[q], data[q + 1], struct.unpack_from("<H", data, q + 2)[0]
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", data, q + 4)[0] + 1
            q += 4 + slen
        assert bsize
        out.append((p, p + 12 + xlen, bsize - 12 - xlen - 8, bsize, struct.unpack_from("<I", data, p + bsize - 4)[0]))
        p += bsize
    return out


def flip_crc_word(data, blk):
    """`data` with one bit of block blk's CRC32 word flipped"""
    off, _, _, bsize, _ = bgzf_blocks(data)[blk]
    d = bytearray(data)
    d[off + bsize - 8 + 1] ^= 0x04
    return bytes(d)


def surviving_payload_flip(data, blk):
    """`data` with one bit of block blk's DEFLATE payload flipped such that zlib still inflates the payload to ISIZE bytes —
    of a different CRC-32.  Candidates: the single-bit flips from the middle of the payload onward, in order; none of the
    first 200 surviving is a failure of the test, not a skip (58 - 63 % of such flips survive on sequence data)."""
    off, pay, clen, bsize, isize = bgzf_blocks(data)[blk]
    want = struct.unpack_from("<I", data, off + bsize - 8)[0]
    for k in range(200):
        bit = (clen // 2) * 8 + k
        if bit >= clen * 8:
            break
        d = bytearray(data)
        d[pay + bit // 8] ^= 1 << (bit % 8)
        z = zlib.decompressobj(-15)
        try:
            got = z.decompress(bytes(d[pay:pay + clen]), isize + 1)
        except zlib.error:
            continue
        if z.eof and len(got) == isize and (zlib.crc32(got) & 0xFFFFFFFF) != want:
            return bytes(d)
    raise AssertionError("no single-bit payload flip among the first 200 survives zlib's inflate")


def flip_stored_byte(data, blk):
    """`data` with a data byte of block blk's payload changed; the block must be made of stored deflate blocks (level 0):
    it inflates to whatever its bytes say.  (The byte is the middle one of the longest stored piece: no LEN / NLEN field.)"""
    off, pay, clen, bsize, isize = bgzf_blocks(data)[blk]
    p, best = pay, (0, 0)
    while p < pay + clen:
        assert (data[p] & 6) == 0, "not a stored block"
        n, nn = struct.unpack_from("<HH", data, p + 1)
        assert n == (~nn & 0xFFFF)
        best = max(best, (n, p + 5))
        last = data[p] & 1
        p += 5 + n
        if last:
            break
    assert best[0] > 1000
    d = bytearray(data)
    d[best[1] + best[0] // 2] ^= 0x21
    return bytes(d)


# ---- the tests -----------------------------------------------------------------------------------------------------
def test_crc32_core_equals_zlib(tmp_path):
    exe = str(tmp_path / "crc32_core_test")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "tools", "crc32_core_test.cpp"), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # 22 edge lengths + 400 seeded random ones, four kinds of content each
    assert r.stdout.strip() == "%d buffers checked" % ((22 + 400) * 4)


def _small_bam(tmp_path):
    from nextpolish2_amd.bamio import pileup_to_records, write_bam
    from nextpolish2_amd.synth import Synth
    s = Synth(3000, depth=8, seed=77, read_len_mean=1000.0, read_len_sd=150.0, read_len_min=800)
    recs = pileup_to_records(s.pileup, tid=0, rng=np.random.default_rng(3), decorate=True)
    path = str(tmp_path / "m.bam")
    write_bam(path, [("ctgA", s.pileup.L)], recs)
    return path


@pytest.mark.parametrize("damage", ["none", "crc_word", "payload"])
def test_host_reader_checks_the_first_blocks_crc(tmp_path, damage):
    """np2_bam_open reads the header through Bgzf::read_block: a first block whose CRC32 word has a bit flipped, or whose
    payload has one flipped that zlib still inflates to ISIZE bytes, is refused with NP2_E_ARG and the word CRC32."""
    from nextpolish2_amd import io as np2io
    from nextpolish2_amd.api import Np2Error
    path = _small_bam(tmp_path)
    data = open(path, "rb").read()
    if damage == "none":
        np2io.Bam(path).close()
        return
    bad = flip_crc_word(data, 0) if damage == "crc_word" else surviving_payload_flip(data, 0)
    assert bad != data and len(bad) == len(data)
    open(path, "wb").write(bad)
    with pytest.raises(Np2Error) as e:
        np2io.Bam(path)
    assert e.value.code == -1
    assert "CRC32" in str(e.value) and "file offset 0" in str(e.value)
