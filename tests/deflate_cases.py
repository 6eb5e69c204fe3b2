"""The corpus of the BGZF deflater's tests (test_deflate_cpu.py, test_gpu_deflate.py): blocks built for the edges of the
encoder (csrc/np2_deflate_core.hpp walks a block in stripes of 64 x 64 bytes, hashes 8 bytes, codes at most 15 bits) and
streams built for the edges of the block cutter.  Seeded; the two fixtures are inflated with Python's gzip."""
import functools
import gzip
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ASM_GZ = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
FASTQ_GZ = os.path.join(HERE, "golden", "ref_pairs", "sr.R1.2000.fastq.gz")
BLOCK = 65280
LENGTHS = (0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 260, 4095, 4096, 4097, 65279, 65280)
STREAM_LENGTHS = (65279, 65280, 65281, 2 * 65280 + 1)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@functools.lru_cache(maxsize=None)
def fixture(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def dna(rng, n):
    """random bases, a newline after every 60"""
    lines = (n + 60) // 61 + 1
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(lines, 61))].copy()
    a[:, 60] = 10
    return a.tobytes()[:n]


def fib_block(rng):
    """symbol frequencies 1, 1, 2, 3, 5, 8, ... (22 of them: an unlimited Huffman code reaches 21 bits) and 18 bytes that
    occur once: forty distinct bytes, shuffled"""
    f, syms = [1, 1], []
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    for i, k in enumerate(f):
        syms += [40 + i] * k
    syms += list(range(100, 118))
    a = np.array(syms, np.uint8)
    rng.shuffle(a)
    return a.tobytes()


def all_bytes_block(rng):
    """every byte value, and repeats of every length from 3 to 258 (each word twice in a row, a new byte in between)"""
    out = bytearray(range(256))
    for ln in list(range(3, 259, 5)) + [258]:
        w = rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
        out += w + w + bytes([ln & 255])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def blocks():
    """[(name, bytes)], every block at most 65280 bytes"""
    rng = np.random.default_rng(20260119)
    fq = fixture(FASTQ_GZ)
    rnd = rng.integers(0, 256, size=BLOCK, dtype=np.uint8).tobytes()
    d = dna(rng, BLOCK)
    alt = b"AC" * (BLOCK // 2)
    out = []
    for n in LENGTHS:
        out.append((f"repeat_{n}", b"G" * n))
        out.append((f"alternate_{n}", alt[:n]))
        out.append((f"random_{n}", rnd[:n]))
        out.append((f"dna_{n}", d[:n]))
        out.append((f"fastq_{n}", fq[1000:1000 + n]))
    for n in (65279, 65280):  # the second half repeats the first at distance exactly 32768
        half = rng.integers(0, 256, size=32768, dtype=np.uint8).tobytes()
        out.append((f"dist32768_{n}", (half + half)[:n]))
    # a 300-byte word whose earlier copies lie 32769 and 40000 bytes back: out of a match's reach
    far = bytearray(rng.integers(0, 256, size=BLOCK, dtype=np.uint8).tobytes())
    word = rng.integers(0, 256, size=300, dtype=np.uint8).tobytes()
    far[100:400] = word
    far[100 + 32769:400 + 32769] = word
    far2 = bytearray(far)
    far2[100 + 32769:400 + 32769] = rnd[:300]
    far2[100 + 40000:400 + 40000] = word
    out.append(("far32769", bytes(far)))
    out.append(("far40000", bytes(far2)))
    both = bytearray(far)
    both[100 + 40000:400 + 40000] = word
    out.append(("far_both", bytes(both)))
    fb = fib_block(rng)
    out.append(("fibonacci", fb))
    out.append(("fibonacci_4097", fb[:4097]))
    out.append(("all_bytes", all_bytes_block(rng)))
    assert all(len(b) <= BLOCK for _, b in out)
    return out


@functools.lru_cache(maxsize=None)
def streams():
    """[(name, bytes, block_bytes)] for the block cutter"""
    fq, asm = fixture(FASTQ_GZ), fixture(ASM_GZ)
    out = [(f"fastq_{n}", fq[:n], 0) for n in STREAM_LENGTHS]
    out.append(("block_bytes_1", asm[:300], 1))
    out.append(("block_bytes_100", asm[:4097], 100))
    out.append(("block_bytes_65280", fq[:65281], 65280))
    out.append(("empty", b"", 0))
    return out


def corpus_bytes(n):
    """n bytes of the block corpus, repeated as often as it takes"""
    one = b"".join(b for _, b in blocks())
    return (one * (n // len(one) + 1))[:n]


def corpus_file(path):
    """the block corpus as tests/tools/deflate_core_test.cpp reads it; returns the number of cases"""
    with open(path, "wb") as f:
        for _, b in blocks():
            f.write(struct.pack("<I", len(b)) + b)
    return len(blocks())


def check_stream(z, data, block_bytes=0):
    """a whole BGZF stream `z` of `data`, every field of it; returns the total of the blocks' DEFLATE bytes"""
    bb = block_bytes or BLOCK
    at, pos, payload_total, n_blocks = 0, 0, 0, 0
    assert z[-28:] == EOF_BLOCK
    while at < len(z):
        assert z[at:at + 4] == b"\x1f\x8b\x08\x04", at
        assert z[at + 4:at + 10] == b"\0\0\0\0\0\xff", at       # MTIME 0, XFL 0, OS unknown
        assert z[at + 10:at + 16] == b"\x06\0BC\x02\0", at      # XLEN 6, the BC subfield of 2 bytes
        bsize = struct.unpack_from("<H", z, at + 16)[0] + 1
        assert bsize <= 65536 and at + bsize <= len(z)
        payload = z[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", z, at + bsize - 8)
        last = at + bsize == len(z)
        piece = b"" if last else data[pos:pos + bb]
        assert isize == len(piece) and (last or isize > 0), (at, isize, len(piece))
        assert len(payload) <= len(piece) + 5
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) == piece and d.eof and d.unused_data == b"", at
        assert crc == zlib.crc32(piece), at
        if last:
            assert z[at:] == EOF_BLOCK
        else:
            payload_total += len(payload)
        pos += isize
        at += bsize
        n_blocks += 1
    assert pos == len(data) and n_blocks == (len(data) + bb - 1) // bb + 1
    assert gzip.decompress(z) == data
    return payload_total
