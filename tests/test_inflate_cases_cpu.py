"""The hand-built DEFLATE streams of tests/inflate_cases.py through the inflater's stream loop (csrc/np2_inflate_core.hpp) on
the CPU: tests/tools/inflate_cases_test.cpp, the one-lane machine, as a stand-alone program under the address and
undefined-behaviour sanitizers, each case's output a heap block of exactly ISIZE bytes.  Every valid stream (zlib is its
judge when the corpus is built) gives status 0 and its bytes' CRC-32; every malformed stream is refused with the status its
one fault has by the words of np2inf::Status, written by hand in the corpus — and, the sanitizers being the bound, writes
nothing past its ISIZE on the way.  (The device-only half — wide step, ring, input window — is tests/test_gpu_inflate_cases.py.)"""
import os
import subprocess

import pytest

import inflate_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_cases")
    exe, corpus = str(d / "inflate_cases_test"), str(d / "corpus.bin")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HERE, "tools", "inflate_cases_test.cpp"), "-lz"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want = ic.corpus_file(corpus)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=600)
    lines = [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]
    # (a sanitizer report ends the program at the case it names: the cases before it are in `lines`)
    assert r.returncode == 0 and not r.stderr, ("after case", want[len(lines) - 1][0] if lines else None, r.stderr[-3000:])
    assert len(lines) == len(want)
    return {name: (got, (status, crc)) for (name, status, crc), got in zip(want, lines)}


def test_the_corpus_holds_what_it_was_built_for():
    v, r = ic.valid(), ic.refused()
    assert len({c[0] for c in v}) == len(v) > 350
    assert {c[2] for c in r} == set(range(1, 11))  # every status the stream loop can give
    assert all(len(ic.block_of(c)) <= 65536 and len(c[2]) <= 65536 for c in v)
    assert max(len(c[1]) for c in v) == ic.MAX_PAYLOAD and max(len(c[2]) for c in v) == 65536


def test_valid_streams_inflate_to_their_bytes(results):
    bad = []
    for name, payload, data in ic.valid() + ic.valid_lenient():
        (status, crc), (_, want_crc) = results[name]
        if status != ic.ST_OK or crc != want_crc:
            bad.append((name, status, hex(crc), hex(want_crc)))
    assert not bad, bad[:20]


def test_malformed_streams_are_refused_with_their_status(results):
    bad = []
    for name, block, want, note in ic.refused():
        (status, _), _ = results[name]
        if status != want:
            bad.append((name, "status %d, expected %d" % (status, want), note))
    assert not bad, bad


def test_the_lenient_case_is_refused_by_the_host_pools_inflaters():
    """the known difference: zlib and, where its library is on the machine, libdeflate refuse the incomplete
    literal / length code that the project's inflater takes (test_valid_streams_inflate_to_their_bytes)"""
    import ctypes as C
    import zlib
    (name, payload, data), = ic.valid_lenient()
    with pytest.raises(zlib.error, match="invalid literal/lengths set"):
        zlib.decompressobj(-15).decompress(payload)
    try:
        L = C.CDLL("libdeflate.so.0")
    except OSError:
        return
    L.libdeflate_alloc_decompressor.restype = C.c_void_p
    L.libdeflate_deflate_decompress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.libdeflate_free_decompressor.argtypes = [C.c_void_p]
    d, out, got = L.libdeflate_alloc_decompressor(), C.create_string_buffer(len(data)), C.c_size_t()
    assert L.libdeflate_deflate_decompress(d, payload, len(payload), out, len(data), C.byref(got)) == 1  # LIBDEFLATE_BAD_DATA
    L.libdeflate_free_decompressor(d)
