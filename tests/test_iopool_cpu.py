"""The input side's host pool and buffers (csrc/np2_iopool.hpp: IoPool, HostBlockPool, RawBuf) without a device:
tests/tools/iopool_test.cpp, a program of its own, built once with the thread sanitizer and once with the address and
undefined-behaviour sanitizers, one bounded run per scenario and build, the pool at four threads."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZERS = {"thread": ["-fsanitize=thread"], "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SCENARIOS = ["sizes", "one_thread", "during", "during_throws", "two_callers", "rawbuf", "blocks"]


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("iopool") / f"iopool_test_{request.param}")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + SANITIZERS[request.param] +
                       ["-o", out, os.path.join(HERE, "tools", "iopool_test.cpp"), "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_io_pool_under_the_host_sanitizers(exe, scenario):
    r = subprocess.run([exe, scenario], capture_output=True, text=True, timeout=60, env=dict(os.environ, NP2_IO_THREADS="4"))
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-3000:])
