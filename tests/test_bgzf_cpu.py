"""The BGZF header parser every reader shares (csrc/np2_bgzf.hpp) without a device: tests/tools/bgzf_test.cpp, a program of
its own, built with the address and undefined-behaviour sanitizers, one bounded run per scenario."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SCENARIOS = ["accept", "reject", "need"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgzf") / "bgzf_test")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", out, os.path.join(HERE, "tools", "bgzf_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_bgzf_header_parser_under_the_host_sanitizers(exe, scenario):
    r = subprocess.run([exe, scenario], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-3000:])
