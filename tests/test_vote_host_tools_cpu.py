"""The host half of the phasing vote (csrc/np2_vote_host.hpp over csrc/np2_phase_host.hpp: merge of the shards' votes, rows
from pairs, the threaded decision) without a device and without the library: tests/tools/vote_host_test.cpp, a program of
its own, built once with the thread sanitizer and once with the address and undefined-behaviour sanitizers, one bounded
run per scenario and build.  A sanitizer report goes to stderr and fails the run."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZERS = {"thread": ["-fsanitize=thread"], "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
# every threaded path, whatever the graph's size
LOWERED = {"NP2_VOTE_AHEAD_MIN": "0", "NP2_VOTE_PIECES_MIN": "0"}


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vote_host") / f"vote_host_test_{request.param}")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + SANITIZERS[request.param] +
                       ["-o", out, os.path.join(HERE, "tools", "vote_host_test.cpp"), "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, args, **env):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("scenario", ["rows", "merge"])
def test_rows_and_merge_under_the_host_sanitizers(exe, scenario):
    assert _run(exe, [scenario], NP2_VOTE_THREADS="4") == "ok\n"


def test_large_vote_on_one_thread_and_on_eight(exe):
    """60 000 reads, 1.2 M pairs: past the 2^18-pair, 2^20-edge and 2^15-key thresholds of the threaded paths.  The losers'
    hash from the pair list and from the rows, on one thread and on eight: all four equal."""
    hashes = []
    for threads in ("1", "8"):
        lines = _run(exe, ["threads"], NP2_VOTE_THREADS=threads, **LOWERED).split()
        assert lines[0] == "pairs" and lines[2] == "rows", lines
        hashes += [lines[1], lines[3]]
    assert len(set(hashes)) == 1, hashes


def test_recorded_vote_equals_the_oracles_decision(exe, tmp_path):
    """The vote recorded from a 16 Mb diploid contig (tests/golden/votes), on eight threads, whole and cut in two: the losers
    are the ORACLE's (tests/golden/make_vote_fixture.py), not this code's."""
    from nextpolish2_amd.api import Vote
    z = np.load(os.path.join(HERE, "golden", "votes", "vote_16Mb_diploid.npz"))
    v = Vote.unpack(z["packed"])
    for name, ext in (("pair_key", "u64"), ("pair_cnt", "u32"), ("read_id", "u32"), ("first_pos", "u32"), ("ref_w", "i32"), ("flags", "u8")):
        a = getattr(v, name)
        a.astype(a.dtype.newbyteorder("<")).tofile(str(tmp_path / f"{name}.{ext}"))
    _run(exe, ["recorded", str(tmp_path), str(int(z["n_reads"][0]))], NP2_VOTE_THREADS="8")
    for form in ("whole", "cut"):
        assert np.array_equal(np.fromfile(str(tmp_path / f"losers_{form}.u32"), dtype="<u4"), z["losers"]), form
