"""Every BGZF block a read path inflates must carry the CRC-32 of its inflated bytes (csrc/np2_crc32.hip: k_bgzf_crc32 behind
k_bgzf_inflate on the device; libdeflate_crc32 / zlib's crc32 in the host pool): the kernel against zlib, and a damaged
block — a flipped CRC word, a payload bit flip that still inflates to ISIZE bytes, a changed byte of a stored block —
refused with NP2_E_ARG "BGZF CRC32 mismatch (block at file offset N)" on the device path, the host pool, the resident
stream, reference-interval shards and the command line.  The switches are read once per process: subprocesses."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import write_bam_raw
from nextpolish2_amd.synth import Synth
from test_crc32_cpu import bgzf_blocks, flip_crc_word, flip_stored_byte, surviving_payload_flip
from test_gpu_inflate import _bundle4, bgzf_block

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 65279, 65280, 65535, 65536]


def _pol():
    return Polisher([Synth(2000, seed=3).yak(21)])


# ---- 1. the kernel against zlib ---------------------------------------------------------------------------------------------
def test_crc32_kernel_equals_zlib():
    rng = np.random.default_rng(17)
    pol = _pol()
    lens = list(EDGE_LENGTHS)
    # (pieces lie back to back: odd lengths in between move the long ones over every alignment mod 16)
    for a in range(16):
        lens += [1, int(rng.integers(1, 65537)), 1024, 65536 - a, 0, 17]
    lens += [int(x) for x in rng.integers(0, 65537, 60)]
    parts = []
    for i, n in enumerate(lens):
        kind = i % 4
        if kind == 0:
            parts.append(np.zeros(n, dtype=np.uint8))
        elif kind == 1:
            parts.append(np.full(n, 0xFF, dtype=np.uint8))
        elif kind == 2:
            parts.append(rng.integers(0, 256, n, dtype=np.uint8))
        else:
            parts.append(((1 << rng.integers(0, 4, n)) << 4 | (1 << rng.integers(0, 4, n))).astype(np.uint8))
    data = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert {int(o) % 16 for o in off[:-1]} == set(range(16))
    got, ms = np2io.crc32_device(pol, data, off)
    want = np.array([zlib.crc32(p.tobytes()) & 0xFFFFFFFF for p in parts], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), lens[i], int(off[i]) % 16, hex(int(got[i])), hex(int(want[i]))) for i in bad[:10]]
    assert ms >= 0
    # every edge length at every alignment
    lens2, parts2 = [], []
    for a in range(16):
        for n in EDGE_LENGTHS[:-4] + [65536 - 16 * 3 - a]:
            lens2 += [n, 1]
            parts2 += [rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, 1, dtype=np.uint8)]
    off2 = np.concatenate([[0], np.cumsum(lens2)]).astype(np.uint64)
    got2, _ = np2io.crc32_device(pol, np.concatenate(parts2), off2)
    assert np.array_equal(got2, np.array([zlib.crc32(p.tobytes()) & 0xFFFFFFFF for p in parts2], dtype=np.uint32))
    # no piece at all
    g0, _ = np2io.crc32_device(pol, data, np.array([0], dtype=np.uint64))
    assert len(g0) == 0


def test_crc32_device_argument_errors():
    pol = _pol()
    data = np.zeros(70000, dtype=np.uint8)
    for off in ([0, 65537], [0, 100, 50], [0, 100, 70001]):
        with pytest.raises(Np2Error) as e:
            np2io.crc32_device(pol, data, np.array(off, dtype=np.uint64))
        assert e.value.code == -1
    got, _ = np2io.crc32_device(pol, data, np.array([0, 65536, 70000], dtype=np.uint64))
    assert [int(x) for x in got] == [zlib.crc32(bytes(65536)) & 0xFFFFFFFF, zlib.crc32(bytes(4464)) & 0xFFFFFFFF]


# ---- 2. np2_bgzf_inflate_device ---------------------------------------------------------------------------------------------
def test_inflate_device_checks_each_blocks_crc():
    rng = np.random.default_rng(23)
    pol = _pol()
    seq = lambda n: ((1 << rng.integers(0, 4, n)) << 4 | (1 << rng.integers(0, 4, n))).astype(np.uint8).tobytes()
    want = [seq(30000), b"", seq(65280), b"\xff" * 4097, seq(1), seq(50001), b""]
    data = b"".join(bgzf_block(d) for d in want)
    got, _ = np2io.bgzf_inflate_device(pol, data)
    assert got.tobytes() == b"".join(want)
    for make in (flip_crc_word, surviving_payload_flip):
        for blk in (2, 5):
            bad = make(data, blk)
            with pytest.raises(Np2Error) as e:
                np2io.bgzf_inflate_device(pol, bad)
            assert e.value.code == -1 and "CRC32" in str(e.value) and "(block %d)" % blk in str(e.value), str(e.value)
    # the end-of-file marker's shape must carry CRC 0
    with pytest.raises(Np2Error) as e:
        np2io.bgzf_inflate_device(pol, flip_crc_word(data, 1))
    assert "CRC32" in str(e.value) and "(block 1)" in str(e.value)
    # a block whose stream does not inflate keeps the inflate's message (its output is partial: not summed)
    off, pay, clen, bsize, isize = bgzf_blocks(data)[2]
    d = bytearray(data)
    d[pay] |= 0x06  # block type 3
    with pytest.raises(Np2Error) as e:
        np2io.bgzf_inflate_device(pol, bytes(d))
    assert "BGZF inflate failed" in str(e.value) and "CRC32" not in str(e.value)


# ---- 3. one contig, every inflater ------------------------------------------------------------------------------------------
_CONTIG_CODE = ("import sys, json, numpy as np; sys.path.insert(0, %r)\n"
                "from nextpolish2_amd import Opts\nfrom nextpolish2_amd import io as np2io\n"
                "from nextpolish2_amd.api import Np2Error\n"
                "pol = np2io.polisher_from_yak_files([sys.argv[3]])\n"
                "res = {}\n"
                "for name, ref_path, out in [a.split(':') for a in sys.argv[4:]]:\n"
                "    ref = open(ref_path, 'rb').read()\n"
                "    try:\n"
                "        bam = np2io.Bam(sys.argv[1])\n"
                "        c = np2io.contig_from_bam(pol, bam, name, ref, np2io.FrontOpts())\n"
                "        ex = np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8))\n"
                "        b, p = pol.polish_resident(c, Opts())\n"
                "        np.savez(out, reads=ex.reads, nib=ex.nibbles, b=b, p=p)\n"
                "        res[name] = {'code': 0, 'msg': ''}\n"
                "    except Np2Error as e:\n"
                "        res[name] = {'code': e.code, 'msg': str(e)}\n"
                "print('RESULT ' + json.dumps(res))\n" % ROOT)


def _run_contigs(bam, yak, jobs, env, timeout=600):
    """contig_from_bam + export + polish of jobs = [(name, ref file, npz to write)] in a fresh process -> ({name: {code, msg}}, stderr)"""
    r = subprocess.run([sys.executable, "-c", _CONTIG_CODE, str(bam), "-", str(yak)] + ["%s:%s:%s" % j for j in jobs],
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:]), r.stderr


def _one_ref_bam(tmp_path, level):
    s = Synth(60000, depth=25, seed=1041, read_len_mean=9000.0, read_len_sd=1500.0)
    path = str(tmp_path / ("m%d.bam" % level))
    write_bam_raw(path, [("ctgA", s.pileup.L)], [s.bam_records(0)], level=level)
    (tmp_path / "ref.txt").write_bytes(s.pileup.ref.tobytes())
    np2io.write_yak(str(tmp_path / "k21.yak"), s.yak(21))
    return s, path


def _same(a, b):
    a, b = np.load(a), np.load(b)
    return all(np.array_equal(a[k], b[k]) for k in ("reads", "nib", "b", "p"))


@pytest.mark.parametrize("damage", ["crc_word", "payload", "stored"])
def test_contig_with_a_damaged_block_is_refused_by_every_inflater(tmp_path, damage):
    s, path = _one_ref_bam(tmp_path, 0 if damage == "stored" else 6)
    data = open(path, "rb").read()
    blks = bgzf_blocks(data)
    assert len(blks) >= 9
    mid = len(blks) // 2  # (a block in the middle of the file: records of the contig before and behind it)
    bad = {"crc_word": flip_crc_word, "payload": surviving_payload_flip, "stored": flip_stored_byte}[damage](data, mid)
    assert len(bad) == len(data) and bad != data
    bad_path = str(tmp_path / "bad.bam")
    open(bad_path, "wb").write(bad)
    open(bad_path + ".bai", "wb").write(open(path + ".bai", "rb").read())
    ref = str(tmp_path / "ref.txt")
    for mode in ("libdeflate", "zlib", "gpu"):
        res, err = _run_contigs(bad_path, tmp_path / "k21.yak", [("ctgA", ref, str(tmp_path / "x.npz"))], {"NP2_INFLATE": mode, "NP2_IO_PROFILE": "1"})
        assert res["ctgA"]["code"] == -1, (mode, res)
        assert "CRC32" in res["ctgA"]["msg"] and "file offset %d)" % blks[mid][0] in res["ctgA"]["msg"], (mode, res)
    if damage == "crc_word":  # the switch does what it says: the bytes are the undamaged file's
        good, _ = _run_contigs(path, tmp_path / "k21.yak", [("ctgA", ref, str(tmp_path / "good.npz"))], {"NP2_INFLATE": "gpu"})
        assert good["ctgA"]["code"] == 0, good
        for mode in ("gpu", "libdeflate"):
            res, _ = _run_contigs(bad_path, tmp_path / "k21.yak", [("ctgA", ref, str(tmp_path / ("off_%s.npz" % mode)))], {"NP2_INFLATE": mode, "NP2_BGZF_CRC": "0"})
            assert res["ctgA"]["code"] == 0, (mode, res)
            assert _same(str(tmp_path / "good.npz"), str(tmp_path / ("off_%s.npz" % mode))), mode


# ---- 4. / 5. several references ---------------------------------------------------------------------------------------------
def _blocks_of_one_reference(data, tid):
    """indices of the BGZF blocks of BAM `data` that hold bytes of records of reference `tid` and of no other reference
    (found by walking the undamaged inflated stream)"""
    blks = bgzf_blocks(data)
    pieces = [zlib.decompress(data[pay:pay + clen], -15) for _, pay, clen, _, _ in blks]
    start = np.concatenate([[0], np.cumsum([len(p) for p in pieces])])
    st = b"".join(pieces)
    assert st[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<I", st, 4)[0]
    n_ref = struct.unpack_from("<I", st, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<I", st, p)[0] + 4
    refs_in = [set() for _ in blks]
    while p < len(st):
        bs, ref_id = struct.unpack_from("<Ii", st, p)
        b0 = int(np.searchsorted(start, p, side="right")) - 1
        b1 = int(np.searchsorted(start, p + 4 + bs - 1, side="right")) - 1
        for b in range(b0, b1 + 1):
            refs_in[b].add(ref_id)
        p += 4 + bs
    assert p == len(st)
    return [i for i, r in enumerate(refs_in) if r == {tid}], blks


def _damaged_copy(tmp_path, data, tid):
    own, blks = _blocks_of_one_reference(data, tid)
    assert len(own) >= 3, own
    blk = own[len(own) // 2]
    bad = flip_crc_word(data, blk)
    d = tmp_path / "bad"
    d.mkdir()
    (d / "m.bam").write_bytes(bad)
    (d / "m.bam.bai").write_bytes((tmp_path / "m.bam.bai").read_bytes())
    return d / "m.bam", blks[blk][0]


def test_damage_in_one_reference_leaves_the_others_readable(tmp_path):
    recs, (sA, sB, sD), ctgC, y21 = _bundle4(tmp_path)
    data = (tmp_path / "m.bam").read_bytes()
    bad_bam, bad_off = _damaged_copy(tmp_path, data, 0)
    (tmp_path / "refA.txt").write_bytes(sA.pileup.ref.tobytes())
    (tmp_path / "refD.txt").write_bytes(sD.pileup.ref.tobytes())
    yak = tmp_path / "k21.yak"
    for mode in ("libdeflate", "gpu", "gpu_per_ref"):
        env = {"NP2_INFLATE": mode.split("_")[0], "NP2_IO_PROFILE": "1"}
        if mode == "gpu_per_ref":
            env["NP2_BAM_RESIDENT_MB"] = "0"
        good, _ = _run_contigs(tmp_path / "m.bam", yak, [("ctgD", str(tmp_path / "refD.txt"), str(tmp_path / ("goodD_%s.npz" % mode)))], env)
        assert good["ctgD"]["code"] == 0, (mode, good)
        res, err = _run_contigs(bad_bam, yak, [("ctgA", str(tmp_path / "refA.txt"), str(tmp_path / "xA.npz")),
                                               ("ctgD", str(tmp_path / "refD.txt"), str(tmp_path / ("badD_%s.npz" % mode)))], env)
        assert res["ctgA"]["code"] == -1 and "CRC32" in res["ctgA"]["msg"], (mode, res)
        assert "file offset %d)" % bad_off in res["ctgA"]["msg"], (mode, res)
        assert res["ctgD"]["code"] == 0, (mode, res)
        assert _same(str(tmp_path / ("goodD_%s.npz" % mode)), str(tmp_path / ("badD_%s.npz" % mode))), mode
        if mode == "gpu":  # the resident stream was given up, the per-reference path read ctgD
            assert "stretch of the resident stream" not in err and "resident BAM:" not in err, err[-2000:]
            assert "fetch_records_gpu:" in err, err[-2000:]
    assert _same(str(tmp_path / "goodD_gpu.npz"), str(tmp_path / "goodD_libdeflate.npz"))


@pytest.mark.parametrize("mode", ["gpu", "libdeflate"])
def test_command_line_writes_the_contigs_before_the_damage_then_fails(tmp_path, mode):
    _bundle4(tmp_path)
    data = (tmp_path / "m.bam").read_bytes()
    bad_bam, bad_off = _damaged_copy(tmp_path, data, 3)
    env = dict(os.environ, PYTHONPATH=ROOT, NP2_INFLATE=mode)
    outs = {}
    for what, bam in (("good", tmp_path / "m.bam"), ("bad", bad_bam)):
        out = tmp_path / ("out_%s.fa" % what)
        r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-L", "10000", "-o", str(out), str(bam),
                            str(tmp_path / "g.fa.gz"), str(tmp_path / "k21.yak")], capture_output=True, env=env, timeout=600)
        if what == "good":
            assert r.returncode == 0, r.stderr.decode()[-3000:]
        else:
            assert r.returncode != 0
            assert "CRC32" in r.stderr.decode(), r.stderr.decode()[-3000:]
        outs[what] = out.read_bytes()
    cut = outs["good"].index(b">ctgD")
    assert cut > 100000 and outs["good"].count(b">") == 4
    assert outs["bad"][:cut] == outs["good"][:cut]
    assert b">ctgD" not in outs["bad"] and outs["bad"].count(b">") == 3


# ---- 6. a reference-interval shard ------------------------------------------------------------------------------------------
_SHARD_CODE = ("import sys, json; sys.path.insert(0, %r)\n"
               "from nextpolish2_amd import io as np2io\nfrom nextpolish2_amd.api import Np2Error\n"
               "pol = np2io.polisher_from_yak_files([sys.argv[3]])\n"
               "ref = open(sys.argv[2], 'rb').read()\n"
               "bam = np2io.Bam(sys.argv[1])\n"
               "try:\n"
               "    sh = np2io.ShardFromBam(pol, bam, 'ctgA', ref, int(sys.argv[4]), int(sys.argv[5]), halo=2048)\n"
               "    n = len(sh.own_offsets)\n"
               "    sh.abort()\n"
               "    print('RESULT ' + json.dumps({'code': 0, 'msg': '', 'n': n}))\n"
               "except Np2Error as e:\n"
               "    print('RESULT ' + json.dumps({'code': e.code, 'msg': str(e)}))\n" % ROOT)


@pytest.mark.parametrize("mode", ["gpu", "libdeflate"])
def test_shard_zone_with_a_damaged_block_is_refused(tmp_path, mode):
    s, path = _one_ref_bam(tmp_path, 6)
    data = open(path, "rb").read()
    blks = bgzf_blocks(data)
    mid = len(blks) // 2
    bad_path = str(tmp_path / "bad.bam")
    open(bad_path, "wb").write(surviving_payload_flip(data, mid))
    open(bad_path + ".bai", "wb").write(open(path + ".bai", "rb").read())

    def run(bam):
        r = subprocess.run([sys.executable, "-c", _SHARD_CODE, bam, str(tmp_path / "ref.txt"), str(tmp_path / "k21.yak"), "20480", "40960"],
                           capture_output=True, text=True, env=dict(os.environ, NP2_INFLATE=mode), timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    good = run(path)
    assert good["code"] == 0 and good["n"] > 10, good
    res = run(bad_path)
    assert res["code"] == -1 and "CRC32" in res["msg"] and "file offset %d)" % blks[mid][0] in res["msg"], res
