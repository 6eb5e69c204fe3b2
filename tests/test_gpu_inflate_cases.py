"""The device inflater (csrc/np2_inflate.hip: k_bgzf_inflate) on the hand-built DEFLATE streams of tests/inflate_cases.py:
the shapes no encoder writes, aimed at what exists on the device alone — the wide step and its output cap, the LDS ring and
the threshold behind which a match reads the flushed output, the staged input window, codes beyond the primary tables — and
malformed blocks, each refused with the status of its one fault.  (The stream loop both machines share runs the same corpus
on the CPU under the sanitizers: tests/test_inflate_cases_cpu.py.)

Why these inputs are bounded on the device by construction, whatever their bytes say: output memory is written only by
inf_flush and inf_finish, both behind the `out + n <= isize` checks of the stream loop and the wide step (and the kernel
takes no block whose ISIZE or payload exceeds 64 KiB); every ring index is masked with INF_RING - 1 and every input window
index with INF_IN - 1; a far match reads the flushed output only behind `dist <= at`; input is read only below `clen`
(inf_stage writes zeros beyond it).  So the tests here check the verdict — bytes and status —, not memory safety.

Like its siblings the file ends the session on a device error (NP2_E_DEVICE): nothing more may run on a device that has
reported one, and the error is a finding to be explained from the code.  The refusals come last."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bamout_model as bm
import inflate_cases as ic
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import pileup_to_records, write_bam
from nextpolish2_amd.synth import Synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE = -1, -2


def device_error(what, e):
    """Nothing more may run on a device that has reported an error: the session ends here."""
    pytest.exit(f"device error in {what}: {e}", returncode=3)


@pytest.fixture(scope="module")
def pol():
    p = Polisher([Synth(2000, seed=3).yak(21)])
    yield p
    p.close()


def inflate(pol, what, data):
    try:
        return np2io.bgzf_inflate_device(pol, data)[0]
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(what, e)
        raise


# ---- 1. the valid blocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_valid_blocks_inflate_to_their_bytes(pol, order):
    """every valid and lenient block in one buffer, one launch, a wavefront a block; then in reversed order, so that every
    block is decoded once behind another block's leftovers in LDS"""
    cases = ic.valid() + ic.valid_lenient()
    if order == "reversed":
        cases = cases[::-1]
    try:
        got = inflate(pol, "valid blocks, " + order, b"".join(ic.block_of(c) for c in cases))
    except Np2Error as e:
        m = re.search(r"block (\d+)", str(e))
        raise AssertionError("case %s: %s" % (cases[int(m.group(1))][0] if m else "?", e))
    print("%s: %d blocks in one launch" % (order, len(cases)))
    assert len(got) == sum(len(c[2]) for c in cases)
    bad, at = [], 0
    for name, _, data in cases:
        piece = got[at:at + len(data)].tobytes()
        at += len(data)
        if piece != data:
            first = next(i for i in range(len(data)) if piece[i] != data[i])
            bad.append((name, "first wrong byte %d of %d" % (first, len(data))))
    assert not bad, (len(bad), bad[:30])


# ---- 2. a BAM from a foreign encoder, end to end -------------------------------------------------------------------------------
def test_contig_from_a_hand_encoded_bam(tmp_path):
    """One small contig's records as a BAM whose blocks the hand writer encoded — dynamic blocks with 13- and 14-bit length
    codes and 9-bit distance codes, empty stored blocks in between, a fixed block — with the model's index over the written
    blocks' offsets: read with NP2_INFLATE=gpu and =libdeflate it gives the exported pileup of the same records written
    by bamio.write_bam."""
    L = 3000
    s = Synth(L, depth=8, seed=1000 + L % 97, read_len_mean=L / 3, read_len_sd=L / 20, read_len_min=L // 3)
    recs = pileup_to_records(s.pileup, tid=0, rng=np.random.default_rng(3), decorate=True)
    for i, r in enumerate(recs):
        r["name"] = b"r%d" % i
    refs = [("ctgA", L)]
    plain, foreign = str(tmp_path / "plain.bam"), str(tmp_path / "foreign.bam")
    write_bam(plain, refs, recs)
    S, off = bm.stream(refs, recs)
    blocks = [ic.bgzf(ic.encode_foreign(S[at:at + bm.BLOCK]), S[at:at + bm.BLOCK]) for at in range(0, len(S), bm.BLOCK)]
    for b, at in zip(blocks, range(0, len(S), bm.BLOCK)):  # (zlib reads what the hand writer wrote)
        assert zlib.decompress(b, 31) == S[at:at + bm.BLOCK]
    data = b"".join(blocks) + bm.EOF_BLOCK
    open(foreign, "wb").write(data)
    open(foreign + ".bai", "wb").write(bm.bai(refs, recs, off, bm.block_offsets(data)))
    (tmp_path / "ref.txt").write_bytes(s.pileup.ref.tobytes())
    np2io.write_yak(str(tmp_path / "k21.yak"), s.yak(21))
    code = ("import os, sys, numpy as np; sys.path.insert(0, %r)\n"
            "from nextpolish2_amd import io as np2io\n"
            "pol = np2io.polisher_from_yak_files([sys.argv[2]])\n"
            "ref = open(sys.argv[1], 'rb').read()\n"
            "out = {}\n"
            "for i, path in enumerate(sys.argv[4:]):\n"
            "    for mode in ('gpu', 'libdeflate'):\n"
            "        os.environ['NP2_INFLATE'] = mode\n"
            "        sys.stderr.write('leg %%d %%s\\n' %% (i, mode)); sys.stderr.flush()\n"
            "        bam = np2io.Bam(path)\n"
            "        c = np2io.contig_from_bam(pol, bam, 'ctgA', ref, np2io.FrontOpts())\n"
            "        ex = np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8))\n"
            "        out['%%d_%%s_reads' %% (i, mode)], out['%%d_%%s_nib' %% (i, mode)] = ex.reads, ex.nibbles\n"
            "        bam.close()\n"
            "np.savez(sys.argv[3], **out)\n" % ROOT)
    npz = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "ref.txt"), str(tmp_path / "k21.yak"), npz, plain, foreign],
                       capture_output=True, text=True, env=dict(os.environ, NP2_IO_PROFILE="1"), timeout=600)
    if r.returncode < 0 or "hipError" in r.stderr or "HSA_STATUS" in r.stderr or "illegal memory access" in r.stderr:
        device_error("contig from a hand-encoded BAM", r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    legs = r.stderr.split("leg ")[1:]
    assert len(legs) == 4
    for leg in legs:  # (the device path really ran where it was asked for)
        assert ("fetch_records_gpu:" in leg) == (leg.split()[1] == "gpu"), leg[-2000:]
    got = np.load(npz)
    assert len(got["0_libdeflate_reads"]) > 8
    for k in ("reads", "nib"):
        for leg in ("0_gpu", "1_gpu", "1_libdeflate"):
            assert np.array_equal(got["%s_%s" % (leg, k)], got["0_libdeflate_" + k]), (leg, k)


# ---- 3. the refusals (last: see above) -----------------------------------------------------------------------------------------
def test_malformed_blocks_are_refused_with_their_status(pol):
    """each malformed block between two valid ones, a call each: NP2_E_ARG naming block 1 and the status of its fault (by
    the words of np2inf::Status, written by hand in the corpus); afterwards the context inflates as before"""
    rng = np.random.default_rng(41)
    good = rng.integers(0, 4, 5000, dtype=np.uint8).tobytes() + b"\xff" * 3000
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    good_block = ic.bgzf(co.compress(good) + co.flush(), good)
    bad = []
    for name, block, status, note in ic.refused():
        try:
            inflate(pol, "refusal " + name, good_block + block + good_block)
            bad.append((name, "accepted", note))
        except Np2Error as e:
            if not (e.code == E_ARG and "BGZF inflate failed (block 1, status %d)" % status in str(e)):
                bad.append((name, "expected status %d: %s" % (status, e), note))
    assert not bad, bad
    print("%d calls of three blocks each" % len(ic.refused()))
    assert inflate(pol, "a valid block after the refusals", good_block).tobytes() == zlib.decompress(good_block, 31) == good
