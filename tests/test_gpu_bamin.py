"""BAM input on the device (include/np2_io.h: "BAM input"; k_bamin_walk, k_bamin_fields, k_bamin_pack behind the device
inflater): io.Sam on unsorted BAM files against io.Sam on the SAM text of the same records, byte for byte in the written .bam
and .bai and in every export; against the host twin (np2_bamin_host) and the plain-Python model (tests/bamin_model.py); under
block cuts and piece sizes that split every part of a record; refusals; the project's readers and command lines on top."""
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import bamfull_model as fm
import bamin_model as im
import bamout_model as bm
from bamin_model import raw_record
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from test_frontend_cpu import same_pileup
from test_gpu_bamfull import EXTRA, accepted_records, run_module, two_refs, write_text  # noqa: F401  (two_refs is a fixture)
from test_gpu_dirty_memory import POISON

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE, E_UNSUPPORTED = -1, -2, -4
REFS = bm.REFS
LEAN_KEYS = ("tid", "pos", "cigar", "seq", "name", "flag", "mapq")


def device_error(e, what):
    """nothing more may run on a device that has reported an error: the session ends here"""
    pytest.exit(f"device error in {what}: {e}", returncode=3)


@pytest.fixture(scope="module")
def pol():
    p = Polisher([])
    yield p
    p.close()


def synthetic(n=60, seed=5):
    """a mapping on two references: records of about 100 to 300 bytes, decorated with qualities, mates and tags, some unmapped"""
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        l = rng.randrange(40, 121)
        recs.append(bm.rec(rng.randrange(2), rng.randrange(1, 4000), [("S", 3), ("M", l - 10), ("I", 2), ("M", 5)], l_seq=l, name=b"read%d" % i,
                           flag=rng.choice([0, 16, 0, 2048]), mapq=rng.randrange(61), seed=i))
    fm.decorate(recs, REFS, 3)
    recs[7]["flag"] |= 4
    recs[23]["tid"] = -1
    recs[23].pop("rnext", None)
    return recs


def write_bam(path, recs, extras=EXTRA, refs=REFS, **kw):
    """-> the inflated stream"""
    s = im.inflated(refs, recs, extras)
    with open(path, "wb") as f:
        f.write(im.bgzf(s, **kw))
    return s


def device(pol, paths, tie="strand", keep_all=True, out=None, what="BAM input"):
    """io.Sam over `paths` -> dict: the written files' bytes (when `out`), every export, the stats"""
    try:
        sam = np2io.Sam(pol, [str(p) for p in paths], tie=tie, keep_names=True, keep_all=keep_all)
        try:
            r = dict(stats=sam.stats(), bamin=sam.bamin_stats(), refs=sam.refs())
            r["recs"], r["tids"], r["cigar"], r["seq4"] = sam.export(pol)
            r["names"], r["name_ref"] = sam.export_names(pol)
            if keep_all:
                r["tails"], r["tail_ref"] = sam.export_tails(pol)
                r["header"] = sam.header_text()
            if out:
                r["out"] = sam.write_bam(pol, str(out))
                r["bam"], r["bai"] = open(out, "rb").read(), open(str(out) + ".bai", "rb").read()
        finally:
            sam.close()
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(e, what)
        raise
    return r


def same_handle(a, b, what=""):
    """two device() results hold the same bytes (SEQ, names and tails lie as the records were met: equal input orders)"""
    for k in ("bam", "bai", "header", "refs"):
        assert a.get(k) == b.get(k), (what, k)
    for k in ("recs", "tids", "cigar", "seq4", "names", "name_ref", "tails", "tail_ref"):
        assert (k in a) == (k in b) and (k not in a or a[k].tobytes() == b[k].tobytes()), (what, k)
    for k in ("records", "unmapped", "kept", "cigar_words", "seq_bytes"):
        assert a["stats"][k] == b["stats"][k], (what, k)


def contents(r, full):
    """per record what it holds, whatever the offsets: for a device() result or a twin / model dict"""
    out = []
    for i in range(len(r["recs"])):
        x = r["recs"][i]
        c0, s0, nr = int(x["cigar_off"]), int(x["seq_off"]), int(r["name_ref"][i])
        item = [int(x["pos"]), int(x["flag"]), int(x["mapq"]), int(r["tids"][i]), r["cigar"][c0:c0 + int(x["n_cigar"])].tobytes(),
                r["seq4"][s0:s0 + (int(x["l_seq"]) + 1) // 2].tobytes(), r["names"][nr >> 8:(nr >> 8) + (nr & 255)].tobytes()]
        if full:
            t0, hq = int(r["tail_ref"][i]) >> 1, int(r["tail_ref"][i]) & 1
            aux_len, = struct.unpack_from("<I", r["tails"].tobytes(), t0 + 12)
            item += [hq, r["tails"][t0:t0 + 16 + hq * int(x["l_seq"]) + aux_len].tobytes()]
        out.append(tuple(item))
    return out


def three_way(dev, stream, tie="strand", full=True, what=""):
    """the device's handle == the host twin == the model, record by record in the sorted order"""
    host, model = np2io.bamin_host(stream, keep_names=True, keep_all=full, tie=tie), im.decode(stream, keep_names=True, keep_all=full)
    im.same(host, model, what)
    assert host["code"] == 0
    h = contents(host, full)
    key = lambda j: (int(host["tids"][j]), int(host["recs"][j]["pos"]) + 1, (int(host["recs"][j]["flag"]) >> 4) & 1 if tie == "strand" else 0)
    order = sorted(range(len(h)), key=key)
    assert contents(dev, full) == [h[j] for j in order], what
    assert dev["stats"]["records"] == len(host["status"]) and dev["stats"]["kept"] == len(h)


# ---- 1. the central equality -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def central(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamin")
    given = accepted_records() + synthetic()
    random.Random(11).shuffle(given)
    lean = [{k: r[k] for k in LEAN_KEYS} for r in given]
    T, TL = write_text(tmp / "t.sam", REFS, given, extra=EXTRA), write_text(tmp / "tl.sam", REFS, lean, extra=EXTRA)
    stream = write_bam(tmp / "b.bam", given)
    lean_stream = write_bam(tmp / "bl.bam", lean)
    return dict(tmp=tmp, given=given, T=T, TL=TL, B=str(tmp / "b.bam"), BL=str(tmp / "bl.bam"), stream=stream, lean_stream=lean_stream)


@pytest.mark.parametrize("tie", ["strand", "input"])
def test_an_unsorted_bam_gives_what_its_sam_text_gives(pol, central, tie):
    tmp = central["tmp"]
    text = device(pol, [central["T"]], tie=tie, out=tmp / "t.out.bam")
    bam = device(pol, [central["B"]], tie=tie, out=tmp / "b.out.bam")
    same_handle(bam, text, "full")
    three_way(bam, central["stream"], tie, True, "full")
    assert bam["bamin"]["files"] == 1 and bam["bamin"]["records"] == len(central["given"]) == bam["stats"]["records"]
    assert bam["bamin"]["inflated_bytes"] > 0 and text["bamin"]["files"] == 0
    same_handle(device(pol, [central["B"]], tie=tie, keep_all=False, out=tmp / "b.lean.bam"),
                device(pol, [central["T"]], tie=tie, keep_all=False, out=tmp / "t.lean.bam"), "lean from the full BAM")
    lean = device(pol, [central["BL"]], tie=tie, out=tmp / "bl.out.bam")
    same_handle(lean, device(pol, [central["TL"]], tie=tie, out=tmp / "tl.out.bam"), "full from a lean BAM")
    three_way(lean, central["lean_stream"], tie, True, "full from a lean BAM")
    if tie == "strand":
        fm.check_files(REFS, fm.sort_records(central["given"]), bam["bam"], bam["bai"], [EXTRA], "model")


# ---- 2. block cuts --------------------------------------------------------------------------------------------------------------
PARTS = ("block_size", "fixed", "name", "cigar", "seq", "qual", "tags")


def parts_split(stream, bounds):
    """which parts of some record does one of the stream offsets `bounds` fall into (strictly inside)?"""
    _, at = im.header_end(stream)
    hit, bounds = set(), sorted(bounds)
    while at < len(stream):
        bs, = struct.unpack_from("<I", stream, at)
        l_name, n_cig, l_seq = stream[at + 12], struct.unpack_from("<H", stream, at + 16)[0], struct.unpack_from("<I", stream, at + 20)[0]
        edges = [0, 4, 36, 36 + l_name, 36 + l_name + 4 * n_cig, 36 + l_name + 4 * n_cig + (l_seq + 1) // 2]
        edges += [edges[-1] + l_seq, 4 + bs]
        for name, a, b in zip(PARTS, edges, edges[1:]):
            if any(at + a < x < at + b for x in bounds):
                hit.add(name)
        at += 4 + bs
    return hit


@pytest.fixture(scope="module")
def sixty(tmp_path_factory, pol):
    tmp = tmp_path_factory.mktemp("bamin60")
    given = synthetic(60, seed=9)
    stream = write_bam(tmp / "whole.bam", given)
    want = device(pol, [write_text(tmp / "t.sam", REFS, given, extra=EXTRA)], out=tmp / "t.out.bam")
    return tmp, given, stream, want


SPLITS_SEEN = {}


@pytest.mark.parametrize("cut", [1, 3, 7, 64, 255, 4099])
def test_blocks_cut_through_every_part_of_a_record(pol, sixty, cut):
    tmp, given, stream, want = sixty
    assert 55 <= len(given) <= 65 and 6000 < len(stream) < 25000
    write_bam(tmp / f"cut{cut}.bam", given, cut=cut)
    SPLITS_SEEN[cut] = parts_split(stream, im.block_bounds(len(stream), cut))
    assert SPLITS_SEEN[cut] and (cut > 64 or SPLITS_SEEN[cut] == set(PARTS)), (cut, SPLITS_SEEN[cut])
    got = device(pol, [tmp / f"cut{cut}.bam"], out=tmp / f"cut{cut}.out.bam")
    same_handle(got, want, cut)
    assert got["bamin"]["blocks"] >= (len(stream) - im.header_end(stream)[1]) // cut  # (counted from the block in which the header ends)
    if cut == 4099:  # (the last of the cuts)
        assert set().union(*SPLITS_SEEN.values()) == set(PARTS)


# ---- 3. pieces -------------------------------------------------------------------------------------------------------------------
def sized(size, i):
    """a record of exactly `size` bytes (block_size word included; at least 57): block_size [0, 4), the fixed fields [4, 36), the
    name [36, 40), one CIGAR word [40, 44), SEQ [44, 47), qualities [47, 53), and a Z tag that fills the rest"""
    kw = dict(name=b"%03d\0" % i, pos=10 + (i * 37) % 900, tid=i % 2, cigar=((0, 6),), seq=bytes([0x12 + i % 7, 0x48, 0x81]), l_seq=6,
              qual=bytes([i % 90, 1, 2, 93, 0, 7]) if i % 3 else None, flag=16 * (i % 2))
    fill = size - len(raw_record(aux=b"XZZ\0", **kw))
    assert fill >= 0, (size, i)
    return raw_record(aux=b"XZZ" + bytes(65 + (i + j) % 26 for j in range(fill)) + b"\0", **kw)


PIECE_CUT = 17
TARGETS = (2, 20, 38, 42, 45, 50, 55)  # an offset inside each part of a record of sized()


def piece_records(piece):
    """records of 57 .. piece bytes laid out so that a piece's end falls into each part of some record: pieces hold
    piece // PIECE_CUT blocks of PIECE_CUT bytes, from the block in which the header ends; one record is one byte short of a piece"""
    rng = random.Random(piece)
    head = len(fm.header(REFS, [EXTRA]))
    per, first = piece // PIECE_CUT * PIECE_CUT, head // PIECE_CUT * PIECE_CUT
    recs, at, t = [sized(piece - 1, 0)], head + piece - 1, 0
    while t < 2 * len(TARGETS) or len(recs) < 40:
        k = (at - first) // per + 1
        for kk in range(k, k + 30):
            gap = first + kk * per - TARGETS[t % len(TARGETS)] - at
            if gap == 0 or 57 <= gap <= piece:
                if gap:
                    recs.append(sized(gap, len(recs)))
                at, t = at + gap, t + 1
                break
        size = rng.randrange(57, piece)
        recs.append(sized(size, len(recs)))
        at += size
    return recs


@pytest.mark.parametrize("piece", [64, 257, 4096])
def test_records_straddle_pieces_at_every_part(pol, tmp_path, monkeypatch, piece):
    recs, cut = piece_records(piece), PIECE_CUT
    stream = write_bam(tmp_path / "p.bam", recs, cut=cut)
    write_bam(tmp_path / "p_empty.bam", recs, cut=cut, empty_after=len(stream) // cut // 2)
    write_bam(tmp_path / "p_noeof.bam", recs, cut=cut, eof=False)
    want = device(pol, [tmp_path / "p.bam"], out=tmp_path / "one.bam")  # one piece
    three_way(want, stream, what=("one piece", piece))
    per = piece // cut * cut  # the inflated bytes of a piece: whole blocks, from the block in which the header ends
    first = im.header_end(stream)[1] // cut * cut
    assert parts_split(stream, range(first + per, len(stream), per)) == set(PARTS)
    monkeypatch.setenv("NP2_SAM_TEST_PIECE", str(piece))
    for name in ("p", "p_empty", "p_noeof"):
        got = device(pol, [tmp_path / f"{name}.bam"], out=tmp_path / f"{name}.out.bam")
        same_handle(got, want, (name, piece))
    # one byte too long for a piece
    write_bam(tmp_path / "long.bam", recs[:5] + [sized(piece + 1, 99)] + recs[5:], cut=cut)
    with pytest.raises(Np2Error) as e:
        device(pol, [tmp_path / "long.bam"])
    assert e.value.code == E_UNSUPPORTED and "long.bam: record 5: " in str(e.value) and "does not fit a piece" in str(e.value), str(e.value)
    same_handle(device(pol, [tmp_path / "p.bam"], out=tmp_path / "again.bam"), want, "after the refusal")


# ---- 4. several inputs -----------------------------------------------------------------------------------------------------------
def test_bam_and_sam_inputs_mix(pol, tmp_path):
    given = synthetic(45, seed=21)
    a, b, c = given[:15], given[15:30], given[30:]
    write_bam(tmp_path / "a.bam", a, cut=999)
    write_text(tmp_path / "b.sam", REFS, b, extra=EXTRA)
    write_bam(tmp_path / "c.bam", c, cut=77, eof=False)
    got = device(pol, [tmp_path / "a.bam", tmp_path / "b.sam", tmp_path / "c.bam"], out=tmp_path / "mixed.bam")
    want = device(pol, [write_text(tmp_path / "all.sam", REFS, given, extra=EXTRA)], out=tmp_path / "all.bam")
    same_handle(got, want, "BAM + SAM + BAM")
    assert got["bamin"]["files"] == 2 and got["bamin"]["records"] == 30 and got["stats"]["lines"] == want["stats"]["lines"]
    # references that differ, in either kind of file
    other = [REFS[0], (REFS[1][0], REFS[1][1] + 1)] + REFS[2:]
    write_bam(tmp_path / "other.bam", c, refs=other)
    for paths in ([tmp_path / "a.bam", tmp_path / "other.bam"], [tmp_path / "b.sam", tmp_path / "other.bam"]):
        with pytest.raises(Np2Error) as e:
            device(pol, paths)
        assert e.value.code == E_ARG and "other.bam: its @SQ lines differ from those of the first file" in str(e.value)
    # a BAM on standard input
    with open(tmp_path / "a.bam", "rb") as f:
        r = run_module("samsort", ["-", "-o", str(tmp_path / "stdin.bam")], stdin=f)
    assert r.returncode != 0 and b"is a BAM" in r.stderr and b"standard input" in r.stderr and not os.path.exists(tmp_path / "stdin.bam"), r.stderr[-2000:]


# ---- 5. integrity ----------------------------------------------------------------------------------------------------------------
def test_damaged_files_are_refused_and_the_next_one_opens(pol, tmp_path):
    given = synthetic(30, seed=31)
    stream = write_bam(tmp_path / "good.bam", given, cut=1500, level=0)  # stored blocks
    want = device(pol, [tmp_path / "good.bam"], out=tmp_path / "good.out.bam")
    raw = bytearray(open(tmp_path / "good.bam", "rb").read())
    off = 0
    for _ in range(3):  # the fourth block
        off += struct.unpack_from("<H", raw, off + 16)[0] + 1
    raw[off + 18 + 5 + 700] ^= 0x10  # one payload bit of the fourth block (18 header bytes, 5 of the stored block's own)
    open(tmp_path / "flip.bam", "wb").write(raw)
    cases = [("flip.bam", f"BGZF CRC32 mismatch (block at file offset {off})")]
    last = len(fm.encode(REFS, given[-1]))
    open(tmp_path / "trunc.bam", "wb").write(im.bgzf(stream[:-last // 2], cut=1500))
    cases.append(("trunc.bam", f"record {len(given) - 1}: truncated BAM"))
    open(tmp_path / "garbage.bam", "wb").write(im.bgzf(stream + b"\x07\x00\x00", cut=1500))
    cases.append(("garbage.bam", f"record {len(given)}: fewer than 4 bytes behind the last record: not a record"))
    open(tmp_path / "zeros.bam", "wb").write(im.bgzf(stream + b"\0" * 40, cut=1500))
    cases.append(("zeros.bam", f"record {len(given)}: block_size is below 32: not a record"))
    for name, words in cases:
        with pytest.raises(Np2Error) as e:
            device(pol, [tmp_path / name])
        assert e.value.code == E_ARG and name + ": " in str(e.value) and words in str(e.value), (name, str(e.value))
        same_handle(device(pol, [tmp_path / "good.bam"], out=tmp_path / "after.bam"), want, "after " + name)


# ---- 6. the project's readers on a handle opened from an unsorted BAM -------------------------------------------------------------
@pytest.fixture(scope="module")
def unsorted_bam(two_refs):
    _, refs, given, _, tmp = two_refs
    path = str(tmp / "unsorted.bam")
    write_bam(path, given, refs=refs, cut=30011)
    out = str(tmp / "from_bam.sort.bam")
    r = run_module("samsort", [path, "-o", out, "--full"])
    assert r.returncode == 0 and b"[samsort] full BAM" in r.stderr and b"1 of 1 inputs were BAM" in r.stderr, r.stderr.decode()[-3000:]
    fm.check_files(refs, fm.sort_records(given), open(out, "rb").read(), open(out + ".bai", "rb").read(), [EXTRA], "samsort --full of a BAM")
    lean = str(tmp / "from_bam.lean.bam")
    r = run_module("samsort", [path, "-o", lean])
    assert r.returncode == 0 and b"[samsort] lean BAM" in r.stderr, r.stderr.decode()[-3000:]
    bm.check_files(refs, fm.sort_records(given), open(lean, "rb").read(), open(lean + ".bai", "rb").read(), "samsort of a BAM")
    return path, out, lean


@pytest.mark.parametrize("mode", ["gpu", "host"])
def test_a_handle_from_an_unsorted_bam_gives_the_pileup_of_the_sorted_file(pol, two_refs, unsorted_bam, monkeypatch, mode):
    synths, refs, _, _, _ = two_refs
    monkeypatch.setenv("NP2_INFLATE", mode)  # (read at every fetch)
    sam, bam = np2io.Sam(pol, [unsorted_bam[0]]), np2io.Bam(unsorted_bam[1])
    assert sam.refs() == refs == bam.refs()
    for (name, _), s in zip(refs, synths):
        ref = s.pileup.ref
        want = np2io.export_contig(pol, np2io.contig_from_bam(pol, bam, name, ref.tobytes()), ref)
        got = np2io.export_contig(pol, np2io.contig_from_sam(pol, sam, name, ref.tobytes()), ref)
        assert len(want.reads) > 10 and same_pileup(got, want), (name, mode)
    sam.close(), bam.close()


def test_lowdepth_and_cli_on_an_unsorted_bam(two_refs, unsorted_bam):
    from test_oracle import yak_from_seqs
    synths, refs, _, sam_text, tmp = two_refs
    fa = tmp / "genome_bamin.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s.pileup.ref.tobytes()) for (n, _), s in zip(refs, synths)))
    outs = []
    for bam in unsorted_bam[1:]:
        r = run_module("lowdepth", [bam, str(fa), "-d", "12", "-l", "500", "--bed", bam + ".bed"])
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        outs.append((r.stdout, open(bam + ".bed", "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].count(b">") >= 1
    haps = [synths[0].hap1.decode(), synths[0].hap2.decode(), synths[1].hap1.decode()]
    np2io.write_yak(str(tmp / "bi21.yak"), yak_from_seqs(haps, 21))
    np2io.write_yak(str(tmp / "bi31.yak"), yak_from_seqs(haps, 31))
    rest = [str(fa), str(tmp / "bi21.yak"), str(tmp / "bi31.yak")]
    # refused before any work, without a device
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1")
    cli = [sys.executable, "-m", "nextpolish2_amd.cli", "-L", "10000"]
    r = subprocess.run(cli + [unsorted_bam[0], "--bam_unsorted", "-S"] + rest, capture_output=True, env=env, timeout=120)
    assert r.returncode != 0 and b"-S needs the SEQ of a read's primary record" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(cli + [unsorted_bam[0], "--bam_unsorted"] + rest, capture_output=True, env=dict(env, WORLD_SIZE="2", RANK="0"), timeout=120)
    assert r.returncode != 0 and b"runs on one rank" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(cli + [unsorted_bam[0], "--sorted_bam", str(tmp / "no.bam")] + rest, capture_output=True, env=env, timeout=120)
    assert r.returncode != 0 and b"the mapping given is a BAM already" in r.stderr, r.stderr[-2000:]  # without the flag nothing changes
    want = run_module("cli", ["-L", "10000", unsorted_bam[1]] + rest)
    assert want.returncode == 0 and want.stdout.count(b">") == 2, want.stderr.decode()[-3000:]
    kept = str(tmp / "kept_from_bam.bam")
    got = run_module("cli", ["-L", "10000", unsorted_bam[0], "--bam_unsorted", "--sam_tie", "strand", "--sorted_bam", kept, "--sorted_bam_full"] + rest)
    assert got.returncode == 0, got.stderr.decode()[-3000:]
    assert got.stdout == want.stdout
    for ext in ("", ".bai"):
        assert open(kept + ext, "rb").read() == open(unsorted_bam[1] + ext, "rb").read()


# ---- 7. recycled memory: the scheme of test_gpu_dirty_memory.py -------------------------------------------------------------------
_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import test_gpu_bamin as t\n"
                "from nextpolish2_amd import Polisher, api\n"
                "byte, out = int(sys.argv[1]), sys.argv[2]\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        p = Polisher([])\n"
                "        for i, k in enumerate('ABA'):\n"
                "            r = t.device(p, ['%%s.%%s.bam' %% (out, k)], out='%%s.%%d.bam' %% (out, i))\n"
                "            open('%%s.%%d.tails' %% (out, i), 'wb').write(r['tails'].tobytes())\n"
                "        p.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, os.path.join(ROOT, "tests")))


def test_on_poisoned_recycled_blocks(tmp_path):
    """the central equality once, a small input A, a larger B and A again on one context, every pool block filled with a byte
    before it is handed out: the files equal the model's, the padding between the tails included"""
    byte = POISON[0]
    a = synthetic(25, seed=41)
    inputs = {"A": a, "B": accepted_records() + a}
    out = str(tmp_path / "w")
    for k, v in inputs.items():
        write_bam(f"{out}.{k}.bam", v, cut=4099)
    env = dict(os.environ, PYTHONPATH=ROOT, NP2_BGZF_TEST_BATCH="2", NP2_SAM_TEST_PIECE=str(1 << 16))
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte), out], capture_output=True, env=env, timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        device_error(r.stderr.decode(errors="replace")[-2000:], f"BAM input under poison {byte:#x}")
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    outs = []
    for i, k in enumerate("ABA"):
        tails, bam, bai = (open(f"{out}.{i}.{e}", "rb").read() for e in ("tails", "bam", "bam.bai"))
        given = [r for r in inputs[k] if r["tid"] >= 0 and not r.get("flag", 0) & 4]
        fm.check_files(REFS, fm.sort_records(given), bam, bai, [EXTRA], (k, byte))
        assert tails == fm.tails(REFS, given, range(len(given)))[0].tobytes()
        outs.append((tails, bam, bai))
    assert outs[0] == outs[2]
