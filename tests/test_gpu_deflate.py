"""BGZF output on the device (csrc/np2_deflate.hip: k_bgzf_deflate, one wavefront per block) against its host twin
(np2_bgzf_deflate_host, the same core on the CPU, which tests/test_deflate_cpu.py checks against zlib field by field): the
kernel's bytes are the twin's, the project's own inflater reads them back, the writer cuts the same blocks whatever the
sizes of the writes and survives dirty buffers, and the command lines' .gz outputs gunzip to their plain outputs."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import deflate_cases as dc
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.synth import Synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV = dict(os.environ, PYTHONPATH=ROOT)
E_DEVICE = -2
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
REF_PAIRS = [os.path.join(HERE, "golden", "ref_pairs", f"sr.{r}.2000.fastq.gz") for r in ("R1", "R2")]


def device_error(what, e):
    """Nothing more may run on a device that has reported an error: the session ends here."""
    pytest.exit(f"device error in {what}: {e}", returncode=3)


def guarded(what, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(what, e)
        raise


def run_cli(what, args, env=ENV):
    r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    if r.returncode < 0 or "hipError" in err or "HSA_STATUS" in err or "illegal memory access" in err:
        device_error(what, err[-2000:])
    assert r.returncode == 0, err[-3000:]
    return r


@pytest.fixture(scope="module")
def pol():
    p = Polisher([Synth(2000, seed=3).yak(21)])
    yield p
    p.close()


@pytest.fixture(scope="module")
def twin():
    """the host twin's stream of every case, computed once"""
    t = {("block", name): np2io.bgzf_deflate_host(b) for name, b in dc.blocks()}
    t.update({("stream", name): np2io.bgzf_deflate_host(b, bb) for name, b, bb in dc.streams()})
    return t


# ---- 1, 2. the kernel's bytes are the twin's, and the project's inflater reads them back ------------------------------------------
def test_device_stream_equals_the_twin_and_inflates_on_the_device(pol, twin):
    cases = [("block", name, b, 0) for name, b in dc.blocks()] + [("stream", name, b, bb) for name, b, bb in dc.streams()]
    for kind, name, b, bb in cases:
        z, ms = guarded(name, np2io.bgzf_deflate_device, pol, b, bb)
        assert ms >= 0
        assert z == twin[(kind, name)], (kind, name, len(z), len(twin[(kind, name)]))
        back, _ = guarded(name, np2io.bgzf_inflate_device, pol, z)
        assert back.tobytes() == b, (kind, name)


def test_device_argument_errors(pol):
    with pytest.raises(Np2Error) as e:
        np2io.bgzf_deflate_device(pol, b"abc", 65281)
    assert e.value.code == -1 and "65280" in str(e.value)
    L = np2io._bind()
    import ctypes as C
    src, out, n = np.frombuffer(b"ACGT" * 100, np.uint8), np.empty(40, np.uint8), C.c_uint64()
    rc = L.np2_bgzf_deflate_device(pol._h, src.ctypes.data, len(src), 0, out.ctypes.data, len(out), C.byref(n), None)
    want = len(np2io.bgzf_deflate_host(src))
    assert rc == -1 and n.value == want and str(want) in L.np2_io_last_error().decode()


# ---- 3. the writer ------------------------------------------------------------------------------------------------------------------
def write_in_pieces(path, data, sizes=(1, 7, 65279, 65281, 1000000)):
    w = np2io.BgzfWriter(path)
    at, i = 0, 0
    while at < len(data):
        n = sizes[i % len(sizes)]
        w.write(data[at:at + n])
        at, i = at + n, i + 1
    w.close()
    return w


def test_writer_cuts_the_twins_blocks_whatever_the_writes(tmp_path, monkeypatch):
    monkeypatch.setenv("NP2_BGZF_TEST_BATCH", "3")  # 3 MB are 48 blocks: sixteen batches, both buffers many times over
    data = dc.corpus_bytes(3_000_000)
    path = str(tmp_path / "w.gz")
    w = guarded("writer", write_in_pieces, path, data)
    z = open(path, "rb").read()
    with gzip.open(path, "rb") as f:
        assert f.read() == data
    assert z == np2io.bgzf_deflate_host(data)
    assert z[-28:] == dc.EOF_BLOCK
    assert (w.bytes_in, w.bytes_out) == (len(data), len(z)) and w.kernel_ms > 0
    # nothing written: the EOF block alone
    empty = str(tmp_path / "e.bgz")
    with np2io.BgzfWriter(empty) as w0:
        pass
    assert open(empty, "rb").read() == dc.EOF_BLOCK and (w0.bytes_in, w0.bytes_out) == (0, 28)
    # a file that cannot be opened
    with pytest.raises(Np2Error) as e:
        np2io.BgzfWriter(str(tmp_path / "no_such_dir" / "x.gz"))
    assert e.value.code == -1 and "cannot open" in str(e.value)


# ---- 4. dirty memory ------------------------------------------------------------------------------------------------------------------
_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import deflate_cases as dc\n"
                "from nextpolish2_amd import api\n"
                "from nextpolish2_amd import io as np2io\n"
                "byte, out = int(sys.argv[1]), sys.argv[2]\n"
                "a, b = dc.corpus_bytes(3_000_000)[1_000_000:1_100_000], dc.corpus_bytes(2_000_000)\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        for i, data in enumerate((a, b, a)):\n"
                "            w = np2io.BgzfWriter('%%s.%%d.gz' %% (out, i))\n"
                "            for at in range(0, len(data), 300007):\n"
                "                w.write(data[at:at + 300007])\n"
                "            w.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, HERE))


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0xA5])
def test_writer_on_poisoned_recycled_buffers(tmp_path, byte):
    """A (100 KB), B (2 MB), A again on fresh writers of one process: the second A runs in blocks B left dirty (the pools
    hand a writer's buffers to the next), and every block the pools hand out is filled with `byte` first.  (A process of
    its own: the hook's counters are the process's, and tests/test_gpu_dirty_memory.py reads them.)"""
    out = str(tmp_path / "w")
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte), out], capture_output=True, env=ENV, timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        device_error(f"writer under poison {byte:#x}", r.stderr.decode(errors="replace")[-2000:])
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    a, b = dc.corpus_bytes(3_000_000)[1_000_000:1_100_000], dc.corpus_bytes(2_000_000)
    za, zb, za2 = (open(f"{out}.{i}.gz", "rb").read() for i in range(3))
    assert za == za2 == np2io.bgzf_deflate_host(a)
    assert zb == np2io.bgzf_deflate_host(b)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def test_srqc_out_gz_gunzips_to_the_plain_outputs(tmp_path):
    plain, packed = str(tmp_path / "p"), str(tmp_path / "z")
    run_cli("srqc", ["nextpolish2_amd.srqc"] + REF_PAIRS + ["--out_fq", plain, "--report", str(tmp_path / "p.tsv")])
    run_cli("srqc --out_gz", ["nextpolish2_amd.srqc"] + REF_PAIRS + ["--out_fq", packed, "--out_gz", "--report", str(tmp_path / "z.tsv")])
    for i in range(2):
        want = open(f"{plain}.{i}.fq", "rb").read()
        z = open(f"{packed}.{i}.fq.gz", "rb").read()
        assert len(want) > 100000 and z[-28:] == dc.EOF_BLOCK and z == np2io.bgzf_deflate_host(want)
        assert gzip.decompress(z) == want
    assert open(str(tmp_path / "p.tsv")).read() == open(str(tmp_path / "z.tsv")).read()


def test_cli_out_fa_gz_gunzips_to_the_plain_fasta_and_qv_reads_it(tmp_path):
    asm = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
    front = ["nextpolish2_amd.cli", "-t", "5", "-L", "1000", os.path.join(BUNDLE, "hifi.map.sort.bam"), asm, os.path.join(BUNDLE, "k21.yak"),
             os.path.join(BUNDLE, "k31.yak")]
    plain, packed = str(tmp_path / "out.fa"), str(tmp_path / "out.fa.gz")
    run_cli("cli -o out.fa", front + ["-o", plain])
    run_cli("cli -o out.fa.gz", front + ["-o", packed])
    want = open(plain, "rb").read()
    assert want == gzip.open(os.path.join(BUNDLE, "expected.fa.gz"), "rb").read()
    z = open(packed, "rb").read()
    assert gzip.decompress(z) == want and z == np2io.bgzf_deflate_host(want)
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli"] + front[1:] + ["-o", packed], capture_output=True, env=ENV, timeout=300)
    assert r.returncode != 0 and b"already exists" in r.stderr and open(packed, "rb").read() == z  # the refusal to overwrite stays
    qv = [run_cli("qv", ["nextpolish2_amd.qv", f, os.path.join(BUNDLE, "k21.yak")]).stdout for f in (plain, packed)]
    assert qv[0] == qv[1] and qv[0].count(b"\n") >= 2


def test_triobin_bins_gz_gunzip_to_the_plain_bins(tmp_path):
    from test_gpu_trio import parent_yak
    s = Synth(30000, depth=10, seed=11, diploid=True, read_len_mean=5000.0, read_len_sd=800.0)
    dumps = []
    for name, hap in (("pat", s.hap1), ("mat", s.hap2)):
        dumps.append(str(tmp_path / f"{name}.yak"))
        np2io.write_yak(dumps[-1], parent_yak(hap, 21))
    rng = np.random.default_rng(5)
    reads = [(s.hap1 if i % 2 else s.hap2)[a:a + 3000] for i, a in enumerate(rng.integers(0, 20000, 9))]
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))
    outs = {}
    for tag, ext in (("plain", ""), ("packed", ".gz")):
        outs[tag] = [str(tmp_path / f"{tag}.{side}.fa{ext}") for side in ("pat", "mat")]
        run_cli("triobin", ["nextpolish2_amd.triobin"] + dumps + [fa, "-o", str(tmp_path / f"{tag}.tsv"), "--pat_fa", outs[tag][0], "--mat_fa", outs[tag][1]])
    for p, z in zip(outs["plain"], outs["packed"]):
        want = open(p, "rb").read()
        assert len(want) > 3000 and gzip.decompress(open(z, "rb").read()) == want
        assert open(z, "rb").read() == np2io.bgzf_deflate_host(want)
    assert open(str(tmp_path / "plain.tsv"), "rb").read() == open(str(tmp_path / "packed.tsv"), "rb").read()


def test_lowdepth_out_gz_gunzips_to_the_plain_fasta(tmp_path):
    asm = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")
    front = ["nextpolish2_amd.lowdepth", os.path.join(BUNDLE, "hifi.map.sort.bam"), asm, "-d", "1", "-l", "100"]
    plain, packed = str(tmp_path / "f.fa"), str(tmp_path / "f.fa.bgz")
    to_stdout = run_cli("lowdepth", front).stdout
    run_cli("lowdepth -o f.fa", front + ["-o", plain])
    run_cli("lowdepth -o f.fa.bgz", front + ["-o", packed])
    want = open(plain, "rb").read()
    assert len(want) > 50000 and want == to_stdout  # (standard output stays plain)
    z = open(packed, "rb").read()
    assert gzip.decompress(z) == want and z == np2io.bgzf_deflate_host(want)
