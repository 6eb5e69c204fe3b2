#!/usr/bin/env python3
"""Cost of the BGZF deflate kernel (csrc/np2_deflate.hip); the figures of profiles/deflate_cost.txt come from here.

    python tools/deflate_probe.py [--mb 2.0 --cov 60] [--out profiles/deflate_cost.txt]

Two inputs: the 66 196 test reads of tests/golden/ref_bundle/sr.seq.*.gz as FASTQ text (the fixture holds their bases; the
header is @read<i> and the quality line that of read i mod 2000 of tests/golden/ref_pairs, cut or repeated to the read's
length), and the simulated 150-base reads of tools/kcount_probe.py's `sim` (one read a line).  Per input:
  - k_bgzf_deflate by HIP events (np2_bgzf_deflate_device's kernel_ms, the best of three) and GB/s of input;
  - k_bgzf_inflate by HIP events on the stream the deflater just wrote, GB/s of inflated bytes;
  - zlib level 1 on one host thread over the same 65280-byte blocks;
  - the compressed size against zlib levels 1 and 6 on those blocks.
Then the wall time of `python -m nextpolish2_amd.srqc --out_fq` on the FASTQ text with and without --out_gz (fresh
processes, the best of three), and the size ratios of the two test fixtures the CPU test holds to 1.05 x zlib level 1."""
import argparse
import gzip
import importlib.util
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import Polisher  # noqa: E402
from nextpolish2_amd import io as np2io  # noqa: E402
from nextpolish2_amd.synth import Synth  # noqa: E402

BLOCK = 65280
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fastq_of_the_test_reads():
    quals = [q for q in gzip.open(os.path.join(GOLDEN, "ref_pairs", "sr.R1.2000.fastq.gz"), "rb").read().split(b"\n")[3::4]]
    out, i = [], 0
    for f in range(3):
        for seq in gzip.open(os.path.join(GOLDEN, "ref_bundle", f"sr.seq.{f}.gz"), "rb").read().split():
            q = quals[i % len(quals)]
            q = (q * (len(seq) // len(q) + 1))[:len(seq)]
            out.append(b"@read%d\n%s\n+\n%s\n" % (i, seq, q))
            i += 1
    return b"".join(out), i


def zlib_blocks(data, level):
    t0, n = time.perf_counter(), 0
    for at in range(0, len(data), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += len(c.compress(data[at:at + BLOCK]) + c.flush())
    return n, time.perf_counter() - t0


def measure(pol, label, data, say):
    n_blk = (len(data) + BLOCK - 1) // BLOCK
    best, z = None, None
    for _ in range(3):
        z, ms = np2io.bgzf_deflate_device(pol, data)
        best = ms if best is None else min(best, ms)
    ours = len(z) - 26 * n_blk - 28
    ibest = None
    for _ in range(3):
        back, ims = np2io.bgzf_inflate_device(pol, z)
        ibest = ims if ibest is None else min(ibest, ims)
    assert back.tobytes() == data
    z1, t1 = zlib_blocks(data, 1)
    z6, t6 = zlib_blocks(data, 6)
    say(f"{label}: {len(data) / 1e6:.1f} MB in {n_blk} blocks")
    say(f"  k_bgzf_deflate {best:.2f} ms = {len(data) / best / 1e6:.2f} GB/s of input")
    say(f"  k_bgzf_inflate on that stream {ibest:.2f} ms = {len(data) / ibest / 1e6:.2f} GB/s inflated")
    say(f"  zlib level 1, one host thread, the same blocks: {t1:.2f} s = {len(data) / t1 / 1e6:.1f} MB/s (level 6: {len(data) / t6 / 1e6:.1f} MB/s)")
    say(f"  DEFLATE bytes: device {ours} ({ours / len(data):.3f} of the input), zlib 1 {z1} (device / zlib 1 = {ours / z1:.3f}), "
        f"zlib 6 {z6} (device / zlib 6 = {ours / z6:.3f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=2.0)
    ap.add_argument("--cov", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_cost.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("BGZF deflate on the device: tools/deflate_probe.py " + " ".join(sys.argv[1:]))
    pol = Polisher([Synth(2000, seed=3).yak(21)])
    fq, n_reads = fastq_of_the_test_reads()
    measure(pol, f"the {n_reads} test reads as FASTQ text", fq, say)
    spec = importlib.util.spec_from_file_location("kcount_probe", os.path.join(ROOT, "tools", "kcount_probe.py"))
    kp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kp)
    with tempfile.TemporaryDirectory() as td:
        plain, _ = kp.simulate(a.mb, a.cov, 1, td)
        sim = open(plain[0], "rb").read()
        measure(pol, f"simulated 150-base reads ({a.mb} Mb x {a.cov}), one a line", sim, say)
        del sim
        pol.close()
        src = os.path.join(td, "reads.fq")
        open(src, "wb").write(fq)
        for tag, extra in (("plain", []), ("--out_gz", ["--out_gz"])):
            walls = []
            for rep in range(3):
                prefix = os.path.join(td, f"o.{tag.strip('-')}.{rep}")
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.srqc", src, "--out_fq", prefix, "--report", prefix + ".tsv"] + extra,
                                   capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
                walls.append(time.perf_counter() - t0)
                if r.returncode:
                    say(f"srqc {tag} failed: {r.stderr[-500:]}")
                    break
            out = prefix + ".0.fq" + (".gz" if extra else "")
            say(f"srqc --out_fq {tag}: wall {min(walls):.2f} s (of {', '.join(f'{w:.2f}' for w in walls)}), output {os.path.getsize(out) / 1e6:.1f} MB")
    for name in ("ref_test_asm.fa.gz", os.path.join("ref_pairs", "sr.R1.2000.fastq.gz")):
        data = gzip.open(os.path.join(GOLDEN, name), "rb").read()
        n_blk = (len(data) + BLOCK - 1) // BLOCK
        ours = len(np2io.bgzf_deflate_host(data)) - 26 * n_blk - 28
        z1, _ = zlib_blocks(data, 1)
        say(f"test fixture {name}: {len(data)} B, host twin {ours} B, zlib 1 {z1} B, ratio {ours / z1:.3f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
