"""Cost of the BAM writer (csrc/np2_bamout.hip, np2_bamout_host.cpp) on the device; the figures of profiles/bamout_cost.txt come
from here.

    python tools/bamout_probe.py all [--out FILE]   # the inputs once, then one child process under its own time limit
    python tools/bamout_probe.py run --dir D
    python tools/bamout_probe.py full [--out FILE]  # the full BAM (NP2_SAM_KEEP_ALL) beside the lean one, same records, one process
    python tools/bamout_probe.py runfull --dir D

The input is tools/sam_probe.py's: a synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi), its records shuffled and
written as SAM text, plain and gzip.  In one process, alternating:
  - SAM text -> BAM + .bai (np2_sam_open_ex with the names kept + np2_sam_write_bam), wall time, from plain text and from gzip,
    and of it np2_sam_write_bam alone; beside SAM text -> resident pileup (np2_sam_open + np2_contig_from_sam) on the same input;
  - the HIP-event times np2_bamout_stats_t carries: k_bam_sizes with its scan, k_bam_emit, the deflate kernel, the index kernels,
    the bytes/s of the two over the stream, and the ratio of k_bam_emit to the deflate kernel on the same bytes;
  - np2_contig_from_bam on the written file, on the fetch path NP2_INFLATE names or the default.
`full` gives every record of that text base qualities and a minimap2-like tag set (NM ms AS nn tp cm s1 s2 de rl, SA on every
fifth record, an MD of the read's length on every third) and a @PG and a @RG line, and runs, alternating in one process, the
lean handle (the names kept) and the full handle (NP2_SAM_KEEP_ALL) over that one text: k_sam_tail_len + scan and
k_sam_tail_emit beside k_sam_fields + scans and k_sam_pack in GB/s of text and as a share of the wait for the reader;
k_bam_emit and k_bgzf_deflate in GB/s of each stream; the two files' sizes.
`all` and `full` stop at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

STEP_LIMIT = 300  # seconds per child


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def leg_run(a):
    from nextpolish2_amd import Polisher, io as np2io
    ref = open(a.dir + "/ecoli.ref", "rb").read()
    pol = Polisher([])
    out = a.dir + "/written.bam"

    def to_bam(path):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path], keep_names=True)
        t1 = time.perf_counter()
        st = sam.write_bam(pol, out)
        t2 = time.perf_counter()
        sam.close()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3, st

    def to_pileup(path):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path])
        c = np2io.contig_from_sam(pol, sam, sam.refs()[0][0], ref)
        ms = (time.perf_counter() - t0) * 1e3
        c.free()
        sam.close()
        return ms

    to_bam(a.dir + "/ecoli.sam"), to_pileup(a.dir + "/ecoli.sam")  # (warm: staging blocks, code objects, the writer's batches)
    walls = {k: [] for k in ("SAM text -> BAM + .bai", "  of it np2_sam_write_bam", "SAM gzip -> BAM + .bai", "  of it np2_sam_write_bam (gzip)",
                             "SAM text -> resident pileup", "SAM gzip -> resident pileup", "np2_contig_from_bam on the written file")}
    stats = []
    for _ in range(a.runs):  # alternating
        w, b, st = to_bam(a.dir + "/ecoli.sam")
        walls["SAM text -> BAM + .bai"].append(w), walls["  of it np2_sam_write_bam"].append(b), stats.append(st)
        w, b, st = to_bam(a.dir + "/ecoli.sam.gz")
        walls["SAM gzip -> BAM + .bai"].append(w), walls["  of it np2_sam_write_bam (gzip)"].append(b), stats.append(st)
        walls["SAM text -> resident pileup"].append(to_pileup(a.dir + "/ecoli.sam"))
        walls["SAM gzip -> resident pileup"].append(to_pileup(a.dir + "/ecoli.sam.gz"))
        bam = np2io.Bam(out)
        t0 = time.perf_counter()
        c = np2io.contig_from_bam(pol, bam, bam.refs()[0][0], ref)
        walls["np2_contig_from_bam on the written file"].append((time.perf_counter() - t0) * 1e3)
        c.free()
        bam.close()
    st = stats[0]
    print(f"{st['records']} records, stream {st['stream_bytes'] / 1e6:.1f} MB in {st['blocks']} blocks -> file {st['file_bytes'] / 1e6:.1f} MB; "
          f".bai {os.path.getsize(out + '.bai')} bytes, {st['bins']} bins, {st['chunks']} chunks", flush=True)
    for what, w in walls.items():
        print(f"  {what}: wall ms {spread(w)}", flush=True)
    for key, what in (("sizes_ms", "k_bam_sizes + scan"), ("emit_ms", "k_bam_emit"), ("deflate_ms", "k_bgzf_deflate"), ("index_ms", "index kernels, scans and sort")):
        xs = [s[key] for s in stats]
        rate = f"; {st['stream_bytes'] / statistics.median(xs) / 1e6:.1f} GB/s of the stream" if key in ("emit_ms", "deflate_ms") and statistics.median(xs) > 0 else ""
        print(f"  {what}: ms {spread(xs)}{rate}", flush=True)
    ratios = [s["emit_ms"] / s["deflate_ms"] for s in stats if s["deflate_ms"] > 0]
    print(f"  k_bam_emit / k_bgzf_deflate on the same bytes: {spread(ratios)}", flush=True)
    pol.close()


def decorate_text(src, dst):
    """the alignment lines of `src` with QUAL and a minimap2-like tag set, @PG and @RG lines behind the @SQ lines"""
    import numpy as np
    rng = np.random.default_rng(9)
    with open(src, "rb") as f, open(dst, "wb") as g:
        i, in_header = 0, True
        for line in f:
            if line.startswith(b"@"):
                g.write(line)
                continue
            if in_header:
                g.write(b"@RG\tID:hifi\tSM:ecoli\tPL:PACBIO\n@PG\tID:minimap2\tPN:minimap2\tVN:2.28\tCL:minimap2 -ax map-hifi asm.fa hifi.fq\n")
                in_header = False
            fields = line.rstrip(b"\n").split(b"\t")
            n = len(fields[9]) if fields[9] != b"*" else 0
            if n:
                fields[10] = (rng.integers(20, 60, n, dtype=np.uint8) + 33).tobytes()
            nm = int(rng.integers(0, 40))
            tags = [b"NM:i:%d" % nm, b"ms:i:%d" % (2 * n - nm), b"AS:i:%d" % (2 * n - 3 * nm), b"nn:i:0", b"tp:A:P", b"cm:i:%d" % (n // 9),
                    b"s1:i:%d" % (n - nm), b"s2:i:0", b"de:f:0.%04d" % nm, b"rl:i:%d" % (i % 70000)]
            if i % 5 == 0:
                tags.append(b"SA:Z:ecoli,%d,+,%dS%dM,60,%d;" % (1 + i, n // 3, n - n // 3, nm))
            if i % 3 == 0:
                tags.append(b"MD:Z:" + b"".join(b"%dA" % 300 for _ in range(n // 301)) + b"%d" % (n % 301))
            g.write(b"\t".join(fields + tags) + b"\n")
            i += 1


def leg_runfull(a):
    from nextpolish2_amd import Polisher, io as np2io
    pol = Polisher([])
    path, out = a.dir + "/ecoli.full.sam", a.dir + "/written.bam"
    text_bytes = os.path.getsize(path)

    def one(full):
        t0 = time.perf_counter()
        sam = np2io.Sam(pol, [path], keep_names=True, keep_all=full)
        t1 = time.perf_counter()
        st = sam.write_bam(pol, out)
        t2 = time.perf_counter()
        st.update(sam.stats()), st.update(sam.tail_stats())
        st["open_wall_ms"], st["write_wall_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
        sam.close()
        return st

    one(False), one(True)  # (warm: staging blocks, code objects, the writer's batches)
    runs = {False: [], True: []}
    for _ in range(a.runs):  # alternating
        for full in (False, True):
            runs[full].append(one(full))
    print(f"text {text_bytes / 1e6:.1f} MB with qualities and tags; alternating lean (names kept) and full (NP2_SAM_KEEP_ALL) handles", flush=True)
    med = lambda full, key: statistics.median(r[key] for r in runs[full])
    for full in (False, True):
        st = runs[full][0]
        kind = "full" if full else "lean"
        print(f"{kind}: {st['records']} records, stream {st['stream_bytes'] / 1e6:.1f} MB in {st['blocks']} blocks -> file {st['file_bytes'] / 1e6:.1f} MB"
              + (f"; tails {st['tail_bytes'] / 1e6:.1f} MB" if full else ""), flush=True)
        keys = [("open_wall_ms", "np2_sam_open_ex wall"), ("read_ms", "  of it waiting for the reader"), ("parse_ms", "k_sam_lines, k_sam_fields + scans"),
                ("pack_ms", "k_sam_pack (+ k_sam_name_copy)")]
        keys += [("tail_len_ms", "k_sam_tail_len + scan"), ("tail_emit_ms", "k_sam_tail_emit")] if full else []
        keys += [("write_wall_ms", "np2_sam_write_bam wall"), ("emit_ms", "k_bam_emit"), ("deflate_ms", "k_bgzf_deflate")]
        for key, what in keys:
            xs = [r[key] for r in runs[full]]
            m = statistics.median(xs)
            rate = ""
            if key in ("parse_ms", "pack_ms", "tail_len_ms", "tail_emit_ms") and m > 0:
                rate = f"; {text_bytes / m / 1e6:.1f} GB/s of text"
            if key in ("emit_ms", "deflate_ms") and m > 0:
                rate = f"; {st['stream_bytes'] / m / 1e6:.1f} GB/s of the stream"
            print(f"  {what}: ms {spread(xs)}{rate}", flush=True)
        print(f"  k_bam_emit / k_bgzf_deflate on the same bytes: {spread([r['emit_ms'] / r['deflate_ms'] for r in runs[full] if r['deflate_ms'] > 0])}", flush=True)
    tail = med(True, "tail_len_ms") + med(True, "tail_emit_ms")
    print(f"k_sam_tail_len + scan + k_sam_tail_emit: {tail:.3f} ms = {100 * tail / max(med(True, 'read_ms'), 1e-9):.1f} % of the wait for the reader, "
          f"{100 * tail / max(med(True, 'open_wall_ms'), 1e-9):.1f} % of np2_sam_open_ex; beside k_sam_fields + scans and k_sam_pack {med(True, 'parse_ms') + med(True, 'pack_ms'):.3f} ms", flush=True)
    le, fe = runs[False][0]["stream_bytes"] / med(False, "emit_ms"), runs[True][0]["stream_bytes"] / med(True, "emit_ms")
    print(f"k_bam_emit bytes/s, full / lean: {fe / le:.3f}; file size full / lean: {runs[True][0]['file_bytes'] / runs[False][0]['file_bytes']:.2f}; "
          f"k_bgzf_deflate GB/s full {runs[True][0]['stream_bytes'] / med(True, 'deflate_ms') / 1e6:.1f}, lean {runs[False][0]['stream_bytes'] / med(False, 'deflate_ms') / 1e6:.1f}", flush=True)
    pol.close()


def run_all(a):
    import sam_probe
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        import contextlib
        import io
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            sam_probe.make_inputs(td, a.length, a.depth)
        emit(buf.getvalue().rstrip())
        if a.step == "full":
            decorate_text(td + "/ecoli.sam", td + "/ecoli.full.sam")
        cmd = [sys.executable, os.path.abspath(__file__), "runfull" if a.step == "full" else "run", "--dir", td, "--runs", str(a.runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
        except subprocess.TimeoutExpired as e:
            got = e.stdout or ""
            text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nno result within {STEP_LIMIT} s\n", 124
        emit(f"== BAM writer{', full beside lean' if a.step == 'full' else ''} (exit {rc})\n{text.rstrip()}")
        return rc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "run", "full", "runfull"])
    p.add_argument("--length", type=int, default=4641652, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the inputs are written [the system's temporary directory]; run: where they are")
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step in ("all", "full"):
        return run_all(a)
    leg_runfull(a) if a.step == "runfull" else leg_run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
