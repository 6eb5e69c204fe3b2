"""Cost of the reads door of the resident SAM (np2_sam_from_reads: csrc/np2_alnpack.hip, the PackSink of np2_map_host.cpp) beside
the route it replaces; the figures of profiles/mappolish_cost.txt come from here.

    python tools/mappolish_probe.py all [--out FILE]   # the inputs once, then one child process per step under its own time limit
    python tools/mappolish_probe.py routes --dir D     # FASTA -> resident Sam: the new door beside FASTA -> SAM file -> np2_sam_open
    python tools/mappolish_probe.py cli                # the committed bundle: cli --from_reads beside map -a | cli -, fresh processes

The input of `routes` is tools/map_probe.py's: the synthetic E. coli-sized mapping (4.64 Mb, 30 x simulated HiFi; 10 705 reads,
139 Mb).  Every figure is median, min and max over --runs calls after one warm-up call; the two routes alternate in one process.
  routes: wall seconds of Sam.from_reads beside map_align_files to a plain SAM file followed by Sam() on that file (the parent's
          route, whose parts are listed: files -> SAM, of it write_ms; text -> resident).  Kernel time: the new door's pack_ms
          (k_alnpack_sizes, its scans and k_alnpack; HIP events) beside the text door's parse_ms (k_sam_lines, k_sam_fields and
          scans) and pack_ms (k_sam_pack) on the same records; sort_ms of both.  assemble_ms of the reads door excludes the
          pack kernels (the driver subtracts the sizes-and-scans event time, which pack_ms carries): the two assemble_ms differ by
          the record and CIGAR copies to the host.  The ratio new / parent's route is printed, and the
          saving beside the parent's write_ms + text -> resident time, the least the new door is expected to save.
  cli:    tests/golden's assembly and the 574 reads of its BAM (the E. coli-sized input has no k-mer tables): wall seconds of
          `cli --from_reads hifi.fa.gz` beside `map -a hifi.fa.gz | cli -` as fresh processes, and whether the two FASTA outputs
          are the same bytes.
`all` stops at the first step that fails or runs out of time: nothing more is started on the device after that."""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from map_probe import ECOLI, STEP_LIMIT, spread  # noqa: E402


def leg_routes(a):
    from nextpolish2_amd import Polisher
    from nextpolish2_amd import io as np2io
    pol = Polisher([], device=0)
    ix = np2io.MapIndex(a.dir + "/ecoli.fa")
    fa, sam_path = a.dir + "/reads.fa", a.dir + "/map.sam"
    new, old_map, old_open, ms = [], [], [], {}
    st_new = st_old = None
    for run in range(a.runs + 1):
        t0 = time.perf_counter()
        s = np2io.Sam.from_reads(pol, ix, [fa])
        t1 = time.perf_counter()
        st_new, ast_new = s.stats(), np2io.align_last_stats()
        s.close()
        t2 = time.perf_counter()
        np2io.map_align_files(ix, [fa], sam_path)
        t3 = time.perf_counter()
        ast_old = np2io.align_last_stats()
        s = np2io.Sam(pol, [sam_path])
        t4 = time.perf_counter()
        st_old = s.stats()
        s.close()
        if run:
            new.append(t1 - t0), old_map.append(t3 - t2), old_open.append(t4 - t3)
            for k, v in (("new pack_ms", st_new["pack_ms"]), ("new sort_ms", st_new["sort_ms"]), ("new read_ms", st_new["read_ms"]),
                         ("new assemble_ms", ast_new["assemble_ms"]), ("text parse_ms", st_old["parse_ms"]), ("text pack_ms", st_old["pack_ms"]),
                         ("text sort_ms", st_old["sort_ms"]), ("text read_ms", st_old["read_ms"]), ("parent write_ms", ast_old["write_ms"]),
                         ("parent assemble_ms", ast_old["assemble_ms"])):
                ms.setdefault(k, []).append(v)
    ix.close()
    assert all(st_new[f] == st_old[f] for f in ("records", "kept", "unmapped", "cigar_words", "seq_bytes")), (st_new, st_old)
    print(f"reads FASTA ({os.path.getsize(fa)} bytes), SAM ({os.path.getsize(sam_path)} bytes): {st_new['records']} reads, {st_new['kept']} kept, "
          f"{st_new['cigar_words']} CIGAR words, {st_new['seq_bytes']} SEQ bytes", flush=True)
    old = [m + o for m, o in zip(old_map, old_open)]
    print(f"  wall s, FASTA -> resident Sam, reads door {spread(new)}", flush=True)
    print(f"  wall s, FASTA -> SAM file -> resident Sam {spread(old)}", flush=True)
    print(f"    of it FASTA -> SAM file {spread(old_map)}", flush=True)
    print(f"    of it text -> resident {spread(old_open)}", flush=True)
    for k, xs in ms.items():
        print(f"  {k} {spread(xs)}", flush=True)
    print(f"  ratio reads door / parent's route {spread([n / o for n, o in zip(new, old)])}", flush=True)
    print(f"  saved s {spread([o - n for n, o in zip(new, old)])} beside parent's write_ms + text -> resident "
          f"{spread([w / 1e3 + t for w, t in zip(ms['parent write_ms'], old_open)])}", flush=True)
    return 0


def leg_cli(a):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_model as mm
    golden = os.path.join(ROOT, "tests", "golden")
    asm, bundle = os.path.join(golden, "ref_test_asm.fa.gz"), os.path.join(golden, "ref_bundle")
    _, _, reads, names, _ = mm.bundle_reads(os.path.join(bundle, "hifi.map.sort.bam"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    tail = [asm, bundle + "/k21.yak", bundle + "/k31.yak", "-L", "10000"]
    with tempfile.TemporaryDirectory() as td:
        with gzip.open(td + "/hifi.fa.gz", "wb") as f:
            for n, r in zip(names, reads):
                f.write(b">" + n.encode() + b"\n" + r + b"\n")
        one, two = [], []
        for run in range(a.runs + 1):
            for out in ("a.fa", "b.fa"):
                if os.path.exists(td + "/" + out):
                    os.remove(td + "/" + out)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "--from_reads", td + "/hifi.fa.gz"] + tail + ["-o", td + "/a.fa"],
                               capture_output=True, text=True, env=env, timeout=STEP_LIMIT)
            t1 = time.perf_counter()
            if r.returncode:
                print(r.stderr[-3000:])
                return r.returncode
            m = subprocess.Popen([sys.executable, "-m", "nextpolish2_amd.map", "-a", asm, td + "/hifi.fa.gz"], stdout=subprocess.PIPE, env=env)
            r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-"] + tail + ["-o", td + "/b.fa"], stdin=m.stdout, capture_output=True,
                               text=True, env=env, timeout=STEP_LIMIT)
            m.stdout.close()
            rc = m.wait(timeout=STEP_LIMIT)
            t2 = time.perf_counter()
            if r.returncode or rc:
                print(r.stderr[-3000:])
                return r.returncode or rc
            if run:
                one.append(t1 - t0), two.append(t2 - t1)
        same = open(td + "/a.fa", "rb").read() == open(td + "/b.fa", "rb").read()
    print(f"bundle, {len(reads)} reads: the two FASTA outputs are {'the same bytes' if same else 'DIFFERENT'}", flush=True)
    print(f"  wall s, cli --from_reads {spread(one)}", flush=True)
    print(f"  wall s, map -a | cli - {spread(two)}", flush=True)
    return 0 if same else 1


def run_all(a):
    out = open(a.out, "a") if a.out else None

    def emit(text):
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        r = subprocess.run([sys.executable, os.path.join(HERE, "map_probe.py"), "inputs", "--dir", td, "--length", str(a.length), "--depth", str(a.depth)],
                           capture_output=True, text=True, timeout=900)
        emit(r.stdout + (r.stderr[-3000:] if r.returncode else ""))
        if r.returncode:
            return r.returncode
        for step in ("routes", "cli"):
            cmd = [sys.executable, os.path.abspath(__file__), step, "--dir", td, "--runs", str(a.runs)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
                text, rc = r.stdout + (r.stderr[-3000:] if r.returncode else ""), r.returncode
            except subprocess.TimeoutExpired as e:
                got = e.stdout or ""
                text, rc = f"{got if isinstance(got, str) else got.decode(errors='replace')}\nstep {step}: no result within {STEP_LIMIT} s\n", 124
            emit(f"== {step} (exit {rc})\n{text}")
            if rc != 0:
                return rc
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("step", choices=["all", "routes", "cli"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--dir", default=None, help="all: where the temporary directory goes; routes: where the inputs are")
    p.add_argument("--length", type=int, default=ECOLI, help="positions of the synthetic contig [4641652]")
    p.add_argument("--depth", type=int, default=30)
    p.add_argument("--out", default=None, help="all: append every step's output to this file")
    a = p.parse_args()
    if a.step == "all":
        return run_all(a)
    return {"routes": leg_routes, "cli": leg_cli}[a.step](a) or 0


if __name__ == "__main__":
    sys.exit(main())
