"""Cost of the edit report (csrc/np2_edits.hip) on the device; the figures of profiles/edits_cost.txt come from here.

    python tools/edits_probe.py kernels [--reps 5]      # per contig of the yeast-sized synthetic assembly bench.py uses: the six
                                                        # stages' HIP-event times, np2_edits_last beside np2_edits_buffers
    python tools/edits_probe.py cli [--runs 5]          # files -> FASTA wall time on the same assembly with / without --edits
    python tools/edits_probe.py all [-o FILE]           # both, written to FILE [profiles/edits_cost.txt]

np2_edits_last works where the polish left its consensus; np2_edits_buffers is what the command line calls (it fetches the
positions with the bases and hands both back up): the difference between the two walls is the price of that choice."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nextpolish2_amd import Opts, Polisher, io as np2io  # noqa: E402
from nextpolish2_amd.api import EDIT_KINDS, EDIT_STAGES  # noqa: E402
from nextpolish2_amd.synth import Synth  # noqa: E402


LINES = []


def say(text):
    LINES.append(text)
    print(text, flush=True)


def spread(xs):
    return f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, max {max(xs):.3f} (n = {len(xs)})"


def assembly():
    from bench import YEAST, make_assembly
    syn = make_assembly(list(YEAST), 30, 1, True)
    return syn, [Synth.yak_assembly(syn, k) for k in (21, 31)]


def leg_kernels(a):
    syn, yaks = assembly()
    pol = Polisher(yaks)
    stage = {s: [0.0] * a.reps for s in EDIT_STAGES}
    wall_last, wall_buf = [0.0] * a.reps, [0.0] * a.reps
    kinds, raw, same, bp = [0] * 5, 0, 0, 0
    for s in syn:
        c = pol.upload(s.pileup)
        bases, pos = pol.polish_resident(c, Opts())
        ref = s.pileup.ref.tobytes()
        first = pol.edits_last(c)  # (warm: blocks, code object)
        assert pol.edits_buffers(ref, bases, pos).records() == first.records()
        for i in range(a.reps):  # alternating
            t0 = time.perf_counter()
            r = pol.edits_last(c)
            wall_last[i] += time.perf_counter() - t0
            for k, v in r.kernel_ms.items():
                stage[k][i] += v
            t0 = time.perf_counter()
            pol.edits_buffers(ref, bases, pos)
            wall_buf[i] += time.perf_counter() - t0
        kinds = [x + y for x, y in zip(kinds, first.totals["n_kind"])]
        raw, same, bp = raw + first.totals["raw_runs"], same + first.totals["same_runs"], bp + len(ref)
        c.free()
    say(f"yeast-sized synthetic assembly: {len(syn)} contigs, {bp} bp, k21 + k31: {raw} raw runs, {same} rewritten the same, "
        f"edits {dict(zip(EDIT_KINDS, kinds))}")
    for k in EDIT_STAGES:
        say(f"  stage {k:8s} kernels, ms summed over the contigs: {spread(stage[k])}")
    say(f"  np2_edits_last, wall ms over the contigs: {spread([1e3 * x for x in wall_last])}")
    say(f"  np2_edits_buffers (contig, bases and positions sent up first), wall ms: {spread([1e3 * x for x in wall_buf])}")
    pol.close()


def leg_cli(a):
    from nextpolish2_amd import cli
    from nextpolish2_amd.bamio import write_bam_raw
    syn, yaks = assembly()
    with tempfile.TemporaryDirectory(dir=a.dir) as td:
        bam, fa = td + "/a.bam", td + "/a.fa"
        write_bam_raw(bam, [(s.pileup.name, s.pileup.L) for s in syn], [s.bam_records(i) for i, s in enumerate(syn)])
        with open(fa, "wb") as f:
            for s in syn:
                f.write(b">%s\n%s\n" % (s.pileup.name.encode(), s.pileup.ref.tobytes()))
        yk = []
        for y in yaks:
            yk.append(td + f"/k{y.k}.yak")
            np2io.write_yak(yk[-1], y)
        base = [bam, fa] + yk + ["-t", "2", "-L", "20000"]
        walls = {"plain": [], "edits": []}
        cli.main(base + ["-o", td + "/warm.fa"])
        for i in range(a.runs):  # alternating
            for what, extra in (("plain", []), ("edits", ["--edits", td + f"/e{i}.vcf", "--edits_summary", td + f"/e{i}.tsv"])):
                t0 = time.perf_counter()
                cli.main(base + extra + ["-o", td + f"/o.{what}.{i}.fa"])
                walls[what].append(time.perf_counter() - t0)
        same = open(td + "/o.plain.0.fa", "rb").read() == open(td + "/o.edits.0.fa", "rb").read()
        for what, w in walls.items():
            say(f"files -> FASTA, yeast-sized assembly, {what}: wall s {spread(w)}")
        n_rec = sum(1 for ln in open(td + "/e0.vcf", "rb") if not ln.startswith(b"#"))
        say(f"FASTA identical with and without --edits: {same}; VCF records: {n_rec}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "cli", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "edits_cost.txt"))
    a = ap.parse_args()
    if a.what != "all":
        return {"kernels": leg_kernels, "cli": leg_cli}[a.what](a)
    leg_kernels(a)
    leg_cli(a)
    with open(a.out, "w") as f:
        f.write("Cost of the edit report (csrc/np2_edits.hip), from tools/edits_probe.py all on one MI355X.\n\n" + "\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
