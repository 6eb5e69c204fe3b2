"""The read front end on the records of front_cases.py: anchors that straddle a lane or a pass of the columnariser
(csrc/np2_front.hip), records without any, stream lengths on either side of every boundary — through every way records reach
it: np2_contig_from_records, a BAM whose blocks are cut at a byte limit as htslib cuts them (host pool walk; device walk over
the whole file and over one reference's blocks), and SAM text.  Each must give exactly the pileup the plain-Python rule
(front_model.py) and the oracle give (test_front_cases_cpu.py compares those two); a failure names the records."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import front_cases as fc
from nextpolish2_amd import Opts, Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd._types import Pileup
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.bamio import read_bam, records_to_arrays, write_bam, write_sam
from oracle import np2_oracle as orc
from test_front_cases_cpu import oracle_pileup, pileup_against_model
from test_frontend_cpu import same_pileup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_REFPANIC = -5
LIMITS = (300, 4096, 0xff00)  # fixed fields split between blocks; a few records a block; what samtools writes
LEVELS = (0, 6)
MODES = {"host": dict(NP2_INFLATE="libdeflate"),
         "device": dict(NP2_INFLATE="gpu"),                                   # the whole file inflated once, resident
         "device_per_ref": dict(NP2_INFLATE="gpu", NP2_BAM_RESIDENT_MB="0")}  # a reference's blocks uploaded by themselves


def check(pu, tid, what):
    bad = pileup_against_model(pu, tid)
    assert bad == [], "%s, contig %s: differs from the rule at %s" % (what, fc.REFS[tid][0], " ".join(bad[:20]))
    assert same_pileup(pu, oracle_pileup(tid)), what


def arrays(tid):
    return records_to_arrays(fc.records(tid)[0])


@pytest.mark.parametrize("tid", [0, 1])
def test_records_path(tid):
    pol = Polisher([])
    arr, cig, seq4, _, _ = arrays(tid)
    ref = fc.contig(tid).encode()
    c = np2io.contig_from_records(pol, ref, arr, cig, seq4, fc.front_opts())
    check(np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8)), tid, "np2_contig_from_records")
    c.free()
    pol.close()


@pytest.mark.parametrize("op", ["N", "P"])
def test_records_path_reports_the_panic(op):
    pol = Polisher([])
    ref = fc.contig(0).encode()
    recs = fc.records(0)[0]
    k = [r["pos"] < fc.PANIC_POS for r in recs].index(False)
    arr, cig, seq4, _, _ = records_to_arrays(recs[:k] + [fc.panic_record(0, op)] + recs[k:])
    with pytest.raises(Np2Error, match="Unknown cigar") as e:
        np2io.contig_from_records(pol, ref, arr, cig, seq4, fc.front_opts())
    assert e.value.code == E_REFPANIC
    # ... and the context goes on working
    arr, cig, seq4, _, _ = arrays(0)
    c = np2io.contig_from_records(pol, ref, arr, cig, seq4, fc.front_opts())
    check(np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8)), 0, "np2_contig_from_records after a panic")
    pol.close()


CHILD = """import os, sys
import numpy as np
sys.path.insert(0, %r)
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
d, names = sys.argv[1], sys.argv[2].split(",")
fo = np2io.FrontOpts(min_read_len=0, min_map_len=0, min_map_fra=0.0, max_clip_len=100000)
refs = [open(os.path.join(d, "ref%%d.txt" %% t), "rb").read() for t in (0, 1)]
pol = Polisher([])
out = {}
for op in ("N", "P"):  # first the files the reference panics on: what follows shows that the context is still usable
    try:
        np2io.contig_from_bam(pol, np2io.Bam(os.path.join(d, "panic_%%s.bam" %% op)), names[0], refs[0], fo)
        out["panic_" + op] = np.array([0])
    except Np2Error as e:
        out["panic_" + op] = np.array([e.code, int("Unknown cigar" in str(e))])
for f in sorted(os.listdir(d)):
    if not (f.startswith("cut_") and f.endswith(".bam")):
        continue
    bam = np2io.Bam(os.path.join(d, f))
    for t in (0, 1):
        c = np2io.contig_from_bam(pol, bam, names[t], refs[t], fo)
        ex = np2io.export_contig(pol, c, np.frombuffer(refs[t], dtype=np.uint8))
        out["%%s_%%d_reads" %% (f[:-4], t)] = ex.reads
        out["%%s_%%d_nib" %% (f[:-4], t)] = ex.nibbles
        c.free()
    bam.close()
np.savez(sys.argv[3], **out)
""" % ROOT


@pytest.fixture(scope="module")
def bam_runs(tmp_path_factory):
    """every BAM once, and one fresh process per way of reading that reads them all -> {mode: (npz, stderr)}"""
    d = tmp_path_factory.mktemp("front_edges")
    recs = fc.records(0)[0] + fc.records(1)[0]  # one reference's records end inside the block the next one's begin in
    for limit in LIMITS:
        for level in LEVELS:
            write_bam(str(d / ("cut_%d_%d.bam" % (limit, level))), fc.REFS, recs, block_limit=limit, level=level)
    for op in ("N", "P"):
        rr = sorted(recs[:40] + [fc.panic_record(0, op)], key=lambda r: (r["tid"], r["pos"]))
        write_bam(str(d / ("panic_%s.bam" % op)), fc.REFS, rr, block_limit=300, level=6)
    for t in (0, 1):
        (d / ("ref%d.txt" % t)).write_text(fc.contig(t))
    (d / "child.py").write_text(CHILD)
    runs = {}
    for mode, env in MODES.items():
        out = str(d / (mode + ".npz"))
        r = subprocess.run([sys.executable, str(d / "child.py"), str(d), ",".join(n for n, _ in fc.REFS), out], capture_output=True,
                           text=True, env=dict(os.environ, NP2_IO_PROFILE="1", **env), timeout=300)
        assert r.returncode == 0, (mode, r.stderr[-3000:])
        runs[mode] = (np.load(out), r.stderr)
    return runs


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("mode", list(MODES))
def test_bam_cut_at_a_byte_limit(bam_runs, mode, limit, level):
    z, _ = bam_runs[mode]
    for tid in (0, 1):
        key = "cut_%d_%d_%d" % (limit, level, tid)
        pu = Pileup(np.frombuffer(fc.contig(tid).encode(), dtype=np.uint8), z[key + "_reads"], z[key + "_nib"])
        check(pu, tid, "np2_contig_from_bam (%s, blocks of %d bytes, level %d)" % (mode, limit, level))


@pytest.mark.parametrize("mode", list(MODES))
def test_bam_paths_ran_and_report_the_panic(bam_runs, mode):
    z, err = bam_runs[mode]
    n_fetch = err.count("fetch_records_gpu:")
    if mode == "host":
        assert n_fetch == 0, err[-2000:]
    else:  # the device path really ran: 2 panic files and 2 references of each of the 6 files
        assert n_fetch >= 2 * len(LIMITS) * len(LEVELS), err[-2000:]
        assert ("stretch of the resident stream" in err) == (mode == "device"), err[-2000:]
    for op in ("N", "P"):
        assert z["panic_" + op].tolist() == [E_REFPANIC, 1], (op, z["panic_" + op])


@pytest.mark.parametrize("gz", [False, True])
def test_sam_path(tmp_path, gz):
    recs = fc.records(0)[0] + fc.records(1)[0]
    order = np.random.default_rng(5).permutation(len(recs))
    path = str(tmp_path / ("edges.sam.gz" if gz else "edges.sam"))
    write_sam(path, fc.REFS, [recs[k] for k in order], gz=gz)
    pol = Polisher([])
    sam = np2io.Sam(pol, [path])
    assert sam.refs() == fc.REFS
    for tid in (0, 1):
        ref = fc.contig(tid).encode()
        c = np2io.contig_from_sam(pol, sam, fc.REFS[tid][0], ref, fc.front_opts())
        check(np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8)), tid, "np2_contig_from_sam" + (" (gzip)" if gz else ""))
        c.free()
    sam.close()
    pol.close()


@pytest.mark.parametrize("tid", [0, 1])
def test_polish_of_the_resident_pileup_equals_the_oracle(tid):
    from test_oracle import yak_from_seqs
    yak = yak_from_seqs([fc.contig(tid).upper()], 21, count=30)
    pol = Polisher([yak])
    arr, cig, seq4, _, _ = arrays(tid)
    c = np2io.contig_from_records(pol, fc.contig(tid).encode(), arr, cig, seq4, fc.front_opts())
    b, p = pol.polish_resident(c, Opts())
    ob, op = orc.Oracle([yak]).polish(oracle_pileup(tid), Opts())
    assert np.array_equal(b, ob) and np.array_equal(p, op)
    pol.close()


@pytest.mark.parametrize("inflate", ["libdeflate", "gpu"])
def test_reference_bundle_through_straddling_blocks(tmp_path, inflate):
    """The committed bundle's BAM ends every block on a record boundary.  Written again as samtools writes (a block cut
    every 0xff00 bytes, whatever lies there) it must polish to the same committed output, on both inflate paths."""
    bundle = os.path.join(ROOT, "tests", "golden", "ref_bundle")
    asm = os.path.join(ROOT, "tests", "golden", "ref_test_asm.fa.gz")
    refs, recs = read_bam(os.path.join(bundle, "hifi.map.sort.bam"))
    bam = str(tmp_path / "cut.bam")
    write_bam(bam, refs, recs, block_limit=0xff00, level=6)
    assert read_bam(bam) == (refs, recs)
    env = dict(os.environ, PYTHONPATH=ROOT, NP2_INFLATE=inflate, NP2_IO_PROFILE="1")
    r = subprocess.run([sys.executable, "-m", "nextpolish2_amd.cli", "-L", "1000", bam, asm, os.path.join(bundle, "k21.yak"),
                        os.path.join(bundle, "k31.yak")], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert (b"fetch_records_gpu:" in r.stderr) == (inflate == "gpu"), r.stderr.decode()[-2000:]
    assert r.stdout == gzip.open(os.path.join(bundle, "expected.fa.gz"), "rb").read()
