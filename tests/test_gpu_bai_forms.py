"""Indexed BAMs read through .bai indexes in the forms of tests/bai_model.py — the project's own, htslib's (modelled, see
bai_model), a sparse one, one that spells block ends the other way — and through indexes that disagree with their file, on
the host pool, the device walk over the resident stream and the device walk over one reference's blocks.  The expected
answer is always np2_contig_from_records (and np2_depth_from_records) fed with the records an index-free scan of the file
finds; every comparison is exact.  Which path served a reference is read from NP2_IO_PROFILE's "fetch_records_gpu:" line,
so that a silent fall-back to the host cannot make a device case pass unseen.

One fresh process per way of reading (NP2_BAM_RESIDENT_MB is read once per process) runs every job; the tests look at what
it left."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bai_cases as bc
import bai_model as bm
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import depth_from_records
from nextpolish2_amd.bamio import records_to_arrays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"host": dict(NP2_INFLATE="libdeflate"),
         "device": dict(NP2_INFLATE="gpu"),                                   # the whole file inflated once, resident
         "device_per_ref": dict(NP2_INFLATE="gpu", NP2_BAM_RESIDENT_MB="0")}  # a reference's blocks uploaded by themselves
DEVICE_MODES = ("device", "device_per_ref")
HALO = 2048
# (own_lo, own_hi) per reference; the zone is the interval +- HALO.  ctgA: a zone that ends, one that starts and ends and
# one that starts on a multiple of 16384 (the last: at the very base a record's span ends on).  ctgB: a zone that starts in a
# leading empty window, one that ends on a multiple of 16384, one that starts inside the interior empty window.
SHARDS = {0: [(0, 3 * bc.W - HALO), (bc.W + HALO, 3 * bc.W - HALO), (2 * bc.W + HALO, 70000)],
          1: [(12288, 40960), (40960, 4 * bc.W - HALO), (53248, 73728)]}
DISAGREE = "abcdefg"

CHILD = """import json, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import bai_cases as bc
from nextpolish2_amd import Polisher
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
d = sys.argv[1]
jobs = json.load(open(os.path.join(d, "jobs.json")))
refs = {t: open(os.path.join(d, "ref%%d.txt" %% t), "rb").read() for t in range(4)}
pol = Polisher([])
out, bams = {}, {}
for j in jobs:
    key, tid, name = j["key"], j["tid"], bc.REFS[j["tid"]][0]
    sys.stderr.write("@@ %%s\\n" %% key)
    sys.stderr.flush()
    try:
        if j["bam"] not in bams:
            bams[j["bam"]] = np2io.Bam(os.path.join(d, j["bam"]))
        bam = bams[j["bam"]]
        if j["kind"] == "contig":
            c = np2io.contig_from_bam(pol, bam, name, refs[tid], bc.front_opts())
            ex = np2io.export_contig(pol, c, np.frombuffer(refs[tid], dtype=np.uint8))
            out[key + ":reads"], out[key + ":nib"] = ex.reads, ex.nibbles
            c.free()
        elif j["kind"] == "depth":
            runs, stats, depth = np2io.depth_from_bam(pol, bam, name, len(refs[tid]), want_depth=True)
            out[key + ":runs"], out[key + ":depth"] = runs, depth
            out[key + ":stats"] = np.array([stats[k] for k in sorted(stats) if k != "kernel_ms"], dtype=np.uint64)
        else:
            sh = np2io.ShardFromBam(pol, bam, name, refs[tid], j["own"][0], j["own"][1], halo=j["halo"], opts=bc.front_opts())
            out[key + ":offsets"] = sh.own_offsets
            h, plan, n_total = sh.finish(np.array(j["all_off"], dtype=np.uint64))
            rc = np2io._resident(pol, h, name, plan.sub_hi - plan.sub_lo)  # (owns the shard's contig)
            ex = np2io.export_contig(pol, rc, np.frombuffer(refs[tid][plan.sub_lo:plan.sub_hi], dtype=np.uint8))
            out[key + ":reads"], out[key + ":nib"] = ex.reads, ex.nibbles
            out[key + ":plan"] = np.array([getattr(plan, f) for f, _ in plan._fields_] + [n_total], dtype=np.int64)
            rc.free()
        out[key + ":code"] = np.array([0])
    except Np2Error as e:
        out[key + ":code"] = np.array([e.code])
        out[key + ":msg"] = np.array([str(e)])
np.savez(sys.argv[2], **out)
""" % (ROOT, os.path.join(ROOT, "tests"))


def _disagreeing(sc, which):
    """the own-form index of the scan with one thing about ctgA made wrong -> (refs, tail) for pack_bai"""
    refs, tail = bm.index_of(sc, "own")
    bins, lin = [(b, [list(c) for c in ch]) for b, ch in refs[0][0]], list(refs[0][1])
    a = sc.of(0)
    by_beg = {r["beg"]: i for i, r in enumerate(a)}
    isize_of = {fo: n for fo, n, _ in sc.blocks}
    # an interior entry (not the first, not a repeat) whose record's first 9 bytes and the whole next record lie in its block
    w = next(w for w in range(1, len(lin)) if lin[w] > lin[w - 1] and
             sc.voff(a[by_beg[lin[w]] + 1]["send"] - 1) >> 16 == lin[w] >> 16)
    nxt = a[by_beg[lin[w]] + 1]
    v = lin[w]
    if which == "a":    # 9 bytes into the record it named
        lin[w] = v + 9
    elif which == "b":  # the middle of the next record's SEQ bytes
        lin[w] = sc.voff(nxt["spos"] + 36 + len(nxt["name"]) + 1 + 4 * len(nxt["cigar"]) + len(nxt["seq"]) // 4)
        assert lin[w] >> 16 == v >> 16 and all(x < v or x > lin[w] for x in lin[:w] + lin[w + 1:])
    elif which == "c":  # a file offset that is no block's start
        lin[w] = v + (1 << 16)
        assert (lin[w] >> 16) not in isize_of
    elif which == "d":  # an offset inside the block at or beyond its inflated size
        lin[w] = (v & ~0xFFFF) | (isize_of[v >> 16] + 5)
    elif which == "e":  # smaller than its predecessor
        lin[w] = a[1]["beg"]
        assert 0 < lin[w] < lin[w - 1]
    elif which == "f":  # the chunks end in the midst of the reference's records, so early that the 64 KiB read beyond the
        mid = a[len(a) // 8]["beg"]  # index's end do not reach the last of them: the walk has to ask for more
        assert (mid >> 16) + 65536 + 8192 < a[-1]["beg"] >> 16
        for _, ch in bins:
            for c in ch:
                c[0], c[1] = min(c[0], mid), min(c[1], mid)
    elif which == "g":  # the largest chunk end: at the end-of-file marker
        top = max(c[1] for _, ch in bins for c in ch)
        for _, ch in bins:
            for c in ch:
                if c[1] == top:
                    c[1] = sc.blocks[-1][0] << 16
    elif which == "first":  # the reference's first offset: 9 bytes into its first record
        for _, ch in bins:
            for c in ch:
                if c[0] == a[0]["beg"]:
                    c[0] += 9
        assert sc.voff(a[0]["spos"] + 9) == a[0]["beg"] + 9
    refs[0] = ([(b, [tuple(c) for c in ch]) for b, ch in bins], lin)
    return refs, tail


def _admitted(sc, tid):
    """the records of a reference that the front end admits under bc.front_opts(): all but the one with flag 0x4
    (test_bai_forms_cpu.py checks that on the oracle), in file order: the i-th is the contig's read i + 1"""
    return [r for r in sc.of(tid) if not r["flag"] & 4]


# Which path serves a whole reference under the end_at_isize form, as the code decides today and as observed: the device, but
# for ctgA where an interior linear entry falls on a block's end — fetch_chain_starts refuses an offset inside a block that is
# not below the block's inflated size; that happens only where blocks end on record boundaries — and for ctgA read from the
# resident stream, which begins at the first record's block, while ctgA's first offset is spelled at the end of the header's.
END_AT_ISIZE_HOST = {("device", "rec", 0), ("device", "ff00", 0), ("device", "b600", 0), ("device_per_ref", "rec", 0)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    t0 = time.time()
    d = tmp_path_factory.mktemp("gpu_bai_forms")
    _, refs, paths = bc.build(d)
    scans = {cut: bm.scan(p) for cut, p in paths.items()}
    jobs = []

    def variant(cut, tag, refs_tail):
        name = "%s.%s.bam" % (cut, tag)
        os.symlink(paths[cut], str(d / name))
        with open(str(d / name) + ".bai", "wb") as f:
            f.write(bm.pack_bai(*refs_tail))
        return name
    for cut in bc.CUTS:
        for form in bm.FORMS:
            name = variant(cut, form, bm.index_of(scans[cut], form, seed=7))
            for tid in range(4):
                jobs.append(dict(key="%s/%s/%d/contig" % (form, cut, tid), kind="contig", bam=name, tid=tid))
                jobs.append(dict(key="%s/%s/%d/depth" % (form, cut, tid), kind="depth", bam=name, tid=tid))
    for form in ("htslib", "sparse"):
        for tid, cuts in SHARDS.items():
            for k, own in enumerate(cuts):
                jobs.append(dict(key="%s/shard/%d/%d" % (form, tid, k), kind="shard", bam="ff00.%s.bam" % form, tid=tid, own=own, halo=HALO,
                                 all_off=[r["beg"] for r in _admitted(scans["ff00"], tid)]))
    for which in list(DISAGREE) + ["first"]:
        name = variant("ff00", "dis_" + which, _disagreeing(scans["ff00"], which))
        jobs.append(dict(key="dis/%s" % which, kind="contig", bam=name, tid=0))
    with open(str(d / "jobs.json"), "w") as f:
        json.dump(jobs, f)
    (d / "child.py").write_text(CHILD)
    # the expected answers: the scan's records of each reference through the records doors, once
    pol = Polisher([])
    want = {}
    sc = scans["rec"]
    for tid, (name, L) in enumerate(bc.REFS):
        arr, cig, seq4, _, _ = records_to_arrays(sc.of(tid))
        c = np2io.contig_from_records(pol, refs[tid], arr, cig, seq4, bc.front_opts())
        ex = np2io.export_contig(pol, c, np.frombuffer(refs[tid], dtype=np.uint8))
        c.free()
        dr, ds, dd = depth_from_records(pol, L, arr, cig, want_depth=True)
        want[tid] = dict(reads=ex.reads, nib=ex.nibbles, runs=dr, depth=dd, stats=np.array([ds[k] for k in sorted(ds) if k != "kernel_ms"], dtype=np.uint64))
    pol.close()
    out = {}
    for mode, env in MODES.items():
        npz = str(d / (mode + ".npz"))
        t1 = time.time()
        r = subprocess.run([sys.executable, str(d / "child.py"), str(d), npz], capture_output=True, text=True,
                           env=dict(os.environ, NP2_IO_PROFILE="1", **env), timeout=300)
        assert r.returncode == 0, (mode, r.stderr[-3000:])
        served = {}  # job key -> its stretch of the profile
        for part in r.stderr.split("@@ ")[1:]:
            key, _, rest = part.partition("\n")
            served[key] = rest
        out[mode] = (np.load(npz), served)
        print("bai forms: %s: %d jobs in %.1f s" % (mode, len(jobs), time.time() - t1))
    print("bai forms: fixture %.1f s" % (time.time() - t0))
    return dict(out=out, want=want, scans=scans)


def path_of(runs, mode, key):
    return "device" if "fetch_records_gpu:" in runs["out"][mode][1][key] else "host"


def same_contig(z, key, want):
    assert z[key + ":code"].tolist() == [0], (key, z[key + ":msg"].tolist() if key + ":msg" in z else None)
    assert np.array_equal(z[key + ":reads"], want["reads"]), key
    assert np.array_equal(z[key + ":nib"], want["nib"]), key


def test_the_expected_answers_are_not_empty(runs):
    w, sc = runs["want"], runs["scans"]["rec"]
    assert len(w[2]["reads"]) == 1 and not w[2]["depth"].any()  # ctgC: the contig's own row and nothing else
    for tid in (0, 1, 3):  # (row 0 is the contig itself; the record with flag 0x4 is the one that is not admitted)
        assert len(w[tid]["reads"]) - 1 == sum(1 for r in sc.of(tid) if not r["flag"] & 4)
        assert w[tid]["depth"].max() >= 5
    for cut in bc.CUTS:  # one expected answer for the three files: they hold the same records
        assert [(r["tid"], r["pos"], r["flag"], r["cigar"], r["seq"]) for r in runs["scans"][cut].records] == \
               [(r["tid"], r["pos"], r["flag"], r["cigar"], r["seq"]) for r in sc.records]


@pytest.mark.parametrize("cut", list(bc.CUTS))
@pytest.mark.parametrize("form", bm.FORMS)
@pytest.mark.parametrize("mode", list(MODES))
def test_every_form_gives_the_scans_records(runs, mode, form, cut):
    z, _ = runs["out"][mode]
    for tid in range(4):
        key = "%s/%s/%d" % (form, cut, tid)
        same_contig(z, key + "/contig", runs["want"][tid])
        assert z[key + "/depth:code"].tolist() == [0], key
        for k in ("runs", "depth", "stats"):
            assert np.array_equal(z[key + "/depth:" + k], runs["want"][tid][k]), (key, k)


@pytest.mark.parametrize("cut", list(bc.CUTS))
@pytest.mark.parametrize("form", bm.FORMS)
@pytest.mark.parametrize("mode", DEVICE_MODES)
def test_which_path_served_each_form(runs, mode, form, cut):
    """own, htslib, htslib_nometa, sparse: the device, for the pileup and for the depth; end_at_isize: as END_AT_ISIZE_HOST
    lists.  (ctgC has no record: nothing is fetched on any path.)  The host mode never shows the device's line."""
    got = {tid: path_of(runs, mode, "%s/%s/%d/contig" % (form, cut, tid)) for tid in (0, 1, 3)}
    print("served:", mode, form, cut, got)
    if form == "end_at_isize":
        want = {tid: "host" if (mode, cut, tid) in END_AT_ISIZE_HOST else "device" for tid in (0, 1, 3)}
    else:
        want = {tid: "device" for tid in (0, 1, 3)}
    assert got == want
    assert {tid: path_of(runs, mode, "%s/%s/%d/depth" % (form, cut, tid)) for tid in (0, 1, 3)} == want
    assert path_of(runs, mode, "%s/%s/2/contig" % (form, cut)) == "host"
    assert path_of(runs, "host", "%s/%s/0/contig" % (form, cut)) == "host"
    resident = "stretch of the resident stream" in runs["out"][mode][1]["%s/%s/3/contig" % (form, cut)]
    assert resident == (mode == "device" and want[3] == "device")


@pytest.mark.parametrize("form", ["htslib", "sparse"])
@pytest.mark.parametrize("mode", list(MODES))
def test_shard_zones(runs, mode, form):
    """A zone (own interval +- HALO) read by ShardFromBam.  The records it fetched are the fetch rule's answer for the zone on
    the scan: the finished shard holds, under their contig-wide numbers, exactly the admitted ones of those — the records that
    start before own_lo and reach the zone, the 40 kb one among them, and those of the upper halo included — and each with the
    columns the whole contig's expected pileup has for it.  The offsets it publishes are the scan's `beg` of the held records
    that start in its own interval."""
    z, _ = runs["out"][mode]
    sc = runs["scans"]["ff00"]
    long_seen = upper_seen = before_seen = 0
    for tid, cuts in SHARDS.items():
        L = bc.REFS[tid][1]
        adm = _admitted(sc, tid)
        number = {r["beg"]: i + 1 for i, r in enumerate(adm)}
        whole = runs["want"][tid]
        assert len(whole["reads"]) == len(adm) + 1
        for k, (lo, hi) in enumerate(cuts):
            key = "%s/shard/%d/%d" % (form, tid, k)
            zone_lo, zone_hi = max(lo - HALO, 0), min(hi + HALO, L)
            zone = [r for r in bm.fetch_rule(sc, tid, zone_lo, zone_hi) if not r["flag"] & 4]
            assert z[key + ":code"].tolist() == [0], (key, z[key + ":msg"].tolist() if key + ":msg" in z else None)
            own_lo, own_hi, sub_lo, sub_hi, p_zone_lo, p_zone_hi, read_lo, read_hi, n_total = z[key + ":plan"].tolist()
            assert (own_lo, own_hi, p_zone_lo, p_zone_hi, n_total) == (lo, hi, zone_lo, zone_hi, len(adm) + 1), key
            # the fetched records
            reads, nib = z[key + ":reads"], z[key + ":nib"]
            assert len(reads) == 1 + read_hi - read_lo
            held = [read_lo + i - 1 for i in range(1, len(reads)) if not reads["flags"][i] & 1]
            assert len(zone) > 5 and held == [number[r["beg"]] for r in zone], (key, len(held), len(zone))
            upper_seen += sum(1 for r in zone if r["pos"] >= hi)
            before_seen += sum(1 for r in zone if r["pos"] < zone_lo)
            long_seen += sum(1 for r in zone if r["span"] == bc.LONG_LEN and r["pos"] < lo)
            for i in range(1, len(reads)):
                if reads["flags"][i] & 1:
                    continue
                a, g = reads[i], whole["reads"][read_lo + i - 1]
                assert (a["aln_t_s"] + sub_lo, a["aln_t_e"] + sub_lo, a["n_cols"], a["flags"]) == (g["aln_t_s"], g["aln_t_e"], g["n_cols"], g["flags"]), (key, i)
                nb = (int(a["n_cols"]) + 1) // 2
                assert np.array_equal(nib[int(a["nib_off"]):int(a["nib_off"]) + nb], whole["nib"][int(g["nib_off"]):int(g["nib_off"]) + nb]), (key, i)
            # the published offsets
            assert z[key + ":offsets"].tolist() == [r["beg"] for r in zone if lo <= r["pos"] < hi], key
            if mode != "host":
                assert path_of(runs, mode, key) == "device", key
    assert upper_seen >= 20 and before_seen >= 20  # records of the upper halo; records that start before a zone and reach it
    assert long_seen == 2  # the record of 40000 M starts before ctgA's second and third zone and reaches both
    # the zones are where they are meant to be
    assert (SHARDS[1][0][0] - HALO) >> 14 == 0 and (SHARDS[1][2][0] - HALO) >> 14 == 3 and (SHARDS[1][1][1] + HALO) % bc.W == 0
    assert (SHARDS[0][1][0] - HALO) % bc.W == 0 and (SHARDS[0][2][0] - HALO) == sum(bc.ENDS_ON_W)


@pytest.mark.parametrize("which", list(DISAGREE))
@pytest.mark.parametrize("mode", list(MODES))
def test_an_index_that_disagrees_with_its_file(runs, mode, which):
    """ctgA through an own-form index with one thing wrong (see _disagreeing): the records are the file's all the same.  A
    linear entry that is not a record's start, not a block's start or not inside its block (a - d) sends the reference the
    host's way; an entry out of order is passed over (e), an understated end costs a second round (f), an overstated one
    nothing (g): the device serves those."""
    z, _ = runs["out"][mode]
    same_contig(z, "dis/" + which, runs["want"][0])
    if mode != "host":
        got = path_of(runs, mode, "dis/" + which)
        print("served:", mode, "disagreeing", which, got)
        assert got == ("host" if which in "abcd" else "device")
        if which == "f":
            assert "after extending the range" in runs["out"][mode][1]["dis/f"]


@pytest.mark.parametrize("mode", DEVICE_MODES)
def test_a_wrong_first_offset_is_taken_alike_on_both_paths(runs, mode):
    """The reference's first offset moved 9 bytes into its first record.  Neither path can recover from this — the host pool
    trusts that offset too —, so this pins only that the device path's outcome equals the host path's (the same error code, or
    the same records), not a desired answer."""
    zh, zd = runs["out"]["host"][0], runs["out"][mode][0]
    assert zd["dis/first:code"].tolist() == zh["dis/first:code"].tolist()
    print("wrong first offset:", mode, zd["dis/first:code"].tolist(), zd["dis/first:msg"].tolist() if "dis/first:msg" in zd else "records")
    if zh["dis/first:code"].tolist() == [0]:
        assert np.array_equal(zd["dis/first:reads"], zh["dis/first:reads"]) and np.array_equal(zd["dis/first:nib"], zh["dis/first:nib"])
