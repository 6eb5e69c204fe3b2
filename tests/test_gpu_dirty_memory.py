"""Every device path on recycled, non-zero memory.

No pool of csrc/np2_ctx.hpp clears a block it hands out, and DevBuf::ensure rounds every request up: a kernel may assume
nothing about memory it did not write in this call.  A fresh hipMalloc block is all zero bytes and most tests run small
inputs on young contexts, so a forgotten clear, a clear one word short or an over-read past a pad passes there and fails
in a long run.  Here np2_debug_poison fills every block the pools hand out, slack included, with 0x00 (what a fresh block
holds: the control), 0xFF (YAK_EMPTY, "none", the pileup's terminator, every counter's maximum) or 0xA5 (none of those),
and every feature runs a small input A, a larger input B and A again on one context, each against the model the project
already has; the two A results must be identical (the second runs in buffers sized and dirtied by B).

Whoever adds a device buffer adds its feature here."""
import contextlib
import functools
import os

import numpy as np
import pytest

from nextpolish2_amd import BatchPolisher, Opts, Polisher, api
from nextpolish2_amd import io as np2io
from nextpolish2_amd.api import Np2Error
from nextpolish2_amd.synth import Synth
from oracle import np2_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
E_DEVICE = -2  # NP2_E_DEVICE
POISON = (0x00, 0xFF, 0xA5)
FEATURES = {}      # name -> function() -> (results, bytes of the largest device buffer the case is known to take)
_RUNNING = [None]  # (feature, byte) of the case under way, for the message of a device error
_STATE = {"poisoned": False, "dead": False}  # the hook has been on in this process; the device has reported an error


def feature(fn):
    FEATURES[fn.__name__] = fn
    return fn


def device_error(e):
    """Nothing more may run on a device that has reported an error: the session ends here."""
    name, byte = _RUNNING[0] or ("?", None)
    _STATE["dead"] = True
    pytest.exit(f"device error in feature {name} under poison {'off' if byte is None else hex(byte)}: {e}", returncode=3)


@contextlib.contextmanager
def closing(*things):
    """the contexts of a case, closed when it ends — unless the device reported an error"""
    try:
        yield
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(e)
        raise
    finally:
        for t in things:
            if not _STATE["dead"]:
                t.close()


@contextlib.contextmanager
def env(**kw):
    with pytest.MonkeyPatch.context() as mp:
        for k, v in kw.items():
            mp.setenv(k, str(v))
        yield


def frozen(x):
    """a result as plain comparable data, timings left out"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (bytes, str, int, float, bool, type(None))):
        return x
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()) if not k.endswith("_ms"))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    names = getattr(x, "__slots__", None) or sorted(vars(x))
    return tuple((n, frozen(getattr(x, n))) for n in names if not n.endswith("_ms") and not n.startswith("_"))


def same(a, b):
    return frozen(a) == frozen(b)


def pileup_key(pu):
    """what same_pileup compares (the bytes between the reads' streams are nobody's)"""
    from test_frontend_cpu import nib_streams
    return [pu.reads[f] for f in ("aln_t_s", "aln_t_e", "n_cols", "flags")] + [nib_streams(pu)]


def run_feature(name, byte):
    """-> (frozen results, largest buffer, device bytes the hook filled during the case)"""
    _RUNNING[0] = (name, byte)
    _STATE["poisoned"] = _STATE["poisoned"] or byte is not None
    d0 = api.alloc_poison_stats()[0]
    try:
        with api.alloc_poison(byte):
            out, biggest = FEATURES[name]()
    except Np2Error as e:
        if e.code == E_DEVICE:
            device_error(e)
        raise
    return frozen(out), biggest, api.alloc_poison_stats()[0] - d0


# ---- the hook itself -----------------------------------------------------------------------------------------------------------
def test_hook_off_fills_nothing():
    """(first in the file: with the hook never switched on in this process the counters read 0 after a polish)"""
    before = api.alloc_poison_stats()
    s = Synth(20000, depth=15, seed=5, read_len_mean=4000.0, read_len_sd=600.0)
    pol = Polisher([s.yak(21)])
    with closing(pol):
        gb, _ = pol.polish(s.pileup, Opts())
        api.pinned_array(4096)
    assert gb.tobytes() == s.hap1
    assert api.alloc_poison_stats() == before
    if not _STATE["poisoned"]:
        assert before == (0, 0)


def test_pinned_blocks_come_out_poisoned():
    p0 = api.alloc_poison_stats()[1]
    _STATE["poisoned"] = True
    with api.alloc_poison(0xA5):
        a = api.pinned_array(4096)
        assert a.shape == (4096,) and (a == 0xA5).all()
        del a
        b = api.pinned_array(4096)  # the block just released, handed out again
        assert (b == 0xA5).all()
        b[:] = 7
        del b
        with api.alloc_poison(0xFF):
            assert (api.pinned_array(1000, np.uint32) == 0xFFFFFFFF).all()
    assert api.alloc_poison_stats()[1] - p0 >= 3 * 4096


# ---- polish, every stage ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def polish_inputs():
    """A: 9 tiles of 1024 positions, reads crossing 4096-column chunks, long insertions; B: a diploid contig with the vote
    and the recheck passes; tables for k 21 and 31 that hold both"""
    from test_gpu_parity import oracle_traced, wild_pileup
    from test_gpu_trio import scaled_yak
    ref, a = wild_pileup(3, ins_p=0.03, del_p=0.02, sub_p=0.02)
    s = Synth(40000, depth=25, seed=77, diploid=True, read_len_mean=6000.0, read_len_sd=1000.0)
    text = ref.encode() + b"\n" + s.hap1 + b"\n" + s.hap2
    yaks = [scaled_yak(text, k, 30) for k in (21, 31)]
    refs = {"a": oracle_traced(a, yaks, Opts()), "b": oracle_traced(s.pileup, yaks, Opts()), "a3": oracle_traced(a, yaks, Opts(iter_count=3))}
    assert len(refs["b"][0].trace(0, "invalid_ids")) > 0  # (the vote drops reads)
    return a, s.pileup, yaks, refs


def polish_case(iter3=False, **hooks):
    from test_gpu_parity import check_all_stages
    a, b, yaks, refs = polish_inputs()
    with env(**hooks):  # (a context reads its switches when it is made)
        pol = Polisher(yaks)
        with closing(pol):
            a1 = check_all_stages(a, yaks, Opts(), refs["a"], g=pol)
            b1 = check_all_stages(b, yaks, Opts(), refs["b"], g=pol)
            a2 = check_all_stages(a, yaks, Opts(), refs["a"], g=pol)
            assert same(a1, a2)
            out = [a1, b1]
            if iter3:  # pass 2 runs on what pass 1 left
                out.append(check_all_stages(a, yaks, Opts(iter_count=3), refs["a3"], g=pol))
            pol.set_trace(False)
    return out, int(b.nibbles.nbytes)


@feature
def polish():
    return polish_case(iter3=True)


@feature
def polish_front_unfused():
    return polish_case(NP2_FRONT_UNFUSED=1)


@feature
def polish_tile_cap_64():
    return polish_case(NP2_TILE_CAP=64)  # the spill path and the device-wide sort


@functools.lru_cache(maxsize=None)
def batch_inputs():
    specs = [dict(L=20000, seed=304, depth=12), dict(L=30000, seed=302, read_len_mean=4000.0, read_len_sd=700.0),
             dict(L=45000, seed=305, read_err_rate=0.01)]
    syn = [Synth(sp.pop("L"), diploid=True, **sp) for sp in specs]
    yaks = [Synth.yak_assembly(syn, 21), Synth.yak_assembly(syn, 31)]
    o = orc.Oracle(yaks)
    return syn, yaks, [o.polish(s.pileup, Opts()) for s in syn]


@feature
def batch_driver():
    syn, yaks, exp = batch_inputs()
    pol = Polisher(yaks)
    bp = BatchPolisher(pol, 2)  # two slots, three contigs: the second wave runs in the first one's buffers
    with closing(bp, pol):
        contigs = [pol.upload(s.pileup) for s in syn]
        outs = []
        for _ in range(2):
            out = bp.polish(contigs, Opts(), want_pos=True)
            for (b, p), (ob, op) in zip(out, exp):
                assert np.array_equal(b, ob) and np.array_equal(p, op)
            outs.append([(np.array(b), np.array(p)) for b, p in out])
        assert same(outs[0], outs[1])
        for c in contigs:
            c.free()
    return outs[0], max(int(s.pileup.nibbles.nbytes) for s in syn)


@functools.lru_cache(maxsize=None)
def shard_inputs():
    fx = np.load(os.path.join(HERE, "golden", "shards", "shard_votes.npz"))
    s = Synth(120000, seed=881, diploid=True, read_len_mean=7000.0, read_len_sd=1000.0)  # golden/make_shard_fixture.py
    return {k: fx[k] for k in fx.files}, s, [s.yak(21)]


def vote_canon(v):
    o, r = np.argsort(v.pair_key, kind="stable"), np.argsort(v.read_id, kind="stable")
    return [v.pair_key[o], v.pair_cnt[o], v.read_id[r], v.first_pos[r], v.ref_w[r], v.flags[r]]


@feature
def sharded_run():
    from nextpolish2_amd.api import ShardRun, Vote, shard_plan, vote_decide
    from nextpolish2_amd.dist import stitch_shards
    fx, s, yaks = shard_inputs()
    pol = Polisher(yaks)
    with closing(pol):
        outs = []
        for _ in range(2):
            plans = shard_plan(s.pileup, 2, 20000)
            assert np.array_equal(np.array([[getattr(pl, f) for f, _ in pl._fields_] for pl in plans], dtype=np.uint32), fx["plans"])
            ctxs = [pol.clone() for _ in plans]
            with closing(*ctxs):
                runs = [ShardRun(c, s.pileup, pl, Opts(), 1024) for c, pl in zip(ctxs, plans)]
                with closing(*runs):
                    votes = [r.vote() for r in runs]
                    for k, v in enumerate(votes):
                        assert same(vote_canon(v), vote_canon(Vote.from_bytes(fx[f"vote{k}"].tobytes()))), k
                    losers = vote_decide(votes, s.pileup.n_reads, Opts())
                    assert np.array_equal(losers, fx["losers"])
                    for r in runs:
                        r.apply(losers)
                    pieces = [tuple(np.array(x) for x in r.final()) for r in runs]
            for k, (b, p) in enumerate(pieces):
                assert np.array_equal(b, fx[f"piece{k}_bases"]) and np.array_equal(p, fx[f"piece{k}_pos"]), k
            sb, sp = stitch_shards(pieces, plans, 1024)
            assert np.array_equal(sb, fx["oracle_bases"]) and np.array_equal(sp, fx["oracle_pos"])
            outs.append(pieces)
        assert same(outs[0], outs[1])
    return outs[0], len(s.pileup.ref) // 2  # (a shard's stretch of the contig)


# ---- the read front end ------------------------------------------------------------------------------------------------------------
BUNDLE = os.path.join(HERE, "golden", "ref_bundle")
BUNDLE_BAM = os.path.join(BUNDLE, "hifi.map.sort.bam")
ASM = os.path.join(HERE, "golden", "ref_test_asm.fa.gz")


@functools.lru_cache(maxsize=None)
def bundle_front():
    from nextpolish2_amd.bamio import read_bam, records_to_arrays
    (name, ref), = list(np2io.read_fasta(ASM))
    _, recs = read_bam(BUNDLE_BAM)
    arr, cig, seq4, asc, asc_off = records_to_arrays(recs)
    return name, ref, orc.front_end(ref, arr, cig, asc, asc_off, np2io.FrontOpts())


@feature
def contig_from_bam():
    from test_frontend_cpu import same_pileup
    name, ref, exp = bundle_front()
    pol = Polisher([])
    bam = np2io.Bam(BUNDLE_BAM)
    with closing(bam, pol):
        outs = []
        for mode in ("gpu", "libdeflate", "gpu", "libdeflate"):  # the device's inflate and the host pool, each on the other's leftovers
            with env(NP2_INFLATE=mode):
                c = np2io.contig_from_bam(pol, bam, name, ref)
                got = np2io.export_contig(pol, c, np.frombuffer(ref, dtype=np.uint8))
                c.free()
            assert same_pileup(got, exp), mode
            outs.append(pileup_key(got))
        assert same(outs[0], outs[1]) and same(outs[0], outs[2]) and same(outs[0], outs[3])
    return outs[0], os.path.getsize(BUNDLE_BAM)  # (the file's blocks go to the device whole)


@functools.lru_cache(maxsize=None)
def sam_texts():
    import sam_cases as sc
    import sam_model as sm
    a, b = sc.generated(seed=7, n=130), sc.generated(seed=7, n=400)
    assert max(len(ln) for ln in b.split(b"\n")) < 4000 and len(a) > 3 * 4096
    return (a, sm.model(a, "strand")), (b, sm.model(b, "strand"))


@feature
def sam_parse():
    from test_gpu_sam import assert_arrays
    (a, ma), (b, mb) = sam_texts()
    outs = []
    with closing(), env(NP2_SAM_TEST_PIECE=4096):  # records, CIGAR offsets and SEQ offsets carry across the pieces
        for text, m in ((a, ma), (b, mb), (a, ma)):
            *arrays, stats = np2io.sam_parse_bytes(text, tie="strand")
            assert {k: stats[k] for k in m.stats} == m.stats
            assert_arrays(arrays, m.arrays(), "strand")
            outs.append(arrays)
    assert same(outs[0], outs[2])
    return outs[:2], 4096


@functools.lru_cache(maxsize=None)
def sam_contigs(tmp):
    import sam_model as sm
    from nextpolish2_amd.bamio import pileup_to_records, records_to_arrays, write_sam
    ss = [Synth(9000, depth=12, seed=73, diploid=True, read_len_mean=3000.0, read_len_sd=400.0, name="ctgA"),
          Synth(30000, depth=20, seed=71, diploid=True, read_len_mean=5000.0, name="ctgB")]
    recs = []
    for tid, s in enumerate(ss):
        recs += pileup_to_records(s.pileup, tid=tid, rng=np.random.default_rng(5 + tid), decorate=True)
    refs = [(s.pileup.name, s.pileup.L) for s in ss]
    shuffled = [recs[k] for k in np.random.default_rng(8).permutation(len(recs))]
    for i, r in enumerate(shuffled):
        r["name"] = b"read%d" % i
    path = os.path.join(tmp, "shuffled.sam")
    write_sam(path, refs, shuffled)
    m = sm.model(open(path, "rb").read())  # (the model sorts)
    exp = []
    for tid, s in enumerate(ss):
        arr, cig, seq4, asc, asc_off = records_to_arrays([r for r in m.records if r["tid"] == tid])
        exp.append(orc.front_end(s.pileup.ref.tobytes(), arr, cig, asc, asc_off, np2io.FrontOpts()))
    return path, refs, [s.pileup.ref for s in ss], exp


_TMP = []


@pytest.fixture(scope="module", autouse=True)
def _tmp_dir(tmp_path_factory):
    _TMP.append(str(tmp_path_factory.mktemp("dirty")))
    yield
    _TMP.clear()


@feature
def contig_from_sam():
    from test_frontend_cpu import same_pileup
    path, refs, ctg, exp = sam_contigs(_TMP[0])
    pol = Polisher([])
    with closing(pol), env(NP2_SAM_TEST_PIECE=1 << 16):
        assert os.path.getsize(path) > 3 << 16
        sam = np2io.Sam(pol, [path])
        with closing(sam):
            outs = []
            for tid in (0, 1, 0):
                c = np2io.contig_from_sam(pol, sam, refs[tid][0], ctg[tid].tobytes())
                got = np2io.export_contig(pol, c, ctg[tid])
                c.free()
                assert same_pileup(got, exp[tid]), tid
                outs.append(pileup_key(got))
            assert same(outs[0], outs[2])
    return outs[:2], 1 << 16


@functools.lru_cache(maxsize=None)
def depth_inputs():
    import depth_model as dm
    from test_gpu_depth import edge_records
    opts = (dict(min_depth=1, min_len=1), dict(min_depth=2, min_len=3), dict(min_depth=3, min_len=40, min_aligned_fra=1.0))
    cases = []
    for L in (4097, 3 * 8192 + 1):
        recs, cigar = edge_records(L, L)
        cases.append((L, recs, cigar, [dm.model(L, recs, cigar, **o) for o in opts]))
    _, per = dm.read_bam(BUNDLE_BAM)
    return opts, cases, [dm.model(100000, *per[0], **o) for o in (dict(min_depth=60, min_len=1000), dict(min_depth=70, min_len=1))]


def depth_check(got, m):
    from test_gpu_depth import STAT_KEYS
    runs, st, depth = got
    assert depth.dtype == np.uint32 and np.array_equal(depth, m["depth"])
    assert runs.shape == m["runs"].shape and np.array_equal(runs, m["runs"])
    assert {k: st[k] for k in STAT_KEYS} == m["stats"]
    return [runs, {k: st[k] for k in STAT_KEYS}, depth]


@feature
def depth():
    opts, cases, bundle = depth_inputs()
    pol = Polisher([])
    bam = np2io.Bam(BUNDLE_BAM)
    with closing(bam, pol):
        outs = []
        for L, recs, cigar, models in (cases[0], cases[1], cases[0]):
            outs.append([depth_check(api.depth_from_records(pol, L, recs, cigar, want_depth=True, **o), m) for o, m in zip(opts, models)])
        assert same(outs[0], outs[2])
        name, L = bam.refs()[0]
        for mode in ("gpu", "libdeflate"):
            with env(NP2_INFLATE=mode):
                for o, m in zip((dict(min_depth=60, min_len=1000), dict(min_depth=70, min_len=1)), bundle):
                    outs.append(depth_check(np2io.depth_from_bam(pol, bam, name, L, want_depth=True, **o), m))
        assert same(outs[3], outs[5]) and same(outs[4], outs[6])
    return outs[:5], 100000 * 4


# ---- inflate, crc32, k-mer counting, the short-read filters ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inflate_inputs():
    import zlib
    from test_gpu_inflate import bgzf_block

    def run_of(n_blocks, seed):
        r = np.random.default_rng(seed)
        blocks, want = [], []
        for i in range(n_blocks):
            n = int(r.integers(1, 20000))
            text = np.frombuffer((b"GATTACA-%d-" % i) * (n // 8 + 2), dtype=np.uint8)[:n].copy()
            text[r.integers(0, n, n // 50 + 1)] = r.integers(0, 256, n // 50 + 1)
            data, kw = [(bytes(r.integers(0, 256, n, dtype=np.uint8)), dict(level=0)),            # stored
                        (text.tobytes(), dict(level=6, strategy=zlib.Z_FIXED)),                      # fixed codes
                        (text.tobytes(), dict(level=9)),                                             # dynamic codes
                        (b"\xff" * n, dict(level=6)), (b"", dict(level=6))][i % 5]
            blocks.append(bgzf_block(data, **kw))
            want.append(data)
        return b"".join(blocks), b"".join(want)
    return run_of(5, 1), run_of(23, 2)


@feature
def bgzf_inflate_device():
    a, b = inflate_inputs()
    pol = Polisher([])
    with closing(pol):
        outs = []
        for data, want in (a, b, a):
            got, _ = np2io.bgzf_inflate_device(pol, data)
            assert got.tobytes() == want
            outs.append(got)
        assert same(outs[0], outs[2])
    return outs[:2], len(b[1])


@functools.lru_cache(maxsize=None)
def crc_inputs():
    import zlib
    rng = np.random.default_rng(17)
    out = []
    for lens in ([0, 1, 15, 16, 17, 63, 65, 1023, 1025], [3, 65536, 1, 65535, 0, 17, 2049, 65280, 5, 40001, 64, 1024, 7]):
        parts = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        out.append((np.concatenate(parts), off, np.array([zlib.crc32(p.tobytes()) & 0xFFFFFFFF for p in parts], dtype=np.uint32)))
    return out


@feature
def crc32_device():
    a, b = crc_inputs()
    pol = Polisher([])
    with closing(pol):
        outs = []
        for data, off, want in (a, b, a):
            got, _ = np2io.crc32_device(pol, data, off)
            assert np.array_equal(got, want)
            outs.append(got)
    return outs[:2], len(b[0])


@functools.lru_cache(maxsize=None)
def kcount_inputs():
    from test_kcount_cpu import fixture_stream, numpy_count
    s = fixture_stream()
    out = []
    for n in (3 * 8192 - 100, 100000):  # three pieces, and 13 of them
        part = s[:s.rindex(b"\n", 0, n) + 1]
        out.append((part, [numpy_count(part, k, m) for k in (21, 31) for m in (1, 2)]))
    return out


@feature
def count_kmers():
    a, b = kcount_inputs()
    outs = []
    with closing(), env(NP2_KCOUNT_TEST_PIECE=8192, NP2_KCOUNT_TEST_CAP_LOG2=4):  # 16 slots a sub-table: the table grows before a piece's
        # k-mers could fill more than half of it, from the second piece on
        for part, exp in (a, b, a):
            got = []
            for m in (1, 2):
                ys = np2io.count_kmers(part, [21, 31], min_count=m)
                assert np2io.kcount_last_stats()["growths"] >= 1
                got += [(y.k, y.words.copy(), y.bucket_off) for y in ys]  # (the words live in the library's block while the Yak does)
            for (k, w, o), (ew, eo) in zip(sorted(got, key=lambda g: g[0]), exp):
                assert np.array_equal(o, eo) and np.array_equal(w, ew), k
            outs.append(got)
    assert same(outs[0], outs[2])
    return outs[:2], 8192


@functools.lru_cache(maxsize=None)
def srqc_inputs():
    import srqc_model as sm
    o = sm.opts()
    out = []
    for reads in (sm.edge_reads(), sm.generate(n_reads=700) + sm.edge_reads()):  # lengths of every residue mod 16
        out.append((sm.streams(reads), sm.run(reads, o)))
    assert {len(s) % 16 for s, _ in sm.edge_reads()} > {1, 3, 5, 12, 14}
    return o, out


@feature
def srqc_bytes():
    o, (a, b) = srqc_inputs()
    outs = []
    with closing():
        for (seq, qual), (res, masked, totals) in (a, b, a):
            got_masked, got_reads, got_totals = np2io.srqc_bytes(seq, qual, np2io.SrQc(**o), want_masked=True, want_reads=True)
            assert [tuple(r) for r in got_reads.tolist()] == [tuple(r) for r in res]
            assert got_masked == masked and got_totals == totals
            outs.append([got_masked, got_reads, got_totals])
    assert same(outs[0], outs[2])
    return outs[:2], len(b[0][0])


@functools.lru_cache(maxsize=None)
def sradapt_inputs():
    import sradapt_model as am
    import srqc_model as sm
    qc, o = sm.NEUTRAL, am.adopts(seq=am.ADAPTER1, seq2=am.ADAPTER2)  # (the edge pairs are written for the neutral quality options)
    out = []
    for reads in (list(am.edge_pairs()), am.generate(n_pairs=300)[0] + list(am.edge_pairs())):
        out.append((sm.streams(reads), am.run(reads, qc, o)))
    return qc, o, out


@feature
def sradapt_bytes():
    qc, o, (a, b) = sradapt_inputs()
    outs = []
    with closing():
        for (seq, qual), (res, masked, totals) in (a, b, a):
            got_masked, got, got_totals = np2io.sradapt_bytes(seq, qual, np2io.SrQc(**qc), np2io.SrAdapt(**o), want_masked=True, want_reads=True)
            assert [tuple(r) for r in got.tolist()] == [tuple(r) for r in res]
            assert got_masked == masked and got_totals == totals
            outs.append([got_masked, got, got_totals])
    assert same(outs[0], outs[2])
    return outs[:2], len(b[0][0])


# ---- the k-mer scans of an assembly ------------------------------------------------------------------------------------------------------
TILE, HALO = 8192, 32  # csrc/np2_qv_core.hpp, np2_kcount_core.hpp
K = 21


@functools.lru_cache(maxsize=None)
def scan_inputs():
    """two parents a SNP in a hundred apart; sequences of 0, 1, k - 1, k, one tile - 1, + 1 and three tiles + 5 bases cut
    from a text that changes parent every 700 bases, a base in a hundred changed; and the polish the device paths read"""
    from test_gpu_qv import noisy, random_bases, yak_table
    from test_gpu_trio import chimera, parent_yak
    rng = np.random.default_rng(17)
    p = random_bases(rng, 40000)
    m = noisy(rng, p, 0.01)
    base = chimera(p, m, 700)

    def cut(n):
        a = int(rng.integers(0, len(base) - n + 1))
        return noisy(rng, base[a:a + n])
    a = [cut(n) for n in (0, 1, K - 1, K, TILE - 1, TILE + 1)]
    b = [cut(3 * TILE + 5), cut(TILE), b"N" * 100, cut(500).lower(), cut(2 * TILE + 1)]
    s = Synth(20000, depth=15, seed=5, diploid=True, read_len_mean=4000.0, read_len_sd=600.0)
    yaks = [parent_yak(p + b"\n" + s.hap1, K), parent_yak(m + b"\n" + s.hap2, K)]
    return a, b, yaks, [yak_table(y) for y in yaks], s, orc.Oracle(yaks).polish(s.pileup, Opts())


def qv_check(r, seqs, table):
    from test_qv_cpu import numpy_qv
    e_hist = np.zeros(1024, np.uint64)
    for i, s in enumerate(seqs):
        nk, na, h, bits = numpy_qv(s, K, table, 1)
        assert (int(r.stats[i, 0]), int(r.stats[i, 1])) == (nk, na), (i, len(s))
        assert np.array_equal(r.bits[i], bits), (i, len(s))
        e_hist += h
    assert np.array_equal(r.hist, e_hist)
    return r


@feature
def qv():
    a, b, yaks, tables, s, (ob, op) = scan_inputs()
    pol = Polisher(yaks)
    with closing(pol), env(NP2_QV_TEST_STAGE_TILES=2):  # sequences go on from piece to piece
        outs = [qv_check(pol.qv_strings(0, seqs, 1, hist=True, bits=True), seqs, tables[0]) for seqs in (a, b, a)]
        assert same(outs[0], outs[2])
        gb, _ = pol.polish(s.pileup, Opts())
        assert np.array_equal(gb, ob)
        ptr, n = pol.last_result_device()
        seq = gb.tobytes()
        for skip, drop in ((0, 0), (3, 5), (HALO + 1, TILE + 3), (0, 0)):  # any alignment, any end
            sub = seq[skip:len(seq) - drop]
            outs.append(qv_check(pol.qv_device(1, ptr + skip, len(sub), 1, hist=True, bits=True), [sub], tables[1]))
        assert same(outs[3], outs[6])
    return outs[:6], 2 * TILE


def trio_check(r, seqs, tp, tm):
    from test_trio_cpu import numpy_trio
    for i, s in enumerate(seqs):
        e_stats, e_pb, e_mb = numpy_trio(s, K, tp, tm, 2, 5)
        assert tuple(int(x) for x in r.stats[i]) == e_stats, (i, len(s))
        assert np.array_equal(r.pat_bits[i], e_pb) and np.array_equal(r.mat_bits[i], e_mb), (i, len(s))
    return r


@feature
def trio():
    a, b, yaks, (tp, tm), s, (ob, op) = scan_inputs()
    pol = Polisher(yaks)
    with closing(pol), env(NP2_TRIO_TEST_STAGE_TILES=2, NP2_TRIO_TEST_BLOCKS=3):
        outs = [trio_check(pol.trio_strings(0, 1, seqs, 2, 5, bits=True), seqs, tp, tm) for seqs in (a, b, a)]
        assert same(outs[0], outs[2]) and sum(outs[1].total[1:3]) > 0
        gb, _ = pol.polish(s.pileup, Opts())
        assert np.array_equal(gb, ob)
        ptr, n = pol.last_result_device()
        seq = gb.tobytes()
        for skip, drop in ((0, 0), (3, 5), (HALO + 1, TILE + 3), (0, 0)):
            sub = seq[skip:len(seq) - drop]
            outs.append(trio_check(pol.trio_device(0, 1, ptr + skip, len(sub), 2, 5, bits=True), [sub], tp, tm))
        assert same(outs[3], outs[6])
    return outs[:6], 2 * TILE


@functools.lru_cache(maxsize=None)
def bin_expected():
    from test_triobin_cpu import brute_force
    a, b, yaks, (tp, tm), _, _ = scan_inputs()
    reads_a = a + [b""] * 3 + a[2:4]
    reads_b = b + a + [b[0][:700]] * 40
    return [(r, brute_force(r, K, tp, tm, 2, 5, 2, 330)) for r in (reads_a, reads_b)]


@feature
def bin_stream():
    a, b = bin_expected()
    yaks = scan_inputs()[2]
    pol = Polisher(yaks)
    with closing(pol), env(NP2_BIN_TEST_STAGE_TILES=2, NP2_BIN_TEST_BLOCKS=3):
        outs = []
        for reads, exp in (a, b, a):
            r = pol.bin_stream(0, 1, reads, 2, 5, 2, 330, stats=True)
            assert len(r.classes) == len(reads) and r.stats.shape == (len(reads), 7)
            for i, (e_stats, e_cls) in enumerate(exp):
                assert tuple(int(x) for x in r.stats[i]) == e_stats and chr(r.classes[i]) == e_cls, (i, len(reads[i]))
            outs.append(r)
        assert same(outs[0], outs[2])
    return outs[:2], 2 * TILE


def cmp_check(pol, seqs, table):
    from test_cmp_cpu import check_identities, numpy_cmp
    r = pol.cmp_strings(0, seqs, 1, spectra=True)
    stats, spectra, asm_only = numpy_cmp(seqs, K, table, 1)
    assert r.stats == stats
    assert np.array_equal(r.spectra, spectra) and np.array_equal(r.asm_only, asm_only)
    check_identities(r.stats, r.spectra, r.asm_only, 1)
    return r


@feature
def cmp():
    a, b, yaks, tables, _, _ = scan_inputs()
    pol = Polisher(yaks)
    with closing(pol), env(NP2_CMP_TEST_BLOCKS=3):
        outs = [cmp_check(pol, seqs, tables[0]) for seqs in (a, b + b[:1], a)]  # (a sequence twice: copy number 2)
        assert same(outs[0], outs[2]) and outs[1].n_found > 0 and int(outs[1].spectra[2].sum()) > 0
    return outs[:2], sum(len(x) for x in b)


@feature
def rep_bytes():
    from test_gpu_rep import model, same as same_rep, stream_of
    outs = []
    with closing(), env(NP2_REP_TEST_PIECE=4096):
        for n, k in ((8193, 8), (24577, 8), (8193, 8), (8193, 3), (24577, 3), (8193, 3)):
            got = api.rep_bytes(stream_of(n), k=k, min_count=1)
            same_rep(got, model(n, k, min_count=1))
            outs.append([got[0], got[1], {f: v for f, v in got[2].items() if not f.endswith("_ms")}])
    assert same(outs[0], outs[2]) and same(outs[3], outs[5])
    return outs, 4 ** 8 * 4  # the counters of k = 8: the driver's own block, filled like a pool's


# ---- edits ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edits_inputs():
    import edits_cases as Cs
    from test_gpu_edits import GENOME, genome_case
    ref = GENOME[3000:9000]
    other = GENOME[20000:21000]
    pieces, at = [], 0
    for start, ln, text in ((100, 65, other[:3]), (300, 3, other[10:75]), (600, 300, other[100:107]), (1100, 5, other[200:500]),
                            (1600, 300, ref[1600:1750] + b"N" + ref[1751:1900]), (3300, 65, ref[3300:3364] + other[:1] + ref[3364:3365]),
                            (3600, 300, other[600:900])):  # REF and ALT of 65 and of 300 bytes: the wavefront path
        pieces += [(ref[at:start], at), (text, [start] * len(text))]
        at = start + ln
    pieces.append((ref[at:], at))
    return [genome_case(100 + 8193, 8193, rate=0.03), genome_case(100 + 3 * 8192 + 5, 3 * 8192 + 5, rate=0.03), (ref,) + tuple(Cs.out_of(*pieces))]


@feature
def edits():
    import edits_model as M
    from test_gpu_edits import Ctx, DUMPS, same_as_model
    a, b, w = edits_inputs()
    c = Ctx()
    with closing(c.pol):
        outs = []
        for ref, bases, pos in (a, w, b, a, w):
            res, recs, tot = same_as_model(c.pol, c.tables, ref, bases, pos)
            assert len(recs) > 3
            outs.append(res)
        assert same(outs[0], outs[3]) and same(outs[1], outs[4])
    # the consensus the polish left on the device
    (name, ref), = list(np2io.read_fasta(ASM))
    yaks = [np2io.load_yak(p) for p in DUMPS]
    pol = Polisher(yaks)
    bam = np2io.Bam(BUNDLE_BAM)
    with closing(bam, pol):
        ct = np2io.contig_from_bam(pol, bam, name, ref, np2io.FrontOpts())
        for _ in range(2):
            bb, pp = pol.polish_resident(ct, Opts())
            last = pol.edits_last(ct)
            res, recs, tot = same_as_model(pol, [M.Table(y) for y in yaks], ref, bb.tobytes(), pp)
            assert last.records() == res.records() and last.totals == res.totals and np.array_equal(last.support, res.support)
            outs.append(last)
        assert same(outs[5], outs[6]) and len(outs[5]) > 0
        ct.free()
    return outs[:6], 3 * 8192 + 5


# ---- one context, one feature after the other ------------------------------------------------------------------------------------------------
@feature
def mixed_order():
    """the A cases in the order polish, qv, edits, trio, cmp, polish, depth on ONE context with two tables: what one feature
    leaves in the context's shared scratch must not reach the next"""
    import edits_model as M
    from test_gpu_edits import same_as_model
    a, _, yaks, tables, s, (ob, op) = scan_inputs()
    opts, cases, _ = depth_inputs()
    ea = edits_inputs()[0]
    pol = Polisher(yaks)
    with closing(pol):
        outs = []
        for _ in range(2):
            gb, gp = pol.polish(s.pileup, Opts())
            assert np.array_equal(gb, ob) and np.array_equal(gp, op)
            out = [gb, gp, qv_check(pol.qv_strings(0, a, 1, hist=True, bits=True), a, tables[0])]
            out.append(same_as_model(pol, [M.Table(y) for y in yaks], *ea)[0])
            out.append(trio_check(pol.trio_strings(0, 1, a, 2, 5, bits=True), a, *tables))
            out.append(cmp_check(pol, a, tables[0]))
            gb, gp = pol.polish(s.pileup, Opts())
            assert np.array_equal(gb, ob) and np.array_equal(gp, op)
            L, recs, cigar, models = cases[0]
            out.append(depth_check(api.depth_from_records(pol, L, recs, cigar, want_depth=True, **opts[0]), models[0]))
            outs.append(out)
        assert same(outs[0], outs[1])
    return outs[0], int(s.pileup.nibbles.nbytes)


# ---- every (feature, byte) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", POISON, ids=["0x%02X" % b for b in POISON])
@pytest.mark.parametrize("name", list(FEATURES))
def test_feature_on_poisoned_blocks(name, byte):
    out, biggest, grew = run_feature(name, byte)
    print(f"{name} 0x{byte:02X}: poisoned device bytes {grew}, largest known buffer {biggest}")
    assert grew >= biggest  # the case really took poisoned blocks
    if byte == 0x00:  # the control: zero-filled blocks are what fresh ones are, so nothing may differ from the hook off
        off, _, grew_off = run_feature(name, None)
        assert grew_off == 0
        assert out == off
