"""The assembly-to-reference caller on the device (csrc/np2_asmcall.hip): np2_asmcall held byte for byte to the host twin
np2_asmcall_host (which tests/test_asmcall_cpu.py holds to the model) on every hand-built and seeded random case, on recycled
memory poisoned with every byte of test_gpu_dirty_memory.POISON, its refusals with the context usable afterwards, and the
module end to end through MapIndex.align on the known answers.

Every check runs on the device in a child process (one child runs them all on one context and reports each outcome; the
poisoned runs have a child each): this process never opens the device, so what a later module finds in recycled device
memory does not depend on this one."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile
import traceback

import numpy as np
import pytest

import asmcall_model as am
import test_asmcall_cpu as cpu
from nextpolish2_amd import api, asmcall
from test_gpu_dirty_memory import POISON

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the checks: each takes the child's Polisher and raises when it does not hold ---------------------------------------------------
def same_as_host(pol, refs, alignments, **opts):
    """np2_asmcall and np2_asmcall_host on one input: equal byte for byte -> the device's result"""
    query, alns, cigar = am.pack(alignments)
    h_runs, h_vars, h_st, h_cov = api.asmcall_host(refs, query, alns, cigar, want_cov=True, **opts)
    runs, vars_, st, cov = api.asmcall(pol, refs, query, alns, cigar, want_cov=True, **opts)
    assert runs.tobytes() == h_runs.tobytes(), (runs, h_runs)
    assert vars_.tobytes() == h_vars.tobytes(), (vars_, h_vars)
    assert np.array_equal(cov, h_cov)
    assert {k: st[k] for k in am.STAT_KEYS} == {k: h_st[k] for k in am.STAT_KEYS}
    assert st["kernel_ms"] >= 0 and set(st["stage_ms"]) == set(api.ASMCALL_STAGES)
    return runs, vars_, st


def check_random(pol, seed):
    refs, alignments = am.random_case(seed, n_refs=1 + seed % 3, n_alns=6 + seed, max_ops=30 + 15 * seed)
    same_as_host(pol, refs, alignments, min_mapq=5, min_aln=20)


def big_case():
    """more than one block of every look-back kernel: 20 011 reference bases in three references, 300 alignments, hundreds of
    runs, more than 8192 events found"""
    rng = am.random.Random(99)
    refs = [am.random_seq(rng, n) for n in (9001, 17, 10993)]
    out = []
    for i in range(300):
        tid = rng.choice((0, 0, 2))
        L = len(refs[tid])
        n = rng.randint(40, 140)
        pos = rng.randrange(L - n - 10)
        ops = [("S", 2), ("M", n // 3), ("I", 1 + i % 3), ("M", n // 3), ("D", 1 + i % 4), ("M", n - 2 * (n // 3))]
        qn = 2 + n + 1 + i % 3
        out.append(am.aln(refs[tid], pos, ops, rev=bool(i & 1), mism=range(2, qn, 2), tid=tid, own=(rng.randint(0, 10), qn - rng.randint(0, 10))))
    out.append(am.aln(refs[1], 0, [("M", 17)], tid=1, mism=(0, 16)))
    return refs, out


def check_across_blocks(pol):
    refs, alignments = big_case()
    _, _, st = same_as_host(pol, refs, alignments, min_mapq=5, min_aln=30)
    assert st["found_snv"] + st["found_del"] + st["found_ins"] > 8192 and st["runs"] > 10 and st["cov2_bases"] > 1000


REFUSALS = [c for c in cpu.refusal_inputs() if c[1] and not c[0].startswith("NULL")]  # (NULL arguments: check_null_context_and_outputs)


def check_refusal(pol, case):
    """the refusal, and the context serves the next call"""
    name, want, kw = case
    refs, off = kw["refs"], kw.get("ref_off")
    L = api.lib()
    cat = np.frombuffer(b"".join(refs), dtype=np.uint8)
    ro = np.array(off if off is not None else [0, len(cat)], dtype=np.uint64)
    q, alns, cigar = np.frombuffer(kw["query"], dtype=np.uint8), kw["alns"], kw["cigar"]
    o, st = api.np2_asmcall_opts_t(5, 1), api.np2_asmcall_stats_t()
    pr, pv, nr, nv = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    rc = L.np2_asmcall(pol._h, cat.ctypes.data, ro.ctypes.data, kw.get("n_refs", 1), q.ctypes.data, len(q), alns.ctypes.data, len(alns), cigar.ctypes.data,
                       len(cigar), C.byref(o), C.byref(pr), C.byref(nr), C.byref(pv), C.byref(nv), None, C.byref(st))
    assert rc == want and not pr.value and not pv.value
    good = cpu.refusal_inputs()[0][2]
    runs, vars_, st, _ = api.asmcall(pol, good["refs"], good["query"], good["alns"], good["cigar"], min_aln=1)
    assert runs.tolist() == [(0, 5, 45)] and len(vars_) == 1 and st["kept_ins"] == 1


def check_null_context_and_outputs(pol):
    L = api.lib()
    good = cpu.refusal_inputs()[0][2]
    cat, ro = np.frombuffer(good["refs"][0], dtype=np.uint8), np.array([0, 60], dtype=np.uint64)
    q = np.frombuffer(good["query"], dtype=np.uint8)
    o = api.np2_asmcall_opts_t(5, 1)
    pr, pv, nr, nv = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    tail = [C.byref(pr), C.byref(nr), C.byref(pv), C.byref(nv), None, None]
    head = [cat.ctypes.data, ro.ctypes.data, 1, q.ctypes.data, len(q), good["alns"].ctypes.data, 1, good["cigar"].ctypes.data, len(good["cigar"])]
    assert L.np2_asmcall(None, *head, C.byref(o), *tail) == cpu.E_ARG
    assert L.np2_asmcall(pol._h, *head, None, *tail) == cpu.E_ARG
    assert L.np2_asmcall(pol._h, *head, C.byref(o), None, C.byref(nr), C.byref(pv), C.byref(nv), None, None) == cpu.E_ARG
    assert L.np2_asmcall(pol._h, *head, C.byref(o), *tail) == 0 and nr.value == 1
    for p in (pr, pv):
        if p.value:
            L.np2_free(p)


def check_bundle(pol, swapped):
    a, b = cpu.read_fa(cpu.ASM), cpu.read_fa(cpu.EXPECTED)
    refs, contigs = (b, a) if swapped else (a, b)
    text, rows, st = asmcall.call(refs, contigs, pol=pol)
    cpu.check_bundle(text, rows, st, swapped)
    assert st["kernel_ms"] > 0


def check_planted(pol):
    truth, edited, want = cpu.planted()
    for seg, overlap in cpu.TILINGS:
        for rev in (False, True):
            q = am.revcomp(edited) if rev else edited
            text, _, st = asmcall.call([("truth", truth)], [("asm", q)], seg=seg, overlap=overlap, min_aln=seg // 2, pol=pol)
            cpu.check_planted(text, st, len(truth), want, rev)


def check_module_files(pol):
    with tempfile.TemporaryDirectory() as td:
        out, summary, host = os.path.join(td, "calls.txt.gz"), os.path.join(td, "s.tsv"), os.path.join(td, "host.txt")
        assert asmcall.main([cpu.ASM, cpu.EXPECTED, "-o", out, "--summary", summary]) == 0
        text = gzip.open(out, "rt").read()
        assert len(cpu.lines(text, "R")) == 1 and [l[2] for l in cpu.lines(text, "V")] == ["63156", "76368", "79624", "81108"]
        assert asmcall.main([cpu.ASM, cpu.EXPECTED, "-o", host, "--host"]) == 0
        assert open(host).read() == text  # (the host twins give the same file)
        assert open(summary).read().split("\n")[2].split("\t")[:6] == ["total", "100000", "0", "0", "4", "4"]


CHECKS = {}
for _c in cpu.CASES:
    CHECKS["hand/" + _c[0]] = lambda pol, c=_c: same_as_host(pol, c[1], c[2], **c[3])
for _s in range(12):
    CHECKS["random/%d" % _s] = lambda pol, s=_s: check_random(pol, s)
for _c in REFUSALS:
    CHECKS["refusal/" + _c[0]] = lambda pol, c=_c: check_refusal(pol, c)
CHECKS.update({"blocks": check_across_blocks, "null": check_null_context_and_outputs, "bundle/False": lambda pol: check_bundle(pol, False),
               "bundle/True": lambda pol: check_bundle(pol, True), "planted": check_planted, "module": check_module_files})


def run_checks(out_path):
    """the child: every check on one context, in order -> {name: "ok" or the traceback} as JSON.  A device error ends it (exit 3)."""
    from nextpolish2_amd import Polisher
    pol, out = Polisher([]), {}  # (no k-mer table: the caller needs the device only)
    for name, check in CHECKS.items():
        try:
            check(pol)
            out[name] = "ok"
        except api.Np2Error as e:
            out[name] = traceback.format_exc()
            if e.code == -2:
                print(name, e, file=sys.stderr)
                sys.exit(3)
        except Exception:
            out[name] = traceback.format_exc()
    pol.close()
    with open(out_path, "w") as f:
        json.dump(out, f)


_CHILD = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_asmcall as t\nt.run_checks(sys.argv[1])\n" % (ROOT, HERE)


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gpu_asmcall") / "outcome.json")
    r = subprocess.run([sys.executable, "-c", _CHILD, path], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=600)
    if r.returncode == 3 or r.returncode < 0:
        pytest.exit(f"device error in the assembly caller: {r.stderr.decode(errors='replace')[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    return json.load(open(path))


@pytest.mark.parametrize("name", [c[0] for c in cpu.CASES])
def test_device_equals_host_twin_on_hand_built(outcome, name):
    assert outcome["hand/" + name] == "ok", outcome["hand/" + name]


@pytest.mark.parametrize("seed", range(12))
def test_device_equals_host_twin_on_random(outcome, seed):
    assert outcome["random/%d" % seed] == "ok", outcome["random/%d" % seed]


def test_device_equals_host_twin_across_blocks(outcome):
    assert outcome["blocks"] == "ok", outcome["blocks"]


@pytest.mark.parametrize("name", [c[0] for c in REFUSALS])
def test_device_refusals_leave_the_context_usable(outcome, name):
    assert outcome["refusal/" + name] == "ok", outcome["refusal/" + name]


def test_null_context_and_outputs(outcome):
    assert outcome["null"] == "ok", outcome["null"]


_POISON_CODE = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import test_gpu_asmcall as t\n"
                "from nextpolish2_amd import Polisher, api\n"
                "byte = int(sys.argv[1])\n"
                "try:\n"
                "    with api.alloc_poison(byte):\n"
                "        p = Polisher([])\n"
                "        small = [c for c in t.cpu.CASES if c[0] in ('161 words -', 'DEL across a coverage change +', 'last base -', 'two references +')]\n"
                "        big = t.big_case()\n"
                "        for c in small:\n"
                "            t.same_as_host(p, c[1], c[2], **c[3])\n"
                "        t.same_as_host(p, big[0], big[1], min_mapq=5, min_aln=30)\n"
                "        for c in small:\n"
                "            t.same_as_host(p, c[1], c[2], **c[3])\n"
                "        p.close()\n"
                "    assert api.alloc_poison_stats()[0] > 0\n"
                "except api.Np2Error as e:\n"
                "    print(e, file=sys.stderr)\n"
                "    sys.exit(3 if e.code == -2 else 1)\n" % (ROOT, HERE))


@pytest.mark.parametrize("byte", POISON)
def test_on_poisoned_recycled_blocks(byte):
    """small cases, the larger one and the small ones again on one context, every pool block filled with `byte` before it is
    handed out: every result is the host twin's (the second round runs in buffers sized and dirtied by the larger case).  A
    process of its own: the hook's counters are the process's."""
    r = subprocess.run([sys.executable, "-c", _POISON_CODE, str(byte)], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    if r.returncode == 3 or r.returncode < 0:
        pytest.exit(f"device error in the assembly caller under poison {byte:#x}: {r.stderr.decode(errors='replace')[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]


# ---- the module, end to end through MapIndex.align ------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True])
def test_bundle_known_answer(outcome, swapped):
    assert outcome["bundle/%s" % swapped] == "ok", outcome["bundle/%s" % swapped]


def test_planted_edits(outcome):
    assert outcome["planted"] == "ok", outcome["planted"]


def test_module_writes_bgzf_and_summary(outcome):
    assert outcome["module"] == "ok", outcome["module"]
