"""The C-ABI library loads and exports every symbol include/np2.h declares (no compute without a GPU)."""
import ctypes as C
import os
import re

import pytest

from nextpolish2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name="np2.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(np2_[a-z_0-9]+)\s*\(", txt)))


def test_header_declares_expected_entry_points():
    syms = header_symbols()
    assert set(syms) == set(api.ABI_SYMBOLS)


def test_library_exports_every_declared_symbol():
    L = api.lib()
    for s in header_symbols() + header_symbols("np2_io.h"):
        assert hasattr(L, s), s


def test_io_header_declares_expected_entry_points():
    assert set(header_symbols("np2_io.h")) == set(api.IO_ABI_SYMBOLS)


def test_struct_layouts_match_header():
    from nextpolish2_amd._types import np2_opts_t, np2_read_t, np2_yak_t
    assert C.sizeof(np2_read_t) == 24 and np2_read_t.nib_off.offset == 8 and np2_read_t.n_cols.offset == 16
    assert C.sizeof(np2_yak_t) == 32 and np2_yak_t.words.offset == 16
    assert C.sizeof(np2_opts_t) == 16 and np2_opts_t.max_indel_len.offset == 4 and np2_opts_t.model_ref.offset == 12


def test_product_never_imports_the_oracle():
    # the oracle is test infrastructure: nothing under nextpolish2_amd/ may reference it
    pkg = os.path.join(ROOT, "nextpolish2_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".sh")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "np2_oracle" not in txt and "np2o_" not in txt and "oracle/" not in txt.replace("no oracle", ""), f


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    from nextpolish2_amd import Polisher
    from nextpolish2_amd._types import Yak
    y = Yak(21, np.zeros(0, np.uint64), np.zeros(1025, np.uint64))
    with pytest.raises(api.Np2Error) as e:
        Polisher([y])
    assert e.value.code == -2  # NP2_E_DEVICE


def test_product_phasing_vote_agrees_with_the_oracle_on_random_signed_graphs():
    """Two independent restatements of louvain.rs + hashbrown iteration order (oracle/hashbrown_emul.hpp vs
    csrc/np2_phase_host.hpp, the latter with edge-driven aggregation) must pick the same losing reads, including on
    tie-heavy graphs where only the emulated bucket order decides."""
    import numpy as np
    from nextpolish2_amd.api import phase_vote
    from oracle import np2_oracle as orc
    rng = np.random.default_rng(12)
    for trial in range(120):
        n = int(rng.integers(3, 70))
        ids = rng.choice(np.arange(1, 400), size=n, replace=False)
        pairs = {}
        m = int(rng.integers(n, 4 * n))
        for _ in range(m):
            a, b = rng.choice(ids, size=2, replace=False)
            a, b = int(min(a, b)), int(max(a, b))
            # clustered signs: same "haplotype" (id parity) mostly positive, so conflicts are genuine; small integer
            # weights make ties between communities frequent
            same = (a % 2) == (b % 2)
            w = float(rng.integers(1, 3)) * (1.0 if (same or rng.random() < 0.1) else -1.0)
            if rng.random() < 0.05:
                w = -3.0
            pairs[(a, b)] = pairs.get((a, b), 0.0) + w
        plist = [(a, b, w) for (a, b), w in pairs.items()]
        # the oracle applies insert_data(a, b) then insert_data(b, a) per pair in this order
        edges, keys, seen = [], [], set()
        for a, b, w in plist:
            edges.append((a, b, w))
            edges.append((b, a, w))
            for k in (a, b):
                if k not in seen:
                    seen.add(k)
                    keys.append(k)
        ref = None
        if trial % 3 == 0:
            ref = {int(k): float(rng.choice([-1.0, 1.0, 2.0])) for k in rng.choice(ids, size=max(1, n // 3), replace=False)}
        try:
            exp = orc.phase_communities(edges, ref)
        except orc.RefPanic:
            with pytest.raises(api.Np2Error):
                phase_vote(keys, plist, ref)
            continue
        assert phase_vote(keys, plist, ref) == exp, trial


def test_abi_guard_turns_every_exception_into_a_status(tmp_path):
    """csrc/np2_abi.hpp (host-only) built on its own: a returned code passes through, an Np2Error keeps its code and
    message, any other exception becomes NP2_E_NOMEM with "unexpected exception", and the sink runs only after a throw."""
    import subprocess
    exe = str(tmp_path / "abi_guard_test")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "tools", "abi_guard_test.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-3000:]


def _bgzf_file(path, payload):
    from nextpolish2_amd.bamio import _Bgzf
    with open(path, "wb") as f:
        z = _Bgzf(f)
        z.write(payload, atomic=False)
        z.close()


def test_device_free_entry_points_report_bad_input_as_status(tmp_path):
    """Bad input to the entry points that need no device comes back as an NP2_E_* status with its message (the same
    codes and texts the command line and the Python layer have always relayed), never as an abort."""
    import struct
    import numpy as np
    from nextpolish2_amd import bamio, io
    from nextpolish2_amd._types import READ_DTYPE, Pileup
    E_ARG, E_REFPANIC = -1, -5

    missing = str(tmp_path / "missing.fa")
    with pytest.raises(api.Np2Error) as e:
        list(io.read_fasta(missing))
    assert e.value.code == E_ARG and "cannot open" in str(e.value) and missing in str(e.value)
    with pytest.raises(api.Np2Error) as e:
        io.polisher_from_yak_files([str(tmp_path / "missing.yak")])
    assert e.value.code == E_ARG and "cannot open" in str(e.value)

    bad_magic = tmp_path / "bad.yak"
    bad_magic.write_bytes(b"KAY\2" + struct.pack("<III", 21, 10, 10))
    with pytest.raises(api.Np2Error) as e:
        io.load_yak(str(bad_magic))
    assert e.value.code == E_ARG and "incompatible" in str(e.value)
    cut_short = tmp_path / "short.yak"  # a valid header, then 3 of the 1024 bucket headers
    cut_short.write_bytes(b"YAK\2" + struct.pack("<III", 21, 10, 10) + struct.pack("<II", 0, 0) * 3)
    with pytest.raises(api.Np2Error) as e:
        io.load_yak(str(cut_short))
    assert e.value.code == E_ARG and "Failed to parse" in str(e.value)

    text = tmp_path / "text.bam"
    text.write_bytes(b"@HD\tVN:1.6\n")
    with pytest.raises(api.Np2Error) as e:
        io.Bam(str(text))
    assert e.value.code == E_ARG and "not a BGZF block" in str(e.value)
    junk = str(tmp_path / "junk.bam")
    _bgzf_file(junk, b"SAM\1" + bytes(64))
    with pytest.raises(api.Np2Error) as e:
        io.Bam(junk)
    assert e.value.code == E_ARG and "not a BAM file" in str(e.value)
    unindexed = str(tmp_path / "unindexed.bam")
    bamio.write_bam(unindexed, [("ctg", 100)], [])
    os.remove(unindexed + ".bai")
    with pytest.raises(api.Np2Error) as e:
        io.Bam(unindexed)
    assert e.value.code == E_ARG and "Faield random access BAM/SAM!" in str(e.value)

    L = 3000  # room for three 1024-aligned shards at most
    reads = np.zeros(1, dtype=READ_DTYPE)
    reads[0] = (0, L - 1, 0, L, 0)
    pileup = Pileup(b"A" * L, reads, np.zeros(L // 2 + 32, np.uint8))
    assert len(api.shard_plan(pileup, 2)) == 2
    with pytest.raises(api.Np2Error) as e:
        api.shard_plan(pileup, 4)
    assert e.value.code == E_ARG

    # a NaN weight: the net weight between two final communities is neither zero nor negative (louvain.rs's conflict
    # check panics on it)
    with pytest.raises(api.Np2Error) as e:
        api.phase_vote([1, 2, 3], [(1, 2, -1.0), (1, 3, -1.0), (2, 3, float("nan"))])
    assert e.value.code == E_REFPANIC


def test_bam_open_reports_damaged_bgzf_headers(tmp_path):
    """The stream that reads a BAM's header parses its blocks with the parser every reader shares (csrc/np2_bgzf.hpp): a BC
    subfield whose value would lie beyond the extra field, a block size too small for header and trailer, and a file
    shorter than a header are statuses with their messages (no device is needed to open a BAM)."""
    import struct
    from nextpolish2_amd import io
    E_ARG = -1

    def head(extra):
        return struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, len(extra)) + extra
    cases = {
        # XLEN 4: the BC subfield's header ends the extra field; the payload's first bytes stand where BSIZE would be
        "bc_cut.bam": (head(b"BC\2\0") + b"\x1b\0" + b"\3\0" + bytes(8), "BGZF block without BC field"),
        # BSIZE = 12 + XLEN + 7
        "small.bam": (head(b"BC\2\0" + struct.pack("<H", 12 + 6 + 7 - 1)) + b"\3\0" + bytes(8), "truncated BGZF block"),
        "17.bam": ((head(b"BC\2\0" + struct.pack("<H", 27)) + b"\3\0" + bytes(8))[:17], "not a BGZF block"),
    }
    for name, (data, msg) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises(api.Np2Error) as e:
            io.Bam(str(path))
        assert e.value.code == E_ARG and msg in str(e.value), (name, str(e.value))


def test_poison_hook_round_trips_its_setting_without_a_device():
    """np2_debug_poison returns the old setting (off by default, any byte 0..255, off again) and touches no device; in a
    process that has allocated nothing np2_debug_poison_stats reads 0, with either pointer NULL too.  (A child process:
    the counters are process-wide and this one may have polished under poison already.)"""
    import subprocess
    import sys
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "from nextpolish2_amd import api\n"
            "L = api.lib()\n"
            "assert api.alloc_poison_stats() == (0, 0)\n"
            "assert L.np2_debug_poison(0xA5) == -1 and L.np2_debug_poison(0) == 0xA5 and L.np2_debug_poison(255) == 0\n"
            "assert L.np2_debug_poison(-7) == 255 and L.np2_debug_poison(-1) == -1\n"
            "with api.alloc_poison(0xFF):\n"
            "    with api.alloc_poison(None):\n"
            "        assert L.np2_debug_poison(-1) == -1\n"
            "    assert L.np2_debug_poison(0xFF) == 0xFF\n"  # (the inner block put back what it found)
            "assert L.np2_debug_poison(-1) == -1\n"
            "d = C.c_uint64(7); L.np2_debug_poison_stats(C.byref(d), None); assert d.value == 0\n"
            "p = C.c_uint64(7); L.np2_debug_poison_stats(None, C.byref(p)); assert p.value == 0\n"
            "print('ok')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-3000:]
