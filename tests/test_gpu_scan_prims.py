"""The scan primitives of libnp2_hip.so against numpy, at the sizes where their kernels switch or split.

The pipeline reaches these kernels only at the sizes a contig happens to produce; here each one runs through
tests/tools/prims_harness.hip (a host-only shim that calls the library's own np2::launch_* / np2::prim_*) on chosen
lengths: block and octet edges, the 64-block window of the look-back walk, the one-block / look-back and short-scan /
rocPRIM switch points.  Every array carries canaries past what the kernel may write; every look-back launch starts from a
caller-chosen ticket, epoch and status pre-fill and must leave the error word clear."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nextpolish2_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
CANARY = 0xA5C3F00D
EPOCH_MASK = (1 << 30) - 1
LB_PREFIX = 2  # status word state of a published inclusive prefix (np2_lookback.hpp)
SCAN_LB_BLOCK = 8192  # elements per block of k_scan_lb_excl (np2_cand.hip: SCAN_LB_ITEMS * SCAN_LB_THREADS)
TILE_LB_BLOCK = 1024  # tiles per block of k_tile_layout_lb / k_tile_offsets_lb (256 threads x TLB_ITEMS)
CAND_LB_REGIONS = 4096  # regions per block of k_cand_offsets_lb (256 threads x 4 region blocks of 4)

u32p, u64p, i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)


class LbSpec(C.Structure):
    _fields_ = [("status", u64p), ("n_status", C.c_uint32), ("epoch", C.c_uint32), ("ticket", u32p), ("err", u32p)]


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    """tests/tools/prims_harness.hip built against the library under test (flags as in csrc/build.sh)."""
    libdir = os.path.dirname(os.path.abspath(api.LIB_PATH))
    out = str(tmp_path_factory.mktemp("prims") / "libprims_harness.so")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
                        "-fno-omit-frame-pointer", "-x", "hip", "-shared", "-o", out,
                        os.path.join(ROOT, "tests", "tools", "prims_harness.hip"), "-L" + libdir, "-lnp2_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    api.lib()
    L = C.CDLL(out)
    for f in ("ph_scan_lb_blocks", "ph_tile_scan_blocks", "ph_cand_offsets_blocks"):
        getattr(L, f).restype = C.c_uint32
    L.ph_scan_lb_blocks.argtypes = [C.c_uint64]
    L.ph_tile_scan_blocks.argtypes = L.ph_cand_offsets_blocks.argtypes = [C.c_uint32]
    L.ph_scan_lb.argtypes = [C.c_int, u32p, C.c_uint64, C.c_uint64, u32p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int,
                             C.POINTER(LbSpec)]
    L.ph_scan_small.argtypes = [C.c_int, u32p, C.c_uint64, u32p, C.c_uint64, C.c_uint32, u32p, u32p, C.c_int]
    L.ph_prim_scan.argtypes = [C.c_int, u32p, u32p, C.c_uint64, C.POINTER(C.c_int)]
    L.ph_tile_layout.argtypes = [u32p, u32p, u32p, u32p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u32p, C.POINTER(LbSpec)]
    L.ph_tile_offsets.argtypes = [u32p, u32p, u32p, u32p, C.c_uint64, C.c_uint32, u32p, u32p, u32p, C.c_uint32, C.c_uint32,
                                  i64p, u64p, C.POINTER(LbSpec)]
    L.ph_cand_offsets.argtypes = [u32p, u32p, u32p, C.c_uint64, u32p, u32p, C.c_uint64, C.c_uint32, u32p, C.POINTER(LbSpec)]
    for f in ("ph_scan_lb", "ph_scan_small", "ph_prim_scan", "ph_tile_layout", "ph_tile_offsets", "ph_cand_offsets"):
        getattr(L, f).restype = C.c_int
    return L


def P(a):
    """ctypes pointer to a numpy array (None passes a null pointer)."""
    if a is None:
        return None
    return a.ctypes.data_as({np.dtype(np.uint32): u32p, np.dtype(np.uint64): u64p, np.dtype(np.int64): i64p}[a.dtype])


def canaried(n, dtype=np.uint32, lead=0):
    return np.full(lead + n + GUARD, CANARY, dtype)


class Desc:
    """A look-back descriptor's device state: status words (a, b), ticket counter, error word."""

    def __init__(self, n_blocks, ticket=0, epoch=1, status=None, n_status=None):
        self.n_status = n_status or n_blocks + GUARD
        self.status = np.zeros(2 * self.n_status, np.uint64) if status is None else status
        self.ticket0 = ticket & 0xFFFFFFFF
        self.ticket = np.array([self.ticket0], np.uint32)
        self.epoch = epoch
        self.err = np.zeros(1, np.uint32)
        self.n_blocks = n_blocks
        self.pre = self.status.copy()
        self.spec = LbSpec(P(self.status), self.n_status, epoch, P(self.ticket), P(self.err))

    def check(self, what, sums_a=None, sums_b=None):
        """error word clear, one ticket per block, every block's words published as inclusive prefixes of this epoch
        (values checked against sums_* when given), and the words past the grid untouched"""
        assert int(self.err[0]) == 0, f"{what}: error word {int(self.err[0]):#x}"
        assert int(self.ticket[0]) == (self.ticket0 + self.n_blocks) & 0xFFFFFFFF, f"{what}: ticket counter"
        nb, ns = self.n_blocks, self.n_status
        for half, sums in ((self.status[:ns], sums_a), (self.status[ns:], sums_b)):
            w = half[:nb]
            assert np.all((w >> np.uint64(34)) == self.epoch) and np.all(((w >> np.uint64(32)) & np.uint64(3)) == LB_PREFIX), \
                f"{what}: status words not all prefixes of epoch {self.epoch}"
            if sums is not None:
                assert np.array_equal((w & np.uint64(0xFFFFFFFF)).astype(np.uint32), sums.astype(np.uint32)), \
                    f"{what}: inclusive block prefixes"
        assert np.array_equal(self.status[nb:ns], self.pre[nb:ns]) and np.array_equal(self.status[ns + nb:], self.pre[ns + nb:]), \
            f"{what}: status words past the grid written"


def block_incl(x, per_block, nb):
    """inclusive sums over blocks of per_block elements (mod 2^32), one per block"""
    c = np.zeros(nb * per_block, np.uint64)
    c[:len(x)] = x
    return (np.cumsum(c.reshape(nb, per_block).sum(1, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def excl(x):
    """exclusive prefix sums of x with the total appended, as uint32 (the inputs keep totals below 2^32)"""
    c = np.zeros(len(x) + 1, np.uint64)
    np.cumsum(x, dtype=np.uint64, out=c[1:])
    assert c[-1] < 2 ** 32
    return c.astype(np.uint32)


def counts(rng, n, budget=2 ** 32 - 1, hi=None):
    """n uint32 counts with a run of zeros, a few large values and a total <= budget"""
    hi = hi or max(1, min(1 << 20, budget // max(n, 1) // 2))
    x = rng.integers(0, hi, n, dtype=np.uint64)
    if n > 16:
        a = int(rng.integers(0, n - n // 5))
        x[a:a + n // 5] = 0  # a run of zeros
    rest = budget - int(x.sum())
    for i in rng.integers(0, max(n, 1), min(n, 4)):  # large values (up to half the rest of the budget each)
        add = rest // 5
        x[i] += add
        rest -= add
    assert int(x.sum()) <= budget
    return x.astype(np.uint32)


def popcount32(w):
    return np.unpackbits(w.view(np.uint8)).reshape(-1, 32).sum(1, dtype=np.uint64) if len(w) else np.zeros(0, np.uint64)


LB_LENGTHS = [0, 1, 7, 8, 9, 8191, 8192, 8193, 64 * 8192 - 1, 64 * 8192, 64 * 8192 + 1, 65 * 8192 + 1, 200 * 8192 + 37]
OFFSETS = [(0, 0), (1, 1), (0, 3), (2, 0)]  # (in, out) element offsets: (0, 0) takes the 16-byte path, the rest the scalar one


def run_scan_lb(ph, x, popc, write_end, in_off=0, out_off=0, desc=None, **dk):
    n = len(x)
    nb = int(ph.ph_scan_lb_blocks(n + 1 if popc else n))
    inb = canaried(n, lead=in_off)
    inb[in_off:in_off + n] = x
    in0 = inb.copy()
    out = canaried(n + 1, lead=out_off)
    d = desc or Desc(nb, **dk)
    assert d.n_blocks == nb
    rc = ph.ph_scan_lb(int(popc), P(inb), len(inb), in_off, P(out), len(out), out_off, n, int(write_end), C.byref(d.spec))
    assert rc == 0, rc
    assert np.array_equal(inb, in0), "input written"
    assert np.all(out[:out_off] == CANARY), "written before out[0]"
    return out[out_off:], d, nb


@pytest.mark.parametrize("n", LB_LENGTHS)
def test_scan_lb_excl_matches_numpy(ph, n):
    rng = np.random.default_rng(n + 1)
    x = counts(rng, n)
    want = excl(x)
    for write_end in (True, False):
        for in_off, out_off in OFFSETS:
            what = f"n={n} write_end={write_end} offsets={in_off},{out_off}"
            out, d, nb = run_scan_lb(ph, x, False, write_end, in_off, out_off, ticket=int(rng.integers(0, 2 ** 32)),
                                     epoch=int(rng.integers(1, 2 ** 30)))
            assert np.array_equal(out[:n], want[:n]), what
            if write_end:  # (n == 0: the `n == 0` line of scan_lb_excl_body writes the zero total)
                assert out[n] == want[n], what
            else:
                assert out[n] == CANARY, what
            assert np.all(out[n + 1:] == CANARY), f"{what}: canary after out[n]"
            d.check(what, block_incl(x, SCAN_LB_BLOCK, nb), np.zeros(nb, np.uint32))


def test_scan_lb_excl_all_zero_and_saturated_totals(ph):
    # a zero input, and one whose total is exactly 2^32 - 1 spread over three blocks
    for x in (np.zeros(3 * 8192 + 5, np.uint32), np.full(3, 0xFFFFFFFF // 3, np.uint32),
              np.r_[np.zeros(2 * 8192, np.uint32), np.uint32(0xFFFFFFFF - 8), np.ones(8, np.uint32)]):
        out, d, nb = run_scan_lb(ph, x, False, True)
        assert np.array_equal(out[:len(x) + 1], excl(x)) and np.all(out[len(x) + 1:] == CANARY)
        d.check(f"n={len(x)}")


@pytest.mark.parametrize("n_words", LB_LENGTHS)
def test_scan_lb_popc_matches_numpy(ph, n_words):
    rng = np.random.default_rng(7 * n_words + 3)
    w = rng.integers(0, 2 ** 32, n_words, dtype=np.uint64).astype(np.uint32)
    if n_words > 16:  # runs of all-zero and all-one words
        w[n_words // 3:n_words // 3 + n_words // 7] = 0
        w[n_words // 2:n_words // 2 + n_words // 7 + 1] = 0xFFFFFFFF
    elif n_words:
        w[::2] = 0xFFFFFFFF
    want = excl(popcount32(w))
    for in_off, out_off in OFFSETS:
        what = f"n_words={n_words} offsets={in_off},{out_off}"
        out, d, nb = run_scan_lb(ph, w, True, False, in_off, out_off, ticket=int(rng.integers(0, 2 ** 32)))
        assert np.array_equal(out[:n_words + 1], want), what
        assert np.all(out[n_words + 1:] == CANARY), f"{what}: canary after out[n_words]"
        d.check(what, block_incl(np.r_[popcount32(w), 0], SCAN_LB_BLOCK, nb), np.zeros(nb, np.uint32))


def stale_status(rng, n_status, epoch):
    """status words of OTHER epochs (epoch - 1, epoch + 1, epoch with bit 29 flipped), any state, garbage values"""
    others = np.array([(epoch - 1) & EPOCH_MASK, (epoch + 1) & EPOCH_MASK, epoch ^ (1 << 29)], np.uint64)
    e = others[rng.integers(0, 3, 2 * n_status)]
    st = rng.integers(1, 4, 2 * n_status, dtype=np.uint64)
    v = rng.integers(0, 2 ** 32, 2 * n_status, dtype=np.uint64)
    assert not np.any(e == epoch)
    return (e << np.uint64(34)) | (st << np.uint64(32)) | v


@pytest.mark.parametrize("ticket", [0, 2 ** 32 - 1, 2 ** 32 - 5, 2 ** 32 - 64, 2 ** 32 - 65, 2 ** 32 - 66])
@pytest.mark.parametrize("epoch", [1, 2 ** 29, 2 ** 30 - 1])
def test_lookback_descriptor_edges(ph, ticket, epoch):
    """the ticket counter wrapping inside the launch, the last epoch before the roll-over, and status words left by other
    epochs (never cleared between launches) with garbage values: the scan must not take any of them"""
    rng = np.random.default_rng(ticket ^ epoch)
    n = 65 * 8192 + 1  # 66 blocks: the walk of the last blocks passes its first window of 64
    x = counts(rng, n)
    want = excl(x)
    nb = int(ph.ph_scan_lb_blocks(n))
    for fill in ("zero", "stale"):
        status = None if fill == "zero" else stale_status(rng, nb + GUARD, epoch)
        out, d, _ = run_scan_lb(ph, x, False, True, ticket=ticket, epoch=epoch, status=status)
        assert np.array_equal(out[:n + 1], want), fill
        d.check(f"ticket={ticket} epoch={epoch} {fill}", block_incl(x, SCAN_LB_BLOCK, nb), np.zeros(nb, np.uint32))


def test_lookback_reuses_status_words_of_earlier_launches(ph):
    """consecutive launches on one set of status words, as a context issues them: epoch e + 1 over the words epoch e
    left (its prefixes of other values), the ticket counter carried on across the 2^32 wrap"""
    rng = np.random.default_rng(5)
    ticket, epoch = 2 ** 32 - 100, 2 ** 30 - 6  # (the last launch takes the last epoch, 2^30 - 1)
    status = stale_status(rng, 300, epoch)
    for n in (200 * 8192 + 37, 65 * 8192 + 1, 8193, 64 * 8192, 0, 130 * 8192):
        x = counts(rng, n)
        nb = int(ph.ph_scan_lb_blocks(n))
        d = Desc(nb, ticket=ticket, epoch=epoch, status=status, n_status=300)
        out, _, _ = run_scan_lb(ph, x, False, True, desc=d)
        assert np.array_equal(out[:n + 1], excl(x)), (n, epoch)
        d.check(f"n={n} epoch={epoch}", block_incl(x, SCAN_LB_BLOCK, nb))
        ticket, epoch, status = int(d.ticket[0]), epoch + 1, d.status
    assert ticket < 2 ** 31 and epoch == 2 ** 30  # (the counter wrapped; every epoch up to the last one was used)


SMALL_LENGTHS = [1, 1023, 1024, 1025, 65535, 65536]


def n_dev_cases(n):
    return [None, 0, n // 2, n - 1, n, n + 7]


@pytest.mark.parametrize("n", SMALL_LENGTHS)
def test_scan_small_excl_matches_numpy(ph, n):
    rng = np.random.default_rng(n)
    x = counts(rng, n)
    for nd in n_dev_cases(n):
        m = n if nd is None else min(nd, n)
        want = excl(x[:m])
        for write_end in (True, False):
            for with_total in (True, False):
                what = f"n={n} n_dev={nd} write_end={write_end}"
                out = canaried(n + 1)
                total = np.array([CANARY], np.uint32) if with_total else None
                ndv = None if nd is None else np.array([nd], np.uint32)
                rc = ph.ph_scan_small(0, P(x), n, P(out), len(out), n, P(ndv), P(total), int(write_end))
                assert rc == 0, rc
                assert np.array_equal(out[:m], want[:m]), what
                assert out[m] == (want[m] if write_end else CANARY), what
                assert np.all(out[m + 1:] == CANARY), f"{what}: written past the device-side count"
                if with_total:
                    assert total[0] == want[m], what


def scan_small(ph, mode, x, nd=None):
    n = len(x)
    out = canaried(n + 1)
    ndv = None if nd is None else np.array([nd], np.uint32)
    rc = ph.ph_scan_small(mode, P(x.view(np.uint32)), n, P(out), len(out), n, P(ndv), None, 0)
    assert rc == 0, rc
    return out.view(np.int32)


def signed_values(rng, n, kind):
    if kind == 2:  # min: negatives, both extremes, a long stretch above the running minimum
        x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64)
        x[rng.integers(0, n, max(1, n // 97))] = -2 ** 31
        x[: n // 3] = np.abs(x[: n // 3]) // 2 + 2 ** 30
        x[-1:] = 2 ** 31 - 1
    else:  # sums that cross zero both ways and stay inside int32
        x = rng.integers(-3000, 3000, n, dtype=np.int64)
        x[: n // 4] += 2000
    return x.astype(np.int32)


def want_incl(x, mode):
    if mode == 2:
        return np.minimum.accumulate(x.astype(np.int64)).astype(np.int32)
    c = np.cumsum(x.astype(np.int64))
    assert np.all(np.abs(c) < 2 ** 31)
    return c.astype(np.int32)


@pytest.mark.parametrize("mode", [1, 2], ids=["incl_sum", "incl_min"])
@pytest.mark.parametrize("n", SMALL_LENGTHS)
def test_scan_small_incl_and_min_match_numpy(ph, n, mode):
    rng = np.random.default_rng(n * 3 + mode)
    x = signed_values(rng, n, mode)
    for nd in n_dev_cases(n):
        m = n if nd is None else min(nd, n)
        got = scan_small(ph, mode, x, nd)
        assert np.array_equal(got[:m], want_incl(x[:m], mode)), (n, nd)
        assert np.all(got.view(np.uint32)[m:] == CANARY), (n, nd)


@pytest.mark.parametrize("n", [65536, 65537])
def test_rocprim_scans_agree_with_short_scans(ph, n):
    """the long forms scan_incl_min / scan_incl_sum switch to above SCAN_SMALL_MAX (65536): rocPRIM with temporary
    storage from prim_temp_bytes must give what the single-block kernels and numpy give on either side of it"""
    rng = np.random.default_rng(n)
    st = C.c_int(-1)
    x = counts(rng, n)
    out = np.full(n, CANARY, np.uint32)
    assert ph.ph_prim_scan(0, P(x), P(out), n, C.byref(st)) == 0 and st.value == 0
    short = canaried(n + 1)
    assert ph.ph_scan_small(0, P(x), n, P(short), len(short), n, None, None, 0) == 0
    assert np.array_equal(out, excl(x)[:n]) and np.array_equal(short[:n], out)
    for mode in (1, 2):
        x = signed_values(rng, n, mode)
        out = np.full(n, CANARY, np.uint32)
        st.value = -1
        assert ph.ph_prim_scan(mode, P(x.view(np.uint32)), P(out), n, C.byref(st)) == 0 and st.value == 0
        want = want_incl(x, mode)
        assert np.array_equal(out.view(np.int32), want), mode
        assert np.array_equal(scan_small(ph, mode, x)[:n], want), mode


TILE_COUNTS = [1, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65 * 1024 + 1]


def tile_counts(rng, n, cap):
    x = rng.integers(0, 2 * cap, n, dtype=np.int64)
    x[rng.random(n) < 0.2] = 0
    if n > 8:
        x[n // 3:n // 3 + n // 8] = 0
    x[rng.integers(0, n, max(1, n // 50))] = rng.integers(cap + 1, 50 * cap, max(1, n // 50))  # over the bucket
    return x.astype(np.uint32)


@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_tile_layout_one_block_and_lookback(ph, n_tiles):
    rng = np.random.default_rng(n_tiles)
    for cap in (64, 4096):
        cur = tile_counts(rng, n_tiles, cap)
        want_scan = excl(cur)
        want_scanb = excl(np.minimum(cur, cap))
        ovf = np.array([int(rng.integers(0, 2 ** 32))], np.uint32)
        nb = int(ph.ph_tile_scan_blocks(n_tiles))
        assert nb == (n_tiles + TILE_LB_BLOCK - 1) // TILE_LB_BLOCK
        for lb in (False, True):
            what = f"n_tiles={n_tiles} cap={cap} lookback={lb}"
            tcur, tn, ts, tsb = (canaried(n_tiles + 1) for _ in range(4))
            tcur[:n_tiles] = cur
            out = np.array([CANARY, 0 if lb else CANARY, CANARY], np.uint32)  # (look-back form: out[1] zero beforehand)
            d = Desc(nb, ticket=int(rng.integers(0, 2 ** 32)), epoch=int(rng.integers(1, 2 ** 30))) if lb else None
            rc = ph.ph_tile_layout(P(tcur), P(tn), P(ts), P(tsb), len(tn), n_tiles, cap, P(ovf), P(out),
                                   C.byref(d.spec) if lb else None)
            assert rc == 0, rc
            assert np.array_equal(tn[:n_tiles], cur) and np.all(tn[n_tiles:] == CANARY), f"{what}: tile_n"
            assert np.array_equal(ts[:n_tiles + 1], want_scan) and np.all(ts[n_tiles + 1:] == CANARY), f"{what}: tile_scan"
            assert np.array_equal(tsb[:n_tiles + 1], want_scanb) and np.all(tsb[n_tiles + 1:] == CANARY), f"{what}: tile_scanb"
            assert list(out) == [want_scan[-1], int(cur.max()), ovf[0]], f"{what}: (total, max, overflow)"
            assert np.all(tcur[:n_tiles] == 0) and np.all(tcur[n_tiles:] == CANARY), f"{what}: tile_cur not reset"
            if lb:
                d.check(what, block_incl(cur, TILE_LB_BLOCK, nb), block_incl(np.minimum(cur, cap), TILE_LB_BLOCK, nb))


@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_tile_offsets_one_block_and_lookback(ph, n_tiles):
    rng = np.random.default_rng(n_tiles + 99)
    n_reset = 13
    for negative in (False, True):
        nn = counts(rng, n_tiles, budget=2 ** 32 - 1)
        nr = counts(rng, n_tiles, budget=2 ** 31, hi=64)
        gain = rng.integers(-2 ** 40, 2 ** 40, n_tiles, dtype=np.int64)
        gain[rng.integers(0, n_tiles, max(1, n_tiles // 10))] = 2 ** 40 - 1
        if negative:  # a negative sum
            gain = -np.abs(gain)
        want_gain = int(gain.sum())
        assert want_gain < 0 or not negative
        nb = int(ph.ph_tile_scan_blocks(n_tiles))
        for lb in (False, True):
            for with_gain in (True, False):
                what = f"n_tiles={n_tiles} negative={negative} lookback={lb} gain={with_gain}"
                noff, roff = canaried(n_tiles), canaried(n_tiles)
                nodes, runs = np.array([CANARY], np.uint32), np.array([CANARY], np.uint32)
                reset = canaried(n_reset)
                tg = np.r_[gain, np.zeros(GUARD, np.int64)]
                # (the look-back form adds into a total k_pf_tile has zeroed)
                gt = np.array([0 if lb else 0xDEADBEEFDEADBEEF], np.uint64)
                d = Desc(nb, ticket=int(rng.integers(0, 2 ** 32)), epoch=int(rng.integers(1, 2 ** 30))) if lb else None
                nn_b, nr_b = np.r_[nn, np.zeros(GUARD, np.uint32)], np.r_[nr, np.zeros(GUARD, np.uint32)]
                rc = ph.ph_tile_offsets(P(nn_b), P(nr_b), P(noff), P(roff), len(noff), n_tiles, P(nodes), P(runs), P(reset), len(reset), n_reset,
                                        P(tg) if with_gain else None, P(gt) if with_gain else None,
                                        C.byref(d.spec) if lb else None)
                assert rc == 0, rc
                assert np.array_equal(noff[:n_tiles], excl(nn)[:n_tiles]) and np.all(noff[n_tiles:] == CANARY), f"{what}: tile_noff"
                assert np.array_equal(roff[:n_tiles], excl(nr)[:n_tiles]) and np.all(roff[n_tiles:] == CANARY), f"{what}: tile_roff"
                assert nodes[0] == excl(nn)[-1] and runs[0] == excl(nr)[-1], f"{what}: totals"
                assert np.all(reset[:n_reset] == 0) and np.all(reset[n_reset:] == CANARY), f"{what}: reset words"
                if with_gain:
                    assert int(gt[0]) == want_gain & (2 ** 64 - 1), f"{what}: gain_total {int(gt[0]):#x} vs {want_gain}"
                if lb:
                    d.check(what, block_incl(nn, TILE_LB_BLOCK, nb), block_incl(nr, TILE_LB_BLOCK, nb))


CAND_REGIONS = [1, 3, 4095, 4096, 4097, 8193, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 3, 130 * 4096 + 2]


@pytest.mark.parametrize("n_reg", CAND_REGIONS)
def test_cand_offsets_one_block_and_lookback(ph, n_reg):
    """Reference from the one-block kernel body (np2_cand.hip, k_cand_offsets, lines 663-683): blk_sum holds three rows
    of n_blk = ceil(n_reg / 4) block sums (candidates, bytes, longest string); blk_coff / blk_soff = exclusive scans of
    the first two rows (lines 669-673), cand_off[n_reg] = *n_cand = total of row 0 and reg_soff[n_reg] = *n_bytes =
    total of row 1 (lines 677-681), *grow = total of row 2 (lines 674-675, 682); nothing else is written."""
    rng = np.random.default_rng(n_reg)
    n_blk = (n_reg + 3) // 4
    rows = [counts(rng, n_blk, hi=4 * 60 + 1), counts(rng, n_blk), counts(rng, n_blk, budget=2 ** 31, hi=3000)]
    blk_sum = np.concatenate(rows)
    nb = int(ph.ph_cand_offsets_blocks(n_reg))
    assert nb == (n_reg + CAND_LB_REGIONS - 1) // CAND_LB_REGIONS
    want_c, want_s, want_g = excl(rows[0]), excl(rows[1]), int(excl(rows[2])[-1])
    for lb in (False, True):
        what = f"n_reg={n_reg} lookback={lb}"
        coff, soff = canaried(n_blk), canaried(n_blk)
        cand_off, reg_soff = canaried(n_reg + 1), canaried(n_reg + 1)
        scal = np.full(3, CANARY, np.uint32)
        d = Desc(nb, ticket=int(rng.integers(0, 2 ** 32)), epoch=int(rng.integers(1, 2 ** 30))) if lb else None
        rc = ph.ph_cand_offsets(P(blk_sum), P(coff), P(soff), len(coff), P(cand_off), P(reg_soff), len(cand_off), n_reg,
                                P(scal), C.byref(d.spec) if lb else None)
        assert rc == 0, rc
        assert np.array_equal(coff[:n_blk], want_c[:n_blk]) and np.all(coff[n_blk:] == CANARY), f"{what}: blk_coff"
        assert np.array_equal(soff[:n_blk], want_s[:n_blk]) and np.all(soff[n_blk:] == CANARY), f"{what}: blk_soff"
        assert cand_off[n_reg] == want_c[-1] and reg_soff[n_reg] == want_s[-1], f"{what}: closing offsets"
        assert np.all(np.delete(cand_off, n_reg) == CANARY) and np.all(np.delete(reg_soff, n_reg) == CANARY), what
        assert list(scal) == [want_c[-1], want_s[-1], want_g], f"{what}: n_cand, n_bytes, grow"
        if lb:
            d.check(what, block_incl(rows[0], 4 * 256, nb), block_incl(rows[1], 4 * 256, nb))
