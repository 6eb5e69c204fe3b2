"""The corpus of the BGZF inflater's case tests (test_inflate_cases_cpu.py, test_gpu_inflate_cases.py): DEFLATE streams
written bit by bit for the edges of the device inflater (csrc/np2_inflate.hip: 64 bit offsets decoded at once, a step's
output capped at 2048 bytes, an 8 KiB output ring in LDS behind which matches read the flushed output, input staged 2 KiB
at a time into a 4 KiB window, primary tables of 10 / 8 bits with a canonical walk for longer codes), and malformed streams
that hold exactly one fault each, with the status (np2inf::Status, csrc/np2_inflate_core.hpp) that fault must be refused
with.  No encoder writes most of these shapes.  Plain Python, seeded, independent of the package: zlib is the judge of
every valid stream when the corpus is built, and must refuse (or stop short on) every stream with a fault in its DEFLATE
bytes.

VALID / VALID_LENIENT: [(name, payload, data)]; REFUSED: [(name, block, status, note)] — built on first use (valid(),
valid_lenient(), refused(); a second and a half of Python); block_of() wraps a valid case in its BGZF block."""
import functools
import random
import struct
import zlib

# np2inf::Status, by the enum's own words
ST_OK = 0
ST_BAD_BTYPE = 1        # block type 3
ST_BAD_STORED = 2       # LEN != ~NLEN
ST_BAD_LENGTHS = 3      # code length repeat without a previous length / too many lengths
ST_OVERSUBSCRIBED = 4   # a code set that is not prefix-free
ST_BAD_SYMBOL = 5       # an unassigned code, length symbol 286 / 287, distance symbol 30 / 31
ST_BAD_DISTANCE = 6     # distance reaches before the start of the output
ST_OUT_OVERRUN = 7      # more output than ISIZE
ST_OUT_SHORT = 8        # stream ended before ISIZE bytes
ST_IN_OVERRUN = 9       # stream ran past the block's compressed bytes
ST_NO_END_CODE = 10     # literal / length code without symbol 256

MAX_PAYLOAD = 65536 - 18 - 8  # BSIZE is 16 bits: the largest payload behind an 18-byte header
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- the writer -----------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB first, as DEFLATE packs its fields; Huffman codes go in bit-reversed (Code.rev)"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    @property
    def bits(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def clone(self):
        w = BitWriter()
        w.acc, w.n, w.out = self.acc, self.n, bytearray(self.out)
        return w

    def done(self):
        self.align()
        return bytes(self.out)


class Code:
    """canonical codes (RFC 1951 3.2.2) of a list of lengths, each stored bit-reversed; the lengths need be neither complete
    nor prefix-free (the numbering is carried out all the same: that is what a refusal case's header says)"""

    def __init__(self, lens):
        self.lens = list(lens)
        mx = max(self.lens + [0])
        cnt = [0] * (mx + 2)
        for l in self.lens:
            if l:
                cnt[l] += 1
        code, nxt = 0, [0] * (mx + 2)
        for b in range(1, mx + 1):
            code = (code + cnt[b - 1]) << 1
            nxt[b] = code
        self.rev = [0] * len(self.lens)
        for s, l in enumerate(self.lens):
            if l:
                c, nxt[l] = nxt[l], nxt[l] + 1
                self.rev[s] = int(format(c & ((1 << l) - 1), "0%db" % l)[::-1], 2)

    def put(self, w, s):
        assert self.lens[s], ("symbol without a code", s)
        w.put(self.rev[s], self.lens[s])


def kraft(lens):
    """the Kraft sum of a list of lengths in units of 2^-15 (32768: complete)"""
    return sum(1 << (15 - l) for l in lens if l)


def len_symbol(n):
    return 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)


def dist_symbol(d):
    return max(i for i in range(30) if DIST_BASE[i] <= d)


def put_tokens(w, tokens, lit, dist):
    """('lit', b) | ('match', len, dist) | ('end',) | ('sym', 'l' | 'd', symbol): that symbol's bare code | ('bits', v, k)"""
    for t in tokens:
        if t[0] == "lit":
            w.put(lit.rev[t[1]], lit.lens[t[1]])
        elif t[0] == "match":
            s, q = len_symbol(t[1]), dist_symbol(t[2])
            lit.put(w, 257 + s)
            w.put(t[1] - LEN_BASE[s], LEN_EXTRA[s])
            dist.put(w, q)
            w.put(t[2] - DIST_BASE[q], DIST_EXTRA[q])
        elif t[0] == "end":
            lit.put(w, 256)
        elif t[0] == "sym":
            (lit if t[1] == "l" else dist).put(w, t[2])
        else:
            assert t[0] == "bits"
            w.put(t[1], t[2])


def token_bits(t, lit, dist):
    if t[0] == "lit":
        return lit.lens[t[1]]
    if t[0] == "end":
        return lit.lens[256]
    assert t[0] == "match"
    s, q = len_symbol(t[1]), dist_symbol(t[2])
    return lit.lens[257 + s] + LEN_EXTRA[s] + dist.lens[q] + DIST_EXTRA[q]


def expand(tokens, out=None):
    """the model of the output: the tokens' bytes appended to `out` (a bytearray: what the stream produced before them)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            _, n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out) and d <= 32768, t
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
        else:
            assert t[0] == "end", t
    return out


def stored(w, data, final, length=None, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    length = len(data) if length is None else length
    w.put(length, 16)
    w.put(length ^ 0xFFFF if nlen is None else nlen, 16)
    w.out += data


FIXED_LIT = Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = Code([5] * 32)


def fixed(w, tokens, final):
    w.put(final, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def dynamic(w, tokens, final, hlit, hdist, hclen, cl_lens, spelled, lit, dist):
    """every header field as the case gives it.  spelled: the code length sequence as the symbols to write, an int 0 .. 15
    or (16 | 17 | 18, count)"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl = Code(cl_lens)
    for s in spelled:
        if isinstance(s, int):
            cl.put(w, s)
        else:
            sym, n = s
            cl.put(w, sym)
            w.put(n - (11 if sym == 18 else 3), {16: 2, 17: 3, 18: 7}[sym])
    put_tokens(w, tokens, lit, dist)


def unspell(spelled):
    out = []
    for s in spelled:
        if isinstance(s, int):
            out.append(s)
        else:
            out += [out[-1] if s[0] == 16 else 0] * s[1]
    return out


def bgzf(payload, data, isize=None, crc=None):
    assert len(payload) <= MAX_PAYLOAD, len(payload)
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(payload) + 25)
    return hdr + payload + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc, len(data) if isize is None else isize)


def split(block):
    """a block of bgzf() -> (payload, crc, isize)"""
    return (block[18:-8],) + struct.unpack("<II", block[-8:])


def block_of(case):
    return bgzf(case[1], case[2])


def fill_tokens(gap, a, b, lit, dist):
    """filler of known bit lengths: tokens a and b (coprime bit counts), as few of b as reach exactly `gap` bits"""
    pa, pb = token_bits(a, lit, dist), token_bits(b, lit, dist)
    for nb in range(pa + 1):
        if gap - nb * pb >= 0 and (gap - nb * pb) % pa == 0:
            return [b] * nb + [a] * ((gap - nb * pb) // pa)
    raise AssertionError(("no filler", gap, pa, pb))


# ---- code sets ------------------------------------------------------------------------------------------------------------
CL_FULL = [4] * 13 + [5] * 6  # a complete code length code with every symbol (HCLEN 19: the last in the order is 15)


class CodeSet:
    """what a dynamic block's header says, and the two codes its tokens are written with"""

    def __init__(self, ll, dl, hlit=None, hdist=None, hclen=19, cl_lens=CL_FULL, spelled=None, check=True):
        self.hlit = len(ll) if hlit is None else hlit
        self.hdist = len(dl) if hdist is None else hdist
        self.hclen, self.cl_lens = hclen, list(cl_lens)
        self.spelled = list(ll) + list(dl) if spelled is None else spelled
        self.lit, self.dist = Code(list(ll) + [0] * (288 - len(ll))), Code(list(dl) + [0] * (32 - len(dl)))
        if check:  # (a valid header: the spelling says these lengths, and the order's tail beyond HCLEN is unused)
            assert unspell(self.spelled) == list(ll)[:self.hlit] + list(dl)[:self.hdist]
            assert len(ll) == self.hlit and len(dl) == self.hdist
            assert all(self.cl_lens[CL_ORDER[i]] == 0 for i in range(hclen, 19)) and kraft(self.cl_lens) == 32768

    def put(self, w, tokens, final):
        dynamic(w, tokens, final, self.hlit, self.hdist, self.hclen, self.cl_lens, self.spelled, self.lit, self.dist)


def sparse(n, d):
    out = [0] * n
    for s, l in d.items():
        out[s] = l
    return out


# every literal / length symbol in 8 or 9 bits, every distance symbol in 4 or 5: nothing leaves the primary tables
LL_SHORT, DL_SHORT = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
# every length symbol beyond the primary table's 10 bits: each match is decoded by the canonical walk
LL_LONG = [8] * 255 + [10, 10] + [13] * 3 + [14] * 26
# distance symbols 3 .. 6 in 1 .. 4 bits, six in 8, every other one in 9: beyond the distance table's 8 bits
DL_LONG = sparse(30, {**{s: 9 for s in range(30)}, **{3: 1, 4: 2, 5: 3, 6: 4, 7: 8, 8: 8, 9: 8, 10: 8, 13: 8, 14: 8}})
assert kraft(LL_SHORT) == kraft(DL_SHORT) == kraft(LL_LONG) == kraft(DL_LONG) == 32768
SHORT = CodeSet(LL_SHORT, DL_SHORT)
LONG_LEN = CodeSet(LL_LONG, DL_SHORT)
LONG_DIST = CodeSet(LL_SHORT, DL_LONG)
PATHS = (("wide", SHORT), ("longlen", LONG_LEN), ("longdist", LONG_DIST))
# two-bit tokens: literal 'A' and the end code in 2 and 3 bits, length 258 in 1, lengths 227 .. 257 in 3; one distance code
TINY = CodeSet(sparse(286, {65: 2, 256: 3, 284: 3, 285: 1}), [1], hlit=286, hdist=1,
               spelled=[(18, 65), 2, (18, 138), (18, 52), 3, (18, 27), 3, 1, 1], cl_lens=sparse(19, {18: 1, 1: 3, 2: 3, 3: 2}), hclen=18)
# an empty dynamic block: the end code alone (an incomplete code of one 1-bit symbol is legal), no distance code
EMPTY_DYN = CodeSet(sparse(257, {256: 1}), [0], spelled=[(18, 138), (18, 118), 1, 0], cl_lens=sparse(19, {18: 1, 0: 2, 1: 2}), hclen=18)


class Stream:
    """a raw DEFLATE stream in the making and the bytes it inflates to"""

    def __init__(self):
        self.w, self.data = BitWriter(), bytearray()

    def stored(self, data, final=0, **kw):
        stored(self.w, data, final, **kw)
        self.data += data
        return self

    def fixed(self, tokens, final=0, end=True):
        fixed(self.w, list(tokens) + ([("end",)] if end else []), final)
        expand(tokens, self.data)
        return self

    def dyn(self, cs, tokens, final=0, end=True):
        cs.put(self.w, list(tokens) + ([("end",)] if end else []), final)
        expand(tokens, self.data)
        return self

    def done(self):
        return self.w.done(), bytes(self.data)


def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


def lits(rng, n, lo=0, hi=255):
    return [("lit", rng.randrange(lo, hi)) for _ in range(n)]


def random_tokens(rng, n, p_match=0.2, have=0):
    """tokens of exactly n bytes: seeded literals and matches of every length and reachable distance"""
    toks, out = [], have
    while out - have < n:
        left = n - (out - have)
        if out and left >= 3 and rng.random() < p_match:
            ln = min(left, rng.choice((3, 4, 5, 10, 63, 64, 65, 100, 257, 258, rng.randrange(3, 259))))
            d = min(out, 32768, rng.choice((1, 2, 3, 4, 64, rng.randrange(1, 300), rng.randrange(1, 32769))))
            toks.append(("match", ln, d))
            out += ln
        else:
            toks.append(("lit", rng.randrange(0, 255)))
            out += 1
    return toks


def tokenize(data):
    """a greedy matcher over 3-byte hashes (the last position of each): any bytes as tokens, for the hand writer as a
    foreign encoder"""
    toks, table, i, n = [], {}, 0, len(data)
    while i < n:
        key = bytes(data[i:i + 3])
        j = table.get(key)
        table[key] = i
        if j is not None and len(key) == 3 and i - j <= 32768:
            ln = 3
            while ln < 258 and i + ln < n and data[j + ln] == data[i + ln]:
                ln += 1
            toks.append(("match", ln, i - j))
            i += ln
        else:
            toks.append(("lit", data[i]))
            i += 1
    return toks


def encode_foreign(data):
    """`data` (at most a BGZF block's) as one payload no common encoder writes: a dynamic block whose length symbols have
    13- and 14-bit codes, an empty stored block (what Z_SYNC_FLUSH leaves), a dynamic block whose distance symbols have
    9-bit codes, an empty stored block, a fixed block"""
    toks = tokenize(data)
    a, b = len(toks) // 3, 2 * len(toks) // 3
    s = Stream()
    s.dyn(LONG_LEN, toks[:a]).stored(b"").dyn(LONG_DIST, toks[a:b]).stored(b"").fixed(toks[b:], final=1)
    payload, got = s.done()
    assert got == bytes(data)
    return payload


# ---- the valid cases ------------------------------------------------------------------------------------------------------
def _code_shapes(add):
    # HLIT 257, HDIST 1 with a zero length, literals only, and the smallest HCLEN a valid block can have: the code length code
    # needs a symbol for a non-zero length, and the first one in the order (16, 17, 18, 0, 8) is 8 -> HCLEN 5.  Literals
    # 0 .. 254 and the end code in 8 bits each is the complete code that gets by with {16, 0, 8}.
    rng = _rng("shape")
    cs = CodeSet([8] * 255 + [0, 8], [0], spelled=[8] + [(16, 6)] * 41 + [(16, 4), (16, 4), 0, 8, 0], cl_lens=sparse(19, {16: 1, 0: 2, 8: 2}), hclen=5)
    add("shape_hlit257_hdist1_zero_hclen5_literals_only", Stream().dyn(cs, lits(rng, 300), 1))
    # HLIT 286, HDIST 30, HCLEN 19
    add("shape_hlit286_hdist30_hclen19", Stream().dyn(SHORT, random_tokens(rng, 5000), 1))
    # both codes with the lengths 1 .. 15 (and a second 15); the code length code with lengths up to 7 bits:
    #   {0: 1, 18: 2, 1 2: 5, 3 .. 13: 6, 14 15: 7} sums to one
    ll = sparse(286, {65: 1, 67: 2, 71: 3, 84: 4, 78: 5, 10: 6, 257: 7, 258: 8, 264: 9, 285: 10, 90: 11, 270: 12, 89: 13, 256: 14, 284: 15, 88: 15})
    dl = sparse(30, {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 9, 9: 10, 10: 11, 16: 12, 22: 13, 25: 14, 26: 15, 29: 15})

    def runs(lens):  # eleven or more zeros as an 18, the rest plain
        out, i = [], 0
        while i < len(lens):
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            if j - i >= 11:
                out.append((18, j - i))
            else:
                j = max(j, i + 1)
                out += lens[i:j]
            i = j
        return out
    cl7 = sparse(19, {**{0: 1, 18: 2, 1: 5, 2: 5, 14: 7, 15: 7}, **{s: 6 for s in range(3, 14)}})
    cs = CodeSet(ll, dl, spelled=runs(ll + dl), cl_lens=cl7, hclen=19)
    toks = [("lit", 65)] * 70 + [("lit", 90)] + [("lit", 67)] * 5 + [("match", 4, 1), ("match", 258, 3), ("lit", 90), ("match", 10, 9)]
    toks += [("lit", b) for b in (65, 67, 71, 84, 78, 10, 89)] * 1400
    toks += [("match", 258, 8193), ("match", 4, 6145), ("match", 258, 2100), ("match", 23, 33), ("match", 258, 9000), ("lit", 88),
             ("match", 258, 8192), ("match", 3, 257), ("match", 240, 1), ("match", 26, 20), ("lit", 90)]
    # used with 11 or more bits: literals 90 89 88, length symbols 270 284 and the end code; with 9 or more: distance symbols 8 .. 26
    add("shape_lengths_1_to_15_cl_7bit", Stream().dyn(cs, toks, 1))
    # 16 repeating across the literal / distance boundary: 256's length 2 goes on through 257 and four distance symbols
    cs = CodeSet(sparse(258, {65: 2, 66: 2, 256: 2, 257: 2}), [2] * 4, spelled=[(18, 65), 2, 2, (18, 138), (18, 51), 2, (16, 5)],
                 cl_lens=sparse(19, {18: 1, 2: 2, 16: 2}), hclen=16)
    ab = [("lit", 65), ("lit", 66), ("lit", 66), ("lit", 65), ("lit", 65)]
    add("shape_rep16_crosses_boundary", Stream().dyn(cs, ab + [("match", 3, d) for d in (1, 2, 3, 4)], 1))
    # 17 x 10 ending exactly on HLIT + HDIST (HLIT 257, HDIST 11: one used 1-bit distance code would need a length symbol,
    # so the distance code is there and unused)
    cs = CodeSet(sparse(257, {65: 1, 256: 1}), [1] + [0] * 10, spelled=[(18, 65), 1, (18, 138), (18, 52), 1, 1, (17, 10)],
                 cl_lens=sparse(19, {1: 1, 18: 2, 17: 2}), hclen=18)
    add("shape_rep17x10_ends_on_total", Stream().dyn(cs, [("lit", 65)] * 9, 1))
    # 18 x 138, the longest run, ending on symbol 256 (it cannot end on HLIT + HDIST in a valid block: 256 has a length, and
    # at most 29 + 30 lengths follow it), and 18 x 59 crossing the boundary and ending exactly on HLIT + HDIST
    cs = CodeSet(sparse(286, {65: 1, 256: 1}), [0] * 30, spelled=[(18, 65), 1, (18, 52), (18, 138), 1, (18, 59)],
                 cl_lens=sparse(19, {1: 1, 18: 1}), hclen=18)
    add("shape_rep18x138_and_18x59_ends_on_total", Stream().dyn(cs, [("lit", 65)] * 70, 1))
    # 18 crossing the boundary and ending inside the distance lengths
    cs = CodeSet(sparse(286, {65: 2, 256: 2, 257: 1}), sparse(30, {2: 1, 3: 1}),
                 spelled=[(18, 65), 2, (18, 138), (18, 52), 2, 1, (18, 30), 1, 1, (18, 26)], cl_lens=sparse(19, {18: 1, 1: 2, 2: 2}), hclen=18)
    add("shape_rep18_crosses_boundary", Stream().dyn(cs, [("lit", 65)] * 5 + [("match", 3, 3), ("match", 3, 4)], 1))
    # HDIST 1: a single distance code of length 1 that is used
    add("shape_single_distance_code_used", Stream().dyn(TINY, [("lit", 65), ("match", 258, 1), ("match", 230, 1)], 1))
    # empty blocks, twenty in a row before the data
    data = lits(rng, 100, 0, 256)
    s = Stream()
    for _ in range(20):
        s.dyn(EMPTY_DYN, [])
    add("shape_empty_dynamic_x20", s.fixed(data, 1))
    s = Stream()
    for _ in range(20):
        s.fixed([])
    add("shape_empty_fixed_x20", s.dyn(SHORT, data, 1))
    s = Stream()
    for _ in range(20):
        s.stored(b"")
    add("shape_empty_stored_x20", s.fixed(data, 1))
    # a fixed block with 9-bit literals, length symbols 280 .. 285 and distance symbol 29 with 13 extra bits (32768)
    toks = lits(rng, 20, 144, 256)
    for ln in (115, 130, 131, 163, 195, 227, 257, 258):
        toks += [("match", ln, 32768), ("lit", rng.randrange(144, 256))]
    add("shape_fixed_9bit_len280_285_dist32768", Stream().stored(bytes(rng.randrange(256) for _ in range(32768))).fixed(toks, 1))


def _small_block(s, kind, rng, final, nine=0):
    """one small block of `kind` appended to Stream s; `nine`: that many 9-bit literals in it (each moves the end by a bit)"""
    if kind == "stored":
        return s.stored(bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40))), final)
    toks = random_tokens(rng, rng.randrange(20, 60), 0.3, have=len(s.data))
    if kind == "fixed":
        return s.fixed(toks + lits(rng, nine, 144, 256), final)
    return s.dyn(SHORT, toks + lits(rng, nine, 226, 256), final)


def _sequences(add):
    # each kind behind each kind, the first ending at each bit phase (a stored block always ends on a byte: phase 0 only;
    # its header, which is what the phase moves, starts at every phase behind the other two kinds)
    for first in ("stored", "fixed", "dynamic"):
        for second in ("stored", "fixed", "dynamic"):
            for phase in range(8) if first != "stored" else (0,):
                rng = _rng("seq_%s_%s_%d" % (first, second, phase))
                state = rng.getstate()
                for nine in range(8):
                    rng.setstate(state)
                    s = _small_block(Stream(), first, rng, 0, nine)
                    if s.w.bits % 8 == phase:
                        break
                else:
                    raise AssertionError("phase not reached")
                add("seq_%s_%s_phase%d" % (first, second, phase), _small_block(s, second, rng, 1))
    rng = _rng("stored")
    for n in (0, 1, MAX_PAYLOAD - 5):  # (header: three bits padded to a byte, LEN, NLEN)
        add("seq_stored_len%d" % n, Stream().stored(bytes(rng.randrange(256) for _ in range(n)), 1))
    # zlib's own streams cut by flushes at seeded places: empty stored blocks (sync, full) and empty fixed blocks (partial)
    for fname in ("Z_SYNC_FLUSH", "Z_FULL_FLUSH", "Z_PARTIAL_FLUSH"):
        data = bytes(rng.choice(b"ACGTN\n!#") for _ in range(30000))
        co, parts, at = zlib.compressobj(6, zlib.DEFLATED, -15), [], 0
        for cut in sorted(rng.randrange(1, len(data)) for _ in range(12)) + [len(data)]:
            parts.append(co.compress(data[at:cut]) + co.flush(getattr(zlib, fname)))
            at = cut
        parts.append(co.flush())
        add("seq_zlib_" + fname.lower(), (b"".join(parts), data))


def _wide_step(add):
    A, M = ("lit", 65), ("match", 258, 1)
    # (the first chain starts at the first token: the tables are built before the wide step is entered)
    add("wide_cap_exceeded_8256_per_window", Stream().dyn(TINY, [A] + [M] * 200, 1))
    add("wide_cap_kept_2048", Stream().dyn(TINY, [A] + [M] * 7 + [("match", 241, 1)] + [M] * 9, 1))
    add("wide_cap_kept_2047", Stream().dyn(TINY, [A] + [M] * 7 + [("match", 240, 1)] + [M] * 9, 1))
    # 1791 bytes kept, the 258-byte match that would make them 2049 cut off
    add("wide_cap_kept_1791_next_258", Stream().dyn(TINY, [A] + [M] * 6 + [("match", 242, 1)] + [M] * 9, 1))
    add("wide_cap_end_code_behind_the_cut", Stream().dyn(TINY, [A] + [M] * 8, 1))
    add("wide_match_dist1_after_literal", Stream().dyn(TINY, [A, ("match", 227, 1), A, M], 1))
    # distance x length, through the wide step (copy_at) and through the symbol loop (copy: a long-coded length symbol, a
    # long-coded distance symbol); the match once behind a seeded run of literals and once more a few literals on
    for path, cs in PATHS:
        for d in (1, 2, 3, 63, 64, 65, 257):
            for ln in (3, 4, 63, 64, 65, 66, 257, 258):
                rng = _rng("wide_%s_%d_%d" % (path, d, ln))
                toks = lits(rng, 257 + rng.randrange(40)) + [("match", ln, d)] + lits(rng, rng.randrange(8)) + [("match", ln, d)] + lits(rng, 3)
                add("wide_%s_dist%d_len%d" % (path, d, ln), Stream().dyn(cs, toks, 1))


def _ring(add):
    for path, cs in PATHS:
        for d in (6143, 6144, 6145, 8191, 8192, 8193, 32767, 32768):
            for r in (2047, 2048, 2049):
                rng = _rng("ring_%s_%d_%d" % (path, d, r))
                p = r
                while p < d:
                    p += 2048
                # (most of the way in a stored block: cheap to write; the last 2100 bytes, more than a flush, as literals)
                head = bytes(rng.randrange(256) for _ in range(p - 2100 - rng.randrange(64)))
                ln = rng.choice((3, 64, 65, 258))
                toks = lits(rng, p - len(head)) + [("match", ln, d), ("lit", 7), ("lit", 9), ("match", 258, d)] + lits(rng, 2)
                add("ring_%s_dist%d_at%d_len%d" % (path, d, p, ln), Stream().stored(head).dyn(cs, toks, 1))
        for p in (5000, 8192, 32768):  # dist == out
            rng = _rng("ring_all_%s_%d" % (path, p))
            head = bytes(rng.randrange(256) for _ in range(p - 300))
            add("ring_%s_dist_equals_out_%d" % (path, p), Stream().stored(head).dyn(cs, lits(rng, 300) + [("match", 258, p), ("match", 3, p)], 1))
    # The aliasing case: one chain holds a 3-byte match A at `at` with distance D, the 258-byte match B and a literal, which
    # lies at at + 261; its ring slot is that of A's source byte k when D = 8192 - 261 + k.  The chain's literals are in the
    # ring before its matches are copied, so A must read that byte from the flushed output (D > 8192 - 2048).
    for k in range(3):
        for at in (8000, 12345, 16383):
            rng = _rng("alias_%d_%d" % (k, at))
            head = bytes(rng.randrange(256) for _ in range(at))
            d = 8192 - 261 + k
            x = head[at - d + k] ^ 0x55
            cs = CodeSet(sparse(286, {x: 2, 256: 2, 257: 2, 285: 2}), sparse(26, {0: 1, 25: 1}), cl_lens=CL_FULL)
            add("ring_alias_k%d_at%d" % (k, at), Stream().stored(head).dyn(cs, [("match", 3, d), ("match", 258, 1), ("lit", x)], 1))


# the longest token the wide step takes: a 10-bit length code + 5 extra bits + an 8-bit distance code + 13 extra bits.
# Literals in 9 bits, length 258 in 2, the end code in 3, lengths 227 .. 257 in 10; distance 257 in 1, distance 1 in 2,
# 16385 .. 24576 in 8 (filler: the 9-bit literal and the 4-bit match (258, 1)).
LL_36 = sparse(286, {**{b: 9 for b in range(256)}, **{285: 2, 256: 3, 284: 10, 283: 10, 282: 4, 281: 5, 280: 6, 279: 7, 278: 8, 277: 9}})
DL_36 = sparse(30, {16: 1, 0: 2, 1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 28: 8, 29: 8})
CS_36 = CodeSet(LL_36, DL_36)
LONGEST = ("match", 255, 24569)  # (extra bits 28 of 31 and 8184 of 8191: the token's top bits are ones)
assert token_bits(LONGEST, CS_36.lit, CS_36.dist) == 36


def _input_window(add):
    # payload lengths around the staging chunk and the window, and the largest a block holds, with the last token (the end
    # code) ending on the payload's last bit and seven bits before it: a fixed block of 8- and 9-bit literals
    for n in (2047, 2048, 2049, 4095, 4096, 4097, 6144, MAX_PAYLOAD):
        for pad in (0, 7):
            rng = _rng("pay_%d_%d" % (n, pad))
            gap = n * 8 - pad - 3 - 7
            toks = fill_tokens(gap, ("lit", 1), ("lit", 200), FIXED_LIT, FIXED_DIST)
            toks = [("lit", rng.randrange(144) if t[1] == 1 else rng.randrange(144, 256)) for t in toks]
            rng.shuffle(toks)
            s = Stream().fixed(toks, 1)
            assert s.w.bits == n * 8 - pad
            add("input_payload%d_pad%d" % (n, pad), s)
    # the 36-bit token across input byte 2048 and across byte 4096, starting at each bit phase of a 32-bit word
    for phase in range(32):
        rng = _rng("straddle_%d" % phase)
        s = Stream()
        w = s.w.clone()
        CS_36.put(w, [], 0)
        hdr = w.bits  # (the header's bits)
        toks = lits(rng, 257, 0, 256) + [("match", 258, 257)] * 100
        for edge in (2048, 4096):
            used = hdr + sum(token_bits(t, CS_36.lit, CS_36.dist) for t in toks)
            fill = fill_tokens(edge * 8 - 32 + phase - used, ("lit", 0), ("match", 258, 1), CS_36.lit, CS_36.dist)
            toks += [("lit", rng.randrange(256)) if t[0] == "lit" else t for t in fill] + [LONGEST]
        s.dyn(CS_36, toks + lits(rng, 5, 0, 256), 1)
        add("input_straddle_phase%d" % phase, s)


def _sizes(add):
    for n in (0, 1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 65280, 65535, 65536):
        rng = _rng("size_%d" % n)
        add("size_%d" % n, Stream().dyn(SHORT, random_tokens(rng, n, 0.2 if n < 10000 else 0.6), 1))
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    add("size_65536_zeros_from_zlib", (co.compress(bytes(65536)) + co.flush(), bytes(65536)))


def _zlib_takes(payload, data):
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(payload) == data and d.eof and not d.unused_data
    except zlib.error:
        return False


@functools.lru_cache(maxsize=None)
def valid():
    cases = []

    def add(name, s):
        payload, data = s.done() if isinstance(s, Stream) else s
        assert len(payload) <= MAX_PAYLOAD and len(data) <= 65536, (name, len(payload), len(data))
        assert _zlib_takes(payload, data), name
        cases.append((name, payload, data))
    for part in (_code_shapes, _sequences, _wide_step, _ring, _input_window, _sizes):
        part(add)
    assert len({c[0] for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def valid_lenient():
    """An incomplete literal / length code (Kraft sum 1/2) whose missing codes are never used: zlib refuses the header
    ("invalid literal/lengths set"), the project's inflater — table builder code_prepare tests for oversubscription only —
    takes it and gives the right bytes.  Pinned as it is: a known difference."""
    cs = CodeSet(sparse(257, {65: 2, 256: 2}), [0], cl_lens=CL_FULL)
    payload, data = Stream().dyn(cs, [("lit", 65)] * 10, 1).done()
    assert not _zlib_takes(payload, data)
    return [("lenient_incomplete_litlen_unused", payload, data)]


# ---- the refusals ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refused():
    cases = []

    def add(name, s, status, note, isize=None, cut=0, in_bytes=True):
        payload, data = s.done() if isinstance(s, Stream) else s
        if cut:
            payload = payload[:-cut]
        if in_bytes:  # the fault is in the DEFLATE bytes: zlib refuses them too, or wants more
            d = zlib.decompressobj(-15)
            try:
                d.decompress(payload)
                assert not d.eof, name
            except zlib.error:
                pass
        else:
            assert _zlib_takes(payload, data), name
        cases.append((name, bgzf(payload, data, isize=isize), status, note))
    rng = _rng("refused")
    some = lits(rng, 40)
    A = ("lit", 65)

    # ST_BAD_BTYPE
    s = Stream()
    s.w.put(1, 1), s.w.put(3, 2)
    add("btype3_first", s, ST_BAD_BTYPE, "the first block header says type 3", isize=0)
    s = Stream().fixed(some)
    s.w.put(1, 1), s.w.put(3, 2)
    add("btype3_after_valid_block", s, ST_BAD_BTYPE, "a valid non-final fixed block, then type 3")
    # ST_BAD_STORED
    body = bytes(range(50))
    add("stored_nlen_one_bit_off", Stream().stored(body, 1, nlen=(50 ^ 0xFFFF) ^ 0x0100), ST_BAD_STORED, "NLEN is ~LEN with bit 8 flipped")
    # ST_BAD_LENGTHS
    cl = sparse(19, {16: 2, 18: 2, 1: 2, 0: 2})
    bad = CodeSet(sparse(257, {65: 1, 256: 1}), [0], spelled=[(16, 3), (18, 62), 1, (18, 138), (18, 52), 1, 0], cl_lens=cl, hclen=18, check=False)
    add("lengths_16_first", Stream().dyn(bad, [A], 1), ST_BAD_LENGTHS, "symbol 16 (repeat the previous length) is the first length: there is none")
    bad = CodeSet(sparse(257, {65: 1, 256: 1}), [0], spelled=[(18, 65), 1, (18, 138), (18, 52), 1, (17, 3)],
                  cl_lens=sparse(19, {17: 2, 18: 2, 1: 1}), hclen=18, check=False)
    add("lengths_repeat_one_past_total", Stream().dyn(bad, [A], 1), ST_BAD_LENGTHS,
        "257 of HLIT + HDIST = 258 lengths are set, then a run of three zeros: one length too many")
    for field in (30, 31):
        bad = CodeSet(LL_SHORT, DL_SHORT, hlit=257 + field, spelled=LL_SHORT + [0] * (field - 29) + DL_SHORT, check=False)
        add("lengths_hlit_field_%d" % field, Stream().dyn(bad, some, 1), ST_BAD_LENGTHS, "HLIT %d: more than 286 literal / length lengths" % (257 + field))
        bad = CodeSet(LL_SHORT, DL_SHORT, hdist=1 + field, spelled=LL_SHORT + DL_SHORT + [0] * (field - 29), check=False)
        add("lengths_hdist_field_%d" % field, Stream().dyn(bad, some, 1), ST_BAD_LENGTHS, "HDIST %d: more than 30 distance lengths" % (1 + field))
    # ST_OVERSUBSCRIBED
    bad = CodeSet(sparse(257, {65: 1, 256: 1}), [0], spelled=[(18, 65), 1, (18, 138), (18, 52), 1, 0], cl_lens=sparse(19, {18: 1, 1: 1, 0: 1}), hclen=18, check=False)
    add("oversubscribed_code_length_code", Stream().dyn(bad, [A], 1), ST_OVERSUBSCRIBED, "three 1-bit codes in the code length code")
    bad = CodeSet(sparse(257, {65: 1, 66: 1, 256: 1}), [0], cl_lens=CL_FULL, check=False)
    add("oversubscribed_literal_code", Stream().dyn(bad, [A], 1), ST_OVERSUBSCRIBED, "three 1-bit codes in the literal / length code (256 among them)")
    bad = CodeSet(sparse(258, {65: 2, 256: 2, 257: 1}), [1, 1, 1], cl_lens=CL_FULL, check=False)
    add("oversubscribed_distance_code", Stream().dyn(bad, [A], 1), ST_OVERSUBSCRIBED, "a complete literal / length code, three 1-bit codes in the distance code")
    # ST_BAD_SYMBOL
    half = CodeSet(sparse(257, {65: 2, 256: 2}), [0], cl_lens=CL_FULL)  # codes 00 and 01 (as written): 1x is nobody's
    w = BitWriter()
    half.put(w, [A, A, ("bits", 0x7FFF, 15)], 1)
    add("symbol_unassigned_code_used", (w.done(), b"AA"), ST_BAD_SYMBOL,
        "an incomplete literal / length code (lengths 2, 2); after two literals the stream holds 1-bits, no symbol's code", isize=2)
    def raw_fixed(tokens):
        w = BitWriter()
        fixed(w, tokens, 1)
        return w.done()
    for sym in (286, 287):
        add("symbol_fixed_%d" % sym, (raw_fixed(some + [("sym", "l", sym), ("sym", "d", 0), ("end",)]), bytes(expand(some))), ST_BAD_SYMBOL,
            "length symbol %d of the fixed code (ISIZE: the forty literals before it)" % sym)
    for sym in (30, 31):
        add("symbol_fixed_distance_%d" % sym, (raw_fixed(some + [("sym", "l", 257), ("sym", "d", sym), ("end",)]), bytes(43)), ST_BAD_SYMBOL,
            "distance symbol %d of the fixed code behind length symbol 257 (ISIZE: forty literals and the three bytes)" % sym)
    # ST_BAD_DISTANCE (ISIZE is what the tokens would give: nothing else is wrong)

    def too_far(name, cs, toks, note):
        s = Stream()
        cs.put(s.w, toks + [("end",)], 1)
        n = sum(1 if t[0] == "lit" else t[1] for t in toks)
        add(name, (s.w.done(), bytes(n)), ST_BAD_DISTANCE, note)
    too_far("distance_match_first", SHORT, [("match", 3, 1), A], "a match is the first token: no output to copy from")
    too_far("distance_out_plus_1_at_1", SHORT, [A, ("match", 3, 2), A], "one byte of output, distance 2")
    too_far("distance_mid_chain", SHORT, [A, A, A, ("match", 4, 3), ("match", 3, 8), A],
            "seven bytes of output (three literals and a 4-byte match, decoded in the same 64 bits), distance 8")
    too_far("distance_long_coded_length", LONG_LEN, [A, A, A, ("match", 4, 3), ("match", 3, 8), A],
            "the same tokens with 13-bit length codes: seven bytes of output, distance 8")
    # ST_OUT_OVERRUN: ISIZE one too small, by the kind of the last token
    mm = [("match", 20, 33)]
    for name, s in (("wide_literal", Stream().dyn(SHORT, some + [A], 1)), ("wide_match", Stream().dyn(SHORT, some + mm, 1)),
                    ("long_coded_literal", Stream().dyn(CodeSet(sparse(259, {**{b: 8 for b in range(255)}, **{255: 11, 256: 9, 257: 11, 258: 10}}), [0]), some + [("lit", 255)], 1)),
                    ("long_coded_match", Stream().dyn(LONG_LEN, some + mm, 1)), ("stored_byte", Stream().fixed(some).stored(b"xyz", 1))):
        add("isize_one_too_small_" + name, s, ST_OUT_OVERRUN, "a valid stream, ISIZE one less than it gives; its last byte comes from a " + name.replace("_", " "),
            isize=len(s.data) - 1, in_bytes=False)
    # ST_OUT_SHORT
    s = Stream().dyn(SHORT, some + mm, 1)
    add("isize_one_too_large", s, ST_OUT_SHORT, "a valid stream, ISIZE one more than it gives", isize=len(s.data) + 1, in_bytes=False)
    # ST_IN_OVERRUN
    cs = CodeSet(sparse(257, {256: 1, 65: 2, 66: 3, 67: 3}), [0], cl_lens=CL_FULL)  # the end code is the one 1-bit code: 0
    s = Stream()
    w = s.w.clone()
    cs.put(w, [], 0)
    toks = fill_tokens((-w.bits) % 8 + 48, ("lit", 65), ("lit", 66), cs.lit, cs.dist)
    s.dyn(cs, toks, 1)
    assert s.w.bits % 8 == 1  # (the end code is the first bit of the last byte)
    add("payload_cut_before_end_code", s, ST_IN_OVERRUN, "the payload's last byte, which held the 1-bit end code and padding, is cut off: the "
        "zeros read beyond the payload are that code, and it lies wholly beyond the compressed bytes", cut=1)
    s = Stream().fixed(some)
    stored(s.w, bytes(20), 1, length=120)
    add("stored_len_beyond_payload", (s.w.done(), bytes(s.data) + bytes(120)), ST_IN_OVERRUN, "a stored block of LEN 120 with 20 bytes left in the payload (ISIZE counts 120)")
    # ST_NO_END_CODE
    bad = CodeSet([0] * 257, [0], hclen=4, cl_lens=sparse(19, {18: 1, 0: 1}), spelled=[(18, 138), (18, 119), 0], check=False)
    s = Stream()
    bad.put(s.w, [], 1)
    add("no_end_code_hclen4", s, ST_NO_END_CODE, "HCLEN 4 gives lengths to 16, 17, 18 and 0 alone: every literal / length is zero, 256 too", isize=0)
    bad = CodeSet(sparse(257, {65: 1, 66: 1}), [0], cl_lens=CL_FULL, check=False)
    s = Stream()
    bad.put(s.w, [A], 1)
    add("no_end_code_two_literals", s, ST_NO_END_CODE, "a complete literal code of two 1-bit codes, none for 256", isize=1)
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def __getattr__(name):  # the three lists by their names, built on first use
    if name in ("VALID", "VALID_LENIENT", "REFUSED"):
        return {"VALID": valid, "VALID_LENIENT": valid_lenient, "REFUSED": refused}[name]()
    raise AttributeError(name)


def corpus_file(path):
    """every case as a record '<II' clen, isize + payload for tests/tools/inflate_cases_test.cpp -> [(name, status, crc or None)]"""
    want = []
    with open(path, "wb") as f:
        for name, payload, data in valid() + valid_lenient():
            f.write(struct.pack("<II", len(payload), len(data)) + payload)
            want.append((name, ST_OK, zlib.crc32(data) & 0xFFFFFFFF))
        for name, block, status, note in refused():
            payload, _, isize = split(block)
            f.write(struct.pack("<II", len(payload), isize) + payload)
            want.append((name, status, None))
    return want
