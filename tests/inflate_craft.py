"""Deflate streams built bit by bit (RFC 1951), for the device inflate's tests.

zlib's compressor never emits most of what a decoder must accept or refuse: 15-bit codes, code-length
repeats that run from the literal/length lengths into the distance lengths, a distance set of one
code or of none, empty blocks between others.  ``BitWriter`` and ``Deflate`` write such blocks from
chosen code lengths; ``crafted_valid()`` lists the valid ones with their expected bytes,
``crafted_invalid()`` a stream for every status code 1..10, ``zlib_cases()`` the streams Python's zlib
compresses for the block-kind / length / distance cases, and ``mutations()`` bit flips and
truncations of valid streams.  Expected bytes of the valid streams come from the token lists here and
are checked against ``zlib.decompress`` by the tests that use them.
"""
import functools
import zlib

import numpy as np

KD_INF_MAX = 256 << 10
STATUS_NAMES = {1: "header", 2: "btype", 3: "stored", 4: "lens", 5: "symbol", 6: "dist", 7: "over", 8: "short",
                9: "src", 10: "adler"}

# RFC 1951 §3.2.5: (base, extra bits) of length symbols 257..285 and distance symbols 0..29
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def length_symbol(n):
    if n == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= n)
    return 257 + s, LEN_EXTRA[s], n - LEN_BASE[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def canonical_codes(lens):
    """{symbol: (code, length)} by RFC 1951 §3.2.2"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def complete_lengths(k):
    """lengths of a complete prefix code of k >= 2 symbols"""
    p = k.bit_length() - 1
    longer = 2 * (k - (1 << p))
    return [p] * (k - longer) + [p + 1] * longer


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code, most significant bit first"""
        for k in range(n - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


class Deflate:
    """a deflate stream assembled block by block; tokens are ints (literals) or (length, distance)"""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()

    def _apply(self, tokens):
        for t in tokens:
            if isinstance(t, int):
                self.data.append(t)
            else:
                n, d = t
                for _ in range(n):
                    self.data.append(self.data[-d])

    def _tokens(self, tokens, lit, dist):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*lit[t])
            else:
                s, eb, ev = length_symbol(t[0])
                w.code(*lit[s])
                w.bits(ev, eb)
                s, eb, ev = dist_symbol(t[1])
                w.code(*dist[s])
                w.bits(ev, eb)
        w.code(*lit[256])

    def stored(self, payload=b"", final=False, nlen=None):
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align()
        w.bits(len(payload), 16)
        w.bits(len(payload) ^ 0xFFFF if nlen is None else nlen, 16)
        for b in payload:
            w.bits(b, 8)
        self.data += payload
        return self

    def fixed(self, tokens=(), final=False):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self._tokens(tokens, canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST))
        self._apply(tokens)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, rle=False, cl_lens=None, cl_syms=None):
        """lit_lens [257..286] and dist_lens [1..30] as chosen; the lengths are sent one symbol each,
        or run-length coded over their concatenation with ``rle`` (a run at the seam then crosses it).
        ``cl_syms``: the code-length symbols themselves as (symbol, extra value) pairs; ``cl_lens``:
        the 19 code-length code lengths instead of a complete code over the symbols used."""
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        seq = list(lit_lens) + list(dist_lens)
        if cl_syms is None:
            cl_syms = _rle(seq) if rle else [(n, 0) for n in seq]
        if cl_lens is None:
            used = sorted({s for s, _ in cl_syms})
            if len(used) == 1:
                used.append(next(s for s in range(19) if s not in used))
            cl_lens = [0] * 19
            for s, n in zip(used, complete_lengths(len(used))):
                cl_lens[s] = n
        ncl = max(i for i in range(19) if cl_lens[CL_ORDER[i]] or i < 4) + 1
        w.bits(len(lit_lens) - 257, 5)
        w.bits(len(dist_lens) - 1, 5)
        w.bits(ncl - 4, 4)
        for i in range(ncl):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cl = canonical_codes(cl_lens)
        for s, ev in cl_syms:
            w.code(*cl[s])
            if s >= 16:
                w.bits(ev, {16: 2, 17: 3, 18: 7}[s])
        self._tokens(tokens, canonical_codes(lit_lens), canonical_codes(dist_lens))
        self._apply(tokens)
        return self

    def raw(self):
        return self.w.bytes()

    def zlib(self, adler=None):
        a = zlib.adler32(bytes(self.data)) if adler is None else adler
        return b"\x78\x9c" + self.raw() + a.to_bytes(4, "big")


def _rle(seq):
    """code-length symbols (RFC 1951 §3.2.7) of a length sequence, greedy"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


def _lens(n, pairs):
    out = [0] * n
    for s, v in pairs:
        out[s] = v
    return out


def _fifteen():
    """literals 'A'..'N' with 1..14-bit codes, 'O' and end-of-block with 15-bit codes; no distance code"""
    lit = _lens(257, [(65 + k, k + 1) for k in range(14)] + [(79, 15), (256, 15)])
    text = [65 + (k * 7) % 15 for k in range(90)]
    return Deflate().dynamic(text, lit, [0], final=True)


def _seam():
    """a 16-repeat that starts in the literal/length lengths and ends in the distance lengths, zero runs
    coded with 17 and 18"""
    lit = _lens(260, [(97, 4), (98, 4), (99, 4), (256, 4), (257, 2), (258, 2), (259, 2)])
    dist = [2, 2, 2, 2]
    toks = [97, 98, 99, (3, 3), (4, 1), 98, (5, 4), (3, 2), 97]
    d = Deflate().dynamic(toks, lit, dist, final=True, rle=True)
    return d


def _one_distance():
    lit = _lens(258, [(120, 1), (256, 2), (257, 2)])
    return Deflate().dynamic([120, (3, 1), (3, 1), 120], lit, [1], final=True)


def _no_distance():
    lit = _lens(257, [(104, 2), (105, 2), (33, 2), (256, 2)])
    return Deflate().dynamic([104, 105, 33, 33, 104], lit, [0], final=True)


def _empty_stored_between():
    lit = _lens(257, [(48, 1), (49, 2), (256, 2)])
    return Deflate().fixed([ord(c) for c in "abc"] + [(6, 3)]).stored(b"").dynamic([48, 49, 48, 48], lit, [0], final=True)


def _final_empty_fixed():
    return Deflate().fixed([ord(c) for c in "tail"] + [(4, 4)]).fixed((), final=True)


def _final_empty_stored():
    return Deflate().stored(b"stored first").fixed([(12, 12)]).stored(b"", final=True)


def _far_literals(n):
    """n literal bytes with no pattern in them"""
    return np.random.default_rng(32768).integers(0, 256, n, dtype=np.uint8).tolist()


def _distance_32768():
    """the farthest distance there is (symbol 29, all 13 extra bits set), which zlib's compressor never
    emits (it looks back 32,506 bytes at most): at the longest length, at the shortest, then a distance
    of 1 behind them; one fixed block"""
    return Deflate().fixed(_far_literals(32768) + [(258, 32768), (3, 32768), (258, 1)], final=True)


@functools.lru_cache(maxsize=None)
def crafted_valid():
    """[(name, zlib stream, expected bytes)]"""
    out = []
    for name, f in (("fifteen_bit_codes", _fifteen), ("repeat_across_seam", _seam), ("one_distance_code", _one_distance),
                    ("no_distance_code", _no_distance), ("empty_stored_between", _empty_stored_between),
                    ("final_empty_fixed", _final_empty_fixed), ("final_empty_stored", _final_empty_stored),
                    ("distance_32768", _distance_32768)):
        d = f()
        out.append((name, d.zlib(), bytes(d.data)))
    return out


@functools.lru_cache(maxsize=None)
def crafted_invalid():
    """[(name, stream, dst_len, status)]: every status code 1..10, and the distance check at its far end"""
    ten = zlib.compress(b"0123456789", 6)
    over = Deflate()
    over.w.bits(1, 1)
    over.w.bits(2, 2)
    over.w.bits(0, 5)
    over.w.bits(0, 5)
    over.w.bits(0, 4)  # four code-length code lengths: 16, 17, 18, 0
    for n in (1, 1, 1, 0):  # three one-bit codes
        over.w.bits(n, 3)
    sym286 = Deflate()
    sym286.w.bits(1, 1)
    sym286.w.bits(1, 2)
    sym286.w.code(0b11000110, 8)  # literal/length 286 of the fixed code
    far = Deflate()
    far.w.bits(1, 1)
    far.w.bits(1, 2)
    lit, dist = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)
    far.w.code(*lit[97])
    far.w.code(*lit[257])  # length 3
    far.w.code(*dist[4])   # distance 5 + extra
    far.w.bits(0, 1)
    far.w.code(*lit[256])
    # distance 32,768 after 32,767 bytes: one byte too far, at the largest distance the format has
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for b in _far_literals(32767):
        w.code(*lit[b])
    w.code(*lit[257])
    w.code(*dist[29])
    w.bits(8191, 13)  # 24,577 + 8,191 = 32,768
    w.code(*lit[256])
    return [
        ("bad_header", b"\x78\x9d" + ten[2:], 10, 1),
        ("reserved_block_type", b"\x78\x9c\x07" + b"\0" * 8, 4, 2),
        ("stored_nlen", Deflate().stored(b"abcd", final=True, nlen=0x1234).zlib(), 4, 3),
        ("oversubscribed", b"\x78\x9c" + over.raw() + b"\0" * 8, 4, 4),
        ("symbol_286", b"\x78\x9c" + sym286.raw() + b"\0" * 8, 4, 5),
        ("distance_too_far", b"\x78\x9c" + far.raw() + b"\0" * 8, 4, 6),
        ("more_than_expected", ten, 9, 7),
        ("less_than_expected", ten, 11, 8),
        ("truncated", ten[:len(ten) - 7], 10, 9),
        ("adler", ten[:-1] + bytes([ten[-1] ^ 0x40]), 10, 10),
        ("distance_32768_too_far", b"\x78\x9c" + w.bytes() + b"\0" * 8, 32770, 6),
    ]


def _compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, a = b"", 0
    for cut in list(flush_at) + [len(data)]:
        out += c.compress(data[a:cut])
        if cut != len(data):
            out += c.flush(flush)
        a = cut
    return out + c.flush()


@functools.lru_cache(maxsize=None)
def zlib_cases():
    """[(name, zlib stream, expected bytes)] compressed by Python's zlib: block kinds, lengths, distances"""
    rng = np.random.default_rng(20261020)
    text = (b"the quick brown fox jumps over the lazy dog; " * 40)[:1500]
    rnd = rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes()
    small = rng.integers(97, 101, 3000, dtype=np.uint8).tobytes()
    out = []
    for lvl, name in ((0, "stored"), (9, "level9")):
        out.append((f"text_{name}", zlib.compress(text, lvl), text))
    out.append(("text_fixed", _compress(text, 6, zlib.Z_FIXED), text))
    out.append(("sync_flush", _compress(text + rnd[:700] + small, 6, flush_at=(100, 1500, 2200)), text + rnd[:700] + small))
    out.append(("full_flush", _compress(small + text, 9, flush_at=(1, 3000), flush=zlib.Z_FULL_FLUSH), small + text))
    out.append(("fixed_then_flush", _compress(text, 6, zlib.Z_FIXED, flush_at=(7, 8)), text))
    for n in (0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259):
        for lvl in (0, 6):
            d = (text * 2)[:n] if lvl == 0 else bytes([65 + (k % 3 == 0) for k in range(n)])
            out.append((f"len{n}_l{lvl}", zlib.compress(d, lvl), d))
    for n in (65_535, 65_536):
        out.append((f"len{n}_l0", zlib.compress(rnd[:n], 0), rnd[:n]))
    big = (rnd[:50_000] + text * 100 + bytes(KD_INF_MAX))[:KD_INF_MAX]
    out.append(("inf_max_l6", zlib.compress(big, 6), big))
    out.append(("inf_max_l0", zlib.compress(big, 0), big))
    run = b"z" * 259
    out.append(("run_of_one", zlib.compress(run, 9), run))
    for period in (b"ab", b"abc"):
        d = (period * 200)[:517]
        out.append((f"period{len(period)}", zlib.compress(d, 9), d))
    far = rnd[:32_768] + rnd[:300]  # (zlib finds no match here: it looks back 32,506 bytes at most; the
    out.append(("repeat_beyond_zlibs_reach", zlib.compress(far, 9), far))  # real case is crafted_valid's)
    near = rnd[:32_000] + rnd[:300]
    out.append(("distance_32000", zlib.compress(near, 9), near))
    out.append(("small_alphabet", zlib.compress(small, 9), small))
    return out


def all_valid():
    return zlib_cases() + crafted_valid()


def mutations(n=2000, seed=7):
    """[(stream, dst_len)]: single bit flips and truncations of the valid streams below 4 KiB"""
    rng = np.random.default_rng(seed)
    base = [(s, len(e)) for _, s, e in all_valid() if len(s) < 4096]
    out = []
    for k in range(n):
        s, dl = base[int(rng.integers(len(base)))]
        if k % 4 == 3:
            out.append((s[:int(rng.integers(len(s)))], dl))
        else:
            bit = int(rng.integers(8 * len(s)))
            m = bytearray(s)
            m[bit >> 3] ^= 1 << (bit & 7)
            out.append((bytes(m), dl))
    return out


def zlib_verdict(stream, dst_len):
    """the expected bytes where zlib reaches the end of the stream with exactly dst_len bytes, else None"""
    d = zlib.decompressobj()
    try:
        data = d.decompress(stream)
    except zlib.error:
        return None
    return data if d.eof and len(data) == dst_len else None
