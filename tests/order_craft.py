"""Crafted inputs and exact references for the order kernels of kart_amd/csrc/kd_sort.hip: the pk order
of delta records (bitmap placement and the radix sort behind kd_delta_pk_order, and kd_diff2_step's
LDS-free scans) and the side sorts.  Host only: numpy and the int-PK join key of kart_amd/walkkey.py.

A record's pk is known from how the record was crafted (never decoded from its key), and the expected
outputs are the crafted pks themselves sorted by numpy: pk list = sort, perm = stable argsort.  Every
crafted index lies inside its side and every crafted pk inside [pk_lo, pk_hi], so no case can drive a
kernel out of its documented contract.

Every case states the path it is meant to reach (``Case.expect``); ``bitmap_geometry`` /
``radix_geometry`` derive the same figures from the kernel constants below, and the CPU part of
test_order_crafted.py asserts that the two agree and that the constants equal the source's.
"""
from dataclasses import dataclass, field

import numpy as np

from kart_amd import walkkey

# ---- the kernel constants the edges depend on (kd_sort.hip; pinned by test_order_crafted.py) ----
PKM_NT = 256        # threads of a mark / scan / place block
PKM_IPT = 16        # masks per scan thread
PKM_CH = 4096       # masks per block-wide scan chunk (PKM_NT * PKM_IPT)
PKM_CHW = 1024      # masks per LDS-free (one wave) scan chunk (64 * PKM_IPT)
PKC_PT = 8          # chunk totals per thread and trip of k_pkm_cscan (1024 threads)
PKC_WPT = 32        # chunk totals per lane and trip of k_pkm_cscan_w (64 lanes)
RS_RB = 9           # digit bits per radix pass (at most)
RS_NT = 512         # threads of a k_sort_pass block
IPT32 = 16          # items per thread, 32-bit compact keys (tile of 8192)
IPT64 = 8           # items per thread, 64-bit compact keys (tile of 4096)
RS_HIST_CHUNK = 4096  # keys per k_sort_hist block and round (256 threads x 16 keys)
RS_LBW = 4          # look-back words per round trip
RS_MAXRUNS = 4      # compaction runs of a sort plan
PKM_MAX_BLOCKS = 1 << 26  # the pkm_max_blocks option's default: largest bitmap range in blocks

CSCAN_TRIP = 1024 * PKC_PT    # chunks one trip of k_pkm_cscan covers
CSCAN_W_TRIP = 64 * PKC_WPT   # chunks one trip of k_pkm_cscan_w covers
TILE32 = RS_NT * IPT32
TILE64 = RS_NT * IPT64

NONE = 0xFFFFFFFF
INSERT, DELETE, UPDATE, SAME = 0, 1, 2, 3  # record kinds (SAME: in both sides, equal OIDs — step sides only)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# every msgpack width limit of an int pk and its neighbours inside [-2**31, 2**31 - 1]
MSGPACK_EDGES = (-2**31, -32769, -32768, -129, -128, -33, -32, -1, 0, 127, 128, 255, 256, 65535, 65536, 2**31 - 1)


def _cdiv(a, b):
    return -(-a // b)


def bitmap_geometry(lo, hi, wave=False):
    """blocks, scan chunks and chunk-total trips of the bitmap placement over [lo, hi]"""
    nb = (hi >> 6) - (lo >> 6) + 1
    nch = _cdiv(nb, PKM_CHW if wave else PKM_CH)
    return {"nb": nb, "nch": nch, "trips": _cdiv(nch, CSCAN_W_TRIP if wave else CSCAN_TRIP)}


def radix_geometry(lo, hi):
    """plan width, passes, digit width and compact key type of the radix pk order over [lo, hi]"""
    bits = ((lo ^ hi) & ((1 << 64) - 1)).bit_length()
    if bits == 0:  # the single-pk plan: one pass over one bit
        return {"bits": 0, "npass": 1, "width": 1, "ck": 32}
    npass = _cdiv(bits, RS_RB)
    return {"bits": bits, "npass": npass, "width": _cdiv(bits, npass), "ck": 32 if bits <= 32 else 64}


def takes_bitmap(lo, hi, pkm_max=PKM_MAX_BLOCKS):
    return bitmap_geometry(lo, hi)["nb"] <= pkm_max


# ---- pk sets ------------------------------------------------------------------------------------
def pk_set(lo, hi, blocks, density, rng=None):
    """ascending pks of [lo, hi] from a spec: ``blocks`` = absolute 64-pk block numbers (pk >> 6),
    ``density`` = one entry for all or one per block: "full", "bit0", "bit63", or a fraction of the
    block's 64 pks (at least one, chosen by ``rng``)"""
    blocks = list(blocks)
    dens = list(density) if isinstance(density, (list, tuple)) else [density]
    out = []
    for i, b in enumerate(blocks):
        d = dens[i % len(dens)]
        if d == "full":
            bits = range(64)
        elif d == "bit0":
            bits = [0]
        elif d == "bit63":
            bits = [63]
        else:
            bits = np.nonzero(rng.random(64) < d)[0].tolist() or [int(rng.integers(0, 64))]
        out += [64 * b + j for j in bits if lo <= 64 * b + j <= hi]
    return np.unique(np.asarray(out, np.int64))


def seam_blocks(nb):
    """relative blocks at the seams of the scans: the first and last blocks, each thread's 16 masks,
    the chunk of 4096 and of 1024"""
    rel = set(range(0, 40)) | set(range(nb - 40, nb))
    for s in (PKM_IPT, PKM_CHW, PKM_CH, 2 * PKM_CH, 2 * PKM_CHW, 3 * PKM_CHW, 4 * PKM_CHW):
        rel |= {s - 2, s - 1, s, s + 1}
    return sorted(r for r in rel if 0 <= r < nb)


# ---- record lists over two int sides -----------------------------------------------------------
@dataclass
class Case:
    """one kd_delta_pk_order call: the first len(pks) records are the head, in record order; ``tail``
    are records beyond the device count (the poisoned tail); ``over``: the device count exceeds the
    capacity by that much (it clamps)"""
    name: str
    lo: int
    hi: int
    pks: np.ndarray
    kinds: np.ndarray = None          # per head record; default: insert / delete / update in turn
    tail: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    over: int = 0
    expect: dict = field(default_factory=dict)  # the stated path: see test_order_crafted.py

    @property
    def cap(self):
        return int(len(self.pks) + len(self.tail))

    @property
    def dn(self):
        return int(len(self.pks)) + self.over

    @property
    def n(self):
        return min(self.dn, self.cap)


@dataclass
class Crafted:
    key_a: np.ndarray   # side keys, ascending
    key_b: np.ndarray
    pk_a: np.ndarray    # pk of each side entry
    pk_b: np.ndarray
    rec: np.ndarray     # uint32 [cap, 2]
    rkey: np.ndarray    # uint64 [cap]: each record's join key (the d_keys form)
    rec_pk: np.ndarray  # int64 [cap]: each record's pk, by construction
    want_pk: np.ndarray
    want_perm: np.ndarray


def _side(pks):
    """(keys ascending, pk of each entry) of a side holding these pks"""
    pks = np.asarray(pks, np.int64)
    keys = walkkey.int_keys(pks) if pks.size else np.zeros(0, np.uint64)
    o = np.argsort(keys, kind="stable")
    return np.ascontiguousarray(keys[o]), np.ascontiguousarray(pks[o])


def reference(rec_pk, n):
    """(pks ascending, record index of each) of the first n records: exact integer work"""
    perm = np.argsort(rec_pk[:n], kind="stable")
    return rec_pk[:n][perm], perm.astype(np.uint32)


def materialise(case):
    """the two sides, the record list (head then poisoned tail) and the expected outputs of a Case"""
    pks = np.concatenate([np.asarray(case.pks, np.int64), np.asarray(case.tail, np.int64)])
    kinds = np.arange(pks.size) % 3 if case.kinds is None else np.concatenate(
        [np.asarray(case.kinds), np.arange(len(case.tail)) % 3])
    kinds = np.asarray(kinds, np.int64)
    key_a, pk_a = _side(pks[kinds != INSERT])
    key_b, pk_b = _side(pks[kinds != DELETE])
    rkey = walkkey.int_keys(pks) if pks.size else np.zeros(0, np.uint64)
    ia = np.searchsorted(key_a, rkey)
    ib = np.searchsorted(key_b, rkey)
    rec = np.stack([np.where(kinds != INSERT, ia, NONE), np.where(kinds != DELETE, ib, NONE)], 1).astype(np.uint32)
    want_pk, want_perm = reference(pks, case.n)
    return Crafted(key_a, key_b, pk_a, pk_b, np.ascontiguousarray(rec), np.ascontiguousarray(rkey), pks, want_pk, want_perm)


def check_crafted(case, m):
    """the builders' invariants: unique pks inside the bounds, valid side indices that lead back to the
    record's pk, the intended record order, a tail disjoint from the head"""
    assert case.lo <= case.hi and case.cap > 0
    assert np.unique(m.rec_pk).size == m.rec_pk.size, "pks are unique"
    assert m.rec_pk.size == 0 or (m.rec_pk.min() >= case.lo and m.rec_pk.max() <= case.hi), "pks inside the bounds"
    assert np.array_equal(m.rec_pk[:len(case.pks)], np.asarray(case.pks, np.int64)), "record order as crafted"
    assert not np.intersect1d(case.pks, case.tail).size, "tail disjoint from the head"
    assert case.over == 0 or len(case.tail) == 0
    for side, (keys, spk) in enumerate(((m.key_a, m.pk_a), (m.key_b, m.pk_b))):
        assert np.all(keys[1:] > keys[:-1]), "side keys strictly ascending"
        idx = m.rec[:, side]
        has = idx != NONE
        assert np.all(idx[has] < keys.size), "record indices inside the side"
        assert np.array_equal(spk[idx[has]], m.rec_pk[has]) and np.array_equal(keys[idx[has]], m.rkey[has])
    assert not np.any((m.rec[:, 0] == NONE) & (m.rec[:, 1] == NONE))
    assert np.all(m.want_pk[1:] > m.want_pk[:-1]) and np.array_equal(m.rec_pk[m.want_perm], m.want_pk)


def _shuffled(pks, seed):
    return np.random.default_rng(seed).permutation(np.asarray(pks, np.int64))


def _seam_case(name, lo_block, nb, seed):
    """bounds pk_lo = 64k + 63, pk_hi = 64m (the first block holds bit 63 only, the last bit 0 only),
    records in the seam blocks: full blocks, bit-0-only and bit-63-only masks, random masks"""
    rng = np.random.default_rng(seed)
    if nb == 1:
        lo, hi = 64 * lo_block, 64 * lo_block + 63
        pks = pk_set(lo, hi, [lo_block], "full")
    else:
        lo, hi = 64 * lo_block + 63, 64 * (lo_block + nb - 1)
        pks = pk_set(lo, hi, [lo_block + r for r in seam_blocks(nb)], ["full", "bit0", 0.3, "bit63", 0.7], rng)
        if lo_block < 0 <= lo_block + nb - 1 and nb > 2:
            pks = np.union1d(pks, pk_set(lo, hi, [-1], "full"))  # the block [-64, -1]
        pks = np.union1d(pks, np.asarray([lo, hi], np.int64))    # bounds exact
    g =bitmap_geometry(lo, hi)
    assert g["nb"] == nb
    return Case(name, lo, hi, _shuffled(pks, seed), expect={"path": "bitmap", "nb": nb, "nch": _cdiv(nb, 4096), "trips": 1})


def bitmap_cases():
    """kd_delta_pk_order on the bitmap path (block-wide scans), small shapes"""
    out = []
    for nb, lo_block in ((1, 7), (15, -15), (16, -8), (17, -9), (4095, 100), (4096, -4096), (4097, -2048), (8193, 5)):
        out.append(_seam_case(f"nb{nb}", lo_block, nb, nb))
    # bounds loose by a whole empty chunk on both ends, the records in blocks -1, 0, 1
    lo, hi = 64 * (-1 - 4096), 64 * (2 + 4096) - 1
    out.append(Case("loose", lo, hi, _shuffled(pk_set(lo, hi, [-1, 0, 1], ["full", "bit0", "bit63"]), 3),
                    expect={"path": "bitmap", "nb": 8195, "nch": 3, "trips": 1}))
    # record orders (8 blocks, -3 .. 4)
    lo, hi = -192, 319
    allp = np.arange(lo, hi + 1, dtype=np.int64)
    e8 = {"path": "bitmap", "nb": 8, "nch": 1, "trips": 1}
    out.append(Case("asc", lo, hi, allp, expect=e8))
    out.append(Case("desc", lo, hi, allp[::-1].copy(), expect=e8))
    # blocks interleaved A A A B B A A A B B ...: block A gets two heads in one wave
    a, b = list(range(-64, 0)), list(range(128, 192))
    aba = []
    while len(aba) < 100:
        aba += [a.pop() for _ in range(3)] + [b.pop(0) for _ in range(2)]
    out.append(Case("aba", lo, hi, np.asarray(aba, np.int64), expect=e8))
    # a run of equal blocks across lanes 63 | 0: records 62 .. 66 share block 70, the rest one block each
    lo, hi = 0, 64 * 80 - 1
    seam = [64 * i + (i * 7) % 64 for i in range(62)] + [64 * 70 + j for j in (5, 63, 0, 31, 32)] + \
           [64 * i + 1 for i in (75, 72, 79, 62)]
    e80 = {"path": "bitmap", "nb": 80, "nch": 1, "trips": 1}
    out.append(Case("run_63_0", lo, hi, np.asarray(seam, np.int64), expect=e80))
    # a run of exactly 64 (one full block, scrambled), then another, then three strays
    run = np.concatenate([_shuffled(np.arange(64 * 9, 64 * 10), 1), _shuffled(np.arange(64 * 3, 64 * 4), 2),
                          np.asarray([0, 64 * 80 - 1, 64 * 9 - 1], np.int64)])
    out.append(Case("run_64", lo, hi, run, expect=e80))
    # counts around the wave and the block
    lo, hi = -64 * 9 + 63, 64 * 7
    pool = _shuffled(np.arange(lo, hi + 1), 17)
    for n in (1, 63, 64, 65, 255, 256, 257):
        out.append(Case(f"n{n}", lo, hi, pool[:n].copy(), expect={"path": "bitmap", "nb": 17, "nch": 1, "trips": 1}))
    # device counts: below the capacity with a poisoned tail, above it (clamps), zero
    lo, hi = -64 * 16, 64 * 17 - 1
    pool = _shuffled(np.arange(lo, hi + 1), 23)
    e33 = {"path": "bitmap", "nb": 33, "nch": 1, "trips": 1}
    out.append(Case("dn_below", lo, hi, pool[:300].copy(), tail=pool[300:800].copy(), expect=e33))
    out.append(Case("dn_above", lo, hi, pool[:300].copy(), over=1000, expect=e33))
    out.append(Case("dn_zero", lo, hi, pool[:0].copy(), tail=pool[:300].copy(), expect=e33))
    return out


def msgpack_case():
    """every msgpack width limit and its neighbours over [-2**31, 2**31 - 1]: 2**26 blocks, the largest
    bitmap range (16,384 chunks: two full trips of k_pkm_cscan)"""
    lo, hi = -2**31, 2**31 - 1
    p = set()
    for e in MSGPACK_EDGES:
        p |= {x for x in (e - 1, e, e + 1) if lo <= x <= hi}
    return Case("msgpack", lo, hi, _shuffled(sorted(p), 5),
                expect={"path": "bitmap", "nb": 1 << 26, "nch": 16384, "trips": 2})


def span31_case():
    """2**31 + 2**20 pks: 33,570,817 blocks, 8,197 chunks, so k_pkm_cscan takes a second trip; records
    in the first chunk, the 8,193rd (the second trip's first), the one before the last, and the last"""
    lo = -2**30
    hi = lo + 2**31 + 2**20
    rng = np.random.default_rng(31)
    lb = lo >> 6
    blocks = [lb, lb + 1, lb + 4095]
    for ch in (8191, 8192, 8195):
        blocks += [lb + ch * PKM_CH, lb + ch * PKM_CH + 17, lb + ch * PKM_CH + 4095]
    pks = np.union1d(pk_set(lo, hi, blocks, ["full", 0.4, "bit63", "bit0"], rng), np.asarray([lo, hi], np.int64))
    return Case("span31", lo, hi, _shuffled(pks, 31),
                expect={"path": "bitmap", "nb": 33_570_817, "nch": 8197, "trips": 2})


# ---- radix pk order (pkm_max_blocks = 0) -----------------------------------------------------------
def _range_of_bits(bits, base):
    """[lo, hi] whose plan is ``bits`` wide: ``base`` with its low ``bits`` bits cleared / set"""
    m = (1 << bits) - 1
    return base & ~m, (base & ~m) | m


def _random_pks(lo, hi, n, seed):
    """n unique pks of [lo, hi], lo and hi among them, in a random record order"""
    rng = np.random.default_rng(seed)
    span = hi - lo + 1
    if span <= 8 * n:
        off = rng.permutation(span).astype(np.uint64)
    else:  # offsets from lo as uint64 (a span of 2**64 included)
        off = np.zeros(0, np.uint64)
        while off.size < n:
            off = np.unique(np.concatenate([off, rng.integers(0, span, 2 * n, dtype=np.uint64)]))
        off = rng.permutation(off)
    off = off[(off != 0) & (off != np.uint64(span - 1))][:max(n - 2, 0)]
    off = np.concatenate([off, np.asarray([0, span - 1] if n >= 2 else [0], np.uint64)])
    pks = (off + np.asarray([lo & ((1 << 64) - 1)], np.uint64)).view(np.int64)  # (mod 2**64: lo + offset as int64)
    return np.ascontiguousarray(pks[rng.permutation(pks.size)])


def radix_cases():
    """kd_delta_pk_order with pkm_max_blocks = 0: every plan width class, the tile seams of both key
    types, a hot digit, device counts"""
    out = []

    def add(name, lo, hi, pks, stated, **kw):
        stated = dict(stated, path="radix")
        out.append(Case(name, lo, hi, np.asarray(pks, np.int64), expect=stated, **kw))

    one = {"bits": 0, "npass": 1, "width": 1, "ck": 32}
    for name, v in (("one", 77), ("one_min", I64_MIN), ("one_max", I64_MAX)):
        add(name, v, v, [v], one)
    add("w1", 4242, 4243, [4243, 4242], {"bits": 1, "npass": 1, "width": 1, "ck": 32})
    # (bits, base, n, passes, digit width): u32 keys, then u64 keys with 9-bit digits
    for bits, base, n, npass, width in ((9, 3 << 40, 512, 1, 9), (10, -(5 << 33), 1000, 2, 5), (18, 1 << 20, 8191, 2, 9),
                                        (19, -(1 << 50), 8192, 3, 7), (27, 7 << 32, 8193, 3, 9),
                                        (28, -(9 << 28), 2 * 8192 + 1, 4, 7), (32, 1 << 32, 8193, 4, 8),
                                        (33, 11 << 33, 4095, 4, 9), (36, -(1 << 60), 4096, 4, 9), (37, 1 << 37, 4097, 5, 8),
                                        (45, -(3 << 45), 4097, 5, 9), (46, 5 << 46, 4095, 6, 8), (63, 0, 4096, 7, 9)):
        lo, hi = _range_of_bits(bits, base)
        add(f"w{bits}", lo, hi, _random_pks(lo, hi, n, bits), {"bits": bits, "npass": npass, "width": width,
                                                                "ck": 32 if bits <= 32 else 64})
    w64 = {"bits": 64, "npass": 8, "width": 8, "ck": 64}
    add("w64_full", I64_MIN, I64_MAX, _random_pks(I64_MIN, I64_MAX, 4097, 64), w64)
    add("w64_cross", -5, 1000, _random_pks(-5, 1000, 700, 65), w64)  # a sign-crossing range: 64 bits however small
    # one hot digit: 27 bits = 3 digits of 9; every record but one holds the same middle digit, over 6
    # tiles and 5 records: the look-back of pass 1 walks RS_LBW words per round trip on that digit
    lo, hi = _range_of_bits(27, 1 << 40)
    rng = np.random.default_rng(27)
    n = 6 * TILE32 + 5
    cells = rng.permutation(512 * 512)[:n - 1]
    hot = lo + ((cells // 512) << 18) + (301 << 9) + (cells % 512)
    pks = np.concatenate([hot[:20000], [lo + (17 << 18) + (300 << 9) + 5], hot[20000:]]).astype(np.int64)
    add("hot_digit", lo, hi, pks, {"bits": 27, "npass": 3, "width": 9, "ck": 32})
    # the same on 64-bit keys: 36 bits = 4 digits of 9, digit 2 hot, 7 tiles of 4096
    lo, hi = _range_of_bits(36, -(1 << 44))
    n = 7 * TILE64 + 3
    cells = rng.permutation(np.unique(rng.integers(0, 1 << 27, 2 * n)))[:n - 1].astype(np.int64)
    hot = lo + ((cells >> 18) << 27) + (99 << 18) + (cells & ((1 << 18) - 1))
    pks = np.concatenate([hot[:9000], [lo + (100 << 18) + 1], hot[9000:]]).astype(np.int64)
    add("hot_digit64", lo, hi, pks, {"bits": 36, "npass": 4, "width": 9, "ck": 64})
    # device counts: below a capacity many tiles larger (poisoned tail), zero
    lo, hi = _range_of_bits(20, 1 << 30)
    pool = _random_pks(lo, hi, 5000 + 6 * TILE32, 20)
    e20 = {"bits": 20, "npass": 3, "width": 7, "ck": 32}
    add("dn_below", lo, hi, pool[:5000], e20, tail=pool[5000:].copy())
    add("dn_zero", lo, hi, pool[:0], e20, tail=pool[:3 * TILE32].copy())
    lo, hi = _range_of_bits(40, 1 << 41)
    pool = _random_pks(lo, hi, 3000 + 6 * TILE64, 40)
    add("dn_below64", lo, hi, pool[:3000], {"bits": 40, "npass": 5, "width": 8, "ck": 64}, tail=pool[3000:].copy())
    return out


def radix_tiles(case):
    """tiles of the capacity and of the count, at the case's key type"""
    tile = TILE32 if radix_geometry(case.lo, case.hi)["ck"] == 32 else TILE64
    return _cdiv(case.cap, tile), _cdiv(case.n, tile)


# ---- two crafted sides for kd_diff2_step ---------------------------------------------------------
@dataclass
class StepCase:
    name: str
    lo: int
    hi: int
    pks: np.ndarray     # ascending
    kinds: np.ndarray   # INSERT / DELETE / UPDATE / SAME per pk
    expect: dict = field(default_factory=dict)


@dataclass
class StepSides:
    key_a: np.ndarray
    oid_a: np.ndarray
    pk_a: np.ndarray
    key_b: np.ndarray
    oid_b: np.ndarray
    pk_b: np.ndarray
    counts: dict


def materialise_step(case):
    """base and target sides (keys ascending, 20-byte OIDs): a DELETE is in the base only, an INSERT in
    the target only, an UPDATE in both with different OIDs, SAME in both with equal OIDs"""
    rng = np.random.default_rng(len(case.name) + case.pks.size)
    pks, kinds = np.asarray(case.pks, np.int64), np.asarray(case.kinds)
    oid = rng.integers(0, 256, (pks.size, 20), dtype=np.uint8)
    oid2 = oid.copy()
    oid2[kinds == UPDATE, 7] ^= 0x5A
    sel_a, sel_b = kinds != INSERT, kinds != DELETE
    keys = walkkey.int_keys(pks)
    oa, ob = np.argsort(keys[sel_a], kind="stable"), np.argsort(keys[sel_b], kind="stable")
    counts = {"inserts": int((kinds == INSERT).sum()), "deletes": int((kinds == DELETE).sum()),
              "updates": int((kinds == UPDATE).sum())}
    return StepSides(np.ascontiguousarray(keys[sel_a][oa]), np.ascontiguousarray(oid[sel_a][oa]), pks[sel_a][oa],
                     np.ascontiguousarray(keys[sel_b][ob]), np.ascontiguousarray(oid2[sel_b][ob]), pks[sel_b][ob], counts)


def check_step(case, s):
    assert np.unique(case.pks).size == case.pks.size and case.pks.min() >= case.lo and case.pks.max() <= case.hi
    for keys, spk in ((s.key_a, s.pk_a), (s.key_b, s.pk_b)):
        assert np.all(keys[1:] > keys[:-1]) and np.array_equal(walkkey.int_keys(spk), keys)
    assert min(s.counts.values()) > 0 and (np.asarray(case.kinds) == SAME).any()


def _step_case(name, lo_block, nb, chunks, stated, seed):
    """pks at the seams of the one-wave chunks: the first and last blocks of ``chunks`` (each with its
    thread seams), bounds exact"""
    rng = np.random.default_rng(seed)
    lo, hi = 64 * lo_block + 63, 64 * (lo_block + nb - 1)
    rel = set(seam_blocks(nb))
    for ch in chunks:
        for r in (0, 1, 15, 16, 17, 511, 1007, 1008, 1022, 1023):
            rel.add(ch * PKM_CHW + r)
    rel = sorted(r for r in rel if 0 <= r < nb)
    pks = pk_set(lo, hi, [lo_block + r for r in rel], ["full", "bit0", 0.3, "bit63", 0.6], rng)
    pks = np.union1d(pks, np.asarray([lo, hi], np.int64))
    kinds = rng.integers(0, 4, pks.size)
    kinds[:4] = (INSERT, DELETE, UPDATE, SAME)
    return StepCase(name, lo, hi, pks, kinds, expect=dict(stated, path="bitmap_wave"))


def step_cases():
    """kd_diff2_step with pkm_wave = 1: one-wave chunks of 1024 masks, four waves per scan block"""
    out = []
    for nb, nch in ((1023, 1), (1024, 1), (1025, 2), (3072, 3), (3073, 4), (4097, 5)):
        out.append(_step_case(f"nb{nb}", -(nb // 2), nb, range(nch), {"nb": nb, "nch": nch, "trips": 1}, nb))
    # 2**27 + 2**17 pks: 2,099,201 blocks, 2,051 chunks: k_pkm_cscan_w takes a second trip
    lo = -2**20
    nb = (2**27 + 2**17) // 64 + 1
    c = _step_case("span27", lo >> 6, nb, (0, 1, 2046, 2047, 2048, 2049, 2050), {"nb": nb, "nch": 2051, "trips": 2}, 27)
    out.append(c)
    return out


# ---- side sorts -------------------------------------------------------------------------------------
def stable_reference(keys):
    """(order, sorted keys) of a side sort: np.argsort(kind="stable")"""
    order = np.argsort(keys, kind="stable")
    return order.astype(np.uint32), keys[order]


def sort_plan(keys):
    """(vary mask, compact width, passes) of a side sort of these keys, gaps between more than
    RS_MAXRUNS runs of varying bits not counted (the crafted keys have at most RS_MAXRUNS)"""
    keys = np.asarray(keys, np.uint64)
    vary = int(np.bitwise_or.reduce(keys ^ keys[0]))
    runs = len([r for r in bin(vary)[2:].split("0") if r])
    assert runs <= RS_MAXRUNS
    bits = bin(vary).count("1")
    return vary, bits, _cdiv(bits, RS_RB)


def dup_cases():
    """duplicate keys that do take passes: name -> uint64 keys"""
    rng = np.random.default_rng(4)
    out = {}
    out["two_values"] = rng.permutation(np.repeat(np.asarray([5, 4], np.uint64), 10_000))          # 1 bit, 1 pass
    out["513_values"] = rng.permutation(np.repeat(np.arange(513, dtype=np.uint64) << np.uint64(20), 20))  # 10 bits
    d = rng.permutation(1 << 16)[:9000].astype(np.uint64)
    out["doubled_adjacent"] = np.repeat(d, 2)
    out["doubled_far"] = np.concatenate([d, d])
    wide = rng.integers(0, 1 << 63, 6000, dtype=np.uint64)                                         # 64-bit compact keys
    out["doubled_wide"] = np.concatenate([wide, wide[::-1]])
    # copies of one key in different lanes, waves and tiles (tile of 8192: 17 varying bits)
    k = (rng.permutation(1 << 17)[:3 * TILE32 + 7].astype(np.uint64)) << np.uint64(3)
    for pos in (0, 1, 63, 64, 65, 700, TILE32 - 1, TILE32, TILE32 + 64, 2 * TILE32 + 5, k.size - 1):
        k[pos] = k[40]
    out["copies_lanes_waves_tiles"] = k
    return {n: np.ascontiguousarray(v, np.uint64) for n, v in out.items()}


# ---- mask bookkeeping: a sequence of calls on one context ---------------------------------------
def book_cases():
    """[(form, case)]: bitmap calls of a large range, a small one, a larger one (both mask buffers
    regrow) and the same again, then a radix call and a wave-form step between further bitmap calls.
    Every range starts at block 0 and call k holds only pks = k (mod 11), so the calls' pk sets are
    disjoint and a bit left over from an earlier call lies below or between this call's bits."""
    forms = (("bitmap", 20_000), ("bitmap", 100), ("bitmap", 50_000), ("bitmap", 50_000), ("radix", 20_000),
             ("bitmap", 20_000), ("step", 3073), ("bitmap", 100), ("bitmap", 50_000))
    out = []
    for k, (form, nb) in enumerate(forms):
        lo, hi = 0, 64 * nb - 1
        blocks = sorted(set(range(min(nb, 100))) | set(seam_blocks(nb)))
        pks = pk_set(lo, hi, blocks, "full")
        pks = pks[pks % 11 == k]
        if form == "step":
            kinds = np.arange(pks.size) % 4
            out.append((form, StepCase(f"book{k}", lo, hi, pks, kinds, expect={"path": "bitmap_wave", "nb": nb,
                                                                               "nch": _cdiv(nb, PKM_CHW), "trips": 1})))
        elif form == "radix":
            out.append((form, Case(f"book{k}", lo, hi, _shuffled(pks, k), expect=dict(radix_geometry(lo, hi), path="radix"))))
        else:
            out.append((form, Case(f"book{k}", lo, hi, _shuffled(pks, k), expect={"path": "bitmap", "nb": nb,
                                                                              "nch": _cdiv(nb, PKM_CH), "trips": 1})))
    return out
