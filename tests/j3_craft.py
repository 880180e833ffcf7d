"""Crafted three-way merges for k_join3b / k_apart3b / k_partition2<384> (kd_classify2.hip), and a
host model of the join's tile geometry written from the kernels' definitions (never by calling
them): which ancestor range a tile gets, which name rows and chunks it stages, where k_apart3b's
guess lands.  tests/test_join3_seams.py builds inputs with these, asserts on the CPU that each
lands on the seam it is meant for, and holds the GPU to the oracle on them.  CPU only, except
perm_side(), which uploads."""
import os
import re
from types import SimpleNamespace

import numpy as np

from kart_amd import _native as N

# the join's compile-time shape (kd_classify2.hip; read_defaults() parses the source's own values)
TILE, NT, ACAP, HALO, NAME_CH = 384, 192, 320, 8, 1000
GROUP = 64  # tiles per group sum of the placement (C2_GROUP)
APART_STEP, APART_PROBES = 256, 8  # k_apart3b: lb_guided<8>(..., 256)
NONE = 0xFFFFFFFF
KMAX = np.uint64(0xFFFFFFFFFFFFFFFF)
SEGMENTS = (8, 9, 10, 17, 64)  # reversed runs of a displaced order: rows move 7, 8, 9, 16 and 63

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kart_amd", "csrc")


def _c_int(expr, names):
    """a #define's integer expression (names, + - * /, one `a == b ? x : y`) evaluated as C would"""
    expr = expr.split("//")[0].strip()
    m = re.fullmatch(r"\((.+?)\?(.+?):(.+)\)", expr)
    if m:
        expr = "(%s) if (%s) else (%s)" % (m.group(2), m.group(1), m.group(3))
    assert re.fullmatch(r"[\w\s()+\-*/=<>]+", expr), expr
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(names)))


def read_defaults():
    """the defaults kd_classify2.hip declares for the constants above"""
    text = open(os.path.join(_CSRC, "kd_classify2.hip")).read()

    def define(name, names):
        (v,) = re.findall(r"^#ifndef %s\n#define %s[ \t]+(.+)$" % (name, name), text, re.M)
        return _c_int(v, names)

    ipt, nt = define("KD_J3B_IPT", {}), define("KD_J3B_NT", {})
    names = {"J3B_TILE": ipt * nt, "J3B_NT": nt, "J3B_IPT": ipt}
    (group,) = re.findall(r"^constexpr u64 C2_GROUP = (\d+);", text, re.M)
    (guided,) = re.findall(r"\blb_guided<(\d+)>\([^;]*?,\s*(\d+)\);", text)
    return dict(TILE=ipt * nt, NT=nt, ACAP=define("KD_J3B_ACAP", names), HALO=define("KD_J3B_HALO", names),
                NAME_CH=define("KD_J3B_NAME_CH", names), GROUP=int(group), APART_STEP=int(guided[1]),
                APART_PROBES=int(guided[0]))


def makefile_flags():
    """the default compiler flags of kart_amd/csrc/Makefile (FLAGS with its continuation lines)"""
    text = open(os.path.join(_CSRC, "Makefile")).read()
    return re.search(r"^FLAGS\s*=((?:.*\\\n)*.*)$", text, re.M).group(1)


# ---------------------------------------------------------------------------------------------
# sides
# ---------------------------------------------------------------------------------------------
def oids(keys, ver):
    """20-byte OIDs from the keys; a version v > 0 flips bits of byte key % 20, so two versions of a
    path differ in one byte and over the paths in every dword"""
    k = np.asarray(keys, np.uint64)
    x = k[:, None] * np.uint64(0x9E3779B97F4A7C15) + (np.arange(20, dtype=np.uint64) * np.uint64(0xBF58476D1CE4E5B9))[None, :]
    o = ((x >> np.uint64(29)) & np.uint64(0xFF)).astype(np.uint8)
    o[np.arange(k.size), (k % np.uint64(20)).astype(np.int64)] ^= np.asarray(ver, np.int64).astype(np.uint8)
    return o


def arena(names):
    off = np.zeros(len(names) + 1, np.uint64)
    if names:
        off[1:] = np.cumsum([len(b) for b in names])
    return np.frombuffer(b"".join(names), np.uint8).copy(), off


def int_side(keys, oid):
    from kart_amd import packing

    keys = np.ascontiguousarray(keys, np.uint64)
    return packing.PackedSide(keys, np.ascontiguousarray(oid, np.uint8).reshape(-1, 20), N.KD_KEY_INT, np.arange(keys.size))


def hash_side(keys, oid, names):
    """a KD_KEY_HASH side in sorted form from explicit keys, OIDs and filenames (list of bytes)"""
    from kart_amd import packing

    keys = np.ascontiguousarray(keys, np.uint64)
    data, off = arena(list(names))
    return packing.PackedSide(keys, np.ascontiguousarray(oid, np.uint8).reshape(-1, 20), N.KD_KEY_HASH,
                              np.arange(keys.size), data, off)


# what each kind of path holds on (ancestor, ours, theirs): -1 absent, else the OID's version
KINDS = {"same": (0, 0, 0), "omod": (0, 1, 0), "tmod": (0, 0, 1), "conf": (0, 1, 2), "bothmod": (0, 1, 1),
         "addadd": (-1, 1, 1), "addconf": (-1, 1, 2), "oadd": (-1, 1, -1), "tadd": (-1, -1, 1),
         "odel": (0, -1, 0), "tdel": (0, 0, -1), "odel_tmod": (0, -1, 1), "omod_tdel": (0, 1, -1),
         "bothdel": (0, -1, -1)}


class Case:
    """one merge: ascending union keys, per path the OID version each side holds (-1: absent) and
    the filename's length.  The sides come out in sorted form, with int keys or as KD_KEY_HASH sides
    (the same keys, with the filenames)."""

    def __init__(self, key, va, vo, vt, lens=8, seed=1):
        key = np.asarray(key, np.uint64)
        assert key.size == 0 or (key[1:] > key[:-1]).all()
        self.key = key
        self.v = [np.asarray(v, np.int64) for v in (va, vo, vt)]
        self.lens = np.broadcast_to(np.asarray(lens, np.int64), key.shape).copy()
        off = np.concatenate([[0], np.cumsum(self.lens)])
        blob = np.random.default_rng(seed).integers(0, 256, int(off[-1]), dtype=np.uint8).tobytes()
        self.idx = [np.flatnonzero(v >= 0) for v in self.v]
        self.k = [key[i].copy() for i in self.idx]
        self.oid = [oids(key[i], v[i]) for i, v in zip(self.idx, self.v)]
        self.names = [[blob[off[u]:off[u + 1]] for u in i.tolist()] for i in self.idx]

    @classmethod
    def of_kinds(cls, key, kinds, **kw):
        v = np.array([KINDS[k] for k in kinds], np.int64).reshape(-1, 3)
        return cls(key, v[:, 0], v[:, 1], v[:, 2], **kw)

    def side(self, s, hashed):
        return hash_side(self.k[s], self.oid[s], self.names[s]) if hashed else int_side(self.k[s], self.oid[s])

    def sides(self, hashed):
        return [self.side(s, hashed) for s in range(3)]

    def flat(self):
        """(kK, oK, kO, oO, kT, oT): the oracle's arguments"""
        return [x for s in range(3) for x in (self.k[s], self.oid[s])]

    def offs(self, order=None):
        """name offsets of the three sides as the kernel reads them: sorted form, or (order: one per
        side) the walk-order arenas of the late-materialised form"""
        out = []
        for s in range(3):
            ln = np.array([len(b) for b in self.names[s]], np.int64)
            if order is not None:
                ln = ln[inverse(order[s])]
            out.append(np.concatenate([[0], np.cumsum(ln)]).astype(np.int64))
        return out


def inverse(order):
    inv = np.empty(len(order), np.int64)
    inv[np.asarray(order, np.int64)] = np.arange(len(order))
    return inv


def displaced(n, segments=()):
    """the identity order, except that each (start, length) segment is reversed (clipped to [0, n))"""
    order = np.arange(n, dtype=np.int64)
    for s, ln in segments:
        a, b = max(int(s), 0), min(int(s) + int(ln), n)
        if b > a:
            assert (order[a:b] == np.arange(a, b)).all(), "segments overlap"
            order[a:b] = order[a:b][::-1].copy()
    return order


def default_displaced(n, phase=0):
    """reversed segments of every length of SEGMENTS, spread over the side"""
    segs, s, k = [], 5 + phase, phase
    while s < n:
        segs.append((s, SEGMENTS[k % len(SEGMENTS)]))
        s += SEGMENTS[k % len(SEGMENTS)] + 61
        k += 1
    return displaced(n, segs)


def perm_side(engine, side, order):
    """the late-materialised form of a sorted side: keys stay sorted; OIDs, names and name offsets in
    walk order, order[x] = the walk row of sorted entry x (uploaded as uint32); engine.merge3 then
    takes kd_merge3_device_perm"""
    from kart_amd import packing
    from kart_amd.device import DevBuf, DevPermSide, _WalkSide

    order = np.asarray(order, np.int64)
    assert np.array_equal(np.sort(order), np.arange(side.n))
    w = _WalkSide(side, inverse(order))  # walk row r holds sorted entry inverse[r]
    up = lambda a, dt, width=1: DevBuf.from_numpy(engine, a if a is not None and a.size else np.zeros(width, dt))
    name = name_off = None
    if side.name is not None:
        name, name_off = up(w.name, np.uint8), up(w.name_off, np.uint64)
    dp = DevPermSide(engine, side.n, side.key_mode, up(side.key, np.uint64), up(w.oid.reshape(-1), np.uint8, 20),
                     up(order.astype(np.uint32), np.uint32), name, name_off)
    return packing.PackedSide(side.key, w.oid, side.key_mode, order, w.name, w.name_off, dperm=dp)


# ---------------------------------------------------------------------------------------------
# host model of the tile geometry
# ---------------------------------------------------------------------------------------------
def split_by_definition(ka, kb, d):
    """the merge-path split of diagonal d (ties: A first): the smallest i in [lo, hi] with i == hi or
    A[i] > B[d - 1 - i]; and whether the predicate is monotone there (any search finds that split)"""
    lo, hi = max(d - len(kb), 0), min(d, len(ka))
    p = np.array([ka[i] > kb[d - 1 - i] for i in range(lo, hi)] + [True])
    return lo + int(np.argmax(p)), bool((np.diff(p.astype(int)) >= 0).all())


def chunks(a, b):
    """16-byte chunks that stage arena bytes [a, b) (the arena itself is 16-byte aligned)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where(b > a, ((a & 15) + (b - a) + 15) // 16, 0)


def geometry(kK, kO, kT, perm=False, offO=None, offT=None):
    """per tile t of the ours/theirs union (TILE items): the split (i, j) of diagonal min(TILE t, nO + nT),
    apart[t] = lower bound in K of min(O[i_t], T[j_t]) (0 and nK at the ends), the ancestor range
    [k0, k1e) with its one-key lookahead, nk, whether it is staged (lk), the staged name rows
    [rA0, rA1) / [rB0, rB1), their chunks and whether they fit (lnames; with offsets), and
    k_apart3b's guess"""
    kK, kO, kT = (np.asarray(k, np.uint64) for k in (kK, kO, kT))
    nK, nO, nT = kK.size, kO.size, kT.size
    total = nO + nT
    nt = (total + TILE - 1) // TILE
    side = np.concatenate([np.zeros(nO, np.int64), np.ones(nT, np.int64)])
    merged = np.lexsort((side, np.concatenate([kO, kT])))
    cum = np.concatenate([[0], np.cumsum(side[merged] == 0)]).astype(np.int64)
    d = np.minimum(TILE * np.arange(nt + 1, dtype=np.int64), total)
    i = cum[d]
    j = d - i
    a = np.where(i < nO, np.concatenate([kO, [KMAX]])[np.minimum(i, nO)], KMAX)
    b = np.where(j < nT, np.concatenate([kT, [KMAX]])[np.minimum(j, nT)], KMAX)
    first = np.minimum(a, b)
    apart = np.searchsorted(kK, first, "left").astype(np.int64)
    if nt:
        apart[0], apart[-1] = 0, nK
    with np.errstate(all="ignore"):
        guess = (i.astype(np.float64) / nO * nK) if nO else (d.astype(np.float64) / max(total, 1) * nK)
    guess = np.minimum(np.nan_to_num(guess).astype(np.int64), nK)
    g = SimpleNamespace(nt=nt, d=d, i=i, j=j, first=first, apart=apart, guess=guess)
    g.i0, g.i1, g.j0, g.j1 = i[:-1], i[1:], j[:-1], j[1:]
    g.k0, g.k1 = apart[:-1], apart[1:]
    g.k1e = g.k1 + (g.k1 < nK)
    g.nk = g.k1e - g.k0
    g.lk = g.nk <= ACAP
    H = HALO if perm else 0
    g.rA0, g.rA1 = np.maximum(g.i0 - H, 0), np.minimum(g.i1 + H, nO)
    g.rB0, g.rB1 = np.maximum(g.j0 - H, 0), np.minimum(g.j1 + 1 + H, nT)
    if offO is not None:
        g.chA = chunks(np.asarray(offO)[g.rA0], np.asarray(offO)[g.rA1])
        g.chB = chunks(np.asarray(offT)[g.rB0], np.asarray(offT)[g.rB1])
        g.ch = g.chA + g.chB
        g.lnames = g.ch <= NAME_CH
    return g


def case_geometry(case, perm=False, order=None):
    _, offO, offT = case.offs(order if perm else None)
    return geometry(case.k[0], case.k[1], case.k[2], perm, offO, offT)


def paths(case):
    """every path of the ours/theirs union in key order: its sorted index on each side (-1: absent),
    the tile that walks it (the tile of its first item; a pair's theirs entry may be the next tile's
    first, where the lookbehind key drops it), whether it is a matched pair and whether it differs"""
    kK, kO, kT = case.k
    U = np.union1d(kO, kT)

    def find(k):
        x = np.minimum(np.searchsorted(k, U), max(k.size - 1, 0))
        return np.where(k[x] == U, x, -1) if k.size else np.full(U.size, -1, np.int64)

    p = SimpleNamespace(key=U, ia=find(kK), io=find(kO), it=find(kT))
    p.tile = (np.searchsorted(kO, U) + np.searchsorted(kT, U)) // TILE
    p.matched = (p.io >= 0) & (p.it >= 0)
    eq = (case.oid[1][np.maximum(p.io, 0)] == case.oid[2][np.maximum(p.it, 0)]).all(axis=1)
    p.differ = ~(p.matched & eq)
    return p


def classify3(kK, oK, kO, oO, kT, oT):
    """libgit2's per-path rule over dicts: o == t -> ours; a == o -> theirs (a merge delta);
    a == t -> ours; else conflict.  The clean count is oracle/kd_oracle.c's: a path resolved to a
    side counts when that side holds it.  -> (conflicts [n, 3], merge deltas [m, 2], n_clean)"""
    sides = []
    for k, o in ((kK, oK), (kO, oO), (kT, oT)):
        raw = np.ascontiguousarray(o, np.uint8).tobytes()
        sides.append({int(key): (x, raw[20 * x:20 * x + 20]) for x, key in enumerate(np.asarray(k).tolist())})
    A, O, T = sides
    conf, md, clean = [], [], 0
    for key in sorted(set(A) | set(O) | set(T)):
        (xa, a), (xo, o), (xt, t) = (s.get(key, (NONE, None)) for s in (A, O, T))
        if o == t:
            clean += o is not None
        elif a == o:
            clean += t is not None
            md.append((xo, xt))
        elif a == t:
            clean += o is not None
        else:
            conf.append((xa, xo, xt))
    return (np.array(conf, np.uint32).reshape(-1, 3), np.array(md, np.uint32).reshape(-1, 2), int(clean))
