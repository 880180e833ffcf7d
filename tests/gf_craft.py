"""Hand-built inputs for the geometry filter (kd_geomfilter.hip): feature blobs laid out at chosen
arena positions around ``decode_side``'s 112-byte register window, GPKG headers and envelopes at
every decision edge, legend tables at their limits, malformed blobs, and delta lists around the
tile, wave and scan seams.

A crafted *set* is a list of calls (``Call``): the two arenas, the per-side legend tables and
geometry indices, the pairs, the filter and the rect flag of one kd_geom_filter invocation, with the
oracle's answer (``O.geom_filter``) cached per index-envelope width.  Nothing reads a fixture; every
set is generated, deterministic and small, and built once per process.
"""
import ctypes
import functools
import hashlib
import math
import struct

import numpy as np

import fd_craft as F
from kart_amd import _native as N
from kart_amd import spatial as S
from oracle import oracle as O

NONE = O.NONE
NIL = b"\xc0"
G = ord("G")
TILE = 4096  # GF_TILE: deltas per workgroup (16 rounds of 256)
SPT_TILES = 8192  # k_gf_scan: tiles per pass (1024 threads x GF_SPT 8)


def hexof(tag):
    return hashlib.sha1(str(tag).encode()).hexdigest()


H0, H2, HN, HU = hexof("geom first"), hexof("geom third"), hexof("no geom"), hexof("unknown")
TAB = [(H0, 0), (H2, 2), (HN, -1)]  # the usual table: (legend hex, geometry value index)


# ------------------------------------------------------------------------------------------
# GPKG values


def _d(v, le=True):
    return struct.pack("<d" if le else ">d", v)


def gpkg(flags, env=(), wkb=b"", magic=b"GP", version=0, srs=4326):
    """a StandardGeoPackageBinary value: header, envelope doubles in the header's byte order, WKB"""
    le = bool(flags & 1)
    return (magic + bytes([version, flags]) + struct.pack("<i" if le else ">i", srs) +
            b"".join(_d(v, le) for v in env) + wkb)


def wkb_point(x, y, typ=1, bo=1):
    """bo: the WKB byte-order byte (1 little endian; 0 and any other value big endian)"""
    le = bo == 1
    return bytes([bo]) + struct.pack("<I" if le else ">I", typ) + _d(x, le) + _d(y, le)


def wkb_poly(x0, x1, y0, y1):
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    return struct.pack("<BIII", 1, 3, 1, len(pts)) + b"".join(_d(x) + _d(y) for x, y in pts)


def point(x, y, flags=0x01, **kw):
    return gpkg(flags, (), wkb_point(x, y, **kw))


def poly(x0, x1, y0, y1, flags=0x03):
    return gpkg(flags, (x0, x1, y0, y1), wkb_poly(x0, x1, y0, y1))


# ------------------------------------------------------------------------------------------
# feature blobs


def ext(payload, form, code=G):
    return F.ext_forms(code, payload)[form]


def feature(hexs, values, vh="fix", count=None, legend_form="s8", top=b"\x92"):
    """top-level header, legend header + hex, values header (fix / a16 / a32), encoded values"""
    n = len(values) if count is None else count
    return top + F.legend_header(hexs, legend_form) + F.array_header(n, vh) + b"".join(values)


def placed(g, gi, vh="fix", form="e8", pad=30):
    """a feature whose geometry value ``g`` (encoded ext, or NIL) is value ``gi`` of 3 (gi -1: a
    legend without a geometry column)"""
    tail = F.str_forms(b"s" * pad)["s8" if pad > 31 else "fix"]
    if gi == 0:
        return feature(H0, [g, b"\x01", tail], vh)
    if gi == 2:
        return feature(H2, [b"\xcb" + struct.pack(">d", 1.5), F.str_forms(b"t" * 5)["fix"], g], vh)
    return feature(HN, [b"\x01", tail], vh)


def filler(length):
    """a well-formed blob (legend without a geometry column) of exactly ``length`` bytes, 45..75"""
    assert 45 <= length <= 75, length
    return F.blob(HN, [F.s_total(length - 44)])


def arena(blobs):
    return F.arena(list(blobs))


# ------------------------------------------------------------------------------------------
# one call and its oracle


def cols_of(tab):
    """GeomCols-shaped arrays of one side's table, in the table's own order"""
    hx = np.frombuffer("".join(h for h, _ in tab).encode(), np.uint8).copy() if tab else np.zeros(40, np.uint8)
    gi = np.array([g for _, g in tab] or [0], np.int16)
    return hx, gi, dict(tab)


class Call:
    """one kd_geom_filter invocation over crafted arenas.

    ``hand``: {(row, side): code} for sides the oracle cannot take (indices past the arena): the
    oracle is given NONE there and the code is stated by hand.  ``notes[row]`` names the row."""

    def __init__(self, name, old_blobs, new_blobs, pairs, filt, rect, old_tab=TAB, new_tab=TAB, notes=None, hand=None):
        self.name = name
        self.blobs = (list(old_blobs), list(new_blobs))
        self.arenas = (arena(old_blobs), arena(new_blobs))
        self.pairs = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))
        self.n = self.pairs.shape[0]
        self.filt, self.rect = tuple(float(x) for x in filt), bool(rect)
        self.tabs = (list(old_tab), list(new_tab))
        self.hand = dict(hand or {})
        self.notes = notes
        self._oracle = {}
        self._heads = None

    def geom_cols(self):
        gc = S.GeomCols.__new__(S.GeomCols)
        gc.old_hex, gc.old_gidx, gc.old_map = cols_of(self.tabs[0])
        gc.new_hex, gc.new_gidx, gc.new_map = cols_of(self.tabs[1])
        return gc

    def oracle_pairs(self):
        p = self.pairs.copy()
        for (row, side) in self.hand:
            p[row, side] = NONE
        return p

    def _with_hand(self, res):
        codes, _, enc, ok = res
        codes = codes.copy()
        for (row, side), c in self.hand.items():
            codes[row, side] = c
        keep = np.nonzero(((codes >= 1) & (codes <= 3)).any(axis=1))[0].astype(np.uint32)
        return codes, keep, enc, ok

    def oracle(self, bits=20, py=False):
        """(codes, keep, enc, ok) — O.geom_filter (or its Python restatement), hand codes applied"""
        key = (bits or 20, py)
        if key not in self._oracle:
            (od, oo), (nd, no) = self.arenas
            fn = O.geom_filter_py if py else O.geom_filter
            self._oracle[key] = self._with_hand(fn(od, oo, nd, no, self.oracle_pairs(), dict(self.tabs[0]),
                                                   dict(self.tabs[1]), self.filt, self.rect, bits or 20))
        return self._oracle[key]

    def heads(self):
        """kd_geom_heads of both arenas under their own tables"""
        if self._heads is None:
            self._heads = []
            for (d, o), tab in zip(self.arenas, self.tabs):
                hx, gi, m = cols_of(tab)
                self._heads.append(S.geom_heads(d, o, hx, gi, len(m)))
        return self._heads

    def geometry(self, side, bi):
        """(status, GPKG bytes | None) of a blob, as the oracle reads it"""
        return O.feature_geometry(self.blobs[side][bi], dict(self.tabs[side]))

    def needs_blob(self):
        """[n, 2] bool: the sides whose geometry a 48-byte head cannot decide (the byte-wise decode
        on the blob: an XYZ / XYM / XYZM envelope, or an XY envelope holding a NaN)"""
        out = np.zeros((self.n, 2), bool)
        memo = ({}, {})
        for d in range(self.n):
            for s in range(2):
                bi = int(self.pairs[d, s])
                if bi == NONE or (d, s) in self.hand:
                    continue
                if bi not in memo[s]:
                    st, g = self.geometry(s, bi)
                    memo[s][bi] = bool(st == 0 and g is not None and head_needs_blob(g))
                out[d, s] = memo[s][bi]
        return out

    def residue(self, row, side):
        bi = int(self.pairs[row, side])
        off = self.arenas[side][1]
        return int(off[bi]) % 16 if bi != NONE and bi + 1 < off.shape[0] else -1

    def describe(self, row):
        note = self.notes[row] if self.notes is not None else ""
        return f"{self.name} row {row} [{note}] residues {self.residue(row, 0)}/{self.residue(row, 1)}"


def head_needs_blob(g):
    if len(g) < 8 or g[:3] != b"GP\x00" or g[3] & 0x30:
        return False
    et = (g[3] >> 1) & 7
    if et > 1:
        return True
    if et == 1 and len(g) >= 40:
        fmt = "<4d" if g[3] & 1 else ">4d"
        return any(math.isnan(v) for v in struct.unpack(fmt, g[8:40]))
    return False


def both_sides(n_old, n_new=None):
    """pairs (i, i), (i, NONE), (NONE, i) over two arenas with as many blobs"""
    n_new = n_old if n_new is None else n_new
    n = min(n_old, n_new)
    i = np.arange(n, dtype=np.uint32)
    none = np.full(n, NONE, np.uint32)
    return np.concatenate([np.stack([i, i], 1), np.stack([i, none], 1), np.stack([none, i], 1)])


# ------------------------------------------------------------------------------------------
# window: the register window of decode_side at every start residue

W_FILT = (0.0, 10.0, 0.0, 10.0)
PT_IN, PT_OUT = point(5.0, 5.0), point(50.0, 5.0)
assert len(PT_IN) == 29
ENV40 = gpkg(0x03, (2.0, 12.0, 2.0, 8.0))  # a stored XY envelope and nothing after it: 40 bytes
EMPTY8 = gpkg(0x11)
PAYLOADS = [("pt29", PT_IN), ("pt28", PT_IN[:28]), ("pt13", PT_IN[:13]), ("pt12", PT_IN[:12]), ("env40", ENV40),
            ("env39", ENV40[:39]), ("empty8", EMPTY8), ("empty7", EMPTY8[:7]), ("poly", poly(2.0, 4.0, 2.0, 4.0)),
            ("polyout", poly(20.0, 30.0, 2.0, 4.0)), ("ptbe", point(5.0, 5.0, flags=0x00, bo=0)),
            ("xyz", gpkg(0x05, (1.0, 2.0, 1.0, 2.0, 0.0, 9.0), wkb_poly(1.0, 2.0, 1.0, 2.0)))]
FIXEXT = [("fx1", b"G"), ("fx2", b"GP"), ("fx4", b"GP\x00\x10"), ("fx8", EMPTY8), ("fx16", PT_IN[:16])]


def window_layouts():
    """(note, blob): every blob shape the fast path distinguishes"""
    L = []
    for vh in ("fix", "a16"):
        for form in ("e8", "e16", "e32"):  # q = 47, 48, 50 (fixarray) and 49, 50, 52 (array16)
            for pn, p in PAYLOADS:
                L.append((f"{vh}/{form}/{pn}", placed(ext(p, form), 0, vh)))
        for pn, p in FIXEXT:
            L.append((f"{vh}/fixext/{pn}", placed(ext(p, "fix"), 0, vh)))
        L.append((f"{vh}/later", placed(ext(PT_IN, "e8"), 2, vh)))
        L.append((f"{vh}/later-out", placed(ext(PT_OUT, "e16"), 2, vh)))
        L.append((f"{vh}/nested-array", feature(H2, [b"\x92\x01\x92\x02\x03", F.str_forms(b"x")["fix"],
                                                      ext(PT_IN, "e8")], vh)))
        L.append((f"{vh}/nested-map", feature(H2, [b"\x81\xa1k\x91\xc0", b"\x07", ext(PT_OUT, "e8")], vh)))
        L.append((f"{vh}/null", placed(NIL, 0, vh)))
        L.append((f"{vh}/null-later", placed(NIL, 2, vh)))
        L.append((f"{vh}/nogeom", placed(None, -1, vh)))
        L.append((f"{vh}/unknown", feature(HU, [ext(PT_IN, "e8"), b"\x01"], vh)))
    # array16 counts whose low byte reads as a nil (0xc0) or an ext8 header (0xc7): the value byte is
    # byte 46, not the count's byte 45
    for cnt in (0xc0, 0xc7):
        L.append((f"a16/count{cnt:#x}", feature(H0, [ext(PT_OUT, "e8")] + [b"\x01"] * (cnt - 1), "a16")))
    # blob lengths 51, 52, 53 (the fast path needs 52): a null geometry, and a short ext, before padding
    for ln in (51, 52, 53):
        L.append((f"len{ln}/null", F.blob(H0, [NIL, F.s_total(ln - 45)])))
        L.append((f"len{ln}/ext", F.blob(H0, [ext(b"GP\x00\x01" + b"\x00" * (ln - 51), "e8")])))
        assert len(L[-1][1]) == ln and len(L[-2][1]) == ln
    return L


def lay_out(layouts, rot=0):
    """each layout at every start residue 0..15, filler blobs between: (blobs, notes, rows of the
    layouts' blobs).  Residues are those of the arena offsets: device arenas start 256-B aligned."""
    blobs, notes, rows = [], [], []
    pos = 0
    for note, b in layouts:
        starts = []
        for k in range(16):
            r = (k + rot) % 16
            pad = (r - pos) % 16
            if pad:
                f = filler(48 + pad)
                blobs.append(f)
                notes.append("filler")
                pos += len(f)
            starts.append(pos)
            rows.append(len(blobs))
            blobs.append(b)
            notes.append(f"{note}@{r}")
            pos += len(b)
        assert set(s % 16 for s in starts) == set(range(16)), note
    return blobs, notes, rows


@functools.lru_cache(maxsize=None)
def window_set():
    """one call: every layout at every residue on both sides (the new side's residues rotated by 5,
    so a delta's two blobs never share one), every blob paired, some sides absent"""
    L = window_layouts()
    ob, onotes, orows = lay_out(L, 0)
    nb, nnotes, nrows = lay_out(L, 5)
    pairs, notes = [], []
    for k, (i, j) in enumerate(zip(orows, nrows)):
        pairs.append((i, NONE if k % 7 == 3 else j))
        notes.append(f"{onotes[i]} | {nnotes[j]}")
    for k, j in enumerate(nrows):
        if k % 7 == 3:
            pairs.append((NONE, j))
            notes.append(f"- | {nnotes[j]}")
    for i in range(0, len(ob), 9):  # fillers and the rest, old side alone
        pairs.append((i, NONE))
        notes.append(f"{onotes[i]} | -")
    pairs.append((NONE, NONE))
    notes.append("- | -")
    return [Call("window", ob, nb, pairs, W_FILT, True, notes=notes)]


# distances of the last blob's start from its arena's end: every one from 52 (the shortest blob the
# register window takes) to 115.  decode_side takes the window only when (a0 & ~3) + 112 <=
# arena_end, i.e. distance + (residue & 3) >= 112, and the staged form loads
# min(ceil((distance + residue) / 16), 7) chunks
END_DIST = list(range(52, 116))


def _end_blob(length, k):
    """a fast-path-shaped blob of exactly ``length`` >= 52 bytes: the layouts of ``window`` that fit"""
    opts = [("null", [NIL])]
    if length >= 56:
        opts.append(("e8/empty8", [ext(EMPTY8, "e8")]))
        opts.append(("fixext/empty8", [ext(EMPTY8, "fix")]))
    if length >= 58:
        opts.append(("a16/e8/empty8", None))
    if length >= 78:
        opts.append(("e8/pt29", [ext(PT_IN, "e8")]))
        opts.append(("e16/pt29", [ext(PT_OUT, "e16")]))
    if length >= 91:
        opts.append(("e32/env40", [ext(ENV40, "e32")]))
    if length >= 80:
        opts.append(("a16/e16/pt29", None))
    note, vals = opts[k % len(opts)]
    if vals is None:  # the array16 values header
        vals = [ext(EMPTY8, "e8")] if note.endswith("empty8") else [ext(PT_IN, "e16")]
        fixed = 46 + sum(len(v) for v in vals)
        b = feature(H0, vals + [F.s_total(length - fixed)], "a16")
    else:
        fixed = 44 + sum(len(v) for v in vals)
        b = F.blob(H0, vals + [F.s_total(length - fixed)])
    assert len(b) == length, (note, length, len(b))
    return note, b


@functools.lru_cache(maxsize=None)
def window_end_set():
    """small arenas whose last blob (52..115 bytes long) starts at every residue: one arena per
    (distance, residue), the old and the new side of a call being two of them.  The second- and
    third-last blobs are a short well-formed one and a fast-path one further than 112 bytes from
    the end, so each arena also holds the window taken and the window refused.  Sixteen more calls
    pack three fast-path-shaped blobs into the tail (below)"""
    arenas = []
    k = 0
    for dist in END_DIST:
        for r in range(16):
            note, last = _end_blob(dist, k)
            k += 1
            lead = placed(ext(PT_IN, "e8"), 0)  # 107 bytes, far from the end: the register window
            mid = filler(45 + ((r - len(lead) - 45) % 16))
            blobs = [lead, mid, last]
            start = len(lead) + len(mid)
            assert start % 16 == r
            arenas.append((blobs, f"end-{dist}@{r}/{note}"))
    calls = []
    for c in range(0, len(arenas), 2):
        (ob, on), (nb, nn) = arenas[c], arenas[c + 1]
        pairs = [(2, 2), (1, 2), (2, NONE), (NONE, 2), (0, 1), (2, 0)]
        calls.append(Call(f"window_end[{on}|{nn}]", ob, nb, pairs, W_FILT, True, notes=[f"{on} | {nn}"] * len(pairs)))
    # fast-path-shaped blobs packed into the arena's tail, as its third-last, second-last and last
    # blob (array16 + ext8, array16 + nil, fixext 8): the last two lie within the last 112 bytes —
    # 107 in the old arena; exactly 112 in the new one, where the second-last takes the window at
    # its very edge — so staging neighbours both load a short run of chunks
    for r in range(16):
        sides = []
        for k2, k3 in ((5, 1), (9, 2)):
            b1 = feature(H0, [ext(EMPTY8, "e8"), F.s_total(1 + r % 3)], "a16")
            b2 = feature(H0, [NIL, F.s_total(k2)], "a16")
            b3 = F.blob(H0, [ext(EMPTY8, "fix"), F.s_total(k3)])
            assert len(b2) >= 52 and len(b2) + len(b3) == (107 if k2 == 5 else 112)
            lead = placed(ext(PT_OUT, "e8"), 0)
            mid = filler(45 + ((r - len(lead) - 45) % 16))
            assert (len(lead) + len(mid)) % 16 == r
            sides.append([lead, mid, b1, b2, b3])
        pairs = [(2, 2), (3, 3), (4, 4), (3, 4), (4, 3), (2, NONE), (NONE, 3), (4, NONE), (0, 1)]
        calls.append(Call(f"window_end[packed@{r}]", sides[0], sides[1], pairs, W_FILT, True,
                          notes=[f"packed@{r}"] * len(pairs)))
    return calls


def end_coverage():
    """{(distance, residue)} of the last blobs of window_end's arenas"""
    seen = set()
    for C in window_end_set():
        for (d, o) in C.arenas:
            seen.add((int(o[-1] - o[-2]), int(o[-2]) % 16))
    return seen


# ------------------------------------------------------------------------------------------
# gpkg: headers, point WKBs, envelopes at the filter's edges, index-envelope edges

G_FILT = (100.0, 120.0, -10.0, 10.0)


def gpkg_values(filt):
    """(note, GPKG bytes) around the filter ``filt``"""
    f0, f1, f2, f3 = filt
    nan, inf = float("nan"), float("inf")
    xm, ym = (f0 + f1) / 2, (f2 + f3) / 2
    V = []
    for flags in range(0x40):  # envelope types 0..7, empty bit, extended bit, both byte orders
        et = (flags >> 1) & 7
        nenv = {0: 0, 1: 4, 2: 6, 3: 6, 4: 8}.get(et, 8)
        env = (xm - 1, xm + 1, ym - 1, ym + 1, 0.0, 1.0, 0.0, 1.0)[:nenv]
        V.append((f"flags{flags:02x}/pt", gpkg(flags, env, wkb_point(xm, ym))))
        V.append((f"flags{flags:02x}/poly", gpkg(flags, env, wkb_poly(xm - 1, xm + 1, ym - 1, ym + 1))))
    V.append(("magic", gpkg(0x01, (), wkb_point(xm, ym), magic=b"GX")))
    V.append(("magic0", gpkg(0x01, (), wkb_point(xm, ym), magic=b"XP")))
    V.append(("version", gpkg(0x01, (), wkb_point(xm, ym), version=1)))
    for typ in (1, 1001, 2001, 3001, 0x20000001, 0x80000001, 2, 1002):
        for bo in (0, 1, 2):
            V.append((f"pt-type{typ:x}/bo{bo}", point(xm, ym, typ=typ, bo=bo)))
            V.append((f"pt-type{typ:x}/bo{bo}/out", point(f1 + 5, ym, typ=typ, bo=bo)))
    for note, x, y in (("nan-x", nan, ym), ("nan-y", xm, nan), ("nan-xy", nan, nan), ("inf-x", inf, ym),
                       ("-inf-x", -inf, ym), ("inf-y", xm, inf), ("-0", -0.0, -0.0), ("x=f0", f0, ym), ("x=f1", f1, ym),
                       ("y=f2", xm, f2), ("y=f3", xm, f3), ("corner", f0, f2), ("in", xm, ym)):
        V.append((f"pt/{note}", point(x, y)))
        V.append((f"pt-be/{note}", point(x, y, flags=0x00, bo=0)))
    E = [("in", (xm - 1, xm + 1, ym - 1, ym + 1)), ("equal", filt), ("cover", (f0 - 1, f1 + 1, f2 - 1, f3 + 1)),
         ("touch-w", (f0 - 5, f0, ym - 1, ym + 1)), ("touch-e", (f1, f1 + 5, ym - 1, ym + 1)),
         ("touch-s", (xm - 1, xm + 1, f2 - 5, f2)), ("touch-n", (xm - 1, xm + 1, f3, f3 + 5)),
         ("zero-w@f0", (f0, f0, ym - 1, ym + 1)), ("zero-w@f1", (f1, f1, ym - 1, ym + 1)),
         ("zero-h@f2", (xm - 1, xm + 1, f2, f2)), ("zero-h@f3", (xm - 1, xm + 1, f3, f3)),
         ("zero-w-in", (xm, xm, ym - 1, ym + 1)), ("zero-h-in", (xm - 1, xm + 1, ym, ym)),
         ("zero-both-in", (xm, xm, ym, ym)), ("edge-in-w", (f0, xm, ym - 1, ym + 1)), ("edge-in-e", (xm, f1, ym - 1, ym + 1)),
         ("edge-in-s", (xm - 1, xm + 1, f2, ym)), ("edge-in-n", (xm - 1, xm + 1, ym, f3)),
         ("cross-w", (f0 - 1, f0 + 1, ym - 1, ym + 1)), ("out", (f1 + 1, f1 + 2, ym - 1, ym + 1)),
         ("out-n", (xm - 1, xm + 1, f3 + 1, f3 + 2)),
         ("inverted-x", (xm + 1, xm - 1, ym - 1, ym + 1)), ("inverted-y", (xm - 1, xm + 1, ym + 1, ym - 1)),
         ("inverted-x-out", (f1 + 9, f1 + 5, ym - 1, ym + 1)),
         ("inf", (-inf, inf, -inf, inf)), ("inf-e", (xm, inf, ym - 1, ym + 1)), ("-0", (-0.0, 0.0, -0.0, 0.0))]
    for k in range(4):
        e = [xm - 1, xm + 1, ym - 1, ym + 1]
        e[k] = nan
        E.append((f"nan{k}", tuple(e)))
    E.append(("nan-all", (nan, nan, nan, nan)))
    # index-envelope edges (kd_geom.h index_env)
    lt = math.nextafter
    E += [("w180", (-90.0, 90.0, 0.0, 1.0)), ("w<180", (-90.0, lt(90.0, 0.0), 0.0, 1.0)), ("w>180", (-90.0, lt(90.0, 99.0), 0.0, 1.0)),
          ("h=1", (10.0, 10.5, 0.0, 1.0)), ("h<1", (10.0, 10.5, 0.0, lt(1.0, 0.0))), ("h>1", (10.0, 10.5, 0.0, lt(1.0, 2.0))),
          ("w=1", (10.0, 11.0, 0.0, 0.5)), ("w<1", (10.0, lt(11.0, 0.0), 0.0, 0.5)),
          ("lat-90", (10.0, 11.0, -90.0, -89.0)), ("lat+90", (10.0, 11.0, 89.0, 90.0)), ("lat-89.95", (10.0, 11.0, -89.95, -89.0)),
          ("lat+89.95", (10.0, 11.0, 89.0, 89.95)), ("lat-out", (10.0, 11.0, -100.0, 100.0)), ("lat-out-s", (10.0, 11.0, -91.0, -90.5)),
          ("lat-out-n", (10.0, 11.0, 90.5, 91.0)), ("x-180", (-180.0, -179.0, 0.0, 1.0)), ("x+180", (179.0, 180.0, 0.0, 1.0)),
          ("x-across", (179.5, 180.5, 0.0, 1.0)), ("x540", (539.0, 540.0, 0.0, 1.0)), ("x-540", (-540.0, -539.0, 0.0, 1.0)),
          ("x720", (719.0, 720.0, 0.0, 1.0)), ("x1e300", (1e300, 1e300, 0.0, 1.0)), ("x-1e300", (-1e300, -1e300 / 2, 0.0, 1.0))]
    for note, e in E:
        V.append((f"env/{note}", gpkg(0x03, e, wkb_poly(*[0.0 if math.isnan(v) or math.isinf(v) else v for v in e]))))
        V.append((f"env-be/{note}", gpkg(0x02, e, wkb_point(xm, ym))))
    for x in (-180.0, 180.0, 540.0, -540.0, 720.0, -720.0, 1e300, -1e300, 179.99999999, -0.0):
        for y in (0.0, 90.0, -90.0, 91.0, -91.0):
            V.append((f"pt/x{x:g}/y{y:g}", point(x, y)))
    return V


@functools.lru_cache(maxsize=None)
def gpkg_set():
    """the same values under four filters: rectangular, not rectangular, zero width, and one whose
    edges are +0.0 (against the -0.0 values); geometry first on the old side (the register window:
    ext8, or ext16 on every third), third on the new side (the byte-wise walk)"""
    calls = []
    for name, filt, rect in (("rect", G_FILT, True), ("poly", G_FILT, False), ("zero-width", (110.0, 110.0, -10.0, 10.0), True),
                             ("zero-edges", (0.0, 20.0, 0.0, 10.0), True)):
        V = gpkg_values(G_FILT if name != "zero-edges" else filt)
        ob = [placed(ext(g, "e16" if k % 3 == 2 else "e8"), 0, "a16" if k % 2 else "fix", pad=k % 17) for k, (_, g) in enumerate(V)]
        nb = [filler(45 + k % 16) for k in range(3)] + [placed(ext(g, "e8"), 2) for _, g in V]
        n = len(V)
        i = np.arange(n, dtype=np.uint32)
        none = np.full(n, NONE, np.uint32)
        pairs = np.concatenate([np.stack([i, none], 1), np.stack([none, i + 3], 1), np.stack([i[::-1], i + 3], 1)])
        notes = [f"{v[0]} | -" for v in V] + [f"- | {v[0]}" for v in V] + [f"{V[n - 1 - k][0]} | {V[k][0]}" for k in range(n)]
        # the new side through the register window as well: its index envelope comes from that decode
        pairs = np.concatenate([pairs, np.stack([none, i], 1)])
        notes += [f"- | fast {v[0]}" for v in V]
        nb = nb + ob
        pairs[3 * n:, 1] += 3 + n
        calls.append(Call(f"gpkg/{name}", ob, nb, pairs, filt, rect, notes=notes))
    return calls


# ------------------------------------------------------------------------------------------
# legends

MAXLEG = 64  # GF_MAXLEG


def _leg_blob(h, gi, g):
    if gi == 0:
        return feature(h, [ext(g, "e8"), b"\x01", F.str_forms(b"s" * 20)["fix"]])
    if gi == 2:
        return feature(h, [b"\x01", F.str_forms(b"t" * 3)["fix"], ext(g, "e8")])
    return feature(h, [b"\x01", b"\x02"])


def _leg_call(name, old_tab, new_tab, use):
    """blobs of the legends ``use`` (indices into the old table; the new side holds the same hexes
    laid out for the new table's geometry index), inside and outside the filter"""
    nmap = dict(new_tab)
    ob, nb, notes = [], [], []
    for k in use:
        h, gi = old_tab[k]
        for g, gn in ((PT_IN, "in"), (PT_OUT, "out")):
            ob.append(_leg_blob(h, gi, g))
            nb.append(_leg_blob(h, nmap.get(h, 0), g))
            notes.append(f"legend {k} {gn}")
    pairs = both_sides(len(ob))
    # (two fillers behind them: every blob above lies further than 112 bytes from its arena's end,
    # so each is decoded from the register window)
    ob, nb = ob + [filler(60), filler(61)], nb + [filler(62), filler(63)]
    return Call(f"legends/{name}", ob, nb, pairs, W_FILT, True, old_tab, new_tab, notes=notes * 3)


@functools.lru_cache(maxsize=None)
def legends_set():
    calls = []
    one = [(hexof("only"), 0)]
    calls.append(_leg_call("one", one, one, [0]))
    # 64 legends: the new table in reverse order with other geometry indices (the same hex has its
    # geometry at 0 on the old side and at 2 on the new side, and so on round)
    old64 = [(hexof(f"leg{k}"), (0, 2, -1)[k % 3]) for k in range(MAXLEG)]
    new64 = [(h, (2, -1, 0)[k % 3]) for k, (h, _) in enumerate(old64)][::-1]
    calls.append(_leg_call("64", old64, new64, [0, 1, 2, 31, 32, 61, 62, 63]))
    # legends equal except in dword 0 (byte 0) or in dword 9 (byte 39): the near twins come first in
    # the table and have no geometry column, so a compare that skips a dword answers MATCHING
    base = hexof("near")
    flip = lambda c: "0" if c != "0" else "1"
    d0, d9 = flip(base[0]) + base[1:], base[:39] + flip(base[39])
    near = [(d9, -1), (d0, -1), (base, 0)]
    calls.append(_leg_call("near", near, near[::-1], [0, 1, 2]))
    # an empty table on one side: every blob of that side has an unknown legend
    calls.append(_leg_call("empty-old", TAB, TAB, [0, 1, 2]))
    calls[-1].tabs = ([], list(TAB))
    calls.append(_leg_call("empty-new", TAB, TAB, [0, 1, 2]))
    calls[-1].tabs = (list(TAB), [])
    return calls


def too_many_legends():
    """65 legends on the new side: kd_geom_filter refuses (KD_EUNSUPPORTED)"""
    tab = [(hexof(f"leg{k}"), 0) for k in range(MAXLEG + 1)]
    return _leg_call("65", tab[:1], tab, [0])


# ------------------------------------------------------------------------------------------
# headers: msgpack header forms around the legend, the top level and the values


def header_rows():
    g8 = ext(PT_IN, "e8")
    tail = [b"\x01", F.str_forms(b"s" * 30)["fix"]]
    R = []
    for lf in ("s8", "s16", "s32"):
        R.append((f"legend-{lf}", feature(H0, [g8] + tail, legend_form=lf)))
        R.append((f"legend-{lf}/later", feature(H2, [b"\x01", b"\x02", g8], legend_form=lf)))
        R.append((f"legend-{lf}/nogeom", feature(HN, tail, legend_form=lf)))
    body = F.array_header(3) + g8 + b"".join(tail)
    R.append(("legend-bin8", b"\x92\xc4\x28" + H0.encode() + body))
    R.append(("legend-str39", b"\x92\xd9\x27" + H0.encode()[:39] + body))
    R.append(("legend-str41", b"\x92\xd9\x29" + H0.encode() + b"0" + body))
    R.append(("legend-fixstr31", b"\x92\xbf" + H0.encode()[:31] + body))
    for note, top in (("top-array16", b"\xdc\x00\x02"), ("top-array32", b"\xdd\x00\x00\x00\x02")):
        R.append((note, feature(H0, [g8] + tail, top=top)))
        R.append((note + "/later", feature(H2, [b"\x01", b"\x02", g8], top=top)))
        R.append((note + "/nogeom", feature(HN, tail, top=top)))
        R.append((note + "/null", feature(H0, [NIL] + tail, top=top)))
    R.append(("top-array16-of-3", feature(H0, [g8] + tail, top=b"\xdc\x00\x03") + b"\x01"))
    R.append(("top-fixarray1", b"\x91" + F.legend_header(H0)))
    R.append(("top-fixarray1+values", feature(H0, [g8] + tail, top=b"\x91")))
    R.append(("top-fixarray3", feature(H0, [g8] + tail, top=b"\x93") + b"\x01"))
    R.append(("top-map1", feature(H0, [g8] + tail, top=b"\x81")))
    R.append(("top-map16", feature(H0, [g8] + tail, top=b"\xde\x00\x01")))
    for vh in ("a16", "a32"):
        R.append((f"values-{vh}", feature(H0, [g8] + tail, vh)))
        R.append((f"values-{vh}/later", feature(H2, [b"\x01", b"\x02", g8], vh)))
        R.append((f"values-{vh}/null", feature(H0, [NIL] + tail, vh)))
    head = b"\x92" + F.legend_header(H0)
    R.append(("values-str", head + F.str_forms(b"abc" * 10)["fix"]))
    R.append(("values-bin", head + F.bin_forms(b"abc" * 10)["b8"]))
    R.append(("values-str/nogeom", b"\x92" + F.legend_header(HN) + F.str_forms(b"abc" * 10)["fix"]))
    # the geometry index at and beyond the values count
    for vh in ("fix", "a16"):
        R.append((f"gidx=count/{vh}", feature(H2, [b"\x01", F.str_forms(b"t" * 20)["fix"]], vh)))
        R.append((f"gidx>count/{vh}", feature(H2, [F.str_forms(b"t" * 20)["fix"]], vh)))
        R.append((f"gidx=count=0/{vh}", feature(H0, [], vh)))
        R.append((f"count=1/{vh}", feature(H0, [g8], vh)))
    # ext values that are not the geometry's
    for form in ("e8", "e16", "e32"):
        R.append((f"ext-type5/{form}", feature(H0, [ext(PT_IN, form, code=5)] + tail)))
        R.append((f"ext-type5/{form}/a16", feature(H0, [ext(PT_IN, form, code=5)] + tail, "a16")))
        whole = feature(H0, [ext(PT_IN + b"\x00" * 40, form)])
        R.append((f"ext-len+1/{form}", whole[:-1]))  # the ext length reaches one byte past the blob
        R.append((f"ext-len-exact/{form}", whole))
    R.append(("fixext-type5", feature(H0, [ext(EMPTY8, "fix", code=5)] + tail)))
    R.append(("not-ext/float", feature(H0, [b"\xcb" + struct.pack(">d", 1.5)] + tail)))
    R.append(("not-ext/bin", feature(H0, [F.bin_forms(PT_IN)["b8"]] + tail)))
    return R


@functools.lru_cache(maxsize=None)
def headers_set():
    R = header_rows()
    ob = [b for _, b in R]
    nb = [filler(45 + 5)] + ob  # the new side's blobs start at other residues
    n = len(ob)
    i = np.arange(n, dtype=np.uint32)
    none = np.full(n, NONE, np.uint32)
    pairs = np.concatenate([np.stack([i, i + 1], 1), np.stack([i, none], 1), np.stack([none, i + 1], 1)])
    return [Call("headers", ob, nb, pairs, W_FILT, True, notes=[r[0] for r in R] * 3)]


# ------------------------------------------------------------------------------------------
# tails: damage after, inside and before the geometry value


def tail_rows():
    """(note, blob, W, where): W the well-formed blob the row was made from; where = 'after' (the
    damage lies strictly after the geometry value's last byte), 'before' (at or before it), 'twin'
    (W itself)"""
    gW = poly(2.0, 4.0, 2.0, 4.0)  # 8 + 32 + 93 bytes
    Wf = feature(H0, [ext(gW, "e8"), b"\x01", F.str_forms(b"s" * 30)["fix"]])
    Wl = feature(H2, [b"\xcb" + struct.pack(">d", 1.5), F.str_forms(b"t" * 5)["fix"], ext(gW, "e8"), b"\x07",
                      F.str_forms(b"s" * 20)["fix"]])
    Wp = feature(H0, [ext(PT_OUT, "e16"), b"\x01", F.str_forms(b"s" * 12)["fix"]], "a16")
    R = []
    for wn, W, gend in (("first", Wf, 44 + 3 + len(gW)), ("later", Wl, 44 + 9 + 6 + 3 + len(gW)),
                        ("first16", Wp, 46 + 4 + len(PT_OUT))):
        assert W[gend - 1:gend] == gW[-1:] or W[gend - 1:gend] == PT_OUT[-1:]
        R.append((f"{wn}/twin", W, W, "twin"))
        R.append((f"{wn}/+1", W + b"\x00", W, "after"))
        R.append((f"{wn}/+9", W + b"\xc0" * 9, W, "after"))
        for k in range(1, len(W) - gend + 1):
            R.append((f"{wn}/cut{k}", W[:-k], W, "after"))
        for at in (gend - 1, gend - 10, gend - len(gW if wn != "first16" else PT_OUT) + 3, 60, 50, 44, 30, 2):
            R.append((f"{wn}/[:{at}]", W[:at], W, "before"))
    # no values at all, then bytes that look like a geometry: nothing there is the geometry value
    for vh, hd0, hd1 in (("fix", b"\x90", b"\x91"), ("a16", b"\xdc\x00\x00", b"\xdc\x00\x01")):
        head = b"\x92" + F.legend_header(H0)
        nulls = NIL + bytes(range(1, 9))
        R.append((f"empty-values/{vh}/null", head + hd0 + nulls, head + (b"\x99" if vh == "fix" else b"\xdc\x00\x09") + nulls,
                  "before"))
        R.append((f"empty-values/{vh}/extG", head + hd0 + ext(PT_IN, "e8"), head + hd1 + ext(PT_IN, "e8"), "before"))
        R.append((f"empty-values/{vh}/ext16G", head + hd0 + ext(PT_IN, "e16"), head + hd1 + ext(PT_IN, "e16"), "before"))
    return R


@functools.lru_cache(maxsize=None)
def tails_set():
    """[0]: the damaged rows; [1]: the same call over each row's W (what the arena form answers for
    the 'after' rows)"""
    R = tail_rows()
    calls = []
    for which in (1, 2):
        ob = [r[which] for r in R]
        nb = [filler(45 + 9)] + ob
        n = len(ob)
        i = np.arange(n, dtype=np.uint32)
        none = np.full(n, NONE, np.uint32)
        pairs = np.concatenate([np.stack([i, i + 1], 1), np.stack([i, none], 1), np.stack([none, i + 1], 1)])
        calls.append(Call("tails" if which == 1 else "tails/W", ob, nb, pairs, W_FILT, True, notes=[r[0] for r in R] * 3))
    calls[0].where = [r[3] for r in R] * 3
    return calls


def tails_arena_expected(bits):
    """the arena form's contract on ``tails``: the oracle's answer for the row where the damage is
    at or before the geometry value's last byte, the oracle's answer for W where it lies after"""
    T, TW = tails_set()
    codes, _, enc, ok = (x.copy() for x in T.oracle(bits))
    wc, _, wenc, wok = TW.oracle(bits)
    after = np.array([w == "after" for w in T.where])
    codes[after] = wc[after]
    enc[after] = wenc[after]
    ok[after] = wok[after]
    keep = np.nonzero(((codes >= 1) & (codes <= 3)).any(axis=1))[0].astype(np.uint32)
    return codes, keep, enc, ok


# ------------------------------------------------------------------------------------------
# tiles: delta counts around the wave, round and tile seams, kept patterns, deferred heads

TILE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
TILE_PATTERNS = ("all", "none", "alternating", "last-lane", "last-delta")
# blob rows of the tiles arena (both sides alike)
T_KEPT, T_NON, T_DEF_NON, T_DEF_KEPT, T_NAN_NON, T_NULL, T_CAND = range(7)


def tile_blobs():
    xyz_out = gpkg(0x05, (50.0, 60.0, 1.0, 2.0, 0.0, 9.0), wkb_poly(50.0, 60.0, 1.0, 2.0))  # deferred, then NON_MATCHING
    xyz_in = gpkg(0x05, (1.0, 2.0, 1.0, 2.0, 0.0, 9.0), wkb_poly(1.0, 2.0, 1.0, 2.0))  # deferred, then MATCHING
    nan_out = gpkg(0x03, (float("nan"), 60.0, 1.0, 2.0), wkb_point(50.0, 5.0))  # NaN envelope: the point decides
    vals = [PT_IN, PT_OUT, xyz_out, xyz_in, nan_out, None, poly(5.0, 15.0, 5.0, 15.0)]
    return [placed(ext(g, "e8") if g is not None else NIL, 0) for g in vals]


def tile_pairs(n, pattern):
    """(pairs, hand): the pattern's kept and dropped deltas, then the deferred heads and the
    out-of-range indices at their fixed rows"""
    d = np.arange(n)
    if pattern == "all":
        kept = np.ones(n, bool)
    elif pattern == "none":
        kept = np.zeros(n, bool)
    elif pattern == "alternating":
        kept = d % 2 == 0
    elif pattern == "last-lane":
        kept = d % 64 == 63
    else:
        kept = d == n - 1
    pairs = np.empty((n, 2), np.uint32)
    pairs[:, 0] = np.where(d % 3 == 0, NONE, T_NON)
    pairs[:, 1] = np.where(kept, np.where(d % 5 == 0, T_CAND, T_KEPT), np.where(d % 4 == 1, NONE, T_NON))
    hand = {}
    if n >= 257:
        # deferred heads: NON_MATCHING beside a NONE side and beside a NON side, both sides
        # deferred, a deferred side beside a kept side, a NaN envelope, one that stays kept
        at = 4091 if n > 4096 else 60
        special = [(T_DEF_NON, T_KEPT), (T_DEF_NON, T_DEF_NON), (T_NAN_NON, T_DEF_KEPT), (T_NULL, T_NAN_NON),
                   (T_DEF_NON, NONE), (T_NON, T_DEF_NON)]
        for k, p in enumerate(special):  # n > 4096: the last two sit at deltas 4095 and 4096
            pairs[at + k] = p
    if n == 257 or n == 4097:
        # 4 sides past the arena / the heads (2 rows per count, 2 counts, 5 patterns: 20 rows in all)
        pairs[7] = (len(tile_blobs()), T_KEPT)
        pairs[200] = (T_NON, 0xFFFFFFFE)
        hand = {(7, 0): 3, (200, 1): 3}
    return pairs, hand


@functools.lru_cache(maxsize=None)
def tiles_set():
    """every delta count x kept pattern.  Rows whose index is past the blobs / heads: rows 7 (old
    side) and 200 (new side) of the counts 257 and 4097 — two per call, 20 rows over the set; the
    oracle is given NONE there and code 3 is stated by hand"""
    blobs = tile_blobs()
    calls = []
    for n in TILE_COUNTS:
        for pat in TILE_PATTERNS:
            pairs, hand = tile_pairs(n, pat)
            calls.append(Call(f"tiles/{n}/{pat}", blobs, blobs[::-1] + blobs, pairs_new_shift(pairs, len(blobs), hand), W_FILT,
                              True, hand=hand))
    return calls


def pairs_new_shift(pairs, k, hand):
    """the new arena holds the blobs behind k others: its indices move by k (hand rows stay)"""
    p = pairs.copy()
    m = p[:, 1] != NONE
    for (row, side) in hand:
        if side == 1:
            m[row] = False
    p[m, 1] += k
    return p


# ------------------------------------------------------------------------------------------
# scan: more tiles than one pass of k_gf_scan

SCAN_N = (SPT_TILES + 1) * TILE
SCAN_ROWS = (0, TILE - 1, SPT_TILES * TILE - 1, SPT_TILES * TILE, SCAN_N - 1)


def scan_blobs():
    return [placed(NIL, 0)]


# ------------------------------------------------------------------------------------------
# the device forms: everything in device memory, the delta count in a device word

SENTINEL = 0xA5
POISON = 0xFFFFFFFE  # pairs beyond the count: never read (an index past every arena if they were)


def _dev_blobs(engine, arenas):
    from kart_amd.device import DevBlobs

    dbs = [DevBlobs(engine, d, o) for d, o in arenas]
    kbs = []
    for db in dbs:
        b = N.KdBlobs()
        b.n, b.data, b.off, b.mem = db.n, db.data.ptr, db.off.ptr, N.KD_MEM_DEVICE
        kbs.append(b)
    return dbs, kbs


def delta_order_heads(heads, pairs, slots):
    """heads in delta order (slot d: delta d's), as the blob reader lays them out; a side whose
    index is past the heads gets a FALLBACK head"""
    out = []
    for s in range(2):
        h = np.zeros(slots, S.GEOM_HEAD)
        col = pairs[:, s].astype(np.int64)
        ok = (pairs[:, s] != NONE) & (col < len(heads[s]))
        h[np.nonzero(ok)[0]] = heads[s][col[ok]]
        bad = np.nonzero((pairs[:, s] != NONE) & ~ok)[0]
        h["goff_status"][bad] = N.KD_GH_FALLBACK << 24
        out.append(h)
    return out


def device_filter(engine, C, bits, form, mode):
    """``form``: 'arena' (kd_geom_filter), 'gather' (kd_geom_filter_deltas over per-entry heads),
    'delta' (kd_geom_filter_deltas, KD_GF_DELTA_HEADS).  ``mode``: 'full' (count = capacity),
    'zero' (count 0), 'below' (the capacity two tiles above the count, the pairs beyond the count
    poisoned).  Outputs are pre-filled with SENTINEL.
    -> (codes, keep, enc, ok, untouched): the outputs up to the count, and whether every output
    byte at or beyond the count (beyond n_keep for keep) still holds the sentinel"""
    from kart_amd.device import DevBuf

    L, ctx = engine.L, engine.ctx
    n = C.n
    cap = n + (2 * TILE if mode == "below" else 0)
    cnt = 0 if mode == "zero" else n
    nb = bits // 2
    pairs = np.full((max(cap, 1), 2), POISON, np.uint32)
    pairs[:n] = C.pairs
    dp = DevBuf.from_numpy(engine, pairs)
    dcnt = DevBuf.from_numpy(engine, np.array([cnt], np.uint64))
    outs = {"match": DevBuf(engine, 2 * cap + 16), "keep": DevBuf(engine, 4 * cap + 16), "nk": DevBuf(engine, 8)}
    if bits:
        outs["enc"] = DevBuf(engine, cap * nb + 16)
        outs["ok"] = DevBuf(engine, cap + 16)
    for b in outs.values():
        N.check(L.kd_memset(ctx, b.ptr, SENTINEL, b.nbytes), "kd_memset")
    fe = (ctypes.c_double * 4)(*C.filt)
    flags = N.KD_GF_RECT if C.rect else 0
    dbs, kbs = _dev_blobs(engine, C.arenas)
    d_n = ctypes.cast(dcnt.ptr, N.c_u64p)
    nk = ctypes.cast(outs["nk"].ptr, N.c_u64p)
    enc_p = outs["enc"].ptr if bits else None
    ok_p = outs["ok"].ptr if bits else None
    if form == "arena":
        gc = C.geom_cols()
        kc = gc.kd_cols()
        N.check(L.kd_geom_filter(ctx, ctypes.byref(kbs[0]), ctypes.byref(kbs[1]), dp.ptr, cap, d_n, N.KD_MEM_DEVICE,
                                 ctypes.byref(kc), fe, flags, int(bits), outs["match"].ptr, outs["keep"].ptr, nk, enc_p, ok_p,
                                 N.KD_MEM_DEVICE), "kd_geom_filter")
    else:
        heads = C.heads()
        if form == "delta":
            slots = max((cap + 63) // 64 * 64, 64)
            heads = delta_order_heads(heads, pairs[:n] if n else pairs[:0], slots)
            flags |= N.KD_GF_DELTA_HEADS
        dh = [DevBuf.from_numpy(engine, h.view(np.uint8).reshape(-1)) if h.size else DevBuf(engine, 48) for h in heads]
        N.check(L.kd_geom_filter_deltas(ctx, dh[0].ptr, len(heads[0]), dh[1].ptr, len(heads[1]), ctypes.byref(kbs[0]),
                                        ctypes.byref(kbs[1]), dp.ptr, cap, d_n, fe, flags, int(bits), outs["match"].ptr,
                                        outs["keep"].ptr, nk, enc_p, ok_p), "kd_geom_filter_deltas")
    engine.sync()
    k = int(outs["nk"].download(np.uint64, 1)[0])
    assert k <= cnt, (C.name, form, mode, k, cnt)
    match = outs["match"].download(np.uint8, outs["match"].nbytes)
    keep = outs["keep"].download(np.uint8, outs["keep"].nbytes)
    untouched = bool((match[2 * cnt:] == SENTINEL).all() and (keep[4 * k:] == SENTINEL).all())
    enc = ok = None
    if bits:
        e = outs["enc"].download(np.uint8, outs["enc"].nbytes)
        o = outs["ok"].download(np.uint8, outs["ok"].nbytes)
        untouched = untouched and bool((e[cnt * nb:] == SENTINEL).all() and (o[cnt:] == SENTINEL).all())
        enc, ok = e[:cnt * nb].reshape(cnt, nb), o[:cnt]
    return match[:2 * cnt].reshape(cnt, 2), keep[:4 * k].view(np.uint32), enc, ok, untouched


def scan_device(engine, form):
    """the ``scan`` set through a device form ('arena' or 'delta'): SCAN_N deltas, all (NONE, NONE)
    — the pairs filled with 0xFF on the device — except SCAN_ROWS, whose new side is a null-geometry
    blob.  -> (codes [SCAN_N, 2], keep)"""
    from kart_amd.device import DevBuf

    L, ctx = engine.L, engine.ctx
    n = SCAN_N
    dp = DevBuf(engine, 8 * n)
    N.check(L.kd_memset(ctx, dp.ptr, 0xFF, dp.nbytes), "kd_memset")
    for r in SCAN_ROWS:
        dp.upload(np.array([NONE, 0], np.uint32), offset=8 * r)
    dcnt = DevBuf.from_numpy(engine, np.array([n], np.uint64))
    match, keep, nkb = DevBuf(engine, 2 * n), DevBuf(engine, 4 * n), DevBuf(engine, 8)
    fe = (ctypes.c_double * 4)(*W_FILT)
    blobs = scan_blobs()
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    dbs, kbs = _dev_blobs(engine, (empty, arena(blobs)))
    d_n = ctypes.cast(dcnt.ptr, N.c_u64p)
    nk = ctypes.cast(nkb.ptr, N.c_u64p)
    if form == "arena":
        gc = S.GeomCols.__new__(S.GeomCols)
        gc.old_hex, gc.old_gidx, gc.old_map = cols_of(TAB)
        gc.new_hex, gc.new_gidx, gc.new_map = cols_of(TAB)
        kc = gc.kd_cols()
        N.check(L.kd_geom_filter(ctx, ctypes.byref(kbs[0]), ctypes.byref(kbs[1]), dp.ptr, n, d_n, N.KD_MEM_DEVICE,
                                 ctypes.byref(kc), fe, N.KD_GF_RECT, 0, match.ptr, keep.ptr, nk, None, None, N.KD_MEM_DEVICE),
                "kd_geom_filter")
    else:
        # delta-order heads: one zeroed array serves both sides (the old side is absent everywhere)
        hx, gi, m = cols_of(TAB)
        head = S.geom_heads(*arena(blobs), hx, gi, len(m))
        dh = DevBuf(engine, 48 * n)
        dh.zero()
        for r in SCAN_ROWS:
            dh.upload(head.view(np.uint8).reshape(-1), offset=48 * r)
        N.check(L.kd_geom_filter_deltas(ctx, dh.ptr, n, dh.ptr, n, ctypes.byref(kbs[0]), ctypes.byref(kbs[1]), dp.ptr, n, d_n,
                                        fe, N.KD_GF_RECT | N.KD_GF_DELTA_HEADS, 0, match.ptr, keep.ptr, nk, None, None),
                "kd_geom_filter_deltas")
    engine.sync()
    k = int(nkb.download(np.uint64, 1)[0])
    assert k <= n
    return match.download(np.uint8, 2 * n).reshape(n, 2), keep.download(np.uint32, k)


SETS = {"window": window_set, "window_end": window_end_set, "gpkg": gpkg_set, "legends": legends_set,
        "headers": headers_set, "tiles": tiles_set}
