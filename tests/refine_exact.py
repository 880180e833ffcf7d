"""An independent exact Intersects(feature, filter polygon) and a small WKB / GPKG builder — the
reference the tests of kd_geom_refine are held against.

Every coordinate is a double, and a double is an exact rational: orientations are computed in
``fractions.Fraction``, box tests as plain comparisons of doubles (which are exact).  The filter's
region is the even-odd interior of all its rings, boundary included; a feature polygon's region the
even-odd interior of its own rings, boundary included; touching counts as intersecting.
"""
import struct
from fractions import Fraction

import numpy as np

POINT, LINESTRING, POLYGON, MULTIPOINT, MULTILINESTRING, MULTIPOLYGON = 1, 2, 3, 4, 5, 6
DIMS = {"XY": (0, 0), "Z": (1000, 1), "M": (2000, 1), "ZM": (3000, 2)}  # type offset, extra ordinates


# ---------------------------------------------------------------------------------------------
# WKB / GPKG builder.  A geometry is (type, data): Point (x, y); LineString [pts]; Polygon [rings];
# MultiPoint [pts]; MultiLineString [lines]; MultiPolygon [polygons]
def _coords(pts, dim, e):
    extra = DIMS[dim][1]
    return b"".join(struct.pack(e + "dd", float(x), float(y)) + struct.pack(e + "d" * extra, *([7.5, -3.25][:extra]))
                    for x, y in pts)


def wkb(geom, dim="XY", le=True, sub_le=None):
    """ISO WKB of ``geom``; ``sub_le``: the byte order of a multi-geometry's parts (default: ``le``)"""
    typ, data = geom
    e = "<" if le else ">"
    head = struct.pack(e + "BI", 1 if le else 0, typ + DIMS[dim][0])
    if typ == POINT:
        return head + _coords([data], dim, e)
    if typ == LINESTRING:
        return head + struct.pack(e + "I", len(data)) + _coords(data, dim, e)
    if typ == POLYGON:
        return head + struct.pack(e + "I", len(data)) + b"".join(
            struct.pack(e + "I", len(r)) + _coords(r, dim, e) for r in data)
    sle = le if sub_le is None else sub_le
    return head + struct.pack(e + "I", len(data)) + b"".join(wkb((typ - 3, part), dim, sle) for part in data)


def vertices(geom):
    typ, data = geom
    if typ == POINT:
        return [data]
    if typ in (LINESTRING, MULTIPOINT):
        return list(data)
    if typ in (POLYGON, MULTILINESTRING):
        return [p for r in data for p in r]
    return [p for poly in data for r in poly for p in r]


def gpkg(wkb_bytes, env=None, le=True):
    """GPKG value: header (with an XY envelope when ``env`` = (minx, maxx, miny, maxy) is given) + WKB"""
    e = "<" if le else ">"
    flags = (1 if le else 0) | (2 if env is not None else 0)
    out = b"GP\x00" + bytes([flags]) + struct.pack(e + "i", 4326)
    if env is not None:
        out += struct.pack(e + "dddd", *env)
    return out + wkb_bytes


def gpkg_of(geom, dim="XY", le=True, sub_le=None):
    """GPKG value of ``geom`` with the envelope of its vertices (none for a point)"""
    v = vertices(geom)
    env = None
    if geom[0] != POINT and v:
        xs, ys = [p[0] for p in v], [p[1] for p in v]
        env = (min(xs), max(xs), min(ys), max(ys))
    return gpkg(wkb(geom, dim, le, sub_le), env, le)


def parse_gpkg(g):
    """the geometry of a GPKG value (types 1-6, any dimension, either byte order)"""
    g = bytes(g)
    assert g[:2] == b"GP"
    off = 8 + {0: 0, 1: 32, 2: 48, 3: 48, 4: 64}[(g[3] >> 1) & 7]
    geom, _ = _parse(g, off)
    return geom


def _parse(b, p):
    e = "<" if b[p] == 1 else ">"
    t = struct.unpack_from(e + "I", b, p + 1)[0]
    typ, stride = t % 1000, {0: 16, 1: 24, 2: 24, 3: 32}[t // 1000]
    p += 5

    def pts(p, n):
        return [struct.unpack_from(e + "dd", b, p + i * stride) for i in range(n)], p + n * stride

    if typ == POINT:
        v, p = pts(p, 1)
        return (typ, v[0]), p
    n = struct.unpack_from(e + "I", b, p)[0]
    p += 4
    if typ == LINESTRING:
        v, p = pts(p, n)
        return (typ, v), p
    if typ == POLYGON:
        rings = []
        for _ in range(n):
            k = struct.unpack_from(e + "I", b, p)[0]
            v, p = pts(p + 4, k)
            rings.append(v)
        return (typ, rings), p
    parts = []
    for _ in range(n):
        (st, d), p = _parse(b, p)
        assert st == typ - 3
        parts.append(d)
    return (typ, parts), p


# ---------------------------------------------------------------------------------------------
# exact predicates
ZEROS = [0]  # how many determinants came out exactly zero so far (a test of general position reads it)


def orient(a, b, c):
    """sign of det(a - c, b - c), exactly"""
    ax, ay, bx, by, cx, cy = (Fraction(float(v)) for v in (a[0], a[1], b[0], b[1], c[0], c[1]))
    d = (ax - cx) * (by - cy) - (ay - cy) * (bx - cx)
    if d == 0:
        ZEROS[0] += 1
    return (d > 0) - (d < 0)


class Edges:
    """the segments of closed rings or open lines, with their boxes"""

    def __init__(self, chains, closed):
        a, b = [], []
        for ch in chains:
            ch = [(float(x), float(y)) for x, y in ch]
            if closed and ch and ch[0] != ch[-1]:
                ch = ch + [ch[0]]
            a += ch[:-1]
            b += ch[1:]
        self.A = np.array(a, np.float64).reshape(-1, 2)
        self.B = np.array(b, np.float64).reshape(-1, 2)
        self.lo, self.hi = np.minimum(self.A, self.B), np.maximum(self.A, self.B)
        self.n = self.A.shape[0]

    def contains(self, p):
        """p in the even-odd interior of the rings, or on one of them"""
        x, y = float(p[0]), float(p[1])
        if not self.n:
            return False
        box = np.nonzero((self.lo[:, 0] <= x) & (x <= self.hi[:, 0]) & (self.lo[:, 1] <= y) & (y <= self.hi[:, 1]))[0]
        for i in box:
            if orient(self.A[i], self.B[i], (x, y)) == 0:
                return True  # on the boundary
        ua, ub = self.A[:, 1] > y, self.B[:, 1] > y
        par = 0
        for i in np.nonzero(ua != ub)[0]:
            if self.hi[i, 0] < x:
                continue
            if self.lo[i, 0] > x:
                par ^= 1
            elif (orient(self.A[i], self.B[i], (x, y)) > 0) == bool(ub[i]):
                par ^= 1
        return bool(par)

    def meets(self, other):
        """some segment of self meets some segment of other (touching included)"""
        if not self.n or not other.n:
            return False
        olo, ohi = other.lo.min(0), other.hi.max(0)
        for i in np.nonzero((self.lo[:, 0] <= ohi[0]) & (self.hi[:, 0] >= olo[0]) & (self.lo[:, 1] <= ohi[1]) &
                            (self.hi[:, 1] >= olo[1]))[0]:
            a, b = self.A[i], self.B[i]
            cand = np.nonzero((other.lo[:, 0] <= self.hi[i, 0]) & (other.hi[:, 0] >= self.lo[i, 0]) &
                              (other.lo[:, 1] <= self.hi[i, 1]) & (other.hi[:, 1] >= self.lo[i, 1]))[0]
            for j in cand:
                c, d = other.A[j], other.B[j]
                o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
                if o1 * o2 < 0 and o3 * o4 < 0:
                    return True
                # (the boxes overlap: a collinear end point inside the other segment's box lies on it)
                if (o1 == 0 and _inbox(a, b, c)) or (o2 == 0 and _inbox(a, b, d)) or (o3 == 0 and _inbox(c, d, a)) or \
                        (o4 == 0 and _inbox(c, d, b)):
                    return True
        return False


def _inbox(a, b, p):
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


class ExactFilter:
    """Intersects against a polygon filter given as [polygon][ring][(x, y)] or a flat list of rings"""

    def __init__(self, polygons):
        rings = [r for poly in polygons for r in poly]
        self.rings = [[(float(x), float(y)) for x, y in r] for r in rings]
        self.E = Edges(self.rings, True)
        self.first = [r[0] for r in self.rings]

    def intersects(self, geom):
        typ, data = geom
        if typ == POINT:
            return self.E.contains(data)
        if typ == MULTIPOINT:
            return any(self.E.contains(p) for p in data)
        if typ == LINESTRING:
            return self._line(data)
        if typ == MULTILINESTRING:
            return any(self._line(ln) for ln in data)
        if typ == POLYGON:
            return self._poly(data)
        if typ == MULTIPOLYGON:
            return any(self._poly(p) for p in data)
        raise ValueError(typ)

    def _line(self, pts):
        if any(self.E.contains(p) for p in pts):
            return True
        return Edges([pts], False).meets(self.E)

    def _poly(self, rings):
        rings = [r for r in rings if r]
        if any(self.E.contains(p) for r in rings for p in r):
            return True
        F = Edges(rings, True)
        if F.meets(self.E):
            return True
        return any(F.contains(q) for q in self.first)
