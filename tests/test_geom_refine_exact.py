"""kd_geom_refine with KD_GF_EXACT: the sides FP64 cannot certify — every touching configuration, near
misses inside the static bound — decided on the GPU by the determinant's exact sign.  Every side of
every test is compared with refine_exact.ExactFilter.intersects (rational arithmetic)."""
import math
import struct
import types

import numpy as np
import pytest

import refine_exact as X
from kart_amd import _native as N
from kart_amd import dataset as D
from kart_amd import packing, synth, walkkey
from kart_amd import spatial as S
from test_dropin import version
from test_geom_refine import FILTERS, GIDX, HEX, HEXARR, LEGEND, NONE, _head_geometries, arena_of, ring, variants
from fixtures import load

SHIFT = (1570000.25, 5180000.5)  # the scaled lattice: coordinates k * 2^-10 + SHIFT, exactly representable


def refine_sides(engine, polygons, gpkgs, exact):
    """the GPKG values as the new sides of inserts, every one a candidate: (codes of the new sides, stats)"""
    n = len(gpkgs)
    ar = arena_of(gpkgs)
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    heads = S.geom_heads(*ar, HEXARR, GIDX, 1)
    pairs = np.stack([np.full(n, NONE, np.uint32), np.arange(n, dtype=np.uint32)], 1)
    codes = np.stack([np.full(n, 4, np.uint8), np.ones(n, np.uint8)], 1)
    sf = S.SpatialFilter.from_polygons(polygons, exact=exact)
    out, keep, st = S.geom_refine(engine, sf.polygon_arrays(), np.zeros(0, S.GEOM_HEAD), heads, pairs, codes, (empty, ar),
                                  exact=sf.exact)
    assert (out[:, 0] == 4).all()
    assert np.array_equal(keep, np.nonzero((out[:, 1] >= 1) & (out[:, 1] <= 3))[0])
    assert sum(st.values()) == n
    return out[:, 1], st


def expect(polygons, geoms):
    E = X.ExactFilter(polygons)
    return np.array([2 if E.intersects(g) else 0 for g in geoms], np.uint8)


def moved(geom, f):
    """geom with every vertex (x, y) replaced by f(x, y)"""
    typ, data = geom
    if typ == X.POINT:
        return (typ, f(*data))
    if typ in (X.LINESTRING, X.MULTIPOINT):
        return (typ, [f(*p) for p in data])
    if typ in (X.POLYGON, X.MULTILINESTRING):
        return (typ, [[f(*p) for p in r] for r in data])
    return (typ, [[[f(*p) for p in r] for r in poly] for poly in data])


# ---------------------------------------------------------------------------------------------
# CPU: the Python surface
def test_exact_keyword_on_the_surface():
    sq = [[[(0, 0), (4, 0), (4, 3), (1, 5)]]]
    assert S.SpatialFilter.from_polygons(sq).exact is False and S.SpatialFilter.from_polygons(sq, exact=True).exact is True
    assert S.SpatialFilter.from_ring(sq[0][0], "geom", exact=True).exact
    assert S.SpatialFilter.from_wkt("POLYGON((0 0, 4 0, 1 5, 0 0))", exact=True).exact
    assert S.SpatialFilter((0, 1, 0, 1), exact=True).exact and not S.SpatialFilter((0, 1, 0, 1)).exact
    fx = load("repo_points")
    sf = S.SpatialFilter.from_polygons(sq, "geom", exact=True)
    assert sf.for_schema(fx.schema("head")).exact and not S.SpatialFilter.from_polygons(sq).for_schema(fx.schema("head")).exact
    import inspect

    from kart_amd.device import FilterPipeline

    assert inspect.signature(S.geom_refine).parameters["exact"].default is False
    assert inspect.signature(FilterPipeline.__init__).parameters["exact"].default is False


# ---------------------------------------------------------------------------------------------
# GPU 1, 2: the touching configurations and one-ulp near misses of test_gpu_refine_degenerate_never_false
SQ = [[[(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0), (0.0, 0.0)]]]
TRI = [[[(0.0, 0.0), (10.0, 0.0), (5.0, 10.0), (0.0, 0.0)]]]
TOUCHING = [
    (SQ, (X.POINT, (10.0, 10.0))), (SQ, (X.LINESTRING, [(10.0, 10.0), (20.0, 21.0)])),  # vertex on vertex
    (SQ, (X.POLYGON, [[(10.0, 10.0), (20.0, 10.5), (20.0, 20.0), (10.0, 10.0)]])),
    (SQ, (X.POLYGON, [[(10.0, 0.0), (20.0, 0.0), (20.0, 10.0), (10.0, 10.0), (10.0, 0.0)]])),  # shared edge
    (SQ, (X.POLYGON, [[(10.0, 2.0), (20.0, 2.0), (20.0, 8.0), (10.0, 8.0), (10.0, 2.0)]])),
    (SQ, (X.POINT, (10.0, 5.0))), (SQ, (X.MULTIPOINT, [(30.0, 30.0), (10.0, 5.0)])),  # point on an edge
    (SQ, (X.POINT, (5.0, 0.0))), (SQ, (X.POINT, (5.0, 10.0))), (SQ, (X.POINT, (0.0, 0.0))),  # ... a horizontal one
    (SQ, (X.LINESTRING, [(10.0, 2.0), (10.0, 8.0)])), (SQ, (X.LINESTRING, [(10.0, -5.0), (10.0, 5.0)])),  # collinear
    (SQ, (X.LINESTRING, [(-5.0, 10.0), (5.0, 10.0)])), (SQ, (X.LINESTRING, [(10.0, 5.0), (20.0, 5.0)])),
    (SQ, (X.LINESTRING, [(15.0, 0.0), (5.0, 20.0)])),  # through the corner (10, 10)
    (TRI, (X.POINT, (5.0, 10.0))), (TRI, (X.POINT, (10.0, 0.0))), (TRI, (X.POINT, (2.5, 5.0))),  # apex, corner, slanted edge
    (TRI, (X.LINESTRING, [(5.0, 10.0), (5.0, 20.0)])), (TRI, (X.POLYGON, [[(5.0, 10.0), (0.0, 20.0), (10.0, 20.0), (5.0, 10.0)]])),
    (TRI, (X.POLYGON, [[(-5.0, -5.0), (20.0, -5.0), (20.0, 20.0), (-5.0, 20.0), (-5.0, -5.0)],
                       [(0.0, 0.0), (10.0, 0.0), (5.0, 10.0), (0.0, 0.0)]])),  # the filter fills F's hole exactly
]
UP, DN = (lambda v: math.nextafter(v, math.inf)), (lambda v: math.nextafter(v, -math.inf))
NEAR = [
    (SQ, (X.POINT, (UP(10.0), 5.0))), (SQ, (X.POINT, (DN(10.0), 5.0))), (SQ, (X.POINT, (5.0, DN(0.0)))),
    (SQ, (X.POINT, (5.0, UP(0.0)))), (SQ, (X.POINT, (5.0, UP(10.0)))), (TRI, (X.POINT, (2.5, UP(5.0)))),
    (TRI, (X.POINT, (2.5, DN(5.0)))), (TRI, (X.POINT, (UP(7.5), 5.0))), (TRI, (X.POINT, (DN(7.5), 5.0))),
    (SQ, (X.LINESTRING, [(UP(10.0), 2.0), (UP(10.0), 8.0)])), (SQ, (X.LINESTRING, [(20.0, 5.0), (UP(10.0), 5.0)])),
    (TRI, (X.LINESTRING, [(UP(7.5), 5.0), (20.0, 6.0)])), (TRI, (X.LINESTRING, [(DN(7.5), 5.0), (20.0, 6.0)])),
    (SQ, (X.POLYGON, [[(UP(10.0), 0.0), (20.0, 0.0), (20.0, 10.0), (UP(10.0), 10.0), (UP(10.0), 0.0)]])),
]


@pytest.mark.gpu
@pytest.mark.parametrize("polys", [SQ, TRI], ids=["square", "triangle"])
def test_gpu_exact_touching_is_decided(engine, polys):
    """every touching configuration in all 8 encodings: 2 with exact, at least one left 1 without"""
    t = [g for p, g in TOUCHING if p is polys]
    assert expect(polys, t).tolist() == [2] * len(t)
    vals = [v for g in t for v in variants(g)]
    got, st = refine_sides(engine, polys, vals, True)
    assert got.tolist() == [2] * len(vals), np.nonzero(got != 2)[0]
    assert st == {"true": len(vals), "false": 0, "undecided": 0, "unsupported": 0}
    fast, fst = refine_sides(engine, polys, vals, False)
    assert (fast == 1).any() and fst["undecided"] == int((fast == 1).sum()) and fst["false"] == 0


@pytest.mark.gpu
def test_gpu_exact_near_misses(engine):
    """one ulp off the boundary: the code is the exact answer on every side, no 1 anywhere"""
    for polys in (SQ, TRI):
        nm = [g for p, g in NEAR if p is polys]
        want = expect(polys, nm)
        got, st = refine_sides(engine, polys, [X.gpkg_of(g) for g in nm], True)
        assert np.array_equal(got, want), (got, want)
        assert st["undecided"] == 0 and st["unsupported"] == 0
    assert 0 < sum(int((expect(p, [g for q, g in NEAR if q is p]) == 0).sum()) for p in (SQ, TRI)) < len(NEAR)


# ---------------------------------------------------------------------------------------------
# GPU 3: lattice storm
# (a frame one unit wide, where no lattice point is strictly inside, and a quadrilateral with slanted edges
# and lattice points strictly inside it, in the frame's hole)
LATTICE_FILTER = [[[(2, 2), (10, 2), (10, 10), (2, 10), (2, 2)], [(3, 3), (9, 3), (9, 9), (3, 9), (3, 3)]],
                  [[(5, 5), (7, 4), (8, 7), (5, 7), (5, 5)]]]


def lattice_geoms(rng, n, lo, hi):
    """n geometries of all six types with integer coordinates in [lo, hi]^2, each within 3 of a centre"""
    def pts(k, c):
        p = np.clip(c + rng.integers(-3, 4, (k, 2)), lo, hi)
        return [(float(x), float(y)) for x, y in p]

    out = []
    for _ in range(n):
        t = int(rng.integers(1, 7))
        c = rng.integers(lo, hi + 1, 2)
        if t == X.POINT:
            out.append((t, pts(1, c)[0]))
        elif t == X.MULTIPOINT:
            out.append((t, pts(int(rng.integers(1, 6)), c)))
        elif t == X.LINESTRING:
            out.append((t, pts(int(rng.integers(2, 7)), c)))
        elif t == X.MULTILINESTRING:
            out.append((t, [pts(int(rng.integers(2, 5)), c) for _ in range(int(rng.integers(1, 4)))]))
        elif t == X.POLYGON:
            r = pts(int(rng.integers(3, 7)), c)
            h = pts(3, c)
            out.append((t, [r + [r[0]]] + ([h + [h[0]]] if rng.random() < 0.3 else [])))
        else:
            polys = []
            for _ in range(int(rng.integers(1, 4))):
                r = pts(int(rng.integers(3, 6)), c)
                polys.append([r + [r[0]]])
            out.append((t, polys))
    return out


def scaled(x, y):
    return (x * 2.0 ** -10 + SHIFT[0], y * 2.0 ** -10 + SHIFT[1])


def lattice_case(seed, n, lo, hi, scale):
    """(filter, geometries, expected codes, the share of sides whose exact test met a zero determinant)"""
    geoms = lattice_geoms(np.random.default_rng(seed), n, lo, hi)
    filt = LATTICE_FILTER
    if scale:
        geoms = [moved(g, scaled) for g in geoms]
        filt = [[[scaled(*p) for p in r] for r in poly] for poly in filt]
    E = X.ExactFilter(filt)
    want, met = [], 0
    for g in geoms:
        z0 = X.ZEROS[0]
        want.append(2 if E.intersects(g) else 0)
        met += X.ZEROS[0] > z0
    return filt, geoms, np.array(want, np.uint8), met / n


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [False, True], ids=["integers", "scaled_shifted"])
def test_gpu_exact_lattice_storm(engine, scale):
    """2,000 lattice geometries against a lattice polygon with a hole (and a second polygon inside the
    hole): at least half of the sides meet an
    exactly zero determinant in the helper, and every one is decided as the helper decides"""
    filt, geoms, want, share = lattice_case(20261020, 2000, 0, 12, scale)
    assert share >= 0.5, share
    assert 200 < int((want == 0).sum()) and 200 < int((want == 2).sum())
    dims = list(X.DIMS)
    vals = [X.gpkg_of(g, dims[i % 4], i % 3 != 0, i % 5 != 0) for i, g in enumerate(geoms)]
    got, st = refine_sides(engine, filt, vals, True)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), geoms[i], int(got[i]), int(want[i])) for i in bad[:4]]
    assert st == {"true": int((want == 2).sum()), "false": int((want == 0).sum()), "undecided": 0, "unsupported": 0}


# ---------------------------------------------------------------------------------------------
# GPU 4: seams — a 130-vertex feature ring (three chunks of 63 segments) against a 300-vertex filter
# (299 edges: three tiles of 128)
def _grid(v):
    return round(v * 65536.0) / 65536.0


def half_disc(r):
    """the half disc x <= 0 of radius 8 as a closed 300-vertex ring whose straight edge (0, -8) -> (0, 8) is
    edge number r"""
    arc = [(_grid(8 * math.cos(a)), _grid(8 * math.sin(a)))
           for a in (math.pi / 2 + math.pi * (i + 1) / 298 for i in range(297))]
    p = [(0.0, -8.0), (0.0, 8.0)] + arc
    assert len(p) == 299 and all(x < 0 for x, _ in arc)
    p = p[299 - r:] + p[:299 - r] if r else p
    assert p[r] == (0.0, -8.0) and p[(r + 1) % 299] == (0.0, 8.0)
    return [[p + [p[0]]]]


def spiked_ring(k, x):
    """a closed 130-vertex ring around (4, 0), all of it at x >= 2 but vertex k = (x, 0.5)"""
    p = [(_grid(4 + 2 * math.cos(2 * math.pi * i / 129)), _grid(2 * math.sin(2 * math.pi * i / 129))) for i in range(129)]
    p[k] = (x, 0.5)
    return (X.POLYGON, [p + [p[0]]])


def open_ring(x):
    """130 distinct vertices, not closed in the WKB: v1 .. v128 on a circle around (0, 14), v0 = (-1, 9) and
    v129 = (x, 7) — with x = 1 the closing segment v129 -> v0 passes through the corner (0, 8) of the half disc"""
    mid = [(_grid(2 * math.cos(math.pi - math.pi * i / 127)), _grid(14 + 2 * math.sin(math.pi - math.pi * i / 127)))
           for i in range(128)]
    return (X.POLYGON, [[(-1.0, 9.0)] + mid + [(x, 7.0)]])


def far_points(n, last):
    return (X.MULTIPOINT, [(20.0 + i, 30.0) for i in range(n - 1)] + [last])


TINY = 2.0 ** -20


def seam_cases():
    """(name, filter, the geometry whose only contact with the filter is the named seam, the same a hair apart)"""
    out = []
    for k in (62, 63, 64):
        out.append(("vertex %d" % k, half_disc(5), spiked_ring(k, 0.0), spiked_ring(k, TINY)))
    out.append(("closing segment", half_disc(5), open_ring(1.0), open_ring(1.0 + TINY)))
    for r in (127, 128, 298):
        out.append(("filter edge %d" % r, half_disc(r), spiked_ring(10, 0.0), spiked_ring(10, TINY)))
    # the first vertex of a second filter ring (a small triangle inside the feature) on the feature's
    # boundary; and strictly inside it, where the boundaries are apart and rule (c) alone decides
    f0 = [(_grid(-30 + 9 * math.cos(2 * math.pi * i / 129)), _grid(30 + 9 * math.sin(2 * math.pi * i / 129))) for i in range(129)]
    feat = (X.POLYGON, [f0 + [f0[0]]])  # (130 vertices, far from the half disc)
    mid = ((f0[40][0] + f0[41][0]) / 2, (f0[40][1] + f0[41][1]) / 2)  # (on the grid of 2^-17: exact)
    assert mid[0] * 2 == f0[40][0] + f0[41][0] and mid[1] * 2 == f0[40][1] + f0[41][1]
    tri_on = [mid, (-30.0, 30.0), (-31.0, 30.0), mid]
    tri_in = [(-30.0, 31.0), (-30.0, 30.0), (-31.0, 30.0), (-30.0, 31.0)]
    out.append(("ring vertex on F", half_disc(5) + [[tri_on]], feat, None))
    out.append(("ring inside F", half_disc(5) + [[tri_in]], feat, None))
    for n in (64, 65):
        out.append(("multipoint %d" % n, half_disc(5), far_points(n, (0.0, 0.5)), far_points(n, (TINY, 0.5))))
    return out


@pytest.mark.gpu
def test_gpu_exact_seams(engine):
    for name, filt, touch, apart in seam_cases():
        E = X.ExactFilter(filt)
        assert E.intersects(touch), name
        geoms = [touch]
        if apart is not None:
            assert not E.intersects(apart), name  # (so the named contact is the only one)
            geoms.append(apart)
        want = expect(filt, geoms)
        got, st = refine_sides(engine, filt, [X.gpkg_of(g) for g in geoms], True)
        assert got.tolist() == want.tolist(), (name, got, want)
        assert st["undecided"] == 0 and st["unsupported"] == 0, (name, st)


# ---------------------------------------------------------------------------------------------
# GPU 5: outside the range guard a side is 1 or right, and counted undecided
@pytest.mark.gpu
@pytest.mark.parametrize("s", [1e-310, 1e-200, 1e200, 1e300])
def test_gpu_exact_range_guard(engine, s):
    sq = [[[(0.0, 0.0), (s, 0.0), (s, s), (0.0, s), (0.0, 0.0)]]]
    tri = [[[(0.0, 0.0), (s, 0.0), (0.5 * s, s), (0.0, 0.0)]]]
    for polys in (sq, tri):
        geoms = [(X.POINT, (s, 0.5 * s)), (X.POINT, (0.25 * s, 0.5 * s)), (X.POINT, (0.5 * s, 0.5 * s)),
                 (X.POINT, (1.5 * s, 0.5 * s)), (X.POINT, (0.125 * s, 0.5 * s)),
                 (X.LINESTRING, [(s, s), (1.5 * s, 1.75 * s)]), (X.LINESTRING, [(0.5 * s, s), (0.5 * s, 1.5 * s)]),
                 (X.LINESTRING, [(1.25 * s, 0.0), (1.5 * s, s)]), (X.LINESTRING, [(-0.5 * s, 0.5 * s), (1.5 * s, 0.75 * s)]),
                 (X.POLYGON, [[(s, 0.0), (2 * s, 0.0), (2 * s, s), (s, s), (s, 0.0)]]),
                 (X.POLYGON, [[(1.25 * s, 0.0), (2 * s, 0.0), (2 * s, s), (1.25 * s, 0.0)]]),
                 (X.MULTIPOINT, [(1.5 * s, 1.5 * s), (0.5 * s, 0.0)])]
        want = expect(polys, geoms)
        assert 0 < int((want == 0).sum()) < len(geoms)
        got, st = refine_sides(engine, polys, [X.gpkg_of(g) for g in geoms], True)
        for g, c, w in zip(geoms, got.tolist(), want.tolist()):
            assert c == 1 or c == w, (g, c, w)
        assert st["unsupported"] == 0 and st["undecided"] == int((got == 1).sum())
        assert st["true"] == int((got == 2).sum()) and st["false"] == int((got == 0).sum())


# ---------------------------------------------------------------------------------------------
# GPU 6: refusals unchanged
@pytest.mark.gpu
def test_gpu_exact_refusals_stay_candidates(engine):
    from test_geom_refine import DONUT

    pt = struct.pack("<BIdd", 1, 1, 75.0, 50.0)
    env = (70.0, 80.0, 45.0, 55.0)
    refused = [
        X.gpkg(struct.pack("<BII", 1, 7, 1) + pt, env),                                   # GeometryCollection
        X.gpkg(struct.pack("<BII", 1, 8, 3) + struct.pack("<6d", 74, 50, 75, 51, 76, 50), env),  # CircularString
        X.gpkg(struct.pack("<BI", 1, 0x20000001) + struct.pack("<Idd", 4326, 75.0, 50.0), env),  # EWKB: SRID flag
        X.gpkg(struct.pack("<BI", 1, 0x80000001) + struct.pack("<ddd", 75.0, 50.0, 1.0), env),   # EWKB: Z flag
        X.gpkg(struct.pack("<BIII", 1, 3, 1, 1000) + struct.pack("<8d", 74, 49, 76, 49, 75, 51, 74, 49), env),  # ring count past glen
        X.gpkg(struct.pack("<BII", 1, 3, 0xFFFFFFFF), env),                               # ring number past glen
        X.gpkg(struct.pack("<BII", 1, 2, 0x10000001) + struct.pack("<4d", 74, 49, 76, 51), env),  # count * stride wraps 32 bits
        X.gpkg(struct.pack("<BII", 1, 2, 3) + struct.pack("<6d", 74, 49, float("nan"), 50, 76, 51), env),  # NaN coordinate
        X.gpkg(struct.pack("<BII", 1, 4, 2) + pt + struct.pack("<BIdd", 1, 1, 75.0, float("inf")), env),  # inf in a multipoint
        X.gpkg(struct.pack("<BII", 1, 4, 2) + pt + struct.pack("<BII", 1, 2, 0), env),    # a linestring inside a multipoint
        X.gpkg(struct.pack("<BII", 1, 5, 2) + struct.pack("<BII", 1, 2, 2) + struct.pack("<4d", 74, 49, 76, 51), env),  # missing part
        X.gpkg(struct.pack("<BI", 1, 4001) + struct.pack("<dd", 75.0, 50.0), env),       # dimension code 4
        X.gpkg(struct.pack("<BI", 2, 1) + struct.pack("<dd", 75.0, 50.0), env),          # byte order 2
        X.gpkg(b"\x01\x02\x00", env),                                                     # truncated header
    ]
    good = [X.gpkg_of((X.POINT, (75.0, 50.0))), X.gpkg_of((X.LINESTRING, [(74.0, 49.0), (76.0, 51.0)])),
            X.gpkg_of((X.POINT, (50.0, 50.0)))]
    got, st = refine_sides(engine, DONUT, refused + good, True)
    assert got[:len(refused)].tolist() == [1] * len(refused)
    assert got[len(refused):].tolist() == [2, 2, 0]
    assert st == {"true": 2, "false": 1, "undecided": 0, "unsupported": len(refused)}


# ---------------------------------------------------------------------------------------------
# GPU 7: lists and layouts — ~5,000 deltas (two k_gr_list blocks) through the host entry and the pipeline
def lattice_layer(seed, n_pks):
    """a layer of lattice geometries: pk p is an insert, a delete or an update by p's draw; both sides in
    key order with one blob per entry.  Returns (Layer-like namespace, old geometries by base entry, new
    geometries by target entry)"""
    rng = np.random.default_rng(seed)
    allp = walkkey.walk_order_pks(n_pks, 0, 1 << 24)
    kind = rng.integers(0, 3, allp.shape[0])  # 0 insert, 1 delete, 2 update
    in_b, in_t = kind != 0, kind != 1
    og = lattice_geoms(rng, int(in_b.sum()), 0, 16)
    ng = lattice_geoms(rng, int(in_t.sum()), 0, 16)
    pb, pt = allp[in_b], allp[in_t]
    base = packing.PackedSide(key=walkkey.int_keys(pb), oid=synth.synth_oids(pb, np.zeros(pb.shape[0], np.uint64)), key_mode=0,
                              order=np.arange(pb.shape[0], dtype=np.int64), encoding=packing.INT_PK_ENCODING)
    target = packing.PackedSide(key=walkkey.int_keys(pt), oid=synth.synth_oids(pt, np.ones(pt.shape[0], np.uint64)), key_mode=0,
                                order=np.arange(pt.shape[0], dtype=np.int64), encoding=packing.INT_PK_ENCODING)
    dims = list(X.DIMS)
    bb = arena_of([X.gpkg_of(g, dims[i % 4], i % 3 != 0, i % 5 != 0) for i, g in enumerate(og)])
    tb = arena_of([X.gpkg_of(g, dims[i % 4], i % 2 != 0, i % 7 != 0) for i, g in enumerate(ng)])
    return types.SimpleNamespace(base=base, target=target, base_blobs=bb, target_blobs=tb), og, ng


@pytest.mark.gpu
def test_gpu_exact_lists_and_layouts(engine):
    from kart_amd.device import FilterPipeline

    L, og, ng = lattice_layer(5, 5000)
    ver = types.SimpleNamespace(schema=types.SimpleNamespace(columns=[types.SimpleNamespace(name="geom", id="g")]),
                                legends={HEX: LEGEND})
    gc = S.GeomCols(ver, ver, "geom", "geom")
    sf = S.SpatialFilter.from_polygons(LATTICE_FILTER, exact=True)
    arr = sf.polygon_arrays()
    pipe = FilterPipeline(engine, L.base, L.target, L.base_blobs, L.target_blobs, gc, sf.filter_env, False, 20, heads=True,
                          delta_order=True, polygons=sf, exact=True)
    pipe.step()
    first = pipe.results(), pipe.refine_stats()
    pipe.step()  # (the same step again: the workspaces are there, the outcome is the same)
    counts, delta, codes, keep, _, _ = pipe.results()
    st = pipe.refine_stats()
    assert np.array_equal(first[0][2], codes) and np.array_equal(first[0][3], keep) and first[1] == st
    n = delta.shape[0]
    assert n > 4096 and counts["deltas"] == n
    # the envelope stage alone gives the preset codes (non-candidates among them)
    heads = pipe.heads_host
    preset, _, _, _ = S.geom_filter_heads(engine, heads[0], heads[1], delta, sf.filter_env, False,
                                          arenas=(L.base_blobs, L.target_blobs))
    cand = preset == 1
    assert (preset == 0).any() and (preset == 4).any() and int(cand.sum()) > 2000
    E = X.ExactFilter(LATTICE_FILTER)
    want = preset.copy()
    for d, s in np.argwhere(cand):
        g = (ng if s else og)[int(delta[d, s])]
        want[d, s] = 2 if E.intersects(g) else 0
    assert np.array_equal(codes, want), np.argwhere(codes != want)[:8]
    kept = ((codes >= 1) & (codes <= 3)).any(1)
    assert np.array_equal(keep, np.nonzero(kept)[0]) and counts["kept"] == int(kept.sum())
    assert sum(st.values()) == int(cand.sum()) and st["undecided"] == 0 and st["unsupported"] == 0
    assert st["true"] == int((want[cand] == 2).sum())
    # the host entry over the same deltas and codes: heads indexed by the pairs, then in delta order
    arenas = (L.base_blobs, L.target_blobs)
    hc, hk, hst = S.geom_refine(engine, arr, heads[0], heads[1], delta, preset, arenas, exact=True)
    again = S.geom_refine(engine, arr, heads[0], heads[1], delta, preset, arenas, exact=True)
    assert np.array_equal(hc, again[0]) and np.array_equal(hk, again[1]) and hst == again[2]
    assert np.array_equal(hc, codes) and np.array_equal(hk, keep) and hst == st
    slots = (n + 63) // 64 * 64
    dense = []
    for s in range(2):
        h = np.zeros(slots, S.GEOM_HEAD)
        pres = np.nonzero(delta[:, s] != NONE)[0]
        h[pres] = heads[s][delta[pres, s].astype(np.int64)]
        dense.append(h)
    dc, dk, dst = S.geom_refine(engine, arr, dense[0], dense[1], delta, preset, arenas, delta_heads=True, exact=True)
    assert np.array_equal(dc, codes) and np.array_equal(dk, keep) and dst == st
    # without the flag the same call leaves sides undecided, and decides no side differently
    fc, _, fst = S.geom_refine(engine, arr, heads[0], heads[1], delta, preset, arenas)
    assert fst["undecided"] > 0 and np.array_equal(fc[fc != 1], codes[fc != 1])


# ---------------------------------------------------------------------------------------------
# GPU 8: the drop-in
@pytest.mark.gpu
def test_gpu_exact_filtered_diff_ring_through_features(engine):
    """a filter ring with six HEAD features of `points` among its vertices: with exact=True and no
    intersects callable the drop-in yields exactly the helper's keys and verifies every one on the device"""
    f = FILTERS["points"]
    fx = load(f["fixture"])
    head = version(fx, f["side"])
    geoms = [X.parse_gpkg(g) for g in _head_geometries("points")]
    assert all(g[0] == X.POINT for g in geoms)
    xy = np.array([g[1] for g in geoms])
    c = np.median(xy, 0)
    near = np.argsort(np.hypot(*(xy - c).T))
    pick = xy[near[[40, 80, 120, 160, 200, 240]]]
    assert len({tuple(p) for p in pick}) == 6
    # a star around the picked features' centroid: they are its inner vertices, in order of angle, and
    # between two of them an outer vertex that is no feature — so the filter's envelope, which the
    # reference's quick check treats as open at a point (bbox_intersects_fast), passes through no feature
    cx, cy = pick[:, 0].mean(), pick[:, 1].mean()
    ang = np.arctan2(pick[:, 1] - cy, pick[:, 0] - cx)
    order = np.argsort(ang)
    rout = 1.5 * float(np.hypot(pick[:, 0] - cx, pick[:, 1] - cy).max())
    star = []
    for j, i in enumerate(order):
        a0 = float(ang[i])
        a1 = float(ang[order[(j + 1) % 6]]) + (2 * math.pi if j == 5 else 0.0)
        star += [tuple(float(v) for v in pick[i]), (cx + rout * math.cos((a0 + a1) / 2), cy + rout * math.sin((a0 + a1) / 2))]
    polys = [[star]]
    env = S.SpatialFilter.from_polygons(polys).filter_env
    E = X.ExactFilter(S.SpatialFilter.from_polygons(polys).polygons)
    inside = [E.intersects(g) for g in geoms]
    assert all(S.bbox_intersects_fast(env, (g[1][0], g[1][0], g[1][1], g[1][1])) for g, w in zip(geoms, inside) if w)
    on_ring = sum(tuple(g[1]) in {tuple(p) for p in pick} for g in geoms)
    assert on_ring >= 6 and on_ring < sum(inside) < len(geoms)
    names = fx.names(f["side"])
    want = sorted(head.decode_path_to_1pk(nm) for nm, w in zip(names, inside) if w)
    ds = D.get_dataset_diff(engine, None, head)
    sf = S.SpatialFilter.from_polygons(polys, exact=True)
    assert sf.intersects is None and not sf.rectangle
    got = list(S.filtered_ds_feature_deltas(engine, ds, None, head, sf))
    assert sorted(k for k, _ in got) == want
    assert sf.stats["unverified"] == 0 and sf.stats["refine"]["undecided"] == 0
    loose = S.SpatialFilter.from_polygons(polys)
    more = list(S.filtered_ds_feature_deltas(engine, ds, None, head, loose))
    assert loose.stats["unverified"] > 0 and loose.stats["refine"]["undecided"] >= 6
    assert sorted(k for k, _ in more) == want  # (unverified sides count as matching, and these do match)
