"""kd_geom_refine: the exact stage of the spatially filtered diff — Intersects(feature, filter polygon)
decided on the GPU wherever FP64 certifies the answer, everything else left 1 CANDIDATE.

Reference numbers: the reference's own `points` and `polygons` filter geometries and the feature
counts its checkout expects with them (tests/test_spatial_filter.py:128-170, 600-603), held in
tests/golden/spatial_filter_polygons.json.  Every device decision is compared with refine_exact.py
(Intersects in rational arithmetic, touching included)."""
import ctypes
import json
import math
import os
import struct

import msgpack
import numpy as np
import pytest

import refine_exact as X
from fixtures import GOLDEN, load
from kart_amd import _native as N
from kart_amd import dataset as D
from kart_amd import spatial as S
from kart_amd.schema import Legend
from test_dropin import version

NONE = N.KD_NONE
LEGEND = Legend(["pk"], ["g", "a"])
HEX = LEGEND.hexhash()
HEXARR = np.frombuffer(HEX.encode("ascii"), np.uint8).copy()
GIDX = np.zeros(1, np.int16)

with open(os.path.join(GOLDEN, "spatial_filter_polygons.json")) as _f:
    FILTERS = json.load(_f)["filters"]


def ring(cx, cy, r, n, phase=0.1, r2=None):
    """a closed n-gon (or, with r2, a star alternating between the two radii) around (cx, cy)"""
    pts = []
    for k in range(n):
        rr = r if r2 is None or k % 2 == 0 else r2
        a = phase + 2 * math.pi * k / n
        pts.append((cx + rr * math.cos(a), cy + rr * math.sin(a)))
    return pts + [pts[0]]


def arena_of(gpkgs):
    """(data, off) of feature blobs [legend, [geometry, 1]] around the GPKG values (None: a null blob slot)"""
    blobs = [msgpack.packb([HEX, [msgpack.ExtType(ord("G"), g), 1]], use_bin_type=True) if g is not None else b""
             for g in gpkgs]
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return np.frombuffer(b"".join(blobs) or b"\x00", np.uint8).copy()[:int(off[-1])], off


def refine_new(engine, polygons, gpkgs):
    """the GPKG values as the new sides of inserts, every one a candidate: (codes of the new sides, stats)"""
    n = len(gpkgs)
    ar = arena_of(gpkgs)
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    heads = S.geom_heads(*ar, HEXARR, GIDX, 1)
    pairs = np.stack([np.full(n, NONE, np.uint32), np.arange(n, dtype=np.uint32)], 1)
    codes = np.stack([np.full(n, 4, np.uint8), np.ones(n, np.uint8)], 1)
    sf = S.SpatialFilter.from_polygons(polygons)
    out, keep, st = S.geom_refine(engine, sf.polygon_arrays(), np.zeros(0, S.GEOM_HEAD), heads, pairs, codes,
                                  (empty, ar))
    assert (out[:, 0] == 4).all()
    assert np.array_equal(keep, np.nonzero((out[:, 1] >= 1) & (out[:, 1] <= 3))[0])
    return out[:, 1], st


# ---------------------------------------------------------------------------------------------
# CPU: the exact helper pins the reference's numbers; the Python surface and the binding
def _head_geometries(name):
    f = FILTERS[name]
    fx = load(f["fixture"])
    gcol = fx.schema(f["side"]).geometry_columns[0].id
    out = []
    for b in fx.a[f["side"] + "_blob"]:
        hexh, vals = msgpack.unpackb(fx.blob(int(b)), raw=False)
        out.append(bytes(vals[list(fx.legends[hexh].non_pk_columns).index(gcol)].data))
    return out


@pytest.mark.parametrize("name", ["points", "polygons"])
def test_exact_helper_reference_counts(name):
    """302 of points' 2,143 HEAD features and 44 of polygons' 228 intersect the reference's filters"""
    f = FILTERS[name]
    E = X.ExactFilter(f["polygons"])
    geoms = _head_geometries(name)
    assert len(geoms) == f["features"]
    assert sum(E.intersects(X.parse_gpkg(g)) for g in geoms) == f["matching"]


def test_exact_helper_basics():
    E = X.ExactFilter([[[(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)], [(4, 4), (6, 4), (6, 6), (4, 6), (4, 4)]]])
    assert E.intersects((X.POINT, (1, 1))) and E.intersects((X.POINT, (10, 5))) and E.intersects((X.POINT, (4, 5)))
    assert not E.intersects((X.POINT, (5, 5))) and not E.intersects((X.POINT, (11, 5)))
    assert E.intersects((X.LINESTRING, [(-5, 5), (15, 5.5)]))  # crosses, no vertex inside
    assert not E.intersects((X.POLYGON, [[(4.5, 4.5), (5.5, 4.5), (5, 5.5), (4.5, 4.5)]]))  # inside the hole
    assert E.intersects((X.POLYGON, [[(-5, -5), (20, -5), (20, 20), (-5, 20), (-5, -5)]]))  # the filter inside it
    assert not E.intersects((X.POLYGON, [[(-9, -9), (30, -9), (30, 30), (-9, 30), (-9, -9)],
                                         [(-5, -5), (20, -5), (20, 20), (-5, 20), (-5, -5)]]))  # ... inside its hole
    g = (X.MULTIPOLYGON, [[ring(1, 2, 3, 5)], [ring(7, 7, 1, 4), ring(7, 7, 0.5, 3)]])
    for dim in X.DIMS:
        for le in (True, False):
            assert X.parse_gpkg(X.gpkg_of(g, dim, le, not le)) == g


def test_from_polygons_and_wkt():
    pts = FILTERS["points"]["polygons"]
    sf = S.SpatialFilter.from_polygons(pts, "geom")
    xs, ys = [p[0] for p in pts[0][0]], [p[1] for p in pts[0][0]]
    assert sf.filter_env == (min(xs), max(xs), min(ys), max(ys)) and not sf.rectangle and sf.intersects is None
    assert sf.polygons == [[[tuple(p) for p in pts[0][0]]]]
    wkt = "MULTIPOLYGON(((" + ",".join("%r %r" % tuple(p) for p in pts[0][0]) + ")))"
    assert S.SpatialFilter.from_wkt(wkt).polygons == sf.polygons
    # an open ring is closed; a ring that is its envelope's corners is a rectangle
    assert S.SpatialFilter.from_polygons([[[(0, 0), (4, 0), (4, 2), (0, 2)]]]).rectangle
    assert S.SpatialFilter.from_wkt("POLYGON((0 0, 4 0, 4 2, 0 2, 0 0))").rectangle
    # a multipolygon with a hole
    mp = S.SpatialFilter.from_wkt("multipolygon (((0 0, 10 0, 10 10, 0 10, 0 0), (4 4, 6 4, 6 6, 4 4)), "
                                  "((20 20, 30 20, 25 3e1, 20 20)))", "geom")
    assert [len(p) for p in mp.polygons] == [2, 1] and mp.filter_env == (0.0, 30.0, 0.0, 30.0) and not mp.rectangle
    xy, off = mp.polygon_arrays()
    assert off.tolist() == [0, 5, 9, 13] and xy.shape == (13, 2) and xy.dtype == np.float64
    for bad in ("POINT(1 2)", "LINESTRING(0 0, 1 1)", "POLYGON EMPTY", "GEOMETRYCOLLECTION(POLYGON((0 0,1 0,1 1,0 0)))",
                "POLYGON((0 0, 1 0, 1 1, 0 0)"):
        with pytest.raises(ValueError):
            S.SpatialFilter.from_wkt(bad)
    # from_ring records its ring; for_schema carries the polygons (and the arrays' address)
    tri = S.SpatialFilter.from_ring([(0, 0), (10, 0), (0, 10), (0, 0)], "geom")
    assert tri.polygons == [[[(0.0, 0.0), (10.0, 0.0), (0.0, 10.0), (0.0, 0.0)]]] and tri.intersects is not None
    fx = load("repo_points")
    out = mp.for_schema(fx.schema("head"))
    assert out.polygons == mp.polygons and out.geom_column_name == "geom" and out.polygon_arrays()[0] is xy
    assert S.SpatialFilter.from_rectangle(0, 1, 0, 1).polygons is None


def test_binding_lists_refine():
    assert "kd_geom_refine" in N.SIGNATURES and hasattr(N.lib(), "kd_geom_refine")
    assert ctypes.sizeof(N.KdFilterPoly) == 32


def test_filter_pipeline_polygons_need_heads():
    from kart_amd.device import FilterPipeline

    with pytest.raises(ValueError):
        FilterPipeline(None, None, None, None, None, None, (0, 1, 0, 1), polygons=[[ring(0, 0, 1, 5)]])


# ---------------------------------------------------------------------------------------------
# GPU, crafted
DONUT = [[ring(50, 50, 50, 8, 0.2), ring(50, 50, 12, 7, 0.3)]]  # an octagon with a hole
BAR = [[[(0.0, 48.0), (100.0, 49.5), (100.3, 51.5), (0.2, 50.1), (0.0, 48.0)]]]  # long and thin


def shapes(cx, cy, r):
    """one geometry of every type within r of (cx, cy)"""
    return [
        (X.POINT, (cx + 0.1 * r, cy - 0.2 * r)),
        (X.LINESTRING, [(cx - 0.9 * r, cy - 0.3 * r), (cx + 0.2 * r, cy + 0.7 * r), (cx + 0.8 * r, cy - 0.5 * r)]),
        (X.POLYGON, [ring(cx, cy, 0.95 * r, 6, 0.4), ring(cx, cy, 0.3 * r, 4, 0.1)]),
        (X.MULTIPOINT, [(cx - 0.5 * r, cy + 0.1 * r), (cx + 0.3 * r, cy + 0.6 * r), (cx, cy - 0.8 * r)]),
        (X.MULTILINESTRING, [[(cx - 0.8 * r, cy), (cx - 0.1 * r, cy + 0.5 * r)], [(cx + 0.1 * r, cy - 0.6 * r), (cx + 0.7 * r, cy + 0.2 * r)]]),
        (X.MULTIPOLYGON, [[ring(cx - 0.5 * r, cy, 0.4 * r, 5, 0.2)], [ring(cx + 0.5 * r, cy, 0.4 * r, 3, 0.5)]]),
    ]


def variants(geom):
    """the GPKG value of geom in XY / Z / M / ZM, little and big endian (the parts of a multi-geometry
    in the other byte order for half of them)"""
    return [X.gpkg_of(geom, dim, le, (not le) if i % 2 else le) for i, dim in enumerate(X.DIMS) for le in (True, False)]


def check_exact(engine, polygons, geoms):
    """every geometry in all 8 encodings: the device's code is exactly the helper's answer"""
    E = X.ExactFilter(polygons)
    want, vals = [], []
    for g in geoms:
        w = E.intersects(g)
        for v in variants(g):
            want.append(2 if w else 0)
            vals.append(v)
    got, st = refine_new(engine, polygons, vals)
    bad = np.nonzero(got != np.array(want, np.uint8))[0]
    assert bad.size == 0, [(int(i), geoms[i // 8][0], int(got[i]), want[i]) for i in bad[:8]]
    assert st == {"true": want.count(2), "false": want.count(0), "undecided": 0, "unsupported": 0}
    return want


@pytest.mark.gpu
def test_gpu_refine_crafted_types_and_encodings(engine):
    far = [(X.MULTIPOINT, [(200.0, 200.0), (-50.0, 3.0), (75.0, 50.5)]),
           (X.MULTILINESTRING, [[(200.0, 200.0), (210.0, 205.0)], [(70.0, 49.0), (72.0, 51.0)]]),
           (X.MULTIPOLYGON, [[ring(-80, 50, 5, 4)], [ring(300, 300, 9, 5)], [ring(75, 50, 2, 5)]]),
           (X.MULTIPOLYGON, [[ring(-80 - 20 * i, 50, 5, 4), ring(-80 - 20 * i, 50, 2, 3)] for i in range(4)] + [[ring(75, 50, 2, 5)]]),
           (X.MULTILINESTRING, [[(200.0 + i, 200.0), (210.0, 205.0 + i)] for i in range(7)] + [[(70.0, 49.0), (72.0, 51.0)]])]
    big = [(X.POLYGON, [ring(50, 50, 200, 9, 0.7)]),
           (X.MULTIPOLYGON, [[ring(-500, 0, 30, 4)], [ring(50, 50, 180, 11, 0.1)]])]
    holed = [(X.POLYGON, [ring(50, 50, 300, 9, 0.7), ring(50, 50, 150, 7, 0.2)]),
             (X.MULTIPOLYGON, [[ring(50, 50, 300, 9, 0.7), ring(50, 50, 150, 7, 0.2)], [ring(900, 0, 30, 4)]])]
    geoms = (shapes(75, 50, 5)        # F inside P
             + big                    # P inside F
             + shapes(50, 50, 6)      # F inside P's hole
             + holed                  # P inside F's hole
             + shapes(93, 93, 4)      # the boxes overlap, the geometries do not (beyond the octagon's corner)
             + far)                   # a multipart whose last part alone hits
    want = check_exact(engine, DONUT, geoms)
    assert want.count(2) == 8 * (6 + 2 + 5) and want.count(0) == 8 * (6 + 2 + 6)
    # edges cross with no vertex of either inside the other: a plus sign over the thin bar
    plus = [(X.LINESTRING, [(50.0, 30.0), (50.5, 70.0)]),
            (X.MULTILINESTRING, [[(150.0, 0.0), (160.0, 5.0)], [(20.0, 40.0), (20.5, 60.0)]]),
            (X.POLYGON, [[(60.0, 30.0), (61.0, 30.0), (61.5, 70.0), (60.5, 70.0), (60.0, 30.0)]]),
            (X.MULTIPOLYGON, [[ring(50, 10, 5, 4)], [[(80.0, 30.0), (81.0, 30.0), (81.5, 70.0), (80.5, 70.0), (80.0, 30.0)]]])]
    E = X.ExactFilter(BAR)
    for g in plus:
        assert not any(E.E.contains(p) for p in X.vertices(g))
    assert check_exact(engine, BAR, plus).count(2) == 32


@pytest.mark.gpu
def test_gpu_refine_long_ring_and_large_filter(engine):
    """a 300-vertex feature ring (several vertex chunks) and a 5,000-vertex filter (several LDS tiles)"""
    long_ = [(X.POLYGON, [ring(75, 50, 5, 300)]), (X.POLYGON, [ring(50, 50, 8, 300)]), (X.POLYGON, [ring(50, 50, 60, 300)]),
             (X.POLYGON, [ring(50, 50, 30, 300, 0.0, 5)]), (X.LINESTRING, ring(50, 50, 11, 300)[:-1]),
             (X.LINESTRING, ring(50, 50, 14, 300, 0.0, 9)[:-7]), (X.MULTIPOLYGON, [[ring(93, 93, 4, 300)], [ring(50, 50, 9, 300)]])]
    want = check_exact(engine, DONUT, long_)
    assert 0 < want.count(2) < len(want)
    star = [[ring(50, 50, 50, 4999, 0.05, 40)]]  # 5,000 vertices: ten tiles of 512 edges
    assert len(star[0][0]) == 5000
    geoms = shapes(50, 50, 20) + shapes(50, 92, 3) + shapes(96, 96, 3) + [(X.POLYGON, [ring(50, 50, 70, 12)]),
                                                                         (X.POLYGON, [ring(50, 50, 45, 300)])]
    want = check_exact(engine, star, geoms)
    assert 0 < want.count(2) < len(want)


@pytest.mark.gpu
def test_gpu_refine_degenerate_never_false(engine):
    """touching configurations are true in exact arithmetic: the device may say 2 or leave 1, never 0;
    a near miss of one ulp is 1 or the exact answer"""
    sq = [[[(0.0, 0.0), (10.0, 0.0), (10.0, 10.0), (0.0, 10.0), (0.0, 0.0)]]]
    tri = [[[(0.0, 0.0), (10.0, 0.0), (5.0, 10.0), (0.0, 0.0)]]]
    touching = [
        (sq, (X.POINT, (10.0, 10.0))), (sq, (X.LINESTRING, [(10.0, 10.0), (20.0, 21.0)])),  # vertex on vertex
        (sq, (X.POLYGON, [[(10.0, 10.0), (20.0, 10.5), (20.0, 20.0), (10.0, 10.0)]])),
        (sq, (X.POLYGON, [[(10.0, 0.0), (20.0, 0.0), (20.0, 10.0), (10.0, 10.0), (10.0, 0.0)]])),  # shared edge
        (sq, (X.POLYGON, [[(10.0, 2.0), (20.0, 2.0), (20.0, 8.0), (10.0, 8.0), (10.0, 2.0)]])),
        (sq, (X.POINT, (10.0, 5.0))), (sq, (X.MULTIPOINT, [(30.0, 30.0), (10.0, 5.0)])),  # point on an edge
        (sq, (X.POINT, (5.0, 0.0))), (sq, (X.POINT, (5.0, 10.0))), (sq, (X.POINT, (0.0, 0.0))),  # ... a horizontal one
        (sq, (X.LINESTRING, [(10.0, 2.0), (10.0, 8.0)])), (sq, (X.LINESTRING, [(10.0, -5.0), (10.0, 5.0)])),  # collinear
        (sq, (X.LINESTRING, [(-5.0, 10.0), (5.0, 10.0)])), (sq, (X.LINESTRING, [(10.0, 5.0), (20.0, 5.0)])),
        (sq, (X.LINESTRING, [(15.0, 0.0), (5.0, 20.0)])),  # through the corner (10, 10)
        (tri, (X.POINT, (5.0, 10.0))), (tri, (X.POINT, (10.0, 0.0))), (tri, (X.POINT, (2.5, 5.0))),  # apex, corner, slanted edge
        (tri, (X.LINESTRING, [(5.0, 10.0), (5.0, 20.0)])), (tri, (X.POLYGON, [[(5.0, 10.0), (0.0, 20.0), (10.0, 20.0), (5.0, 10.0)]])),
        (tri, (X.POLYGON, [[(-5.0, -5.0), (20.0, -5.0), (20.0, 20.0), (-5.0, 20.0), (-5.0, -5.0)],
                           [(0.0, 0.0), (10.0, 0.0), (5.0, 10.0), (0.0, 0.0)]])),  # the filter fills F's hole exactly
    ]
    up, dn = lambda v: math.nextafter(v, math.inf), lambda v: math.nextafter(v, -math.inf)
    near = [
        (sq, (X.POINT, (up(10.0), 5.0))), (sq, (X.POINT, (dn(10.0), 5.0))), (sq, (X.POINT, (5.0, dn(0.0)))),
        (sq, (X.POINT, (5.0, up(0.0)))), (sq, (X.POINT, (5.0, up(10.0)))), (tri, (X.POINT, (2.5, up(5.0)))),
        (tri, (X.POINT, (2.5, dn(5.0)))), (tri, (X.POINT, (up(7.5), 5.0))), (tri, (X.POINT, (dn(7.5), 5.0))),
        (sq, (X.LINESTRING, [(up(10.0), 2.0), (up(10.0), 8.0)])), (sq, (X.LINESTRING, [(20.0, 5.0), (up(10.0), 5.0)])),
        (tri, (X.LINESTRING, [(up(7.5), 5.0), (20.0, 6.0)])), (tri, (X.LINESTRING, [(dn(7.5), 5.0), (20.0, 6.0)])),
        (sq, (X.POLYGON, [[(up(10.0), 0.0), (20.0, 0.0), (20.0, 10.0), (up(10.0), 10.0), (up(10.0), 0.0)]])),
    ]
    for polys in (sq, tri):
        E = X.ExactFilter(polys)
        t = [g for p, g in touching if p is polys]
        assert all(E.intersects(g) for g in t)
        got, st = refine_new(engine, polys, [X.gpkg_of(g) for g in t])
        assert set(got.tolist()) <= {1, 2}, got
        assert st["false"] == 0 and st["unsupported"] == 0
        nm = [g for p, g in near if p is polys]
        got, st = refine_new(engine, polys, [X.gpkg_of(g) for g in nm])
        for g, c in zip(nm, got.tolist()):
            assert c == 1 or c == (2 if E.intersects(g) else 0), (g, c)


@pytest.mark.gpu
def test_gpu_refine_refusals_stay_candidates(engine):
    """unsupported or malformed WKB stays 1 and is counted"""
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
    got, st = refine_new(engine, DONUT, refused + good)
    assert got[:len(refused)].tolist() == [1] * len(refused)
    assert got[len(refused):].tolist() == [2, 2, 0]
    assert st == {"true": 2, "false": 1, "undecided": 0, "unsupported": len(refused)}


def _random_geoms(rng, n, lo, hi):
    def pt():
        return (float(rng.uniform(lo, hi)), float(rng.uniform(lo, hi)))

    def star(c, r, k):
        ang = np.sort(rng.uniform(0, 2 * math.pi, k))
        rad = rng.uniform(0.3 * r, r, k)
        p = [(c[0] + float(a) * 0 + float(q * math.cos(a)), c[1] + float(q * math.sin(a))) for a, q in zip(ang, rad)]
        return p + [p[0]]

    out = []
    for _ in range(n):
        t = int(rng.integers(1, 7))
        k = int(rng.integers(3, 41))
        r = float(rng.uniform(0.5, 25))
        if t == X.POINT:
            out.append((t, pt()))
        elif t == X.MULTIPOINT:
            out.append((t, [pt() for _ in range(int(rng.integers(1, 6)))]))
        elif t == X.LINESTRING:
            out.append((t, star(pt(), r, k)[:-1]))
        elif t == X.MULTILINESTRING:
            out.append((t, [star(pt(), r / 2, max(k // 2, 2))[:-1] for _ in range(int(rng.integers(1, 4)))]))
        elif t == X.POLYGON:
            c = pt()
            out.append((t, [star(c, r, k)] + ([star(c, 0.25 * r, 5)] if rng.random() < 0.3 else [])))
        else:
            out.append((t, [[star(pt(), r / 2, max(k // 2, 3))] for _ in range(int(rng.integers(1, 4)))]))
    return out


@pytest.mark.gpu
def test_gpu_refine_general_position(engine):
    """~2,000 random sides against a 64-vertex star with a hole: every side the device decides equals
    the exact answer, and at most 1 in 1,000 stays undecided (with continuous random coordinates exact
    arithmetic meets no zero determinant: checked here on the same inputs)"""
    rng = np.random.default_rng(20261019)
    filt = [[ring(50, 50, 45, 64, 0.05, 22), ring(50, 50, 9, 6, 0.3)]]
    geoms = _random_geoms(rng, 2000, -10.0, 110.0)
    E = X.ExactFilter(filt)
    z0 = X.ZEROS[0]
    want = np.array([2 if E.intersects(g) else 0 for g in geoms], np.uint8)
    assert X.ZEROS[0] == z0, "the exact helper met a zero determinant: not in general position"
    dims = list(X.DIMS)
    vals = [X.gpkg_of(g, dims[i % 4], i % 3 != 0, i % 5 != 0) for i, g in enumerate(geoms)]
    got, st = refine_new(engine, filt, vals)
    dec = got != 1
    assert np.array_equal(got[dec], want[dec]), np.nonzero(dec & (got != want))[0][:8]
    assert st["unsupported"] == 0 and st["undecided"] == int((~dec).sum())
    assert st["undecided"] * 1000 <= len(geoms), st
    assert 300 < int((want == 2).sum()) < 1700


# ---------------------------------------------------------------------------------------------
# GPU: the keep list, the layouts, the drop-in, the pipeline
def _delta_case(rng, n):
    """n deltas (inserts, deletes, updates) over random geometries; preset codes with non-candidates"""
    og = _random_geoms(rng, n, 20.0, 80.0)
    ng = _random_geoms(rng, n, 20.0, 80.0)
    kind = rng.integers(0, 3, n)  # 0 insert, 1 delete, 2 update
    pairs = np.stack([np.where(kind == 0, NONE, np.arange(n)), np.where(kind == 1, NONE, np.arange(n))], 1).astype(np.uint32)
    codes = np.where(pairs == NONE, 4, rng.choice(np.array([1, 1, 1, 1, 1, 1, 1, 0, 2, 3]), (n, 2))).astype(np.uint8)
    arenas = (arena_of([X.gpkg_of(g) for g in og]), arena_of([X.gpkg_of(g) for g in ng]))
    heads = [S.geom_heads(*a, HEXARR, GIDX, 1) for a in arenas]
    return og, ng, pairs, codes, arenas, heads


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_gpu_refine_keep_list(engine, n):
    rng = np.random.default_rng(100 + n)
    filt = [[ring(50, 50, 25, 9, 0.2)]]
    og, ng, pairs, codes, arenas, heads = _delta_case(rng, n)
    sf = S.SpatialFilter.from_polygons(filt)
    out, keep, st = S.geom_refine(engine, sf.polygon_arrays(), heads[0], heads[1], pairs, codes, arenas)
    assert np.array_equal(out[codes != 1], codes[codes != 1])  # non-candidates untouched
    E = X.ExactFilter(filt)
    for d in range(n):
        for s, gs in enumerate((og, ng)):
            if codes[d, s] == 1:
                assert out[d, s] in (1, 2 if E.intersects(gs[d]) else 0), (d, s)
    kept = ((out >= 1) & (out <= 3)).any(1)
    assert np.array_equal(keep, np.nonzero(kept)[0]) and keep.dtype == np.uint32
    assert sum(st.values()) == int((codes == 1).sum()) and st["unsupported"] == 0


def _refine_device(engine, arrays, heads, nheads, pairs, codes, arenas, flags, cap):
    """kd_geom_refine with every buffer in device memory and the delta count read on the device"""
    from kart_amd.device import DevBlobs, DevBuf

    n = pairs.shape[0]
    xy, off = arrays
    fp = N.KdFilterPoly()
    fp.xy, fp.ring_off, fp.n_ring, fp.n_vert = N.ptr(xy), N.ptr(off), off.shape[0] - 1, xy.shape[0]
    hb = [DevBuf.from_numpy(engine, h.view(np.uint8).reshape(-1)) if h.size else DevBuf(engine, 48) for h in heads]
    bl = [DevBlobs(engine, *a) for a in arenas]
    kb = [b.kd_blobs() for b in bl]
    dp = DevBuf(engine, 8 * cap)
    dp.zero()
    dp.upload(pairs)
    dm = DevBuf(engine, 2 * cap)
    dm.zero()
    dm.upload(np.ascontiguousarray(codes, np.uint8))
    dk, dnk, dst = DevBuf(engine, 4 * cap), DevBuf(engine, 8), DevBuf(engine, 32)
    dn = DevBuf.from_numpy(engine, np.array([n], np.uint64))
    N.check(engine.L.kd_geom_refine(engine.ctx, ctypes.byref(fp), hb[0].ptr, nheads[0], hb[1].ptr, nheads[1], N.KD_MEM_DEVICE,
                                    ctypes.byref(kb[0]), ctypes.byref(kb[1]), dp.ptr, cap, dn.ptr, N.KD_MEM_DEVICE, flags,
                                    dm.ptr, dk.ptr, dnk.ptr, dst.ptr, N.KD_MEM_DEVICE), "kd_geom_refine")
    k = int(dnk.download(np.uint64, 1)[0])
    return dm.download(np.uint8, 2 * n).reshape(n, 2), dk.download(np.uint32, k), dst.download(np.uint64, 4).tolist()


@pytest.mark.gpu
def test_gpu_refine_layouts_agree(engine):
    """host per-entry heads, device per-entry heads (device count below the capacity) and delta-order
    heads give the same codes, kept list and counters; a second call with the same filter too"""
    rng = np.random.default_rng(77)
    n = 700
    filt = [[ring(50, 50, 25, 9, 0.2), ring(50, 50, 5, 4, 0.0)]]
    og, ng, _, codes, arenas, heads = _delta_case(rng, n)
    # per-entry order differs from delta order: the deltas visit the entries through a permutation
    po, pn = rng.permutation(n), rng.permutation(n)
    kind = rng.integers(0, 3, n)
    pairs = np.stack([np.where(kind == 0, NONE, po), np.where(kind == 1, NONE, pn)], 1).astype(np.uint32)
    codes = np.where(pairs == NONE, 4, np.where(codes == 4, 1, codes)).astype(np.uint8)
    sf = S.SpatialFilter.from_polygons(filt)
    arr = sf.polygon_arrays()
    ref = S.geom_refine(engine, arr, heads[0], heads[1], pairs, codes, arenas)
    again = S.geom_refine(engine, arr, heads[0], heads[1], pairs, codes, arenas)
    assert np.array_equal(ref[0], again[0]) and np.array_equal(ref[1], again[1]) and ref[2] == again[2]
    assert (ref[0] == 0).any() and (ref[0] == 2).any()
    stl = [ref[2][k] for k in ("true", "false", "undecided", "unsupported")]
    dc, dk, dst = _refine_device(engine, arr, heads, (n, n), pairs, codes, arenas, 0, n + 37)
    assert np.array_equal(dc, ref[0]) and np.array_equal(dk, ref[1]) and dst == stl
    # delta order: slot d = delta d's head, whole 64-delta chunks
    slots = (n + 37 + 63) // 64 * 64
    dense = []
    for s in range(2):
        h = np.zeros(slots, S.GEOM_HEAD)
        pres = np.nonzero(pairs[:, s] != NONE)[0]
        h[pres] = heads[s][pairs[pres, s].astype(np.int64)]
        dense.append(h)
    hc, hk, hst = S.geom_refine(engine, arr, dense[0], dense[1], pairs, codes, arenas, delta_heads=True)
    assert np.array_equal(hc, ref[0]) and np.array_equal(hk, ref[1]) and hst == ref[2]
    dc, dk, dst = _refine_device(engine, arr, dense, (slots, slots), pairs, codes, arenas, N.KD_GF_DELTA_HEADS, n + 37)
    assert np.array_equal(dc, ref[0]) and np.array_equal(dk, ref[1]) and dst == stl
    # another filter at another address, then the first again: the cached device copy follows
    other = S.SpatialFilter.from_polygons([[ring(30, 30, 8, 5)]])
    oc, _, _ = S.geom_refine(engine, other.polygon_arrays(), heads[0], heads[1], pairs, codes, arenas)
    assert not np.array_equal(oc, ref[0])
    back = S.geom_refine(engine, arr, heads[0], heads[1], pairs, codes, arenas)
    assert np.array_equal(back[0], ref[0]) and np.array_equal(back[1], ref[1])


@pytest.mark.gpu
def test_gpu_refine_rejects_bad_arguments(engine):
    ar = arena_of([X.gpkg_of((X.POINT, (1.0, 1.0)))])
    heads = S.geom_heads(*ar, HEXARR, GIDX, 1)
    pairs = np.array([[NONE, 0]], np.uint32)
    codes = np.array([[4, 1]], np.uint8)
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    none = np.zeros(0, S.GEOM_HEAD)
    with pytest.raises(N.Unsupported):  # no heads at all
        S.geom_refine(engine, S.SpatialFilter.from_polygons([[ring(0, 0, 5, 5)]]).polygon_arrays(), none, none, pairs, codes,
                      (empty, ar))
    big = (np.zeros(((1 << 20) + 1, 2)), np.array([0, (1 << 20) + 1], np.uint64))
    with pytest.raises(N.Unsupported):  # more than 2^20 filter vertices
        S.geom_refine(engine, big, none, heads, pairs, codes, (empty, ar))
    open_ring = (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]]), np.array([0, 3], np.uint64))
    with pytest.raises(N.KdError):  # a ring that is not closed
        S.geom_refine(engine, open_ring, none, heads, pairs, codes, (empty, ar))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["points", "polygons"])
def test_gpu_filtered_diff_reference_filters(engine, name):
    """the drop-in with the reference's own filters: `points` keeps 302 of 2,143 features, `polygons`
    44 of 228 — decided on the device, nothing left unverified (without the refine stage 45 polygon
    features pass the envelope and all 45 count as unverified matches)"""
    f = FILTERS[name]
    fx = load(f["fixture"])
    head = version(fx, f["side"])
    sf = S.SpatialFilter.from_polygons(f["polygons"])
    assert sf.intersects is None and not sf.rectangle
    ds = D.get_dataset_diff(engine, None, head)
    got = list(S.filtered_ds_feature_deltas(engine, ds, None, head, sf))
    assert len(got) == f["matching"]
    assert sf.stats["unverified"] == 0
    assert sf.stats["refine"]["true"] == f["matching"] and sf.stats["refine"]["undecided"] == 0
    assert [k for k, _ in got] == sorted(k for k, _ in got)
    # the same set as the exact helper's
    E = X.ExactFilter(f["polygons"])
    geoms = _head_geometries(name)
    names = fx.names(f["side"])
    want = sorted(head.decode_path_to_1pk(nm) for nm, g in zip(names, geoms) if E.intersects(X.parse_gpkg(g)))
    assert sorted(k for k, _ in got) == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [{"delta_order": True}, {"delta_order": True, "gather": True}, {"delta_order": False}])
def test_gpu_filter_pipeline_polygons(engine, mode):
    """FilterPipeline(heads=True, polygons=a 16-gon inscribed in C5_FILTER) over synth.c5_layer(3000):
    every side the envelope filter decided keeps its code, every candidate is the exact answer or 1"""
    import types

    from kart_amd import synth
    from kart_amd.device import FilterPipeline
    from oracle import oracle as O

    L = synth.c5_layer(3000, seed=13)
    ver = types.SimpleNamespace(schema=L.schema, legends=L.legends)
    gc = S.GeomCols(ver, ver, "geom", "geom")
    f = synth.C5_FILTER
    gon = [[[((f[0] + f[1]) / 2 + (f[1] - f[0]) / 2 * math.cos(2 * math.pi * k / 16),
              (f[2] + f[3]) / 2 + (f[3] - f[2]) / 2 * math.sin(2 * math.pi * k / 16)) for k in range(16)]]]
    pipe = FilterPipeline(engine, L.base, L.target, L.base_blobs, L.target_blobs, gc, f, False, 20, heads=True,
                          polygons=gon, **mode)
    pipe.step()
    pipe.step()
    counts, delta, codes, keep, enc, ok = pipe.results()
    st = pipe.refine_stats()
    cols = {h: 0 for h in L.legends}
    (od, oo), (nd, no) = L.base_blobs, L.target_blobs
    oc, okeep, oenc, ook = O.geom_filter(od, oo, nd, no, delta, cols, cols, f, False, 20)
    assert np.array_equal(codes[oc != 1], oc[oc != 1])
    assert np.array_equal(ok, ook) and np.array_equal(enc[ok == 1], oenc[ook == 1])
    E = X.ExactFilter(S.SpatialFilter.from_polygons(gon).polygons)
    cand = np.argwhere(oc == 1)
    nfalse = 0
    for d, s in cand:
        data, off = L.target_blobs if s else L.base_blobs
        b = int(delta[d, s])
        h = pipe.heads_host[s][b]
        o = int(off[b]) + (int(h["goff_status"]) & 0xFFFFFF)
        want = 2 if E.intersects(X.parse_gpkg(data[o:o + int(h["glen"])].tobytes())) else 0
        assert codes[d, s] in (1, want), (d, s, codes[d, s], want)
        nfalse += codes[d, s] == 0
    assert st["false"] == nfalse and sum(st.values()) == cand.shape[0] and st["unsupported"] == 0
    kept = ((codes >= 1) & (codes <= 3)).any(1)
    assert np.array_equal(keep, np.nonzero(kept)[0]) and counts["kept"] == int(kept.sum())
