"""The spatially filtered diff's step with and without the exact stage (kd_geom_refine), timed.

FilterPipeline over synth.c5_layer with delta-order heads, once with the rectangle filter (classify2 +
kd_geom_filter_deltas: the step bench.py --workload c5 times) and once with a 64-vertex polygon of the
same envelope (the same step + kd_geom_refine), alternating ``--rounds`` times in one process; then
the refine's kernels with events around each launch.  Prints one JSON object and writes it to --out.

C5's synthetic rings are not valid polygons (random vertices, no ring closed on purpose): the run is a
timing of the stage on a realistic candidate mix, not a statement about which features match.

    python scripts/refine_bench.py --n 20000000 --steps 200 --out profiles/geom_refine/bench.json

``--exact`` adds the exact second pass (KD_GF_EXACT): the polygon step with the flag on the same input
(nothing is undecided there: what the empty pass costs), and a second filter whose ring is routed through
the first vertices of ``--touch`` of the layer's candidate features, so that thousands of sides touch it —
with the flag off (how many sides stay undecided) and on (the exact kernels' time by events, their sides
per second), and the Python exact helper over a sample of those sides for scale.

    python scripts/refine_bench.py --exact --out profiles/geom_refine_exact/bench.json
"""
import argparse
import json
import math
import os
import struct
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFINE_KERNELS = ("k_gr_list", "k_gr_points", "k_gr_wave", "k_gf_count", "k_gf_scan", "k_gf_place")
EXACT_KERNELS = ("k_gr_relist", "k_gr_points_x", "k_gr_wave_x", "k_gr_stats")


def polygon_of(env, k):
    """a k-gon inscribed in the envelope's ellipse: for k a multiple of 4 its envelope is `env`"""
    cx, cy, rx, ry = (env[0] + env[1]) / 2, (env[2] + env[3]) / 2, (env[1] - env[0]) / 2, (env[3] - env[2]) / 2
    return [[[(cx + rx * math.cos(2 * math.pi * i / k), cy + ry * math.sin(2 * math.pi * i / k)) for i in range(k)]]]


def first_vertex(g):
    """(x, y) of the first vertex of a GPKG value's WKB (types 1-6), or None"""
    es = {0: 0, 1: 32, 2: 48, 3: 48, 4: 64}.get((g[3] >> 1) & 7)
    if es is None or len(g) < 8 + es + 5:
        return None
    p = 8 + es
    for _ in range(3):  # geometry -> part -> ring
        e = "<" if g[p] == 1 else ">"
        t = struct.unpack_from(e + "I", g, p + 1)[0] % 1000
        p += 5
        if t == 1:
            break
        if struct.unpack_from(e + "I", g, p)[0] == 0:
            return None
        p += 4
        if t == 2:
            break
        if t == 3:
            if struct.unpack_from(e + "I", g, p)[0] == 0:
                return None
            p += 4
            break
    if len(g) < p + 16:
        return None
    x, y = struct.unpack_from(e + "dd", g, p)
    return (x, y) if math.isfinite(x) and math.isfinite(y) else None


def side_gpkg(L, pipe, delta, d, s):
    data, off = L.target_blobs if s else L.base_blobs
    b = int(delta[d, s])
    h = pipe.heads_host[s][b]
    o = int(off[b]) + (int(h["goff_status"]) & 0xFFFFFF)
    return data[o:o + int(h["glen"])].tobytes()


def ring_through(points):
    """a closed ring through the points in order of angle around their centroid (star-shaped: simple)"""
    pts = sorted(set(points))
    cx, cy = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    pts.sort(key=lambda p: math.atan2(p[1] - cy, p[0] - cx))
    return [[pts + [pts[0]]]]


def kernel_times(eng, step, names, launches=20):
    """ms per launch of the named kernels, events around every launch (untimed steps)"""
    eng.prof_reset()
    eng.prof_select(None)
    eng.prof_enable(True)
    for _ in range(launches):
        step()
    eng.sync()
    eng.prof_enable(False)
    kern = {}
    for k in names:
        n, ms = eng.prof_get(k)
        if n:
            kern[k] = round(ms / n, 5)
    return kern


def timed(eng, step, steps):
    eng.device_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    eng.device_sync()
    return (time.perf_counter() - t0) / steps * 1e3


def exact_part(a, eng, L, mk, rect, rcodes, polyx, st, ms_poly, ms_polyx):
    """the --exact measurements (see the module's docstring)"""
    import random

    from kart_amd.spatial import SpatialFilter

    med = lambda v: sorted(v)[len(v) // 2]
    xst = polyx.refine_stats()
    assert xst == st, (xst, st)  # (nothing was undecided: the flag changes no count)
    out = {"nothing_to_decide": {
        "ms_per_step_polygon_exact": [round(x, 4) for x in ms_polyx],
        "added_by_empty_pass_ms": round(med(ms_polyx) - med(ms_poly), 4),
        "polygon_spread_ms": round(max(ms_poly) - min(ms_poly), 4),
        "refine_stats": xst,
        "kernel_ms_per_launch_events": kernel_times(eng, polyx.step, REFINE_KERNELS + EXACT_KERNELS)}}
    # a filter routed through the first vertices of candidate features
    _, delta, _, _, _, _ = rect.results()
    cand = [(int(d), int(s)) for d, s in zip(*(rcodes == 1).nonzero())]
    random.Random(1).shuffle(cand)
    pts = []
    for d, s in cand:
        v = first_vertex(side_gpkg(L, rect, delta, d, s))
        if v is not None:
            pts.append(v)
        if len(pts) >= a.touch:
            break
    tsf = SpatialFilter.from_polygons(ring_through(pts))
    loose, tight = mk(tsf), mk(tsf, exact=True)
    for p in (loose, tight):
        for _ in range(max(1, a.warmup)):
            p.step()
    eng.sync()
    lst, tst = loose.refine_stats(), tight.refine_stats()
    _, tdelta, lcodes, _, _, _ = loose.results()
    _, _, tcodes, _, _, _ = tight.results()
    assert ((lcodes == tcodes) | (lcodes == 1)).all(), "the exact pass changed a side the fast pass decided"
    ms_l, ms_t = [], []
    for _ in range(a.rounds):
        ms_l.append(timed(eng, loose.step, a.steps))
        ms_t.append(timed(eng, tight.step, a.steps))
    kern = kernel_times(eng, tight.step, REFINE_KERNELS + EXACT_KERNELS)
    x_ms = kern.get("k_gr_points_x", 0.0) + kern.get("k_gr_wave_x", 0.0)
    handed = lst["undecided"]
    # for scale only: the rational-arithmetic helper of the tests (Python) over a sample of those sides
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refine_exact as X

    und = [(int(d), int(s)) for d, s in zip(*(lcodes == 1).nonzero())]
    random.Random(2).shuffle(und)
    und = und[:a.sample]
    E = X.ExactFilter(tsf.polygons)
    geoms = [X.parse_gpkg(side_gpkg(L, loose, tdelta, d, s)) for d, s in und]
    t0 = time.perf_counter()
    ans = [E.intersects(g) for g in geoms]
    py_s = time.perf_counter() - t0
    agree = sum(int(tcodes[d, s]) == (2 if w else 0) for (d, s), w in zip(und, ans))
    out["much_to_decide"] = {
        "filter_vertices": int(tsf.polygon_arrays()[0].shape[0]), "features_visited": len(pts),
        "refine_stats_flag_off": lst, "refine_stats_flag_on": tst,
        "sides_taken_by_exact_pass": handed,
        "ms_per_step_flag_off": [round(x, 4) for x in ms_l], "ms_per_step_flag_on": [round(x, 4) for x in ms_t],
        "added_ms_per_step": round(med(ms_t) - med(ms_l), 4),
        "kernel_ms_per_launch_events": kern,
        "exact_kernels_ms": round(x_ms, 5),
        "exact_sides_per_s": round(handed / (x_ms * 1e-3)) if x_ms else None,
        "python_helper": {"what": "tests/refine_exact.py ExactFilter.intersects (Python, Fractions) over a sample of the "
                                  "undecided sides: for scale only", "sides": len(und), "seconds": round(py_s, 3),
                          "sides_per_s": round(len(und) / py_s, 1) if py_s else None, "agree_with_device": agree}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=64)
    ap.add_argument("--exact", action="store_true", help="also time the exact second pass (KD_GF_EXACT)")
    ap.add_argument("--touch", type=int, default=3000, help="--exact: features the touching filter's ring visits")
    ap.add_argument("--sample", type=int, default=200, help="--exact: sides timed with the Python exact helper")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from kart_amd import synth
    from kart_amd.device import FilterPipeline
    from kart_amd.engine import Engine
    from kart_amd.spatial import GeomCols, SpatialFilter

    t0 = time.time()
    L = synth.c5_layer(a.n)
    gen_s = time.time() - t0
    ver = types.SimpleNamespace(schema=L.schema, legends=L.legends)
    cols = GeomCols(ver, ver, "geom", "geom")
    sf = SpatialFilter.from_polygons(polygon_of(synth.C5_FILTER, a.vertices))
    assert sf.filter_env == tuple(float(x) for x in synth.C5_FILTER), sf.filter_env
    with Engine(0) as eng:
        mk = lambda poly, **kw: FilterPipeline(eng, L.base, L.target, L.base_blobs, L.target_blobs, cols,
                                               poly.filter_env if poly is not None else synth.C5_FILTER, False, 20, heads=True,
                                               delta_order=True, polygons=poly, **kw)
        rect, poly = mk(None), mk(sf)
        polyx = mk(sf, exact=True) if a.exact else None
        for p in (rect, poly) + ((polyx,) if a.exact else ()):
            for _ in range(max(1, a.warmup)):
                p.step()
        eng.sync()
        rc, _, rcodes, rkeep, _, _ = rect.results()
        pc, _, pcodes, pkeep, _, _ = poly.results()
        st = poly.refine_stats()
        cand = int((rcodes == 1).sum())
        assert sum(st.values()) == cand, (st, cand)
        assert ((pcodes == rcodes) | (rcodes == 1)).all(), "the refine changed a side that was no candidate"
        ms_rect, ms_poly, ms_polyx = [], [], []
        for _ in range(a.rounds):
            ms_rect.append(timed(eng, rect.step, a.steps))
            ms_poly.append(timed(eng, poly.step, a.steps))
            if a.exact:
                ms_polyx.append(timed(eng, polyx.step, a.steps))
        kern = kernel_times(eng, poly.step, REFINE_KERNELS + ("k_gf_heads",))
        ex = exact_part(a, eng, L, mk, rect, rcodes, polyx, st, ms_poly, ms_polyx) if a.exact else None
    refine_ms = sum(kern.get(k, 0.0) for k in ("k_gr_list", "k_gr_points", "k_gr_wave"))
    # (k_gf_scan / k_gf_place run twice in a polygon step: once in the filter, once in the rebuild)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {
        "what": "FilterPipeline(c5_layer, delta-order heads) per step: rectangle filter vs a polygon filter of the same "
                "envelope (+ kd_geom_refine); a timing only — C5's synthetic rings are not valid polygons",
        "features": a.n, "deltas": rc["deltas"], "steps": a.steps, "rounds": a.rounds, "filter_vertices": a.vertices,
        "generate_s": round(gen_s, 1),
        "ms_per_step_rectangle": [round(x, 4) for x in ms_rect],
        "ms_per_step_polygon": [round(x, 4) for x in ms_poly],
        "added_ms_per_step": round(med(ms_poly) - med(ms_rect), 4),
        "rectangle_spread_ms": round(max(ms_rect) - min(ms_rect), 4),
        "candidate_sides": cand, "refine_stats": st,
        "decided_share": round((st["true"] + st["false"]) / cand, 6) if cand else None,
        "kept_rectangle": rc["kept"], "kept_polygon": pc["kept"],
        "kernel_ms_per_launch_events": kern,
        "refine_kernels_ms": round(refine_ms, 5),
        "candidate_sides_per_s": round(cand / (refine_ms * 1e-3)) if refine_ms else None,
    }
    if ex is not None:
        out["exact"] = ex
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
