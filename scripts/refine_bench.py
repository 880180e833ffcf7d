"""The spatially filtered diff's step with and without the exact stage (kd_geom_refine), timed.

FilterPipeline over synth.c5_layer with delta-order heads, once with the rectangle filter (classify2 +
kd_geom_filter_deltas: the step bench.py --workload c5 times) and once with a 64-vertex polygon of the
same envelope (the same step + kd_geom_refine), alternating ``--rounds`` times in one process; then
the refine's kernels with events around each launch.  Prints one JSON object and writes it to --out.

C5's synthetic rings are not valid polygons (random vertices, no ring closed on purpose): the run is a
timing of the stage on a realistic candidate mix, not a statement about which features match.

    python scripts/refine_bench.py --n 20000000 --steps 200 --out profiles/geom_refine/bench.json
"""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFINE_KERNELS = ("k_gr_list", "k_gr_points", "k_gr_wave", "k_gf_count", "k_gf_scan", "k_gf_place")


def polygon_of(env, k):
    """a k-gon inscribed in the envelope's ellipse: for k a multiple of 4 its envelope is `env`"""
    cx, cy, rx, ry = (env[0] + env[1]) / 2, (env[2] + env[3]) / 2, (env[1] - env[0]) / 2, (env[3] - env[2]) / 2
    return [[[(cx + rx * math.cos(2 * math.pi * i / k), cy + ry * math.sin(2 * math.pi * i / k)) for i in range(k)]]]


def timed(eng, step, steps):
    eng.device_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    eng.device_sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=64)
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
        mk = lambda poly: FilterPipeline(eng, L.base, L.target, L.base_blobs, L.target_blobs, cols, synth.C5_FILTER, False,
                                         20, heads=True, delta_order=True, polygons=poly)
        rect, poly = mk(None), mk(sf)
        for p in (rect, poly):
            for _ in range(max(1, a.warmup)):
                p.step()
        eng.sync()
        rc, _, rcodes, rkeep, _, _ = rect.results()
        pc, _, pcodes, pkeep, _, _ = poly.results()
        st = poly.refine_stats()
        cand = int((rcodes == 1).sum())
        assert sum(st.values()) == cand, (st, cand)
        assert ((pcodes == rcodes) | (rcodes == 1)).all(), "the refine changed a side that was no candidate"
        ms_rect, ms_poly = [], []
        for _ in range(a.rounds):
            ms_rect.append(timed(eng, rect.step, a.steps))
            ms_poly.append(timed(eng, poly.step, a.steps))
        # the refine's kernels, events around every launch (untimed steps)
        eng.prof_reset()
        eng.prof_select(None)
        eng.prof_enable(True)
        for _ in range(20):
            poly.step()
        eng.sync()
        eng.prof_enable(False)
        kern = {}
        for k in REFINE_KERNELS + ("k_gf_heads",):
            launches, ms = eng.prof_get(k)
            if launches:
                kern[k] = round(ms / launches, 5)
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
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
