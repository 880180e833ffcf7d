"""What finding renames adds to the C3 step, timed.

DiffPipeline over synth.polygons_layer (C3) with a share of the untouched features' pks renumbered
(synth.renumber_pks: each shows as one delete plus one insert of one OID): ``step()`` alone, then
``step()`` + ``renames_step()`` (kd_find_renames on the resident delta list and device count), HIP
events around ``--steps`` steps on a stream of the script's own, alternating ``--rounds`` times in one
process; then the pass's kernels with events around each launch (kd_prof_*).  The pass is timed with
the list's full capacity as its bound (what a caller that never reads the count back passes) and with
the delta count itself (``cap=``).  Prints one JSON object and writes it to --out.

    python scripts/renames_bench.py --n 20000000 --steps 200 --out profiles/find_renames/bench.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RN_KERNELS = ("k_rn_list", "k_gf_scan", "k_rn_zero", "k_rn_build", "k_rn_probe", "k_rn_count", "k_rn_place")


class Events:
    """two HIP events on one stream of the script's own, which the engine launches on"""

    def __init__(self, eng):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.stream, self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self.ok(self.hip.hipStreamCreate(ctypes.byref(self.stream)))
        self.ok(self.hip.hipEventCreate(ctypes.byref(self.a)))
        self.ok(self.hip.hipEventCreate(ctypes.byref(self.b)))
        eng.set_stream(self.stream)

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    def ms_per_step(self, eng, step, steps):
        eng.device_sync()
        self.ok(self.hip.hipEventRecord(self.a, self.stream))
        for _ in range(steps):
            step()
        self.ok(self.hip.hipEventRecord(self.b, self.stream))
        self.ok(self.hip.hipEventSynchronize(self.b))
        ms = ctypes.c_float()
        self.ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b))
        return ms.value / steps


def kernel_times(eng, step, names, launches=20):
    """ms per launch of the named kernels, events around every launch (untimed steps)"""
    eng.prof_reset()
    eng.prof_select(names)
    eng.prof_enable(True)
    for _ in range(launches):
        step()
    eng.sync()
    eng.prof_enable(False)
    eng.prof_select(None)
    kern = {}
    for k in names:
        n, ms = eng.prof_get(k)
        if n:
            kern[k] = {"launches_per_step": n // launches, "ms_per_step": round(ms / launches, 5)}
    return kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--share", type=float, default=0.05, help="share of the untouched features re-keyed")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np

    from kart_amd import synth
    from kart_amd.device import DiffPipeline
    from kart_amd.engine import Engine
    from kart_amd.schema import FieldMaps

    t0 = time.time()
    L, moved = synth.renumber_pks(synth.polygons_layer(a.n), a.share)
    gen_s = time.time() - t0
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    with Engine(0) as eng:
        ev = Events(eng)
        pipe = DiffPipeline(eng, L.base, L.target, L.base_blobs, L.target_blobs, maps)
        pipe.step()
        eng.sync()
        counts, delta, upd, _, _ = pipe.results()
        pipe.use_update_arenas(upd)  # (the C3 step bench.py times)
        nd = counts["deltas"]
        ren = pipe.renames()
        assert ren.shape[0] == moved, (ren.shape, moved)
        d, i = delta[ren[:, 0].astype(np.int64)], delta[ren[:, 1].astype(np.int64)]
        assert np.array_equal(L.base.oid[d[:, 0].astype(np.int64)], L.target.oid[i[:, 1].astype(np.int64)])
        assert np.array_equal(pipe.renames(cap=nd), ren)

        def both():
            pipe.step()
            pipe.renames_step()

        def both_tight():
            pipe.step()
            pipe.renames_step(cap=nd)

        for f in (pipe.step, both, both_tight):
            for _ in range(max(1, a.warmup)):
                f()
        eng.sync()
        ms_step, ms_both, ms_tight = [], [], []
        for _ in range(a.rounds):
            ms_step.append(ev.ms_per_step(eng, pipe.step, a.steps))
            ms_both.append(ev.ms_per_step(eng, both, a.steps))
            ms_tight.append(ev.ms_per_step(eng, both_tight, a.steps))
        kern = kernel_times(eng, pipe.renames_step, RN_KERNELS)
        kern_tight = kernel_times(eng, lambda: pipe.renames_step(cap=nd), RN_KERNELS)
        eng.set_stream(None)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    n_del = counts["deletes"]
    n_ins = counts["inserts"]
    cap = 1024
    while cap < 2 * n_del:
        cap *= 2
    out = {
        "what": "DiffPipeline(C3 with a share of pks renumbered) per step: step() alone vs step() + kd_find_renames on "
                "the resident delta list (device count), HIP events around the steps; bound = the pass's n_delta "
                "argument (list capacity, or the delta count)",
        "features": a.n, "share_renumbered": a.share, "steps": a.steps, "rounds": a.rounds, "generate_s": round(gen_s, 1),
        "counts": counts, "pairs": int(ren.shape[0]), "table_slots": cap,
        "list_capacity": pipe.cap,
        "ms_per_step_alone": [round(x, 4) for x in ms_step],
        "ms_per_step_with_renames_capacity_bound": [round(x, 4) for x in ms_both],
        "ms_per_step_with_renames_count_bound": [round(x, 4) for x in ms_tight],
        "added_ms_capacity_bound": round(med(ms_both) - med(ms_step), 4),
        "added_ms_count_bound": round(med(ms_tight) - med(ms_step), 4),
        "step_spread_ms": round(max(ms_step) - min(ms_step), 4),
        "kernels_capacity_bound": kern,
        "kernels_count_bound": kern_tight,
        "algorithmic_bytes": 8 * nd + 20 * (n_del + n_ins) + 16 * cap,
    }
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
