"""The pruned walk on the host against the pruned walk with its leaf level on the GPU.

Builds the C3-mix repository of §3.7 round 6 (e2e_repo_bench.build_sharded: int-PK points, 8 / 1 / 1 %
updates / deletes / inserts) and a repacked copy (one pack of deltas, where a new-side leaf tree is a
delta against the old side's), then times on one GPU, alternated, REPS repetitions each:

    host      ObjectDB.walk(compare=(0, 1))                       the yardstick
    device    ObjectDB.walk_device(depth=4, deltas=False)
    deltas    ObjectDB.walk_device(depth=4, deltas=True)

Every device result is compared with the host's.  Medians, min-max and the phases (kd_walk_device's own
counters, the delta planner's rbd_* microseconds, and the kernels' summed times from one extra profiled
repetition) go to --out as JSON.

    python scripts/walk_device_bench.py --n 3000000 --out profiles/device_walk/bench.json
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import e2e_repo_bench as E  # noqa: E402
from kart_amd.engine import Engine  # noqa: E402
from kart_amd.odb import ObjectDB  # noqa: E402

KERNELS = ["k_inf_streams", "k_tj_count", "k_gf_scan", "k_tj_emit"] + ["k_dl_apply.%02d" % l for l in range(1, 9)]


def same(a, b):
    return all(x.present == y.present and np.array_equal(x.off, y.off) and np.array_equal(x.paths, y.paths)
               and np.array_equal(x.oids, y.oids) and np.array_equal(x.modes, y.modes) for x, y in zip(a, b))


def measure(eng, gitdir, reps, depth):
    db = ObjectDB(gitdir)
    sub = f"{E.DS}/.table-dataset/feature"
    roots = [subprocess.run(["git", "--git-dir", gitdir, "rev-parse", r], check=True, capture_output=True).stdout.decode().strip()
             for r in ("main^", "main")]
    arms = {
        "host": lambda: (db.walk(roots, sub, (0, 1)), None),
        "device": lambda: db.walk_device(eng, roots, sub, (0, 1), depth=depth, deltas=False),
        "deltas": lambda: db.walk_device(eng, roots, sub, (0, 1), depth=depth, deltas=True),
    }
    want, _ = arms["host"]()
    for name in ("device", "deltas"):  # warm-up and check
        got, _ = arms[name]()
        assert same(got, want), f"{name}: walk_device differs from walk"
    times = {k: [] for k in arms}
    stats = {}
    for _ in range(reps):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            _, st = fn()
            times[name].append(time.perf_counter() - t0)
            if st is not None:
                stats[name] = dict(st)
                if name == "deltas":
                    stats[name].update({k: db.get_option(k) for k in ("rbd_plan_us", "rbd_peek_us", "rbd_host_us", "rbd_device_us")})
    kernels = {}
    for name in ("device", "deltas"):  # one extra repetition with the kernels timed
        eng.prof_enable(True)
        eng.prof_select(KERNELS)
        eng.prof_reset()
        arms[name]()
        kernels[name] = {k: {"launches": n, "ms": round(ms, 3)} for k in KERNELS for n, ms in [eng.prof_get(k)] if n}
        eng.prof_enable(False)
    db.close()
    out = {"leaves_kept": [int(L.n) for L in want]}
    for name in arms:
        t = times[name]
        out[name] = {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4),
                     "runs_s": [round(x, 4) for x in t]}
        if name in stats:
            out[name]["stats"] = stats[name]
            out[name]["kernels_profiled_run"] = kernels[name]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--repack-n", type=int, default=None, help="features of the repacked copy's repository (default: --n)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_walk", "bench.json"))
    a = ap.parse_args()
    res = {"method": __doc__.split("\n\n")[1].replace("\n", " "), "n": a.n, "reps": a.reps, "edits": [0.08, 0.01, 0.01]}
    tmp = tempfile.mkdtemp(prefix="walk_device_bench.")
    try:
        with Engine(0) as eng:
            g = os.path.join(tmp, "r.git")
            t0 = time.perf_counter()
            E.build_sharded(g, a.n, procs=a.procs)
            res["build_s"] = round(time.perf_counter() - t0, 1)
            res["fast_import"] = measure(eng, g, a.reps, 4)
            json.dump(res, open(a.out, "w"), indent=1)
            rn = a.repack_n or a.n
            g2 = os.path.join(tmp, "p.git")
            t0 = time.perf_counter()
            if rn == a.n:
                shutil.copytree(g, g2)
            else:
                E.build_sharded(g2, rn, procs=a.procs)
            subprocess.run(["git", "--git-dir", g2, "repack", "-adfq", "--depth=50", "--window=10", "--threads=%d" % a.procs], check=True)
            res["repack_n"] = rn
            res["repack_s"] = round(time.perf_counter() - t0, 1)
            res["repacked"] = measure(eng, g2, a.reps, 4)
            json.dump(res, open(a.out, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps({k: {m: v[m]["median_s"] for m in ("host", "device", "deltas")} for k, v in res.items() if isinstance(v, dict) and "host" in v}))


if __name__ == "__main__":
    main()
