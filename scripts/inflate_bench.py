"""Blob reads: the host route (kd_odb_read_batch on 16 threads + the upload of its arena) against the
device route (kd_odb_read_batch_device: compressed streams shipped, inflated by k_inf_streams).

Workload: a repository of feature blobs of the kind scripts/e2e_repo_bench.py builds — C3-like polygon
blobs and point blobs, half each, every blob its own deflate stream (git fast-import --depth=0, as Kart
imports).  Reads of --n blobs (default 1M and 4M) in shuffled id order; the two routes alternate
--rounds times in one process.  Per run: wall seconds, the kernel's milliseconds by events, compressed
and inflated bytes, the route's counters.  A second A/B reads the same ids grouped by kind (points, then
polygons), which is what a size-ordered lane assignment would give a wave: its kernel time against the
shuffled order's says whether the longest stream per wave dominates.

  python scripts/inflate_bench.py --out profiles/device_inflate/bench.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kart_amd import synth  # noqa: E402
from kart_amd.schema import Legend  # noqa: E402


def _import_blobs(args):
    """one worker: a chunk of blobs through its own `git fast-import --depth=0` (one pack); their ids"""
    gitdir, data, off = args
    n = off.shape[0] - 1
    raw = data.tobytes()
    ids = bytearray(20 * n)
    parts = []
    for i in range(n):
        b = raw[int(off[i]):int(off[i + 1])]
        ids[20 * i:20 * i + 20] = hashlib.sha1(b"blob %d\0" % len(b) + b).digest()
        parts.append(b"blob\ndata %d\n%s\n" % (len(b), b))
    subprocess.run(["git", "-c", "fastimport.unpackLimit=0", "fast-import", "--quiet", "--depth=0"], input=b"".join(parts),
                   env=dict(os.environ, GIT_DIR=gitdir), check=True)
    return bytes(ids)


def build(gitdir, n, procs=16):
    """n blobs (the first half polygons, the rest points) -> (ids [n, 20], is_polygon [n])"""
    from multiprocessing import Pool

    subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    pl = Legend(["c-fid"], [c["id"] for c in synth.POLYGON_SCHEMA[1:]]).hexhash()
    tl = Legend(["c-fid"], [c["id"] for c in synth.POINT_SCHEMA[1:]]).hexhash()
    npoly = n // 2
    ids = []
    for kind, cnt in (("polygon", npoly), ("point", n - npoly)):
        step = 1 << 20
        for lo in range(0, cnt, step):
            pk = np.arange(lo + 1, min(cnt, lo + step) + 1, dtype=np.int64)
            zero = np.zeros(pk.shape[0], np.uint64)
            data, off = synth.polygon_blobs(pk, zero, zero, pl) if kind == "polygon" else synth.point_blobs(pk, zero, tl)
            cuts = np.linspace(0, pk.shape[0], procs + 1).astype(np.int64)
            jobs = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                s, e = int(off[a]), int(off[b])
                jobs.append((gitdir, data[s:e], (off[a:b + 1] - np.uint64(s)).astype(np.uint64)))
            with Pool(procs) as pool:
                ids += pool.map(_import_blobs, jobs)
            print(f"  {kind} blobs: {min(cnt, lo + step)} of {cnt}", file=sys.stderr, flush=True)
    ids = np.frombuffer(b"".join(ids), np.uint8).reshape(n, 20)
    return ids, np.arange(n) < npoly


def host_route(eng, db, oids, threads):
    from kart_amd.device import DevBuf

    t0 = time.perf_counter()
    data, off, status = db.read_batch(oids, threads)
    t1 = time.perf_counter()
    d, o = DevBuf.from_numpy(eng, data), DevBuf.from_numpy(eng, off)
    eng.sync()
    t2 = time.perf_counter()
    assert not status.any()
    return {"route": "host", "wall_s": t2 - t0, "read_s": t1 - t0, "upload_s": t2 - t1, "inflated_bytes": int(off[-1])}, (d, o)


def device_route(eng, db, oids, threads):
    eng.prof_reset()
    t0 = time.perf_counter()
    blobs, status, stats = db.read_batch_device(eng, oids, threads)
    t1 = time.perf_counter()
    assert not status.any()
    launches, ms = eng.prof_get("k_inf_streams")
    return {"route": "device", "wall_s": t1 - t0, "kernel_ms": ms, "kernel_launches": launches,
            "inflated_bytes": blobs.nbytes, "compressed_bytes": stats["compressed"], "stats": stats}, blobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repo", help="keep / reuse the repository here (default: a temporary directory)")
    ap.add_argument("--out")
    a = ap.parse_args()
    from kart_amd.engine import Engine
    from kart_amd.odb import ObjectDB

    nmax = max(a.n)
    tmp = None
    gitdir = a.repo
    if gitdir is None:
        tmp = tempfile.TemporaryDirectory()
        gitdir = os.path.join(tmp.name, "blobs.git")
    t0 = time.perf_counter()
    ids, is_poly = build(gitdir, nmax)
    print(f"repository of {nmax} blobs built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    result = {"blobs_in_repository": nmax, "threads": a.threads, "rounds": a.rounds, "reads": []}
    with Engine(0) as eng:
        eng.prof_enable(True)
        eng.prof_select(["k_inf_streams"])
        db = ObjectDB(gitdir)
        rng = np.random.default_rng(1)
        for n in a.n:
            pick = rng.permutation(nmax)[:n]
            oids = np.ascontiguousarray(ids[pick])
            # both routes once untimed: page cache, pinned staging, workspace slots
            host_route(eng, db, oids[:min(n, 100_000)], a.threads)
            device_route(eng, db, oids[:min(n, 100_000)], a.threads)
            runs = []
            for r in range(a.rounds):
                for fn in (host_route, device_route):
                    rec, keep = fn(eng, db, oids, a.threads)
                    del keep
                    rec["round"] = r
                    runs.append(rec)
                    print(json.dumps(rec), file=sys.stderr, flush=True)
            # lane order A/B: the same ids grouped by kind (what size-ordered lanes would see)
            grouped = np.ascontiguousarray(ids[np.concatenate([pick[~is_poly[pick]], pick[is_poly[pick]]])])
            order = []
            for r in range(a.rounds):
                for name, o in (("shuffled", oids), ("grouped_by_kind", grouped)):
                    rec, keep = device_route(eng, db, o, a.threads)
                    del keep
                    order.append({"order": name, "round": r, "kernel_ms": rec["kernel_ms"], "wall_s": rec["wall_s"]})
                    print(json.dumps(order[-1]), file=sys.stderr, flush=True)
            med = lambda rows, key: float(np.median([x[key] for x in rows]))  # noqa: E731
            hr, dr = [x for x in runs if x["route"] == "host"], [x for x in runs if x["route"] == "device"]
            result["reads"].append({
                "n": n, "runs": runs, "lane_order_ab": order,
                "median": {"host_wall_s": med(hr, "wall_s"), "host_read_s": med(hr, "read_s"),
                           "host_upload_s": med(hr, "upload_s"), "device_wall_s": med(dr, "wall_s"),
                           "device_kernel_ms": med(dr, "kernel_ms"),
                           "kernel_ms_shuffled": med([x for x in order if x["order"] == "shuffled"], "kernel_ms"),
                           "kernel_ms_grouped": med([x for x in order if x["order"] == "grouped_by_kind"], "kernel_ms")}})
        db.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps({k: v for k, v in result.items() if k != "reads"} | {"medians": [dict(n=x["n"], **x["median"]) for x in result["reads"]]}))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
