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

The repacked leg (--repacked): --features features (half polygons, half points) committed --versions
times at the same paths, each version editing a polygon's geometry or its attributes, or a point's
t50_fid; imported with --depth=0, then `git repack -adf --depth=D --window=W`, after which most blobs are
OFS_DELTA entries.  Every blob of every version is read in shuffled id order by three routes that
alternate --rounds times in one process: the host route, the device route with deltas off (delta blobs
read on the host and uploaded raw) and the device route with deltas on (kd_odb_read_batch_device_ex,
KD_RBD_DELTAS).  For the third: k_inf_streams and k_dl_apply per level by events, the eight counters, and
the host phases the store timed (plan, the header peeks in it, host reads + gather, device).

  python scripts/inflate_bench.py --repacked --features 50000 --versions 8 --out profiles/device_delta/bench.json
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


def _import_version(args):
    """one worker: every feature's blob of one version as a commit of its own branch (the same paths in
    every version, so a repack finds the earlier version of a feature by its name)"""
    gitdir, v, features, choice, pl, tl = args
    npoly = features // 2
    pk = np.arange(1, npoly + 1, dtype=np.int64)
    gver = choice[:v + 1, :npoly].sum(0).astype(np.uint64) if v else np.zeros(npoly, np.uint64)
    aver = np.uint64(v) - gver
    pdata, poff = synth.polygon_blobs(pk, gver, aver, pl)
    qk = np.arange(1, features - npoly + 1, dtype=np.int64)
    qdata, qoff = synth.point_blobs(qk, np.zeros(qk.shape[0], np.uint64), tl)
    if v:  # a point's edit: its t50_fid (bytes 77..81 of synth.point_blobs' layout)
        qdata = qdata.copy()
        h = synth.splitmix64(qk.view(np.uint64) ^ np.uint64(v << 40))
        at = qoff[:-1].astype(np.int64)[:, None] + 77 + np.arange(4)
        qdata[at] = (h[:, None] >> (np.uint64(8) * np.arange(4, dtype=np.uint64))).astype(np.uint8) & np.uint8(0x7F)
    parts, ids = [], bytearray()
    mark = 0
    for data, off in ((pdata, poff), (qdata, qoff)):
        raw = data.tobytes()
        for i in range(off.shape[0] - 1):
            b = raw[int(off[i]):int(off[i + 1])]
            ids += hashlib.sha1(b"blob %d\0" % len(b) + b).digest()
            mark += 1
            parts.append(b"blob\nmark :%d\ndata %d\n%s\n" % (mark, len(b), b))
    parts.append(b"commit refs/heads/v%d\ncommitter t <t@t> %d +0000\ndata 1\nx\n" % (v, 1600000000 + v))
    parts += [b"M 100644 :%d f/%d/%d\n" % (k + 1, k >> 10, k) for k in range(features)]
    parts.append(b"\n")
    subprocess.run(["git", "-c", "fastimport.unpackLimit=0", "fast-import", "--quiet", "--depth=0"], input=b"".join(parts),
                   env=dict(os.environ, GIT_DIR=gitdir), check=True)
    return bytes(ids)


def build_versioned(gitdir, features, versions, depth, window, procs=16):
    """-> unique blob ids [m, 20] of every version, after `git repack -adf --depth --window`; seconds of the repack"""
    from multiprocessing import Pool

    subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    pl = Legend(["c-fid"], [c["id"] for c in synth.POLYGON_SCHEMA[1:]]).hexhash()
    tl = Legend(["c-fid"], [c["id"] for c in synth.POINT_SCHEMA[1:]]).hexhash()
    choice = np.random.default_rng(5).integers(0, 2, (versions, features)).astype(np.int64)  # 1: a geometry edit
    choice[0] = 0
    with Pool(min(procs, versions)) as pool:
        ids = pool.map(_import_version, [(gitdir, v, features, choice, pl, tl) for v in range(versions)])
    t0 = time.perf_counter()
    subprocess.run(["git", "--git-dir", gitdir, "repack", "-adfq", f"--depth={depth}", f"--window={window}", f"--threads={procs}"],
                   check=True)
    ids = np.unique(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 20), axis=0)
    return ids, time.perf_counter() - t0


def device_delta_route(eng, db, oids, threads, deltas):
    eng.prof_reset()
    t0 = time.perf_counter()
    blobs, status, stats = db.read_batch_device(eng, oids, threads, deltas=deltas)
    t1 = time.perf_counter()
    assert not status.any()
    rec = {"route": "device_deltas" if deltas else "device", "wall_s": t1 - t0, "k_inf_streams_ms": eng.prof_get("k_inf_streams")[1],
           "inflated_bytes": blobs.nbytes, "stats": stats}
    if deltas:
        rec["k_dl_apply_ms_by_level"] = [eng.prof_get("k_dl_apply.%02d" % l)[1] for l in range(1, stats["depth"] + 1)]
        rec["k_dl_apply_ms"] = float(sum(rec["k_dl_apply_ms_by_level"]))
        rec["host_phases_s"] = {k: db.get_option("rbd_%s_us" % k) / 1e6 for k in ("plan", "peek", "host", "device")}
    return rec, blobs


def repacked_leg(a):
    from kart_amd.engine import Engine
    from kart_amd.odb import ObjectDB

    tmp = None
    gitdir = a.repo
    if gitdir is None:
        tmp = tempfile.TemporaryDirectory()
        gitdir = os.path.join(tmp.name, "versions.git")
    t0 = time.perf_counter()
    ids, repack_s = build_versioned(gitdir, a.features, a.versions, a.depth, a.window)
    print(f"{ids.shape[0]} blobs built and repacked in {time.perf_counter() - t0:.1f} s (repack {repack_s:.1f} s)", file=sys.stderr,
          flush=True)
    result = {"features": a.features, "versions": a.versions, "blobs": int(ids.shape[0]), "repack": f"-adf --depth={a.depth} --window={a.window}",
              "repack_s": repack_s, "threads": a.threads, "rounds": a.rounds}
    with Engine(0) as eng:
        eng.prof_enable(True)
        db = ObjectDB(gitdir)
        oids = np.ascontiguousarray(ids[np.random.default_rng(1).permutation(ids.shape[0])])
        warm = oids[:min(oids.shape[0], 100_000)]
        host_route(eng, db, warm, a.threads)
        for deltas in (False, True):
            device_delta_route(eng, db, warm, a.threads, deltas)
        runs = []
        for r in range(a.rounds):
            for fn in (host_route, lambda *x: device_delta_route(*x, False), lambda *x: device_delta_route(*x, True)):
                rec, keep = fn(eng, db, oids, a.threads)
                del keep
                rec["round"] = r
                runs.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
        db.close()
    med = lambda rows, key: float(np.median([x[key] for x in rows]))  # noqa: E731
    by = {name: [x for x in runs if x["route"] == name] for name in ("host", "device", "device_deltas")}
    dd = by["device_deltas"]
    result["runs"] = runs
    result["median"] = {"host_wall_s": med(by["host"], "wall_s"), "host_read_s": med(by["host"], "read_s"),
                        "host_upload_s": med(by["host"], "upload_s"), "device_wall_s": med(by["device"], "wall_s"),
                        "device_deltas_wall_s": med(dd, "wall_s"), "k_inf_streams_ms": med(dd, "k_inf_streams_ms"),
                        "k_dl_apply_ms": med(dd, "k_dl_apply_ms"),
                        "k_dl_apply_ms_by_level": np.median([x["k_dl_apply_ms_by_level"] for x in dd], axis=0).tolist(),
                        "host_phases_s": {k: med([x["host_phases_s"] for x in dd], k) for k in ("plan", "peek", "host", "device")},
                        "counters": dd[-1]["stats"], "device_counters": by["device"][-1]["stats"]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        extra = {}
        if os.path.exists(a.out):  # (lines recorded beside the comparison, e.g. the C3 step before / after, are kept)
            old = json.load(open(a.out))
            extra = {k: v for k, v in old.items() if k not in result}
        with open(a.out, "w") as f:
            f.write(json.dumps(result | extra, indent=1) + "\n")
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))
    if tmp is not None:
        tmp.cleanup()


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
    ap.add_argument("--repacked", action="store_true", help="the repacked leg: three routes on a repository of delta chains")
    ap.add_argument("--features", type=int, default=50_000)
    ap.add_argument("--versions", type=int, default=8)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--window", type=int, default=50)
    a = ap.parse_args()
    if a.repacked:
        return repacked_leg(a)
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
