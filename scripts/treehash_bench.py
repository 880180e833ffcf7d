"""kd_tree_hash and write_tree(repo, engine), timed.

1. ``--leaves-int`` leaves (default 100M) in 64-entry leaf trees with 8-character names, then the
   directory levels above them (64 one-character entries per tree) up to the root: every level one
   device-form kd_tree_hash call on resident inputs, the ids of a level read by the next on the device.
2. ``--leaves-hash`` leaves (default 50M) in leaf trees of 1..5 entries with names of 24..40
   characters in arbitrary order, hashed with KD_TH_RANK_NAMES.
   For both, each level's device time is the sum of its kernels' times, HIP events around every
   launch (kd_prof_*), over ``--reps`` repetitions after one untimed call; the call's wall time (which
   includes its one 32-byte readback) is given beside it.
3. A synthetic repository of ``--repo-leaves`` features (default 1M) with three branches: the merge's
   ``write_tree(repo)`` (per-leaf Python + git update-index + git write-tree) against
   ``write_tree(repo, engine)``, in one process, the engine route before and after the index route.
   The script fails unless the ids agree and the engine route is the faster one.

Prints one JSON object and writes it to --out.

    python scripts/treehash_bench.py --out profiles/tree_hash/bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TH_KERNELS = ("k_th_check", "k_th_size", "k_th_scan1", "k_th_scan2", "k_th_scan3", "k_th_frame", "k_th_format", "k_th_sha1")
ALPHA = np.frombuffer(b"-0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz", np.uint8)  # ascending


def timed_level(eng, call, reps):
    """(kernel ms per call by name, wall ms per call) of ``call``"""
    call()  # (workspace growth and first-launch costs stay out)
    eng.sync()
    eng.prof_reset()
    eng.prof_select(TH_KERNELS)
    eng.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = call()
    eng.sync()
    wall = (time.perf_counter() - t0) / reps
    eng.prof_enable(False)
    eng.prof_select(None)
    kern = {}
    for k in TH_KERNELS:
        n, ms = eng.prof_get(k)
        if n:
            kern[k] = round(ms / reps, 4)
    return out, kern, 1e3 * wall


def level_row(name, n, nt, kern, wall_ms, body_bytes):
    dev = sum(kern.values())
    return {"level": name, "entries": int(n), "trees": int(nt), "body_bytes": int(body_bytes), "device_ms": round(dev, 4),
            "call_wall_ms": round(wall_ms, 3), "kernels_ms": kern,
            "entries_per_s": round(n / (dev * 1e-3)) if dev else None, "sha1_GBps": round(body_bytes / (kern.get("k_th_sha1", 0) * 1e6), 2)
            if kern.get("k_th_sha1") else None}


def int_layer(eng, n, reps):
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    rng = np.random.default_rng(1)
    j = np.arange(n, dtype=np.int64) & 63
    names = rng.integers(0x61, 0x7B, (n, 8), dtype=np.uint8)
    names[:, 0] = ALPHA[j]  # ascending inside each 64-entry run
    d_names = DevBuf.from_numpy(eng, names.reshape(-1))
    del names
    d_off = DevBuf.from_numpy(eng, np.arange(n + 1, dtype=np.uint64) * np.uint64(8))
    d_oid = DevBuf(eng, 20 * n)
    chunk = 1 << 24
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        d_oid.upload(rng.integers(0, 256, 20 * m, dtype=np.uint8), offset=20 * s)
    rows, kind, width = [], N.KD_TE_BLOB, 8
    while True:
        nt = (n + 63) // 64
        d_seg = DevBuf.from_numpy(eng, np.minimum(np.arange(nt + 1, dtype=np.uint64) * np.uint64(64), np.uint64(n)))
        (ids, st), kern, wall = timed_level(eng, lambda: eng.tree_hash(d_names, d_off, d_oid, d_seg, kind), reps)
        assert not st.download(np.uint8, nt).any()
        rows.append(level_row("leaf trees" if kind == N.KD_TE_BLOB else "directories", n, nt, kern, wall,
                              n * ((7 if kind == N.KD_TE_BLOB else 6) + 21 + width)))
        if nt == 1:
            return rows, ids.download(np.uint8, 20).tobytes().hex()
        n, kind, width, d_oid = nt, N.KD_TE_TREE, 1, ids
        d_names = DevBuf.from_numpy(eng, ALPHA[np.arange(n) & 63])
        d_off = DevBuf.from_numpy(eng, np.arange(n + 1, dtype=np.uint64))


def hash_layer(eng, n, reps):
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    rng = np.random.default_rng(2)
    sizes = rng.integers(1, 6, n // 3 + 8)
    seg = np.concatenate([[0], np.cumsum(sizes)])
    seg = np.append(seg[seg < n], n).astype(np.uint64)
    nt = seg.size - 1
    lens = rng.integers(24, 41, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    d_names = DevBuf(eng, int(off[-1]))
    chunk = 1 << 28
    for s in range(0, int(off[-1]), chunk):
        m = min(chunk, int(off[-1]) - s)
        d_names.upload(rng.integers(0x61, 0x7B, m, dtype=np.uint8), offset=s)
    d_off, d_seg = DevBuf.from_numpy(eng, off), DevBuf.from_numpy(eng, seg)
    d_oid = DevBuf(eng, 20 * n)
    for s in range(0, n, 1 << 24):
        m = min(1 << 24, n - s)
        d_oid.upload(rng.integers(0, 256, 20 * m, dtype=np.uint8), offset=20 * s)
    (ids, st), kern, wall = timed_level(eng, lambda: eng.tree_hash(d_names, d_off, d_oid, d_seg, N.KD_TE_BLOB, rank=True), reps)
    bad = int(np.count_nonzero(st.download(np.uint8, nt)))
    row = level_row("leaf trees, ranked", n, nt, kern, wall, 28 * n + int(off[-1]))
    row["trees_with_status"] = bad  # (two equal random names in one run: none expected)
    return [row]


def synthetic_repo(td, n):
    """a bare repository with branches anc / ours / theirs over one int-pk dataset of n features: ours
    and theirs edit, delete and insert disjoint features"""
    from fixtures import load
    from kart_amd import synth

    fx = load("conflicts_points")
    side = fx.meta["sides"]["ancestor"]
    ds = fx.meta["ds_path"]
    inner = f"{ds}/.table-dataset"
    gitdir = os.path.join(td, "bench.git")
    subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    nblob = 1024
    out = []
    for b in range(nblob):  # feature blobs shared by many features: the tree writer never reads them
        data = fx.blob(b % len(fx.blob_off[:-1])) + b"%d" % b
        out.append(b"blob\nmark :%d\ndata %d\n" % (b + 1, len(data)) + data + b"\n")
    meta = {f"{inner}/meta/schema.json": json.dumps(side["schema"]).encode(),
            f"{inner}/meta/path-structure.json": json.dumps(side["path_structure"]).encode(),
            ".kart.repostructure.version": b"3\n"}
    for h, lg in fx.legends.items():
        meta[f"{inner}/meta/legend/{h}"] = lg.dumps()
    marks = {}
    for k, (p, data) in enumerate(meta.items()):
        marks[p] = nblob + 1 + k
        out.append(b"blob\nmark :%d\ndata %d\n" % (marks[p], len(data)) + data + b"\n")
    pk = np.arange(n + 2000, dtype=np.int64)
    arena, off = synth.int_pk_paths(pk)
    paths = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(pk.size)]
    pre = f"{inner}/feature/".encode()

    def line(i, ver):
        return b"M 100644 :%d %s%s\n" % ((i + ver) % nblob + 1, pre, paths[i])

    out.append(b"commit refs/heads/anc\nmark :900000\ncommitter t <t@t> 1600000000 +0000\ndata 1\nx\ndeleteall\n")
    out += [b"M 100644 :%d %s\n" % (m, p.encode()) for p, m in marks.items()]
    out += [line(i, 0) for i in range(n)]
    out.append(b"\n")
    step = max(n // 5000, 1)
    for br, lo, ins in (("ours", 0, range(n, n + 1000)), ("theirs", step // 2 + 1, range(n + 1000, n + 2000))):
        out.append(b"commit refs/heads/%s\ncommitter t <t@t> 1600000001 +0000\ndata 1\nx\nfrom :900000\n" % br.encode())
        ed = range(lo, n, step)
        out += [line(i, 1) for i in ed[::2]]
        out += [b"D %s%s\n" % (pre, paths[i]) for i in ed[1::2]]
        out += [line(i, 0) for i in ins]
        out.append(b"\n")
    subprocess.run(["git", "fast-import", "--quiet"], input=b"".join(out), env=dict(os.environ, GIT_DIR=gitdir), check=True)
    return gitdir


def end_to_end(eng, n):
    from kart_amd import merge as M
    from kart_amd.gitsource import GitRepo

    with tempfile.TemporaryDirectory() as td:
        repo = GitRepo(synthetic_repo(td, n))
        try:
            mi = M.merge_repo(eng, repo, "anc", "ours", "theirs")
            assert not mi.conflicts
            runs = []
            for route in ("engine", "index", "engine"):
                t0 = time.perf_counter()
                tid = mi.write_tree(repo, eng) if route == "engine" else mi.write_tree(repo)
                runs.append({"route": route, "seconds": round(time.perf_counter() - t0, 3), "tree": tid})
            leaves = len(mi.entries)
        finally:
            repo.close()
    assert len({r["tree"] for r in runs}) == 1, runs
    eng_s = max(r["seconds"] for r in runs if r["route"] == "engine")
    idx_s = min(r["seconds"] for r in runs if r["route"] == "index")
    assert eng_s < idx_s, runs
    return {"merged_entries": leaves, "runs": runs, "engine_seconds_worst": eng_s, "index_seconds": idx_s,
            "note": "index = write_tree(repo): per-leaf Python + git update-index + git write-tree; engine = "
                    "write_tree(repo, engine); the first engine run writes the objects, the second finds them there"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves-int", type=int, default=100_000_000)
    ap.add_argument("--leaves-hash", type=int, default=50_000_000)
    ap.add_argument("--repo-leaves", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kart_amd.engine import Engine

    res = {"what": "kd_tree_hash per level (device form, resident inputs) and write_tree end to end", "reps": a.reps}
    with Engine(0) as eng:
        if a.repo_leaves:
            res["write_tree_end_to_end"] = end_to_end(eng, a.repo_leaves)
        if a.leaves_int:
            rows, root = int_layer(eng, a.leaves_int, a.reps)
            res["int_layer"] = {"leaves": a.leaves_int, "root": root, "levels": rows,
                                "device_ms_all_levels": round(sum(r["device_ms"] for r in rows), 3)}
        if a.leaves_hash:
            res["hash_layer"] = {"leaves": a.leaves_hash, "levels": hash_layer(eng, a.leaves_hash, a.reps)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
