"""kd_pack_keys_device against the host pair it replaces, in one process.

Inputs resident in HBM: the C3 layer's int-PK paths (--n-int, 100M) and a hash-PK arena (--n-hash, 50M), both
in walk order.  The device call is timed by HIP events on a stream of this script's own over --calls calls after
warm-up, and per kernel with kd_prof_*; alternated with it, kd_pack_int_keys / kd_pack_hash_keys + kd_keys_scan
run on the same host arrays with the process held to --cpus CPUs.  Reports median and min-max of both, the
algorithmic bytes (path bytes + 8 B offset + 8 B key + 1 B status per entry), their fraction of 8.0 TB/s and
the one-time upload that pack_side's route adds and a device-born side does not.

    python scripts/keypack_bench.py --out profiles/keypack/bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kart_amd import _native as N  # noqa: E402
from kart_amd import packing, synth, walkkey  # noqa: E402
from kart_amd.device import DevBuf  # noqa: E402
from kart_amd.engine import Engine  # noqa: E402

PEAK = 8.0e12
KERNELS = ("k_kp_pack", "k_kp_fold", "k_kp_info")


def int_arena(n, chunk=10_000_000):
    pks = walkkey.walk_order_pks(n)
    parts, offs, at = [], [np.zeros(1, np.uint64)], 0
    for a in range(0, n, chunk):
        arena, off = synth.int_pk_paths(pks[a:a + chunk])
        parts.append(arena)
        offs.append(off[1:] + np.uint64(at))
        at += int(off[-1])
        print(f"  int paths {min(n, a + chunk):,}", flush=True)
    return np.concatenate(parts), np.concatenate(offs)


def hash_arena(n):
    paths, plen = synth.text_pk_paths(*synth.text_pks(np.arange(n, dtype=np.int64)))
    print("  hash paths made", flush=True)
    order = synth._walk_order(paths)
    print("  hash paths ordered", flush=True)
    return synth._arena(paths, plen, order)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def bench(eng, hip, stream, name, data, off, enc, calls, tile):
    n = off.shape[0] - 1
    eng.set_option("kp_tile", tile)
    t0 = time.perf_counter()
    d_paths = DevBuf.from_numpy(eng, np.concatenate([data, np.zeros(16, np.uint8)]))
    d_off = DevBuf.from_numpy(eng, off)
    upload_s = time.perf_counter() - t0
    d_keys, d_status, d_info = DevBuf(eng, 8 * n), DevBuf(eng, n), DevBuf(eng, 64)
    hex_ = 1 if enc.encoding == "hex" else 0
    args = (eng.ctx, d_paths.ptr, d_off.ptr, n, enc.key_mode, enc.levels, hex_, d_keys.ptr, d_status.ptr, d_info.ptr)
    keys, status = np.empty(n, np.uint64), np.empty(n, np.uint8)
    info = N.KdKeysInfo()
    L = eng.L

    def host():
        t = time.perf_counter()
        if enc.key_mode == N.KD_KEY_INT:
            bad = L.kd_pack_int_keys(N.ptr(data), N.ptr(off), n, N.ptr(keys), N.ptr(status))
        else:
            bad = L.kd_pack_hash_keys(N.ptr(data), N.ptr(off), n, enc.levels, hex_, N.ptr(keys), N.ptr(status))
        t1 = time.perf_counter()
        N.check(L.kd_keys_scan(N.ptr(keys), n, enc.key_mode, ctypes.byref(info)), "kd_keys_scan")
        assert bad == 0
        return 1e3 * (t1 - t), 1e3 * (time.perf_counter() - t1)

    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    for _ in range(3):  # warm-up (the workspaces grow here)
        N.check(L.kd_pack_keys_device(*args), "kd_pack_keys_device")
    eng.sync()
    host()
    dev_ms, host_pack_ms, host_scan_ms = [], [], []
    for i in range(calls):
        assert hip.hipEventRecord(ev[0], stream) == 0
        N.check(L.kd_pack_keys_device(*args), "kd_pack_keys_device")
        assert hip.hipEventRecord(ev[1], stream) == 0
        assert hip.hipEventSynchronize(ev[1]) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0
        dev_ms.append(ms.value)
        if i % 5 == 0:  # the yardstick, alternated
            p, s = host()
            host_pack_ms.append(p)
            host_scan_ms.append(s)
            print(f"  {name} call {i}: device {ms.value:.3f} ms, host {p:.1f} + {s:.1f} ms", flush=True)
    eng.prof_reset()
    eng.prof_enable(True)
    for _ in range(10):
        N.check(L.kd_pack_keys_device(*args), "kd_pack_keys_device")
    eng.sync()
    per_kernel = {k: (lambda c, ms: {"launches": c, "ms_per_call": ms / 10})(*eng.prof_get(k)) for k in KERNELS}
    eng.prof_enable(False)
    got = N.KdKeypackInfo.from_buffer_copy(d_info.download(np.uint8, 56).tobytes())
    same = (np.array_equal(d_keys.download(np.uint64, n), keys) and got.bad == 0 and
            bytes(got.info) == bytes(info))
    nbytes = int(off[-1]) - int(off[0]) + 17 * n
    med = statistics.median(dev_ms)
    return {
        "entries": n, "path_bytes": int(off[-1]) - int(off[0]), "algorithmic_bytes": nbytes, "tile": tile,
        "device": stats(dev_ms), "device_tb_s": nbytes / (med * 1e-3) / 1e12, "fraction_of_8_tb_s": nbytes / (med * 1e-3) / PEAK,
        "per_kernel": per_kernel, "hbm_tiles": eng.get_option("kp_hbm_tiles"),
        "host_pack": stats(host_pack_ms), "host_scan": stats(host_scan_ms),
        "host_pair_median_ms": statistics.median([p + s for p, s in zip(host_pack_ms, host_scan_ms)]),
        "upload_paths_offsets_s": upload_s, "equal_to_host": bool(same),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-int", type=int, default=100_000_000)
    ap.add_argument("--n-hash", type=int, default=50_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--tiles", default="512,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cpus = sorted(os.sched_getaffinity(0))[:a.cpus]
    os.sched_setaffinity(0, cpus)
    hip = ctypes.CDLL("libamdhip64.so")
    for f in (hip.hipEventRecord,):
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    res = {"cpus": len(cpus), "host_threads": min(32, os.cpu_count() or 1), "calls": a.calls, "runs": {}}
    with Engine(0) as eng:
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        eng.set_stream(stream)
        for name, make, n, enc in (("int", int_arena, a.n_int, packing.INT_PK_ENCODING),
                                   ("hash", hash_arena, a.n_hash, packing.GENERAL_ENCODING)):
            if n <= 0:
                continue
            print(f"{name}: {n:,} paths", flush=True)
            data, off = make(n)
            for tile in (int(t) for t in a.tiles.split(",")):
                r = bench(eng, hip, stream, name, data, off, enc, a.calls, tile)
                res["runs"][f"{name}_tile{tile}"] = r
                print(json.dumps({f"{name}_tile{tile}": r}), flush=True)
            del data, off
        eng.set_stream(None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
