"""bench.py's options: a plain run holds the headline only and every other leg waits behind --full;
--dump-outputs writes what the timed path computed; the layer joined from shards is the one-piece
layer."""
import os
import sys

import numpy as np
import pytest

import bench
from kart_amd import synth


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_every_other_leg_off(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_host_timing and a.no_sort and a.no_radix and a.no_arena_timing and a.no_heads_path
    a = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert not (a.no_cpu_baseline or a.no_host_timing or a.no_sort or a.no_radix or a.no_arena_timing or a.no_heads_path)
    assert _args(monkeypatch, "--full", "--no-cpu-baseline").no_cpu_baseline


@pytest.mark.parametrize("n,same_len", [(30_000, 0.0), (50_001, 0.6), (700, 0.0)])
def test_joined_layer_is_the_one_piece_layer(n, same_len):
    a, b = synth.polygons_layer(n, same_len=same_len), bench.polygons_layer_joined(n, same_len)
    for side in ("base", "target"):
        x, y = getattr(a, side), getattr(b, side)
        for f in ("key", "oid", "order"):
            u, v = getattr(x, f), getattr(y, f)
            assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v) and v.flags.c_contiguous
        assert (x.key_mode, x.encoding) == (y.key_mode, y.encoding)
    for p, q in ((a.base_blobs, b.base_blobs), (a.target_blobs, b.target_blobs)):
        for u, v in zip(p, q):
            assert u.dtype == v.dtype and np.array_equal(u, v)
    assert (a.n_insert, a.n_update, a.n_delete) == (b.n_insert, b.n_update, b.n_delete)
    assert a.legends.keys() == b.legends.keys()


class _H:
    rank = 0


def test_dump_outputs_float64_within_budget_and_repeatable(tmp_path, monkeypatch):
    rows = bench.DUMP_BYTES // 3 // 16  # what fits of a two-column array sharing the budget with two others
    big = np.arange(2 * (rows + 1000), dtype=np.uint32).reshape(-1, 2)
    arrays = {"small": np.array([3, 2, 1], np.uint64), "big": big, "bytes": np.arange(200, dtype=np.uint8)}
    for d in ("a", "b"):
        bench.dump_outputs(_args(monkeypatch, "--dump-outputs", str(tmp_path / d)), _H, arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big", "bytes", "small"] and all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["small"], [3, 2, 1]) and np.array_equal(got["bytes"], np.arange(200))
    assert got["big"].shape == (rows, 2)  # a sample of whole rows, in their order
    assert np.all(np.diff(got["big"][:, 0]) > 0) and np.array_equal(got["big"][:, 1], got["big"][:, 0] + 1)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 1000 * 1000
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")) for k, v in got.items())
    with pytest.raises(AssertionError):  # a value float64 cannot hold is refused, not rounded
        bench.dump_outputs(_args(monkeypatch, "--dump-outputs", str(tmp_path / "c")), _H, {"x": np.array([2**63 + 1], np.uint64)})
    bench.dump_outputs(_args(monkeypatch), _H, arrays)  # no option, no files
    assert sorted(os.listdir(tmp_path)) == ["a", "b", "c"]
