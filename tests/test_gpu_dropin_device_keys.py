"""The drop-in with device_keys on: every side's join keys and their scan are made on the GPU
(kd_pack_keys_device) and the side stays in HBM; everything built from the versions is the same as with it off.
"""
import hashlib
import os

import numpy as np
import pytest

import walk_repos as R
from fixtures import load
from kart_amd import dataset as D
from kart_amd import merge as M
from kart_amd import packing
from kart_amd.gitsource import GitRepo
from test_dropin import version
from test_gpu_dropin_device_inflate import _points_repo
from test_merge_index import _fast_import_repo

pytestmark = pytest.mark.gpu


def _view(engine, old, new):
    """(deltas with their changed fields, exact blob count, how each side was packed)"""
    fd = D.get_dataset_diff(engine, old, new)["feature"]
    D.field_diff(engine, fd, old, new)
    view = {k: (d.type, sorted(d.changed_fields) if d.type == "update" else None) for k, d in fd.items()}
    how = [v.packed.timing.get("keys_on", "host") for v in (old, new) if v is not None and v.n]
    return view, D.get_exact_diff_blob_count(engine, old, new), how


def _both(engine, monkeypatch, make):
    out = []
    for on in (False, True):
        monkeypatch.setattr(D, "DEVICE_KEYS", on)
        view, count, how = _view(engine, *make())
        assert how and all(h == ("gpu" if on else "host") for h in how)
        out.append((view, count))
    assert out[0] == out[1] and len(out[0][0]) > 0
    return out[0]


def test_points_diff_is_the_same(engine, tmp_path, monkeypatch):
    gitdir = str(tmp_path / "repo.git")
    ds = _points_repo(gitdir, True)
    repo = GitRepo(gitdir)
    try:
        view, _ = _both(engine, monkeypatch, lambda: repo.diff_versions("refs/heads/c0", "refs/heads/c1", ds, engine=engine))
        assert sorted(k for k, (t, _) in view.items() if t == "update") == [1095, 1166, 1168, 1181, 1182]
    finally:
        repo.close()


def test_synthetic_diff_is_the_same(engine, tmp_path, monkeypatch):
    gitdir = str(tmp_path / "r.git")
    sub, _ = R.synthetic(gitdir)
    ds = sub.split("/.table-dataset")[0]
    repo = GitRepo(gitdir)
    try:
        _both(engine, monkeypatch, lambda: repo.diff_versions("main^", "main", ds, engine=engine))
    finally:
        repo.close()


@pytest.mark.parametrize("name", ["repo_string_pks", "synth_str"])
def test_hash_pk_diff_is_the_same(engine, monkeypatch, name):
    fx = load(name)
    for case in fx.cases("diff2")[:2]:
        monkeypatch.setattr(D, "DEVICE_KEYS", False)
        if version(fx, case["base"]) is None or version(fx, case["target"]) is None:
            continue
        _both(engine, monkeypatch, lambda: (version(fx, case["base"]), version(fx, case["target"])))
        monkeypatch.setattr(D, "DEVICE_KEYS", True)
        side = version(fx, case["target"]).pack(engine)
        assert side.key_mode == packing.GENERAL_ENCODING.key_mode and (side.dperm is not None or side.dev is not None)


def _legacy(fx, key):
    """the points fixture's version under the 2 x 256 hex layout (no path-structure.json)"""
    v = version(fx, key)
    names = [v.rel_path(i).rsplit("/", 1)[1] for i in range(v.n)]
    paths = []
    for nm in names:
        h = hashlib.sha256(nm.encode()).hexdigest()
        paths.append(f"{h[:2]}/{h[2:4]}/{nm}")
    arena, off = packing._arena(paths)
    return D.DatasetVersion(v.path, v.schema, v.legends, packing.LEGACY_ENCODING, arena, off, v.oids, v.read_blob, meta=v.meta)


def test_legacy_layout_diff_is_the_same(engine, monkeypatch):
    fx = load("repo_points")
    view, _ = _both(engine, monkeypatch, lambda: (_legacy(fx, "head1"), _legacy(fx, "head")))
    assert sorted(k for k, (t, _) in view.items() if t == "update") == [1095, 1166, 1168, 1181, 1182]


@pytest.mark.parametrize("name", ["conflicts_points", "conflicts_polygons", "conflicts_table"])
def test_merge_repo_is_the_same(engine, tmp_path, monkeypatch, name):
    fx = load(name)
    (case,) = fx.cases("merge3")
    repo = GitRepo(_fast_import_repo(tmp_path, fx, case["sides"], ["anc", "ours", "theirs"]))
    try:
        out = []
        for on in (False, True):
            monkeypatch.setattr(D, "DEVICE_KEYS", on)
            mi = M.merge_repo(engine, repo, "anc", "ours", "theirs")
            conflicts = {k: tuple((e.path, e.id, e.mode) if e else None for e in c) for k, c in mi.conflicts.items()}
            entries = {p: (e.id, e.mode) for p, e in mi.entries.items()}
            for k, c in mi.conflicts.items():
                mi.add_resolve(k, [c.ours or c.theirs])
            out.append((conflicts, entries, mi.write_tree(repo, engine)))
        assert out[0] == out[1] and out[0][0]
    finally:
        repo.close()


def test_module_default_and_environment(engine, monkeypatch):
    """device_keys=None follows dataset.DEVICE_KEYS, which is off unless the environment says so; without an
    engine, or with no leaf, nothing changes; GPU_SORT_MIN does not gate the option"""
    assert D.DEVICE_KEYS is (os.environ.get("KD_DEVICE_KEYS", "0") not in ("", "0"))
    fx = load("repo_points")
    assert fx.n("head") < D.GPU_SORT_MIN
    for flag in (False, True):
        monkeypatch.setattr(D, "DEVICE_KEYS", flag)
        s = version(fx, "head").pack(engine)
        assert (s.dev is not None) is flag and (s.timing.get("keys_on") == "gpu") is flag
        assert version(fx, "head").pack(engine, device_keys=not flag).timing.get("keys_on", "host") == ("host" if flag else "gpu")
        s = version(fx, "head").pack()  # no engine
        assert s.dev is None and s.dperm is None and "keys_on" not in s.timing
        assert version(fx, "head").pack(None, device_keys=True).dev is None
    host, dev = version(fx, "head").pack(engine, device_keys=False), version(fx, "head").pack(engine, device_keys=True)
    assert np.array_equal(host.key, dev.key) and np.array_equal(host.oid, dev.oid) and np.array_equal(host.order, dev.order)
    # a side packed by an engine that is gone is packed again
    from kart_amd.engine import Engine

    v = version(fx, "head")
    with Engine(0) as other:
        first = v.pack(other, device_keys=True)
        assert first.dev is not None
    again = v.pack(engine, device_keys=True)
    assert again is not first and np.array_equal(again.key, first.key)
