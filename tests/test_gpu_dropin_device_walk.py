"""The drop-in with device_walk on: the pruned walk of diff_versions / merge_versions reads and joins its
changed leaf trees on the GPU, and everything built from the versions is the same as with it off.
"""
import os

import pytest

import walk_repos as R
from fixtures import load
from kart_amd import dataset as D
from kart_amd import merge as M
from kart_amd.gitsource import GitRepo
from test_gpu_dropin_device_inflate import _points_repo
from test_merge_index import _fast_import_repo

pytestmark = pytest.mark.gpu


def _diff(engine, repo, base, target, ds, on):
    repo.last_walk_stats = None
    old, new = repo.diff_versions(base, target, ds, engine=engine, device_walk=on)
    walked = repo.last_walk_stats
    fd = D.get_dataset_diff(engine, old, new)["feature"]
    D.field_diff(engine, fd, old, new)
    view = {k: (d.type, sorted(d.changed_fields) if d.type == "update" else None) for k, d in fd.items()}
    return view, D.get_exact_diff_blob_count(engine, old, new), walked


def test_points_diff_is_the_same(engine, tmp_path):
    gitdir = str(tmp_path / "repo.git")
    ds = _points_repo(gitdir, True)
    repo = GitRepo(gitdir)
    try:
        off, n_off, w_off = _diff(engine, repo, "refs/heads/c0", "refs/heads/c1", ds, False)
        on, n_on, w_on = _diff(engine, repo, "refs/heads/c0", "refs/heads/c1", ds, True)
        assert on == off and n_on == n_off and len(on) > 0
        assert w_off is None and w_on["tasks"] > 0 and w_on["host_tasks"] == 0
        assert sorted(k for k, (t, _) in on.items() if t == "update") == [1095, 1166, 1168, 1181, 1182]
    finally:
        repo.close()


def test_synthetic_diff_is_the_same(engine, tmp_path):
    gitdir = str(tmp_path / "r.git")
    sub, _ = R.synthetic(gitdir)
    ds = sub.split("/.table-dataset")[0]
    repo = GitRepo(gitdir)
    try:
        off, n_off, _ = _diff(engine, repo, "main^", "main", ds, False)
        on, n_on, w_on = _diff(engine, repo, "main^", "main", ds, True)
        assert on == off and n_on == n_off and w_on["device_tasks"] > 0
    finally:
        repo.close()


@pytest.mark.parametrize("name", ["conflicts_points", "conflicts_polygons", "conflicts_table"])
def test_merge_repo_is_the_same(engine, tmp_path, monkeypatch, name):
    fx = load(name)
    (case,) = fx.cases("merge3")
    repo = GitRepo(_fast_import_repo(tmp_path, fx, case["sides"], ["anc", "ours", "theirs"]))
    try:
        out = []
        for on in (False, True):
            monkeypatch.setattr(D, "DEVICE_WALK", on)
            repo.last_walk_stats = None
            mi = M.merge_repo(engine, repo, "anc", "ours", "theirs")
            assert (repo.last_walk_stats is not None) is on
            conflicts = {k: tuple((e.path, e.id, e.mode) if e else None for e in c) for k, c in mi.conflicts.items()}
            entries = {p: (e.id, e.mode) for p, e in mi.entries.items()}
            for k, c in mi.conflicts.items():
                mi.add_resolve(k, [c.ours or c.theirs])
            out.append((conflicts, entries, mi.write_tree(repo, engine)))
        assert out[0] == out[1] and out[0][0]
    finally:
        repo.close()


def test_module_default_and_environment(engine, tmp_path, monkeypatch):
    """device_walk=None follows dataset.DEVICE_WALK, which is off unless the environment says so; without an
    engine nothing changes"""
    assert D.DEVICE_WALK is (os.environ.get("KD_DEVICE_WALK", "0") not in ("", "0"))
    gitdir = str(tmp_path / "repo.git")
    ds = _points_repo(gitdir, True)
    repo = GitRepo(gitdir)
    try:
        for flag in (False, True):
            monkeypatch.setattr(D, "DEVICE_WALK", flag)
            repo.last_walk_stats = None
            repo.diff_versions("refs/heads/c0", "refs/heads/c1", ds, engine=engine)
            assert (repo.last_walk_stats is not None) is flag
            repo.last_walk_stats = None
            repo.diff_versions("refs/heads/c0", "refs/heads/c1", ds)
            assert repo.last_walk_stats is None
            repo.dataset_versions(["refs/heads/c1"], ds, engine=engine)  # (no compare: no pruned walk)
            assert repo.last_walk_stats is None
    finally:
        repo.close()


def test_different_path_structures_take_the_host_walk(engine, tmp_path):
    import json

    fx = load("repo_points")
    ds = fx.meta["ds_path"]
    inner = f"{ds}/.table-dataset"
    versions = []
    for key, levels in (("head1", 4), ("head", 3)):
        ps = dict(fx.meta["sides"][key]["path_structure"], levels=levels)
        files = {f"{inner}/feature/{nm if levels == 4 else nm[2:]}": fx.blob(int(bi))
                 for nm, bi in zip(fx.names(key), fx.a[f"{key}_blob"])}
        files[f"{inner}/meta/schema.json"] = json.dumps(fx.meta["sides"][key]["schema"]).encode()
        files[f"{inner}/meta/path-structure.json"] = json.dumps(ps).encode()
        for h, lg in fx.legends.items():
            files[f"{inner}/meta/legend/{h}"] = lg.dumps()
        versions.append(files)
    gitdir = str(tmp_path / "two.git")
    roots = R.import_versions(gitdir, versions)
    repo = GitRepo(gitdir)
    try:
        old, new = repo.diff_versions(roots[0], roots[1], ds, engine=engine, device_walk=True)
        assert repo.last_walk_stats is None and not old.partial and not new.partial
        assert old.n == fx.n("head1") and new.n == fx.n("head")
    finally:
        repo.close()
