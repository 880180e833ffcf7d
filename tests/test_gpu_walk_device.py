"""ObjectDB.walk_device against ObjectDB.walk: the same paths, off, oids, modes and present for every
input — whatever the repository, the compare roots, the depth handed over and the pack layout, with the
delta route off and on.
"""
import os

import numpy as np
import pytest

import walk_repos as R
from kart_amd import _native as N
from kart_amd.odb import ObjectDB

pytestmark = pytest.mark.gpu


def _ids(gitdir, roots):
    return [R.git(gitdir, "rev-parse", r) for r in roots]


def same(engine, db, roots, sub, compare, depth, deltas=False):
    want = db.walk(roots, sub, compare)
    got, stats = db.walk_device(engine, roots, sub, compare, depth=depth, deltas=deltas)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.present == w.present
        assert np.array_equal(g.off, w.off)
        assert np.array_equal(g.paths, w.paths)
        assert np.array_equal(g.oids, w.oids)
        assert np.array_equal(g.modes, w.modes)
    assert stats["device_tasks"] + stats["host_tasks"] == stats["tasks"]
    return want, stats


def leaf_depth(db, roots, sub):
    L = db.walk(roots, sub)[0]
    return L.path(0).count("/")


def sweep(engine, gitdir, roots, sub, compares, depths=None):
    """every compare form x depth 0, the leaf depth, one less, one more x deltas off / on"""
    db = ObjectDB(gitdir)
    try:
        ids = _ids(gitdir, roots)
        d = leaf_depth(db, ids, sub)
        out = {}
        for cmp_ in compares:
            for depth in depths if depths is not None else (0, d, d - 1, d + 1):
                for deltas in (False, True):
                    out[cmp_, depth, deltas] = same(engine, db, ids, sub, cmp_, depth, deltas)
        return d, out
    finally:
        db.close()


@pytest.fixture(scope="module")
def points(tmp_path_factory):
    sub, versions = R.points_versions()
    g = str(tmp_path_factory.mktemp("wd") / "points.git")
    return g, R.import_versions(g, versions), sub, versions


def test_points_depth0_pack(engine, points):
    g, roots, sub, _ = points
    d, out = sweep(engine, g, roots, sub, [None, (0, 1)])
    assert d == 4
    for cmp_ in (None, (0, 1)):
        want, stats = out[cmp_, d, False]
        # --depth=0, no loose objects, every leaf tree in the device class (test_tree_craft_ref): all on the GPU
        assert stats["tasks"] > 0 and stats["host_tasks"] == 0 and stats["host"] == 0 and stats["fixups"] == 0
        assert stats["device"] == stats["trees"] and stats["batches"] == 1
        # one level up the trees handed over hold subtrees: every task is the host's, the result the same
        _, up = out[cmp_, d - 1, False]
        assert up["tasks"] > 0 and up["device_tasks"] == 0
        # one level down there is nothing to hand over: the host met the blobs above `depth`
        _, down = out[cmp_, d + 1, False]
        assert down["tasks"] == 0 and down["trees"] == 0
    assert out[None, d, False][1]["tasks"] > out[(0, 1), d, False][1]["tasks"]  # (pruned above the leaves)
    assert sum(L.n for L in out[(0, 1), d, False][0]) < sum(L.n for L in out[None, d, False][0])


def test_points_repacked(engine, points, tmp_path):
    g, roots, sub, _ = points
    b = R.repacked(g, str(tmp_path / "b.git"))
    d, out = sweep(engine, b, roots, sub, [None, (0, 1)], depths=None)
    _, off = out[(0, 1), d, False]
    _, on = out[(0, 1), d, True]
    assert on["deltas"] > 0 and off["deltas"] == 0  # (a changed leaf tree is a delta against its other version)
    assert on["host_tasks"] == 0 and off["host_tasks"] == 0


def test_points_two_packs_and_loose_trees(engine, points, tmp_path):
    _, _, sub, versions = points
    g = str(tmp_path / "c.git")
    roots = R.two_packs_and_loose(g, versions)
    d, out = sweep(engine, g, roots, sub, [None, (0, 1)], depths=(0, 4))
    assert out[(0, 1), 4, False][1]["host"] > 0  # (the loose trees are read on the host and uploaded)
    assert out[(0, 1), 4, False][1]["host_tasks"] == 0


def test_points_batches(engine, points):
    g, roots, sub, _ = points
    db = ObjectDB(g)
    try:
        ids = _ids(g, roots)
        db.set_option("walk_batch_bytes", 20000)
        assert db.get_option("walk_batch_bytes") == 20000
        for deltas in (False, True):
            _, stats = same(engine, db, ids, sub, None, 4, deltas)
            assert stats["batches"] >= 3 and stats["host_tasks"] == 0
        db.set_option("walk_batch_bytes", 1)  # one task per batch
        _, stats = same(engine, db, ids, sub, (0, 1), 4)
        assert stats["batches"] == stats["tasks"]
        with pytest.raises(N.KdError):
            db.set_option("walk_batch_bytes", 0)
    finally:
        db.close()


def test_synthetic_repository(engine, tmp_path):
    g = str(tmp_path / "r.git")
    sub, roots = R.synthetic(g)
    sweep(engine, g, roots, sub, [None, (0, 1)])


def test_hash_pk_layout(engine, tmp_path):
    sub, versions = R.string_pk_versions()
    g = str(tmp_path / "s.git")
    roots = R.import_versions(g, versions)
    d, out = sweep(engine, g, roots, sub, [None, (0, 1)])
    assert out[(0, 1), d, False][1]["host_tasks"] == 0
    sweep(engine, R.repacked(g, str(tmp_path / "s2.git")), roots, sub, [(0, 1)], depths=(d,))


def test_legacy_layout_and_host_class_tasks(engine, tmp_path):
    """2-level hex directories; at leaf depth: a tree on one side only, a tree that also holds a subtree
    (KD_TJ_ETREE) and one of 8,000 entries (above KD_INF_MAX): the last two are walked by the host"""
    sub, versions = R.legacy_versions()
    g = str(tmp_path / "l.git")
    roots = R.import_versions(g, versions)
    d, out = sweep(engine, g, roots, sub, [None, (0, 1)])
    assert d == 2
    for cmp_ in (None, (0, 1)):
        want, stats = out[cmp_, d, False]
        assert stats["host_tasks"] == 2 and stats["device_tasks"] > 50
        paths = {want[1].path(i) for i in range(want[1].n)}
        assert "zz/only-new/f" in paths and "7f/mixed/deeper/leaf" in paths and "80/big/e0001000" in paths
        assert "yy/only-old/f" in {want[0].path(i) for i in range(want[0].n)}
    sweep(engine, R.repacked(g, str(tmp_path / "l2.git")), roots, sub, [(0, 1)], depths=(d,))


@pytest.mark.parametrize("name", ["conflicts_points", "conflicts_polygons", "conflicts_table"])
def test_three_roots(engine, tmp_path, name):
    sub, versions = R.conflicts_versions(name)
    g = str(tmp_path / "c.git")
    roots = R.import_versions(g, versions)
    d, out = sweep(engine, g, roots, sub, [(1, 2), (0, 2)])
    assert out[(1, 2), d, False][1]["device_tasks"] > 0 and out[(1, 2), d, False][1]["host_tasks"] == 0


def test_subpath_absent_in_one_root(engine, tmp_path):
    sub, versions = R.legacy_versions()
    g = str(tmp_path / "l.git")
    ids = _ids(g, R.import_versions(g, versions))
    db = ObjectDB(g)
    try:
        for depth in (0, 1):
            want, _ = same(engine, db, ids, sub + "/zz", (0, 1), depth)
            assert [L.present for L in want] == [False, True] and want[1].n == 1
            want, _ = same(engine, db, ids, sub + "/nowhere", None, depth)
            assert [L.present for L in want] == [False, False]
    finally:
        db.close()


def test_deleted_tree_gives_kd_walk_s_error(engine, tmp_path):
    sub, versions = R.string_pk_versions()
    g = str(tmp_path / "s.git")
    roots = R.import_versions(g, versions, loose=True)
    ids = _ids(g, roots)
    victim = R.git(g, "rev-parse", f"{roots[1]}:{sub}/z/z/z/2")
    os.remove(os.path.join(g, "objects", victim[:2], victim[2:]))
    db = ObjectDB(g)
    try:
        with pytest.raises(N.NotFound) as e0:
            db.walk(ids, sub, (0, 1))
        for depth in (0, 4):
            with pytest.raises(N.NotFound) as e1:
                db.walk_device(engine, ids, sub, (0, 1), depth=depth)
            assert e1.value.code == e0.value.code == N.KD_ENOTFOUND and victim in str(e1.value)
    finally:
        db.close()
