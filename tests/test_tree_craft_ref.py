"""The Python reference of the leaf join (tree_craft.py) pinned to ObjectDB.walk on the repositories the
device walk's tests use, on the CPU: wherever the reference takes a level of trees as device class, its
join of that level is what the generic git rule gives, and the walk built from it is kd_walk's.
"""
import pytest

import tree_craft as C
import walk_repos as R
from kart_amd.odb import ObjectDB


def _tree_of(db, gitdir, root, sub):
    return bytes.fromhex(R.git(gitdir, "rev-parse", f"{root}:{sub}"))


def _pin(gitdir, roots, sub, compares):
    db = ObjectDB(gitdir)
    try:
        tops = [_tree_of(db, gitdir, r, sub) for r in roots]
        read = lambda oid: db.read(oid)[1]
        for cmp_ in compares:
            stats = {}
            want = C.walk(read, tops, cmp_, stats=stats)
            got = db.walk([R.git(gitdir, "rev-parse", r) for r in roots], sub, cmp_)
            for r, L in enumerate(got):
                paths = [bytes(L.paths[int(L.off[i]):int(L.off[i + 1])]) for i in range(L.n)]
                assert paths == [p for p, _, _ in want[r]]
                assert L.modes.tolist() == [m for _, m, _ in want[r]]
                assert L.oids.tobytes() == b"".join(o for _, _, o in want[r])
        return stats
    finally:
        db.close()


def test_points(tmp_path):
    sub, versions = R.points_versions()
    g = str(tmp_path / "p.git")
    roots = R.import_versions(g, versions)
    stats = _pin(g, roots, sub, [None, (0, 1)])
    assert stats["levels"] > stats["device_class"] > 0  # (the upper levels hold subtrees)


def test_points_leaf_trees_are_all_device_class(tmp_path):
    """what test_gpu_walk_device asserts as "every task on the device" on the --depth=0 layout"""
    sub, versions = R.points_versions()
    g = str(tmp_path / "p.git")
    roots = R.import_versions(g, versions)
    db = ObjectDB(g)
    try:
        L = db.walk([R.git(g, "rev-parse", r) for r in roots], sub)[0]
        dirs = {bytes(L.paths[int(L.off[i]):int(L.off[i + 1])]).rsplit(b"/", 1)[0] for i in range(L.n)}
        for d in dirs:
            for r in roots:
                st, ents = C.parse(db.read(bytes.fromhex(R.git(g, "rev-parse", f"{r}:{sub}/{d.decode()}")))[1])
                assert st == C.OK and ents
    finally:
        db.close()


def test_string_pks_and_legacy(tmp_path):
    for name, (sub, versions) in (("s", R.string_pk_versions()), ("l", R.legacy_versions())):
        g = str(tmp_path / f"{name}.git")
        roots = R.import_versions(g, versions)
        _pin(g, roots, sub, [None, (0, 1)])


@pytest.mark.parametrize("name", ["conflicts_points", "conflicts_polygons", "conflicts_table"])
def test_conflicts(tmp_path, name):
    sub, versions = R.conflicts_versions(name)
    g = str(tmp_path / "c.git")
    roots = R.import_versions(g, versions)
    _pin(g, roots, sub, [(1, 2), (0, 2)])


def test_synthetic(tmp_path):
    g = str(tmp_path / "r.git")
    sub, roots = R.synthetic(g)
    _pin(g, roots, sub, [(0, 1)])
