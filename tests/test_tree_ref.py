"""The hashlib tree reference against git itself, and the host half of the tree writer on it (CPU):
tree_ref vs `git mktree`, the recorded feature-tree ids of tests/golden/tree_ids.json rebuilt from the
fixtures' names and oids, the pack writer through `git unpack-objects`, and treebuild.feature_tree
(levels, ``known`` subtrees) on RefEngine."""
import json
import os
import subprocess

import numpy as np
import pytest

import tree_ref as R
from fixtures import GOLDEN, load
from kart_amd import treebuild as TB

with open(os.path.join(GOLDEN, "tree_ids.json")) as f:
    TREE_IDS = json.load(f)
SIDES = [(fx, side) for fx, sides in TREE_IDS.items() for side in sides]


@pytest.fixture(scope="module")
def gitdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mktree") / "r.git")
    subprocess.run(["git", "init", "-q", "--bare", d], check=True)
    return d


def mktree(gitdir, entries, kind):
    typ = "tree" if kind == R.TREE else "blob"
    text = b"".join(b"%s %s %s\t%s\0" % (R.MODE[kind].rjust(6, b"0"), typ.encode(), o.hex().encode(), n) for n, o in entries)
    return subprocess.run(["git", "--git-dir", gitdir, "mktree", "-z", "--missing"], input=text, check=True,
                          capture_output=True).stdout.decode().strip()


def _oid(rng):
    return rng.integers(0, 256, 20, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("kind", [R.BLOB, R.TREE])
def test_prefix_order_and_empty_tree(gitdir, kind):
    rng = np.random.default_rng(1)
    names = [b"a", b"a-", b"a0", b"ab", "é".encode()]
    ents = [(n, _oid(rng)) for n in names]
    assert R.tree_id(ents, kind).hex() == mktree(gitdir, ents, kind)
    want = [b"a-", b"a", b"a0", b"ab", "é".encode()] if kind == R.TREE else names
    assert [n for n, _ in sorted(ents, key=lambda e: R.order_key(e[0], kind))] == want
    assert R.tree_id([], kind).hex() == R.EMPTY_TREE == mktree(gitdir, [], kind)


def test_random_trees_against_git(gitdir):
    rng = np.random.default_rng(2)
    alphabet = np.frombuffer(b"ab-0.AZ_~\xc3\xa9\x80\xff", np.uint8)
    for k in range(300):
        kind = R.TREE if k % 3 == 0 else R.BLOB
        names = {bytes(rng.choice(alphabet, int(rng.integers(1, 7)))) for _ in range(int(rng.integers(1, 12)))}
        ents = [(n, _oid(rng)) for n in names]
        assert R.tree_id(ents, kind).hex() == mktree(gitdir, ents, kind), (kind, sorted(names))


def _leaves(fx_name, side):
    fx = load(fx_name)
    return fx.a[f"{side}_names"], fx.a[f"{side}_name_off"].astype(np.uint64), fx.oids(side), fx.encoding(side)


def _flat_tree_id(paths, off, oids):
    """the feature tree's id from nested dicts and hashlib alone (no treebuild)"""
    root = {}
    for i in range(len(off) - 1):
        parts = paths[int(off[i]):int(off[i + 1])].tobytes().split(b"/")
        node = root
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = oids[i].tobytes()

    def build(node):
        if all(isinstance(v, bytes) for v in node.values()):
            return R.tree_id(list(node.items()), R.BLOB)
        return R.tree_id([(k, build(v)) for k, v in node.items()], R.TREE)

    return build(root)


@pytest.mark.parametrize("fx_name,side", SIDES)
def test_reference_rebuilds_recorded_ids(fx_name, side):
    paths, off, oids, _ = _leaves(fx_name, side)
    assert _flat_tree_id(paths, off, oids).hex() == TREE_IDS[fx_name][side]


@pytest.mark.parametrize("fx_name,side", SIDES)
def test_feature_tree_on_ref_engine(fx_name, side):
    paths, off, oids, enc = _leaves(fx_name, side)
    ft = TB.feature_tree(R.RefEngine(), paths, off, oids, enc, bodies=True)
    assert ft.root.hex() == TREE_IDS[fx_name][side]
    assert len(ft.levels) == enc.levels + 1 and list(ft.levels[0][0]) == [b""]
    assert sum(o[0].shape[0] for o in ft.objects) == sum(d.size for d, _ in ft.levels)
    # one whole level-1 subtree's leaves removed, its id passed instead: the same root
    dirs, ids = ft.levels[1]
    d = dirs[len(dirs) // 2]
    w = len(d)
    starts = off[:-1].astype(np.int64)
    inside = np.all(paths[starts[:, None] + np.arange(w + 1)] == np.frombuffer(d + b"/", np.uint8), axis=1)
    assert inside.any()
    keep = np.nonzero(~inside)[0]
    kp, ko = TB.gather_rows(paths, off, keep)
    known = {d.decode(): ids[len(dirs) // 2].tobytes().hex()}
    ft2 = TB.feature_tree(R.RefEngine(), kp, ko, oids[keep], enc, known=known)
    assert ft2.root == ft.root
    # without it the directory does not exist; with leaves and a known id it is an error
    ft3 = TB.feature_tree(R.RefEngine(), kp, ko, oids[keep], enc)
    assert (ft3 is None and keep.size == 0) or ft3.root != ft.root
    with pytest.raises(ValueError):
        TB.feature_tree(R.RefEngine(), paths, off, oids, enc, known=known)


def test_feature_tree_edges():
    enc = load("repo_points").encoding("head")
    e = np.zeros(0, np.uint8)
    assert TB.feature_tree(R.RefEngine(), e, np.zeros(1, np.uint64), np.zeros((0, 20), np.uint8), enc) is None
    # only a known subtree: its ancestors exist
    kid = bytes(range(20))
    ft = TB.feature_tree(R.RefEngine(), e, np.zeros(1, np.uint64), np.zeros((0, 20), np.uint8), enc, known={"A/B": kid})
    assert ft.root == R.tree_id([(b"A", R.tree_id([(b"B", kid)], R.TREE))], R.TREE)
    # hash-key leaves in key order need rank; in walk order they do not
    fx = load("repo_string_pks")
    paths, off, oids, enc = _leaves("repo_string_pks", "head")
    order = np.asarray(fx.packed("head").order, np.int64)
    kp, ko = TB.gather_rows(paths, off, order)
    kp, ko, kid = TB.group_by_directory(kp, ko, oids[order], enc)
    assert TB.feature_tree(R.RefEngine(), kp, ko, kid, enc, rank=True).root.hex() == TREE_IDS["repo_string_pks"]["head"]
    # leaves not grouped by directory
    with pytest.raises(ValueError):
        rev = np.arange(len(off) - 1)[::-1]
        rp, ro = TB.gather_rows(paths, off, rev)
        TB.feature_tree(R.RefEngine(), rp, ro, oids[rev], enc)


def test_pack_objects_round_trip(tmp_path):
    """pack_objects + GitRepo.write_objects: every tree is readable afterwards and lists its entries"""
    from kart_amd.gitsource import GitRepo

    gd = str(tmp_path / "p.git")
    subprocess.run(["git", "init", "-q", "--bare", gd], check=True)
    paths, off, oids, enc = _leaves("conflicts_polygons", "ours")
    ft = TB.feature_tree(R.RefEngine(), paths, off, oids, enc, bodies=True)
    # beside them a tree of 3,300 bytes (a three-byte size header) and the empty tree (a one-byte one)
    big = R.tree_body([(b"n%03d" % i, bytes([i]) * 20) for i in range(100)], R.BLOB)
    extra = (np.frombuffer(R.object_id(big) + R.object_id(b""), np.uint8).reshape(2, 20), np.frombuffer(big, np.uint8),
             np.array([0, len(big), len(big)], np.uint64))
    ids, body, body_off = TB.concat_objects(ft.objects + [extra])
    sizes = np.diff(body_off.astype(np.int64))
    assert sizes.min() == 0 and 16 <= np.sort(sizes)[1] < 2048 <= sizes.max()
    repo = GitRepo(gd)
    try:
        repo.write_objects(TB.pack_objects(ids, body, body_off))
        repo.write_objects(TB.pack_objects(ids, body, body_off))  # objects the repository has are dropped
        repo.write_objects(TB.pack_objects(ids[:0], body[:0], body_off[:1]))
        for t in range(ids.shape[0]):
            want = body[int(body_off[t]):int(body_off[t + 1])].tobytes()
            assert R.object_id(want) == ids[t].tobytes()
            got = subprocess.run(["git", "--git-dir", gd, "cat-file", "tree", ids[t].tobytes().hex()], check=True,
                                 capture_output=True).stdout
            assert got == want
        listing = subprocess.run(["git", "--git-dir", gd, "ls-tree", "-r", ft.root.hex()], check=True,
                                 capture_output=True).stdout.decode().splitlines()
        fx = load("conflicts_polygons")
        assert sorted(ln.split("\t")[1] for ln in listing) == sorted(fx.names("ours"))
        assert repo.odb.tree_entries(ft.root.hex())
    finally:
        repo.close()


def test_ref_engine_status():
    names, off = R.pack_names([b"b", b"a", b"x", b"x", b"a", b"a-", b"q/r", b""])
    oids = np.arange(8 * 20, dtype=np.uint8).reshape(8, 20)
    seg = np.array([0, 2, 4, 6, 7, 8, 8], np.uint64)
    ids, st = R.RefEngine().tree_hash(names, off, oids, seg, R.BLOB)
    assert st.tolist() == [1, 1, 0, 3, 3, 0] and ids[5].tobytes().hex() == R.EMPTY_TREE and not ids[0].any()
    ids, st = R.RefEngine().tree_hash(names, off, oids, seg, R.TREE)
    assert st.tolist() == [1, 1, 1, 3, 3, 0]
    ids, st, body, boff = R.RefEngine().tree_hash(names, off, oids, seg, R.BLOB, rank=True, bodies=True)
    assert st.tolist() == [0, 2, 0, 3, 3, 0]
    assert ids[0].tobytes() == R.tree_id([(b"a", oids[1].tobytes()), (b"b", oids[0].tobytes())], R.BLOB, sort=False)
    assert boff.tolist() == [0, 58, 58, 117, 117, 117, 117] and body.size == 117
