"""MergeIndex.write_tree(repo, engine): the merged tree's id from the merge's arrays — feature trees
through Engine.tree_hash, the trees above them on the host, the objects through one pack — against
write_tree(repo) (git update-index + write-tree) on repositories built from the fixtures.

Each test runs on the CPU with the oracle and the hashlib tree reference standing in for the engine
(host logic only), and under -m gpu with the HIP engine."""
import subprocess

import numpy as np
import pytest

from fixtures import load
from kart_amd import merge as M
from kart_amd.gitsource import GitRepo
from test_merge_index import OracleEngine, _fast_import_repo
from tree_ref import RefEngine


class CpuEngine(OracleEngine, RefEngine):
    """test-only stand-in: the CPU oracle's classification, hashlib's tree ids"""


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def eng(request):
    if request.param == "cpu":
        yield CpuEngine()
    else:
        yield request.getfixturevalue("engine")


def _ls(repo, tree):
    return repo.git("ls-tree", "-r", tree).decode().splitlines()


@pytest.fixture
def polygons_repo(tmp_path):
    fx = load("conflicts_polygons")
    (case,) = fx.cases("merge3")
    repo = GitRepo(_fast_import_repo(tmp_path, fx, case["sides"], ["anc", "ours", "theirs"]))
    yield fx, repo
    repo.close()


def test_conflict_free_merge_writes_ours_tree(eng, polygons_repo):
    _, repo = polygons_repo
    clean = M.merge_repo(eng, repo, "anc", "ours", "ours")
    assert not clean.conflicts
    assert clean.write_tree(repo, eng) == repo.rev_tree("ours")


def test_resolved_merge_equals_index_route(eng, polygons_repo):
    fx, repo = polygons_repo
    mi = M.merge_repo(eng, repo, "anc", "ours", "theirs")
    assert len(mi.conflicts) == 4
    with pytest.raises(ValueError):
        mi.write_tree(repo, eng)
    for k, c in mi.conflicts.items():
        mi.add_resolve(k, [c.ours or c.theirs])
    want = mi.write_tree(repo)
    got = mi.write_tree(repo, eng)
    assert got == want
    listing = _ls(repo, got)
    assert listing == _ls(repo, want) and len(listing) == len(mi.entries)
    # the unpruned route: whole versions through merge_trees give the same feature tree
    ds = fx.meta["ds_path"]
    pre = f"{ds}/.table-dataset/feature/"
    vers = repo.dataset_versions(["anc", "ours", "theirs"], ds)
    assert not any(v.partial for v in vers)
    whole = M.merge_trees(eng, *vers, prefix=pre)
    for k, c in whole.conflicts.items():
        whole.add_resolve(k, [c.ours or c.theirs])
    root = whole.write_tree(repo, eng)
    assert repo.tree_at(root, pre.rstrip("/")) == repo.tree_at(want, pre.rstrip("/"))
    assert [ln.split("\t")[1] for ln in _ls(repo, root)] == [ln.split("\t")[1] for ln in listing if pre in ln]


class Crafted:
    """three sides derived from one fixture side by dropping and replacing rows, with the interface
    _fast_import_repo reads"""

    def __init__(self, fx, key, sides):
        self.fx, self.legends = fx, fx.legends
        names, blob = fx.names(key), fx.a[f"{key}_blob"]
        self.meta = {"ds_path": fx.meta["ds_path"], "sides": {k: fx.meta["sides"][key] for k in sides}}
        self._names = {k: [names[i] for i, _ in rows] for k, rows in sides.items()}
        self.a = {f"{k}_blob": np.array([blob[j] for _, j in rows], np.int64) for k, rows in sides.items()}

    def names(self, key):
        return self._names[key]

    def blob(self, i):
        return self.fx.blob(i)


def test_crafted_clean_merge(eng, tmp_path):
    """ours and theirs edit, insert and delete disjoint features (ours deletes a whole leaf tree):
    a clean merge whose tree both routes write alike, and which holds exactly the expected leaves"""
    fx = load("conflicts_polygons")
    names = fx.names("ancestor")
    n = len(names)
    leaf_dir = [nm.rsplit("/", 1)[0] for nm in names]
    dirs = sorted(set(leaf_dir))
    multi = [d for d in dirs if leaf_dir.count(d) >= 2]
    emptied = set(i for i in range(n) if leaf_dir[i] == multi[0])  # ours deletes this whole leaf tree
    rest = [i for i in range(n) if i not in emptied]
    ins_o, ins_t = rest[0:2], rest[2:4]          # absent from the ancestor
    ed_o, ed_t = rest[4:7], rest[7:10]           # edited: another feature's blob
    del_t = rest[10:13]
    held = [i for i in range(n) if i not in ins_o and i not in ins_t]
    row = lambda i, edited: (i, (i + 1) % n if edited else i)  # noqa: E731
    sides = {
        "anc": [row(i, False) for i in held],
        "ours": [row(i, i in ed_o) for i in held if i not in emptied] + [row(i, False) for i in ins_o],
        "theirs": [row(i, i in ed_t) for i in held if i not in del_t] + [row(i, False) for i in ins_t],
    }
    cf = Crafted(fx, "ancestor", sides)
    repo = GitRepo(_fast_import_repo(tmp_path, cf, ["anc", "ours", "theirs"], ["anc", "ours", "theirs"]))
    try:
        mi = M.merge_repo(eng, repo, "anc", "ours", "theirs")
        assert not mi.conflicts
        want = mi.write_tree(repo)
        got = mi.write_tree(repo, eng)
        assert got == want and _ls(repo, got) == _ls(repo, want)
        pre = fx.meta["ds_path"] + "/.table-dataset/feature/"
        merged = sorted(pre + names[i] for i in range(n) if i not in emptied and i not in del_t)
        assert sorted(ln.split("\t")[1] for ln in _ls(repo, got) if pre in ln) == merged
        assert repo.tree_at(got, pre + multi[0]) is None and repo.tree_at("anc", pre + multi[0]) is not None
        edited = {pre + names[i] for i in ed_o + ed_t}
        anc = dict(ln.split("\t")[::-1] for ln in _ls(repo, "anc"))
        new = dict(ln.split("\t")[::-1] for ln in _ls(repo, got))
        assert {p for p in anc if p in new and anc[p] != new[p]} == edited
        # edited entries are written by the index route only
        mi.entries[".kart.repostructure.version"] = mi.entries[".kart.repostructure.version"]
        with pytest.raises(ValueError):
            mi.write_tree(repo, eng)
    finally:
        repo.close()
