"""field_diff with device_inflate=True: the updates' blobs are inflated on the GPU into device arenas
and kd_fielddiff reads them in place — every update gets the same changed_fields as on the host route.
"""
import json
import os
import subprocess
import sys

import pytest

from fixtures import load
from kart_amd import dataset as D
from kart_amd.gitsource import GitRepo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _points_repo(gitdir, depth0):
    """the repository test_dropin.py's test_gitsource_walk diffs: the points fixture's two versions"""
    fx = load("repo_points")
    subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    ds = fx.meta["ds_path"]
    inner = f"{ds}/.table-dataset"
    lines, mark = [], 0
    for ci, key in enumerate(("head1", "head")):
        files = {}
        for name, bi in zip(fx.names(key), fx.a[f"{key}_blob"]):
            files[f"{inner}/feature/{name}"] = fx.blob(int(bi))
        files[f"{inner}/meta/schema.json"] = json.dumps(fx.meta["sides"][key]["schema"]).encode()
        files[f"{inner}/meta/path-structure.json"] = json.dumps(fx.meta["sides"][key]["path_structure"]).encode()
        for h, lg in fx.legends.items():
            files[f"{inner}/meta/legend/{h}"] = lg.dumps()
        marks = {}
        for p, data in files.items():
            mark += 1
            marks[p] = mark
            lines.append(b"blob\nmark :%d\ndata %d\n" % (mark, len(data)) + data + b"\n")
        lines.append(b"commit refs/heads/c%d\ncommitter t <t@t> %d +0000\ndata 1\nx\n" % (ci, 1600000000 + ci))
        if ci:
            lines.append(b"from refs/heads/c0\n")
        lines.append(b"deleteall\n")
        for p in files:
            lines.append(b"M 100644 :%d %s\n" % (marks[p], p.encode()))
        lines.append(b"\n")
    cmd = ["git", "-c", "fastimport.unpackLimit=0", "fast-import", "--quiet"] + (["--depth=0"] if depth0 else [])
    subprocess.run(cmd, input=b"".join(lines), env=dict(os.environ, GIT_DIR=gitdir), check=True)
    return ds


def _both_routes(engine, repo, base, target, ds):
    """changed_fields by update key with the option off and on, and the device route's counters"""
    out = []
    for on in (False, True):
        old, new = repo.diff_versions(base, target, ds)
        fd = D.get_dataset_diff(engine, old, new)["feature"]
        stats = {}
        n = D.field_diff(engine, fd, old, new, stats=stats, device_inflate=on)
        out.append(({k: d.changed_fields for k, d in fd.items() if d.type == "update"}, n, stats))
    (off_fields, off_n, off_stats), (on_fields, on_n, on_stats) = out
    assert "inflate" not in off_stats
    assert on_n == off_n == len(off_fields) and on_fields == off_fields
    assert all(v is not None for v in on_fields.values())
    return on_fields, on_stats["inflate"]


@pytest.mark.parametrize("depth0", [True, False])
def test_points_repository(engine, tmp_path, depth0):
    gitdir = str(tmp_path / "repo.git")
    ds = _points_repo(gitdir, depth0)
    repo = GitRepo(gitdir)
    try:
        fields, counters = _both_routes(engine, repo, "refs/heads/c0", "refs/heads/c1", ds)
        assert sorted(fields) == [1095, 1166, 1168, 1181, 1182]
        assert sum(map(len, fields.values())) == 13
        assert counters["device"] + counters["host"] == 10 and counters["fixups"] == 0
        if depth0:  # every blob a plain stream: all ten inflated on the GPU
            assert counters["device"] == 10 and counters["compressed"] > 0
    finally:
        repo.close()


def test_synthetic_repository(engine, tmp_path):
    """the repository test_field_diff_one_read_for_both_sides diffs (scripts/e2e_repo_bench.build)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_repo_bench as E

    gitdir = str(tmp_path / "r.git")
    k = E.build(gitdir, 3000)
    repo = GitRepo(gitdir)
    try:
        fields, counters = _both_routes(engine, repo, "main^", "main", E.DS)
        assert len(fields) == k and counters["device"] + counters["host"] == 2 * k
        # the device route remembers no host arena: a value read afterwards takes the per-blob path
        old, new = repo.diff_versions("main^", "main", E.DS)
        fd = D.get_dataset_diff(engine, old, new)["feature"]
        D.field_diff(engine, fd, old, new, device_inflate=True)
        assert not old._arenas and not new._arenas
        d = next(x for x in fd.values() if x.type == "update")
        a, b = d.old_value, d.new_value
        assert sorted(d.changed_fields) == sorted(f for f in a if a[f] != b.get(f))
    finally:
        repo.close()


def test_module_default_and_environment(engine, tmp_path, monkeypatch):
    """device_inflate=None follows dataset.DEVICE_INFLATE, which is off unless the environment says so"""
    assert D.DEVICE_INFLATE is (os.environ.get("KD_DEVICE_INFLATE", "0") not in ("", "0"))
    gitdir = str(tmp_path / "repo.git")
    ds = _points_repo(gitdir, True)
    repo = GitRepo(gitdir)
    try:
        for flag in (False, True):
            monkeypatch.setattr(D, "DEVICE_INFLATE", flag)
            old, new = repo.diff_versions("refs/heads/c0", "refs/heads/c1", ds)
            fd = D.get_dataset_diff(engine, old, new)["feature"]
            stats = {}
            assert D.field_diff(engine, fd, old, new, stats=stats) == 5
            assert ("inflate" in stats) is flag
    finally:
        repo.close()


def test_two_repositories_fall_back(engine, tmp_path):
    """versions read from two repositories share no batched read: the option is ignored silently"""
    ga, gb = str(tmp_path / "a.git"), str(tmp_path / "b.git")
    ds = _points_repo(ga, True)
    _points_repo(gb, True)
    ra, rb = GitRepo(ga), GitRepo(gb)
    try:
        old = ra.dataset_version("refs/heads/c0", ds)
        new = rb.dataset_version("refs/heads/c1", ds)
        fd = D.get_dataset_diff(engine, old, new)["feature"]
        stats = {}
        assert D.field_diff(engine, fd, old, new, stats=stats, device_inflate=True) == 5
        assert "inflate" not in stats
        assert sum(len(d.changed_fields) for d in fd.values()) == 13
    finally:
        ra.close()
        rb.close()
