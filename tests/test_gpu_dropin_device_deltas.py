"""field_diff with device_inflate=True and device_deltas=True on repacked repositories: the updates'
blobs, most of them deltas, are rebuilt on the GPU into device arenas and kd_fielddiff reads them in
place — every update gets the same changed_fields as on the host route.
"""
import os
import subprocess

import pytest

import delta_craft as C
from kart_amd import dataset as D
from kart_amd.gitsource import GitRepo

pytestmark = pytest.mark.gpu

EIGHT = ("device", "host", "compressed", "fixups", "deltas", "links", "depth", "scratch")


def _routes(engine, repo, base, target, ds):
    """changed_fields by update key on the host route, the device route without deltas and with them;
    -> (fields, the counters of the two device routes)"""
    out = []
    for kw in ({"device_inflate": False}, {"device_inflate": True, "device_deltas": False},
               {"device_inflate": True, "device_deltas": True}):
        old, new = repo.diff_versions(base, target, ds)
        fd = D.get_dataset_diff(engine, old, new)["feature"]
        stats = {}
        n = D.field_diff(engine, fd, old, new, stats=stats, **kw)
        out.append(({k: d.changed_fields for k, d in fd.items() if d.type == "update"}, n, stats))
    (hf, hn, hs), (pf, pn, ps), (df, dn, ds_) = out
    assert "inflate" not in hs
    assert hn == pn == dn == len(hf) and pf == hf and df == hf
    assert all(v is not None for v in df.values())
    assert tuple(ps["inflate"]) == EIGHT[:4] and tuple(ds_["inflate"]) == EIGHT
    return df, ps["inflate"], ds_["inflate"]


@pytest.fixture(scope="module")
def versioned(tmp_path_factory):
    gitdir = str(tmp_path_factory.mktemp("dld") / "v.git")
    ds = C.versioned_dataset(gitdir)
    C.repack(gitdir)
    return gitdir, ds


def test_versioned_features_as_a_dataset(engine, versioned):
    gitdir, ds = versioned
    vp = C.verify_pack(gitdir)
    assert sum(d > 0 for d, _, _ in vp.values()) >= 1000, "the fixture no longer repacks into deltas"
    repo = GitRepo(gitdir)
    try:
        for base, target in (("refs/heads/v10", "refs/heads/v11"), ("refs/heads/v0", "refs/heads/v7")):
            fields, plain, deltas = _routes(engine, repo, base, target, ds)
            assert len(fields) == 150 and all(fields.values())
            assert deltas["deltas"] > 0 and deltas["fixups"] == 0 and deltas["host"] == 0
            assert deltas["device"] + deltas["deltas"] == 300
            assert plain["host"] == deltas["deltas"] and plain["device"] == deltas["device"]
    finally:
        repo.close()


def test_points_repository_repacked(engine, tmp_path):
    gitdir = str(tmp_path / "p.git")
    ds = C.points_repo(gitdir)
    C.repack(gitdir)
    # the update blobs that git stored as deltas, from diff-tree and verify-pack
    vp = C.verify_pack(gitdir)
    raw = subprocess.run(["git", "--git-dir", gitdir, "diff-tree", "-r", "refs/heads/c0", "refs/heads/c1"], check=True,
                         capture_output=True).stdout.decode()
    mods = [ln.split("\t")[0].split() for ln in raw.splitlines() if "/feature/" in ln]
    want = sum(vp[bytes.fromhex(o)][0] > 0 for p in mods if p[4] == "M" for o in (p[2], p[3]))
    assert want > 0, "the fixture no longer repacks into deltas"
    repo = GitRepo(gitdir)
    try:
        fields, plain, deltas = _routes(engine, repo, "refs/heads/c0", "refs/heads/c1", ds)
        assert sorted(fields) == [1095, 1166, 1168, 1181, 1182]
        assert sum(map(len, fields.values())) == 13
        assert deltas["device"] + deltas["deltas"] == 10 and deltas["host"] == 0 and deltas["fixups"] == 0
        assert deltas["deltas"] == want == plain["host"]
    finally:
        repo.close()


def test_module_default_and_environment(engine, versioned, monkeypatch):
    """device_deltas=None follows dataset.DEVICE_DELTAS, which is off unless the environment says so, and
    matters only on the device-inflate route"""
    assert D.DEVICE_DELTAS is (os.environ.get("KD_DEVICE_DELTAS", "0") not in ("", "0"))
    gitdir, ds = versioned
    repo = GitRepo(gitdir)
    try:
        for inflate, flag, keys in ((True, False, EIGHT[:4]), (True, True, EIGHT), (False, True, None)):
            monkeypatch.setattr(D, "DEVICE_INFLATE", inflate)
            monkeypatch.setattr(D, "DEVICE_DELTAS", flag)
            old, new = repo.diff_versions("refs/heads/v3", "refs/heads/v4", ds)
            fd = D.get_dataset_diff(engine, old, new)["feature"]
            stats = {}
            assert D.field_diff(engine, fd, old, new, stats=stats) == 150
            assert (tuple(stats["inflate"]) if "inflate" in stats else None) == keys
    finally:
        repo.close()
