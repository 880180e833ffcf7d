"""Small repositories for the device walk's tests, each written by one ``git fast-import``: the golden
fixtures' versions as commits, a synthetic legacy (2-level hex) layout with the odd leaf trees the host
class is for, and the pack layouts a clone, a gc or a second import leave behind.
"""
import hashlib
import os
import shutil
import subprocess
import sys

from fixtures import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def git(gitdir, *args, **kw):
    return subprocess.run(["git", "--git-dir", gitdir, *args], check=True, capture_output=True, **kw).stdout.decode().strip()


def import_versions(gitdir, versions, depth0=True, loose=False, prefix="c", init=True):
    """one commit per version ({path: bytes}) on refs/heads/<prefix><i>, all by one fast-import: one pack
    (``loose``: every object loose instead)"""
    if init:
        subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    lines, marks = [], {}
    for v in versions:
        for data in v.values():
            if data not in marks:
                marks[data] = len(marks) + 1
                lines.append(b"blob\nmark :%d\ndata %d\n" % (marks[data], len(data)) + data + b"\n")
    for ci, v in enumerate(versions):
        lines.append(b"commit refs/heads/%s%d\ncommitter t <t@t> %d +0000\ndata 1\nx\n" % (prefix.encode(), ci, 1600000000 + ci))
        lines.append(b"deleteall\n")
        for p, data in v.items():
            lines.append(b"M 100644 :%d %s\n" % (marks[data], p.encode()))
        lines.append(b"\n")
    cmd = ["git", "-c", "fastimport.unpackLimit=%d" % (10 ** 9 if loose else 0), "fast-import", "--quiet"] + (["--depth=0"] if depth0 else [])
    subprocess.run(cmd, input=b"".join(lines), env=dict(os.environ, GIT_DIR=gitdir), check=True)
    return ["refs/heads/%s%d" % (prefix, i) for i in range(len(versions))]


def fixture_versions(name, keys):
    """(feature tree path, [{path: bytes}]) of a golden fixture's sides"""
    fx = load(name)
    sub = f"{fx.meta['ds_path']}/.table-dataset/feature"
    out = []
    for key in keys:
        out.append({f"{sub}/{nm}": fx.blob(int(bi)) for nm, bi in zip(fx.names(key), fx.a[f"{key}_blob"])})
    return sub, out


def points_versions():
    return fixture_versions("repo_points", ("head1", "head"))


def string_pk_versions():
    """the hash-PK fixture has one version: a second one drops, edits and adds features"""
    sub, (head,) = fixture_versions("repo_string_pks", ("head",))
    paths = sorted(head)
    new = dict(head)
    for i, p in enumerate(paths):
        if i % 11 == 3:
            del new[p]
        elif i % 7 == 2:
            new[p] = head[p] + b"!"
    for i in range(5):
        new[f"{sub}/{'-/2/w/-' if i < 2 else 'z/z/z/%d' % i}/added{i}"] = b"new feature %d" % i
    return sub, [head, new]


def conflicts_versions(name):
    return fixture_versions(name, ("ancestor", "ours", "theirs"))


def legacy_versions():
    """a 2-level hex layout (256-way levels in kind, a few dozen directories here) with, at leaf depth: a
    leaf tree on one side only (both ways), a leaf tree that also holds a subtree, and one of 8,000
    entries (above KD_INF_MAX inflated)"""
    sub = "old/.sno-table/features"
    v1, v2 = {}, {}
    for i in range(400):
        h = hashlib.sha1(b"%d" % i).hexdigest()
        p = f"{sub}/{h[:2]}/{h[2:4]}/{h[4:20]}"
        v1[p] = b"feature %d" % i
        if i % 9 == 1:
            continue
        v2[p] = v1[p] + (b" edited" if i % 5 == 0 else b"")
    v1[f"{sub}/yy/only-old/f"] = b"gone"
    v2[f"{sub}/zz/only-new/f"] = b"born"
    for v, tag in ((v1, b"1"), (v2, b"2")):
        v[f"{sub}/7f/mixed/plain"] = b"plain " + tag
        v[f"{sub}/7f/mixed/deeper/leaf"] = b"deeper " + tag
        v[f"{sub}/7f/mixed/deeper/same"] = b"same"
    for i in range(8000):
        p = f"{sub}/80/big/e{i:07d}"
        v1[p] = b"big"
        v2[p] = b"big" if i % 1000 else b"big edited"
    return sub, [v1, v2]


def synthetic(gitdir, n=3000):
    """scripts/e2e_repo_bench.build: (feature tree path, roots)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_repo_bench as E

    E.build(gitdir, n)
    return f"{E.DS}/.table-dataset/feature", ["main^", "main"]


def repacked(src, dst):
    """a copy whose objects are one pack of deltas (trees become OFS_DELTA against their other version)"""
    shutil.copytree(src, dst)
    git(dst, "repack", "-adfq", "--depth=50", "--window=50")
    return dst


def two_packs_and_loose(gitdir, versions):
    """version 0 in one pack (--depth=0), version 1 in a second pack written with deltas, and a third
    version (version 1 less a few features) whose new trees are loose objects; roots: the first and third"""
    import_versions(gitdir, versions[:1], prefix="a")
    import_versions(gitdir, versions[1:2], depth0=False, prefix="b", init=False)
    v2 = dict(versions[1])
    for p in sorted(v2)[::97]:
        del v2[p]
    import_versions(gitdir, [v2], loose=True, prefix="c", init=False)
    packs = [f for f in os.listdir(os.path.join(gitdir, "objects", "pack")) if f.endswith(".pack")]
    assert len(packs) == 2 and any(len(d) == 2 for d in os.listdir(os.path.join(gitdir, "objects")))
    return ["refs/heads/a0", "refs/heads/c0"]
