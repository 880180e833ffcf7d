"""Git tree objects of a dataset's ``feature/`` tree, hashed level by level on the GPU.

<- ``index.write_tree(repo)`` (kart/merge.py:122).  ``feature_tree`` turns the leaves of one feature
tree (relative paths + blob ids, grouped by directory) into the ids — and, on request, the bodies —
of every tree object under it: one ``kd_tree_hash`` call per directory level, bottom-up, the ids of a
level staying on the device as the next level's entries.  ``pack_objects`` writes tree objects as a
version-2 pack stream for ``GitRepo.write_objects``; ``host_trees`` builds the few trees above the
feature trees (dataset directories, ``.table-dataset``, ``meta/``) with hashlib.

Host work is vectorised numpy: run boundaries come from comparing consecutive directory prefixes;
there are no per-leaf Python objects.
"""
import hashlib
import struct
import zlib
from collections import namedtuple

import numpy as np

from . import _native as N

FILEMODE_TREE = 0o40000

FeatureTree = namedtuple("FeatureTree", ("root", "levels", "objects"))
FeatureTree.__doc__ = """root: the feature tree's id (20 bytes); levels: [(dirs, ids)] from the root level
(dirs == [b""]) down to the leaf trees, dirs a numpy bytes array of directory paths ("A/B"), ids uint8
[k, 20]; objects: with bodies, [(ids, body, body_off)] of every tree computed, else None"""


def _component_width(encoding):
    if encoding.branches == 64:
        return 1
    if encoding.branches == 256:
        return 2
    raise ValueError(f"feature_tree: {encoding.branches} branches per level")


def gather_rows(arena, off, rows):
    """(arena, off) of the strings rows[k] of an (arena uint8, off uint64 [n+1]) string list"""
    off = np.asarray(off).astype(np.int64)
    rows = np.asarray(rows, np.int64)
    lens = off[rows + 1] - off[rows]
    out_off = np.zeros(rows.size + 1, np.int64)
    np.cumsum(lens, out=out_off[1:])
    src = np.arange(int(out_off[-1]), dtype=np.int64) + np.repeat(off[rows] - out_off[:-1], lens)
    return np.asarray(arena, np.uint8)[src], out_off.astype(np.uint64)


def pack_strings(strings):
    """[bytes] -> (uint8 arena, uint64 offsets [n+1]) (small lists: conflicts, tests)"""
    off = np.zeros(len(strings) + 1, np.uint64)
    if strings:
        off[1:] = np.cumsum([len(x) for x in strings])
    return np.frombuffer(b"".join(strings), np.uint8), off


def group_by_directory(rel_paths, rel_off, oids, encoding):
    """leaves in any order -> the same leaves grouped by directory, the directories ascending in git's
    order (a stable sort of the fixed-width directory prefix), which is what feature_tree takes with
    ``rank``"""
    P = int(encoding.levels) * (_component_width(encoding) + 1)
    off = np.asarray(rel_off).astype(np.int64)
    n = off.shape[0] - 1
    if n == 0:
        return rel_paths, rel_off, oids
    if np.any(off[1:] - off[:-1] <= P):
        raise ValueError("group_by_directory: a leaf path is shorter than its directory levels")
    pref = np.asarray(rel_paths, np.uint8)[off[:-1, None] + np.arange(P - 1, dtype=np.int64)]
    order = np.argsort(np.ascontiguousarray(pref).view(f"S{P - 1}").reshape(-1), kind="stable")
    arena, out_off = gather_rows(rel_paths, rel_off, order)
    return arena, out_off, np.asarray(oids, np.uint8).reshape(-1, 20)[order]


def concat_objects(objects):
    """[(ids, body, body_off)] -> one (ids, body, body_off)"""
    if not objects:
        return np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    lens = np.concatenate([np.diff(np.asarray(o[2]).astype(np.int64)) for o in objects])
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return (np.concatenate([np.asarray(o[0], np.uint8).reshape(-1, 20) for o in objects]),
            np.concatenate([np.asarray(o[1], np.uint8) for o in objects]), off)


def _host(x, dtype, count):
    return x if isinstance(x, np.ndarray) else x.download(dtype, count)


def _check(status, what):
    bad = np.nonzero(status)[0]
    if bad.size:
        t = int(bad[0])
        why = {1: "entries not in git's order", 2: "two entries share a name", 3: "a bad entry name"}
        raise ValueError(f"feature_tree: {what} tree {t}: {why.get(int(status[t]), status[t])}")


def _oid20(x):
    b = bytes.fromhex(x) if isinstance(x, str) else bytes(x)
    if len(b) != 20:
        raise ValueError("a tree id is 20 bytes")
    return b


def feature_tree(engine, rel_paths, rel_off, oids, encoding, *, rank=False, known=None, bodies=False):
    """The tree objects of one dataset's ``feature/`` tree.

    rel_paths / rel_off / oids: the leaves ("A/B/C/D/<name>", blob id), grouped by directory, the
    directories ascending in git's order; inside a directory in git's order too, unless ``rank``
    (then any order, up to 512 leaves per directory).  ``encoding``: the dataset's PathEncoding
    (``levels`` directory levels of 1-character names for 64 branches, 2 hex characters for 256).
    ``known``: {directory path ("A/B"): tree id} of subtrees whose id the caller already has — merged
    into their parent's run; a directory with neither leaves nor a known id does not exist.  Their
    ids are merged on the host, so a level with known entries downloads the level below it.
    Returns a FeatureTree, or None when there is neither a leaf nor a known subtree."""
    w, levels = _component_width(encoding), int(encoding.levels)
    P = levels * (w + 1)  # bytes of "A/B/C/D/" in front of a leaf's name
    rel_paths = np.ascontiguousarray(rel_paths, np.uint8).reshape(-1)
    off = np.ascontiguousarray(rel_off).astype(np.int64)
    oids = np.ascontiguousarray(oids, np.uint8).reshape(-1, 20)
    n = int(oids.shape[0])
    if off.shape[0] != n + 1:
        raise ValueError("feature_tree: rel_off must hold n + 1 offsets")
    known = {(k.encode() if isinstance(k, str) else bytes(k)): _oid20(v) for k, v in (known or {}).items()}
    for k in known:
        d, r = divmod(len(k) + 1, w + 1)
        if r or not 1 <= d <= levels or any(k[j * (w + 1) + w:j * (w + 1) + w + 1] not in (b"/", b"") for j in range(d)):
            raise ValueError(f"feature_tree: known directory {k!r} does not fit the encoding")
    if n == 0 and not known:
        return None
    device = hasattr(engine, "ctx")  # the HIP engine: chain the levels through device buffers
    out_levels, objects = [], ([] if bodies else None)

    def run(names, name_off, ids, seg, kind, rk):
        nt = len(seg) - 1
        res = engine.tree_hash(names, name_off, ids, seg, kind, rank=rk, bodies=bodies)
        st = _host(res[1], np.uint8, nt)
        _check(st, "leaf" if kind == N.KD_TE_BLOB else "directory")
        if bodies:
            bo = _host(res[3], np.uint64, nt + 1)
            objects.append([res[0], _host(res[2], np.uint8, int(bo[nt])), bo, nt])
        return res[0]

    # ---- leaf trees: runs of equal directory prefix ----
    S = f"S{P - 1}"
    if n:
        starts = off[:-1]
        if np.any(off[1:] - starts <= P):
            raise ValueError("feature_tree: a leaf path is shorter than its directory levels")
        pref = rel_paths[starts[:, None] + np.arange(P, dtype=np.int64)]  # [n, P]
        if np.any(pref[:, w::w + 1] != ord("/")):
            raise ValueError("feature_tree: a leaf path does not fit the encoding's directory levels")
        pref = np.ascontiguousarray(pref[:, :P - 1]).view(S).reshape(-1)
        first = np.concatenate([[0], np.nonzero(pref[1:] != pref[:-1])[0] + 1]).astype(np.int64)
        dirs = pref[first]
        if np.any(dirs[1:] <= dirs[:-1]):
            raise ValueError("feature_tree: the leaves are not grouped by directory in git's order")
        names, name_off = gather_rows(rel_paths, np.stack([starts + P, off[1:]], 1).reshape(-1), np.arange(n) * 2)
        seg = np.concatenate([first, [n]]).astype(np.uint64)
        leaf_oids = oids
        if device:
            from .device import DevBuf

            leaf_oids = DevBuf.from_numpy(engine, oids.reshape(-1))
        ids = run(names, name_off, leaf_oids, seg, N.KD_TE_BLOB, rank)
    else:
        dirs, ids = np.zeros(0, S), np.zeros((0, 20), np.uint8)

    # ---- directory levels, bottom-up: the trees of depth k are the entries of depth k - 1 ----
    for k in range(levels, 0, -1):
        width = k * (w + 1) - 1
        kn = sorted(p for p in known if len(p) == width)
        if kn:
            ids = _host(ids, np.uint8, 20 * dirs.size).reshape(-1, 20)
            alld = np.concatenate([dirs, np.array(kn, f"S{width}")])
            order = np.argsort(alld, kind="stable")
            alld = alld[order]
            if np.any(alld[1:] == alld[:-1]):
                raise ValueError("feature_tree: a known directory also has leaves (or is given twice)")
            ids = np.concatenate([ids, np.frombuffer(b"".join(known[p] for p in kn), np.uint8).reshape(-1, 20)])[order]
            dirs = alld
        out_levels.append((dirs, ids))
        m = int(dirs.size)
        if m == 0:  # (only shallower known subtrees so far)
            dirs, ids = np.zeros(0, f"S{max(width - w - 1, 1)}"), np.zeros((0, 20), np.uint8)
            continue
        raw = np.ascontiguousarray(dirs).view(np.uint8).reshape(m, width)
        names = np.ascontiguousarray(raw[:, width - w:]).reshape(-1)
        name_off = (np.arange(m + 1, dtype=np.uint64) * np.uint64(w))
        if k > 1:
            parents = np.ascontiguousarray(raw[:, :width - w - 1]).view(f"S{width - w - 1}").reshape(-1)
            first = np.concatenate([[0], np.nonzero(parents[1:] != parents[:-1])[0] + 1]).astype(np.int64)
            pdirs = parents[first]
        else:
            first, pdirs = np.zeros(1, np.int64), np.array([b""], "S1")
        seg = np.concatenate([first, [m]]).astype(np.uint64)
        ids = run(names, name_off, ids, seg, N.KD_TE_TREE, False)
        dirs = pdirs
    out_levels.append((dirs, ids))
    out_levels = [(d, _host(i, np.uint8, 20 * d.size).reshape(-1, 20)) for d, i in reversed(out_levels)]
    if bodies:
        objects = [(_host(i, np.uint8, 20 * nt).reshape(-1, 20), b, bo) for i, b, bo, nt in objects]
    return FeatureTree(out_levels[0][1][0].tobytes(), out_levels, objects)


# ---------------------------------------------------------------------------------------------
def pack_objects(ids, bodies, body_off):
    """A version-2 pack stream of the tree objects bodies[body_off[t]:body_off[t+1]] (zlib per object,
    SHA-1 trailer); ``ids`` [n, 20] only says how many there are — git names objects by content."""
    body_off = np.asarray(body_off).astype(np.int64)
    nobj = int(np.asarray(ids).reshape(-1, 20).shape[0])
    if body_off.shape[0] != nobj + 1:
        raise ValueError("pack_objects: body_off must hold one more offset than there are ids")
    data = np.ascontiguousarray(bodies, np.uint8).tobytes()
    out = [b"PACK" + struct.pack(">II", 2, nobj)]
    for t in range(nobj):
        lo, hi = int(body_off[t]), int(body_off[t + 1])
        size = hi - lo
        c = (2 << 4) | (size & 15)  # OBJ_TREE
        size >>= 4
        head = bytearray()
        while size:
            head.append(c | 0x80)
            c = size & 0x7F
            size >>= 7
        head.append(c)
        out.append(bytes(head))
        out.append(zlib.compress(data[lo:hi], 1))
    pack = b"".join(out)
    return pack + hashlib.sha1(pack).digest()


def _tree_key(e):
    mode, name, _ = e
    return name + b"/" if mode == FILEMODE_TREE else name


def host_trees(files, subtrees):
    """The trees above the feature trees, with hashlib.  files: {path: (mode, oid hex)} of blobs;
    subtrees: {path: tree id (20 bytes)} injected as they are.  Returns (root id bytes, [(id, body)]
    of every tree built).  A path of ``subtrees`` equal to "" is the root itself."""
    if "" in subtrees:
        return subtrees[""], []
    root = {}

    def put(path, leaf):
        parts = path.split("/")
        node = root
        for p in parts[:-1]:
            node = node.setdefault(p, {})
            if not isinstance(node, dict):
                raise ValueError(f"host_trees: {path} lies under a file")
        node[parts[-1]] = leaf

    for path, (mode, oid) in files.items():
        put(path, (int(mode), bytes.fromhex(oid)))
    for path, oid in subtrees.items():
        put(path, (FILEMODE_TREE, bytes(oid)))
    built = []

    def build(node):
        ents = []
        for name, v in node.items():
            if isinstance(v, dict):
                v = (FILEMODE_TREE, build(v))
            ents.append((v[0], name.encode(), v[1]))
        ents.sort(key=_tree_key)
        body = b"".join(b"%o %s\0%s" % e for e in ents)
        oid = hashlib.sha1(b"tree %d\0" % len(body) + body).digest()
        built.append((oid, body))
        return oid

    return build(root), built
