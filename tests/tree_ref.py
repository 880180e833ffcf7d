"""hashlib reference for git tree objects (test infrastructure): tree_body / tree_id with both of
git's order rules, and RefEngine, a stand-in with Engine.tree_hash's interface (host arrays only)."""
import hashlib

import numpy as np

BLOB, TREE = 0, 1
MODE = {BLOB: b"100644", TREE: b"40000"}
EMPTY_TREE = "4b825dc642cb6eb9a060e54bf8d69288fbee4904"
RANK_MAX = 512


def order_key(name, kind):
    """git's tree order: unsigned bytes, a tree's name as if it ended in '/' (a blob's: a prefix first)"""
    return name + b"/" if kind == TREE else name


def tree_body(entries, kind):
    """entries [(name bytes, oid 20 bytes)] in the order given -> the tree object's payload"""
    return b"".join(MODE[kind] + b" " + n + b"\0" + bytes(o) for n, o in entries)


def object_id(body):
    return hashlib.sha1(b"tree %d\0" % len(body) + body).digest()


def tree_id(entries, kind, sort=True):
    """id (20 bytes) of the tree of ``entries``, put into git's order first unless sort=False"""
    if sort:
        entries = sorted(entries, key=lambda e: order_key(e[0], kind))
    return object_id(tree_body(entries, kind))


def name_bad(name):
    return len(name) == 0 or len(name) > 255 or b"/" in name or b"\0" in name


class RefEngine:
    """Engine.tree_hash computed with hashlib"""

    def tree_hash(self, names, name_off, oids, seg, kind, rank=False, bodies=False):
        names = np.ascontiguousarray(names, np.uint8).reshape(-1).tobytes()
        off = [int(x) for x in np.asarray(name_off)]
        oids = np.ascontiguousarray(oids, np.uint8).reshape(-1, 20)
        seg = [int(x) for x in np.asarray(seg)]
        nt = len(seg) - 1
        if rank and kind != BLOB:
            raise ValueError("rank orders blob entries only")
        if rank and any(seg[t + 1] - seg[t] > RANK_MAX for t in range(nt)):
            raise NotImplementedError("rank: runs of up to 512 entries")
        ids, status = np.zeros((nt, 20), np.uint8), np.zeros(nt, np.uint8)
        body, body_off = [], np.zeros(nt + 1, np.uint64)
        for t in range(nt):
            ents = [(names[off[i]:off[i + 1]], oids[i].tobytes()) for i in range(seg[t], seg[t + 1])]
            keys = [order_key(n, kind) for n, _ in ents]
            st = 0
            if rank:
                if len(set(keys)) != len(keys):
                    st = 2
                ents.sort(key=lambda e: order_key(e[0], kind))
            elif any(not a < b for a, b in zip(keys, keys[1:])):
                st = 1
            if any(name_bad(n) for n, _ in ents):
                st = 3
            status[t] = st
            b = b"" if st else tree_body(ents, kind)
            if not st:
                ids[t] = np.frombuffer(object_id(b), np.uint8)
            body.append(b)
            body_off[t + 1] = body_off[t] + np.uint64(len(b))
        if bodies:
            return ids, status, np.frombuffer(b"".join(body), np.uint8), body_off
        return ids, status


def pack_names(names):
    """[bytes] -> (uint8 arena, uint64 offsets [n+1])"""
    off = np.zeros(len(names) + 1, np.uint64)
    if names:
        off[1:] = np.cumsum([len(n) for n in names])
    return np.frombuffer(b"".join(names), np.uint8), off
