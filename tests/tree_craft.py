"""Crafted git tree objects and a Python reference of the leaf join (kd_treeparse.h / kd_tree_join_batch).

The reference is written from the rules, not from the kernel: git's tree format
``<octal mode> SP <name> NUL <20 OID bytes>``, the device class of include/kartdiff.h (each refusal a
KD_TJ_* code, the first one met in byte order), and kd_walk's join of a level restricted to non-tree
entries — the union of the roots' names in unsigned byte order, a name dropped everywhere when the two
compared roots agree on it.  The join is set-based (dicts and sorted()), not a merge of cursors.
"""
import numpy as np

OK, EMODE, ENAME, EOID, ETREE, EORDER, EBIG, ECAP = range(8)
ERANGE = 11
MAX_BYTES = 1 << 30
NONE = 0xFFFFFFFF
CODES = {"EMODE": EMODE, "ENAME": ENAME, "EOID": EOID, "ETREE": ETREE, "EORDER": EORDER, "EBIG": EBIG}


def parse(t):
    """(status, [(mode, name bytes, oid bytes)]) of a raw tree; entries are empty unless status is 0"""
    if len(t) > MAX_BYTES:
        return EBIG, []
    ents, pos, prev = [], 0, None
    while pos < len(t):
        q, nd, mode = pos, 0, 0
        while True:
            if q >= len(t):
                return EMODE, []
            b = t[q]
            if b == 0x20:
                break
            if not 0x30 <= b <= 0x37 or nd == 11:
                return EMODE, []
            mode = mode * 8 + b - 0x30
            nd += 1
            q += 1
        if nd == 0 or mode > 0xFFFFFFFF:
            return EMODE, []
        name = q + 1
        nul = t.find(b"\0", name)
        if nul < 0 or nul == name:
            return ENAME, []
        if len(t) - nul < 21:
            return EOID, []
        if mode == 0o40000:
            return ETREE, []
        nm = t[name:nul]
        if prev is not None and not prev < nm:  # (bytes compare: unsigned, a proper prefix is smaller)
            return EORDER, []
        ents.append((mode, nm, t[nul + 1:nul + 21]))
        prev = nm
        pos = nul + 21
    return OK, ents


def join(trees, compare=None):
    """the task's status and, per root, its kept [(name, mode, oid)]; trees[r] is bytes or None (absent)"""
    maps = []
    for t in trees:
        st, ents = (OK, []) if t is None else parse(t)
        if st:
            return st, [[] for _ in trees]
        maps.append({nm: (mode, oid) for mode, nm, oid in ents})
    kept = [[] for _ in trees]
    for nm in sorted(set().union(*maps)):
        if compare is not None and maps[compare[0]].get(nm) == maps[compare[1]].get(nm):
            continue
        for r, m in enumerate(maps):
            if nm in m:
                kept[r].append((nm,) + m[nm])
    return OK, kept


def join_batch(trees, tasks, prefixes, k, compare=None):
    """what kd_tree_join_batch returns: ([(paths, path_off, oids [n, 20], modes) per root], count [nt, k],
    status [nt]) for tasks = [[tree index or NONE] * k] over the list ``trees`` and one prefix per task"""
    paths = [bytearray() for _ in range(k)]
    offs = [[0] for _ in range(k)]
    oids = [bytearray() for _ in range(k)]
    modes = [[] for _ in range(k)]
    count = np.zeros((len(tasks), k), np.uint32)
    status = np.zeros(len(tasks), np.uint8)
    for t, (task, pre) in enumerate(zip(tasks, prefixes)):
        st, kept = join([None if i == NONE else trees[i] for i in task], compare)
        status[t] = st
        if st:
            continue
        for r in range(k):
            count[t, r] = len(kept[r])
            for nm, mode, oid in kept[r]:
                paths[r] += (pre + b"/" if pre else b"") + nm
                offs[r].append(len(paths[r]))
                oids[r] += oid
                modes[r].append(mode)
    outs = [(np.frombuffer(bytes(paths[r]), np.uint8), np.array(offs[r], np.uint64),
             np.frombuffer(bytes(oids[r]), np.uint8).reshape(-1, 20), np.array(modes[r], np.uint32)) for r in range(k)]
    return outs, count, status


def arena(trees):
    """(data uint8, off uint64 [n + 1]) of a list of raw trees"""
    off = np.zeros(len(trees) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in trees])
    return np.frombuffer(b"".join(trees), np.uint8), off


# ---------------------------------------------------------------------------------------------
# crafted trees
# ---------------------------------------------------------------------------------------------
def mk(entries):
    """a raw tree of [(mode int, name bytes, oid bytes)] in the order given (the caller sorts)"""
    return b"".join(b"%o %s\0%s" % (mode, nm, oid) for mode, nm, oid in entries)


def oid_of(seed):
    """20 bytes that look random and are no special pattern"""
    return np.random.default_rng(seed).integers(1, 256, 20, dtype=np.uint8).tobytes().replace(b" ", b"!")


OID_ZERO = bytes(20)
OID_SPACE = b" " * 20
OID_SPNUL = b" \0" * 10            # every second byte a NUL behind a space
OID_ENTRY = b"100644 a\0" + b"40000 b\0 \0 "  # reads like the front of two entries
assert len(OID_ENTRY) == 20
OID_NULSP = b"\0 " * 10
LONG = bytes(97 + (7 * i) % 26 for i in range(300))  # a 300-byte name


def rand_tree(rng, n, lo=1, hi=40, modes=(0o100644,)):
    """n entries with distinct random names (bytes 1..255 but no NUL), sorted"""
    names = set()
    while len(names) < n:
        ln = int(rng.integers(lo, hi + 1))
        names.add(bytes(rng.integers(1, 256, ln, dtype=np.uint8)))
    return [(int(modes[int(rng.integers(0, len(modes)))]), nm, bytes(rng.integers(0, 256, 20, dtype=np.uint8))) for nm in sorted(names)]


def valid_trees():
    """[(name, raw tree)] small enough to truncate at every byte: every format feature once"""
    rng = np.random.default_rng(5)
    out = [
        ("empty", b""),
        ("one entry", mk([(0o100644, b"a", oid_of(1))])),
        ("one-byte names", mk([(0o100644, bytes([c]), oid_of(c)) for c in (0x01, 0x2F, 0x30, 0x61, 0x7F)])),
        ("300-byte name", mk([(0o100644, LONG, oid_of(2)), (0o100755, LONG + b"x", oid_of(3))])),
        ("oid all zero", mk([(0o100644, b"k1", OID_ZERO), (0o100644, b"k2", oid_of(4))])),
        ("oid all spaces", mk([(0o100644, b"k1", OID_SPACE), (0o100644, b"k2", OID_SPACE)])),
        ("oid of space-NUL pairs", mk([(0o100644, b"k1", OID_SPNUL), (0o100644, b"k2", OID_NULSP), (0o100644, b"k3", OID_ENTRY)])),
        ("high bytes beside ascii", mk([(0o100644, nm, oid_of(10 + i)) for i, nm in
                                         enumerate(sorted([b"a", b"a\x80", b"ab", b"b", b"\x7f", b"\x80", b"\x80a", b"\xc3\xa9", b"\xff"]))])),
        ("prefix of the next", mk([(0o100644, b"ab", oid_of(20)), (0o100644, b"abc", oid_of(21)), (0o100644, b"abcd", oid_of(22))])),
        ("every leaf mode", mk([(0o100644, b"f", oid_of(30)), (0o100755, b"g", oid_of(31)), (0o120000, b"h", oid_of(32)),
                                (0o160000, b"i", oid_of(33))])),
        ("modes beyond git's", mk([(0o7, b"p", oid_of(40)), (0o37777777777, b"q", oid_of(41)), (0o0, b"r", oid_of(42))])),
        ("names with spaces", mk([(0o100644, b" ", oid_of(50)), (0o100644, b" a b ", oid_of(51)), (0o100644, b"100644 z", oid_of(52))])),
        ("int-pk like", mk([(0o100644, b"kc%02d" % i, oid_of(60 + i)) for i in range(8)])),
        ("random", mk(rand_tree(rng, 9, modes=(0o100644, 0o100755, 0o120000)))),
    ]
    for name, t in out:
        assert parse(t)[0] == OK, name
    return out


def crafted_invalid():
    """[(name, raw tree, KD_TJ_* code)]: every refusal by name, each behind one good entry where it can be"""
    good = mk([(0o100644, b"a", oid_of(1))])
    o = oid_of(2)
    out = [
        ("mode: a letter", good + b"10064x b\0" + o, EMODE),
        ("mode: digit 8", good + b"100648 b\0" + o, EMODE),
        ("mode: no digits", good + b" b\0" + o, EMODE),
        ("mode: twelve digits", good + b"000000100644 b\0" + o, EMODE),
        ("mode: eleven digits above u32", good + b"40000000000 b\0" + o, EMODE),
        ("mode: the tree ends inside it", good + b"1006", EMODE),
        ("mode: a NUL in it", good + b"100\x00644 b\0" + o, EMODE),
        ("name: empty", good + b"100644 \0" + o, ENAME),
        ("name: no NUL", good + b"100644 bcd", ENAME),
        ("name: the tree ends behind the space", good + b"100644 ", ENAME),
        ("oid: 19 bytes", good + b"100644 b\0" + o[:19], EOID),
        ("oid: none", good + b"100644 b\0", EOID),
        ("tree: 40000", good + b"40000 d\0" + o, ETREE),
        ("tree: 040000", good + b"040000 d\0" + o, ETREE),
        ("tree: first entry", b"40000 d\0" + o + good, ETREE),
        ("order: the same name twice", good + good, EORDER),
        ("order: descending", mk([(0o100644, b"b", o), (0o100644, b"a", o)]), EORDER),
        ("order: ascending only as signed bytes", mk([(0o100644, b"\x80", o), (0o100644, b"a", o)]), EORDER),
        ("order: the longer name first", mk([(0o100644, b"abc", o), (0o100644, b"ab", o)]), EORDER),
    ]
    for name, t, code in out:
        assert parse(t)[0] == code, name
    return out


def truncations():
    """every proper prefix of every valid tree"""
    return [t[:n] for _, t in valid_trees() for n in range(len(t))]


def mutations(n=2000, seed=77):
    """n seeded single-byte edits of the valid trees: a byte replaced (half of them by one of the format's
    own bytes), removed or inserted"""
    rng = np.random.default_rng(seed)
    pool = [t for _, t in valid_trees() if t]
    special = b"\0 /0178"
    out = []
    for _ in range(n):
        t = bytearray(pool[int(rng.integers(0, len(pool)))])
        at = int(rng.integers(0, len(t)))
        b = special[int(rng.integers(0, len(special)))] if rng.integers(0, 2) else int(rng.integers(0, 256))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            del t[at]
        elif kind == 1:
            t.insert(at, b)
        else:
            t[at] = b
        out.append(bytes(t))
    return out


# ---------------------------------------------------------------------------------------------
# the whole walk, for pinning the reference to kd_walk on real repositories
# ---------------------------------------------------------------------------------------------
def _loose_parse(t):
    out, i = {}, 0
    while i < len(t):
        sp = t.index(b" ", i)
        nul = t.index(b"\0", sp)
        out[t[sp + 1:nul]] = (int(t[i:sp], 8), t[nul + 1:nul + 21])
        i = nul + 21
    return out


def walk(read_tree, tops, compare=None, prefix=b"", stats=None):
    """kd_walk under the trees ``tops`` (one 20-byte id or None per root; read_tree(id) -> raw tree): per
    root [(path, mode, oid)] in git order.  A level whose trees are all in the device class is joined by
    join() and checked against the generic rule (git order: a tree's name continues with '/')"""
    k = len(tops)
    raws = [None if t is None else read_tree(t) for t in tops]
    maps = [{} if r is None else _loose_parse(r) for r in raws]
    keyed = sorted({nm + (b"/" if m[nm][0] == 0o40000 else b""): nm for m in maps for nm in m}.items())
    out = [[] for _ in range(k)]
    level = [[] for _ in range(k)]
    for _, nm in keyed:
        ents = [m.get(nm) for m in maps]
        if compare is not None and ents[compare[0]] == ents[compare[1]]:
            continue
        if any(e is not None and e[0] == 0o40000 for e in ents):
            sub = walk(read_tree, [e[1] if e is not None and e[0] == 0o40000 else None for e in ents], compare,
                       prefix + nm + b"/", stats)
            for r in range(k):
                out[r] += sub[r]
                if ents[r] is not None and ents[r][0] != 0o40000:  # (a blob beside a tree of the same name)
                    out[r].append((prefix + nm, *ents[r]))
            continue
        for r in range(k):
            if ents[r] is not None:
                out[r].append((prefix + nm, *ents[r]))
                level[r].append((nm, *ents[r]))
    st, kept = join(raws, compare)
    if stats is not None:
        stats["levels"] = stats.get("levels", 0) + 1
        stats["device_class"] = stats.get("device_class", 0) + (st == OK)
    if st == OK:
        assert kept == level, prefix
    return out


# ---------------------------------------------------------------------------------------------
# task shapes shared by the GPU test and the sanitizer-built host check
# ---------------------------------------------------------------------------------------------
def edited(rng, ents, frac=0.15):
    """another version of a tree: some OIDs changed, some modes flipped, some entries gone, some new"""
    out = {}
    for mode, nm, oid in ents:
        u = rng.random()
        if u < frac:
            out[nm] = (mode, bytes(rng.integers(0, 256, 20, dtype=np.uint8)))
        elif u < frac * 1.3:
            out[nm] = (0o100755 if mode == 0o100644 else 0o100644, oid)
        elif u < frac * 1.6:
            continue
        else:
            out[nm] = (mode, oid)
    for mode, nm, oid in rand_tree(rng, max(1, int(len(ents) * frac * 0.3)), 1, 12):
        out.setdefault(nm, (mode, oid))
    return [(m, nm, o) for nm, (m, o) in sorted(out.items())]


PREFIXES = [b"", b"a", b"ab/cd", b"feature/00/1f", bytes(97 + i % 26 for i in range(200))]


def mixed(k, seed=1):
    """(trees, tasks, prefixes): every task shape once — absent roots in every combination, the empty
    tree, one entry, identical trees, edited trees, every crafted valid tree against an edit of itself"""
    rng = np.random.default_rng(seed)
    trees, tasks = [], []

    def add(t):
        trees.append(t)
        return len(trees) - 1

    base = [rand_tree(rng, n, 1, 30, (0o100644, 0o100755, 0o120000, 0o160000)) for n in (0, 1, 2, 7, 40)]
    base += [parse(t)[1] for _, t in valid_trees()]
    base = [[(m, nm, o) for m, nm, o in b] for b in base]
    for b in base:
        vers = [b] + [edited(rng, b) for _ in range(k - 1)]
        idx = [add(mk(v)) for v in vers]
        tasks.append(idx)
        tasks.append([idx[0]] * k)  # the same tree in every root
    some = [add(mk(rand_tree(rng, 5, 1, 9))) for _ in range(k)]
    for mask in range(1 << k):  # absent in every combination, all absent too
        tasks.append([some[r] if mask >> r & 1 else NONE for r in range(k)])
    empty = add(b"")
    tasks.append([empty] * k)
    tasks.append([empty if r else some[0] for r in range(k)])
    prefixes = [PREFIXES[t % len(PREFIXES)] for t in range(len(tasks))]
    return trees, tasks, prefixes


def compares(k):
    return [None] + [(i, j) for i in range(k) for j in range(k) if i != j]
