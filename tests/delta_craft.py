"""Hand-made git deltas and packs for the delta tests (a helper, not a test).

A delta encoder, a plain-Python applier that returns the result or the KD_DL_* code kd_delta.h gives
(the applier itself is pinned to git by tests/test_delta_host.py), the corpus the host check and the GPU
test share — all_valid(), crafted_invalid(), mutations() — and writers for packs with OFS_DELTA and
REF_DELTA entries, indexed by git or, where git would refuse the pack, by an index written here.
"""
import functools
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np

(OK, EHEADER, EBASE, ESIZE, EOP, ETRUNC, ECOPY, EOVER, ESHORT, EPARENT) = range(10)
ERANGE = 11


# ---------------------------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------------------------
def varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def copy_op(off, size, all_bytes=False):
    """a copy of `size` bytes (1 .. 0x10000; 0x10000 is encoded as size 0) from base offset `off`;
    all_bytes: every offset and size byte present, zero or not"""
    assert 0 < size <= 0x10000 and 0 <= off < 1 << 32
    sz = 0 if size == 0x10000 else size
    op, args = 0x80, bytearray()
    for b in range(4):
        v = (off >> (8 * b)) & 0xFF
        if v or all_bytes:
            op |= 1 << b
            args.append(v)
    for b in range(3):
        v = (sz >> (8 * b)) & 0xFF
        if v or all_bytes:
            op |= 0x10 << b
            args.append(v)
    return bytes([op]) + bytes(args)


def insert_op(data):
    assert 0 < len(data) < 128
    return bytes([len(data)]) + bytes(data)


def header(base_len, result_len):
    return varint(base_len) + varint(result_len)


def encode(base, ops, all_bytes=False):
    """(delta, result) of ops [("c", off, size) | ("i", bytes)] against `base`"""
    body, out = bytearray(), bytearray()
    for op in ops:
        if op[0] == "c":
            _, off, size = op
            assert off + size <= len(base)
            body += copy_op(off, size, all_bytes)
            out += base[off:off + size]
        else:
            body += insert_op(op[1])
            out += op[1]
    return header(len(base), len(out)) + bytes(body), bytes(out)


# ---------------------------------------------------------------------------------------------
# applier: the result, or the KD_DL_* code (the order of the checks is kd_delta.h's)
# ---------------------------------------------------------------------------------------------
def _size_varint(d, pos):
    v = 0
    for k in range(10):
        if pos >= len(d):
            return None, pos
        c = d[pos]
        pos += 1
        v |= (c & 0x7F) << (7 * k)
        if not c & 0x80:
            return v & ((1 << 64) - 1), pos
    return None, pos


def apply(base, delta, dst_len=None):
    """bytes, or an int code.  dst_len: the dst range's length (None: whatever the header says)"""
    d = delta
    bs, pos = _size_varint(d, 0)
    if bs is None:
        return EHEADER
    rs, pos = _size_varint(d, pos)
    if rs is None:
        return EHEADER
    if bs != len(base):
        return EBASE
    if dst_len is None:
        dst_len = rs
    if rs != dst_len:
        return ESIZE
    out = []
    w = 0
    while pos < len(d):
        op = d[pos]
        pos += 1
        if op == 0:
            return EOP
        if op & 0x80:
            off = sz = 0
            for b in range(4):
                if op & (1 << b):
                    if pos >= len(d):
                        return ETRUNC
                    off |= d[pos] << (8 * b)
                    pos += 1
            for b in range(3):
                if op & (0x10 << b):
                    if pos >= len(d):
                        return ETRUNC
                    sz |= d[pos] << (8 * b)
                    pos += 1
            if sz == 0:
                sz = 0x10000
            if off + sz > len(base):
                return ECOPY
            if sz > dst_len - w:
                return EOVER
            out.append(base[off:off + sz])
            w += sz
        else:
            if op > len(d) - pos:
                return ETRUNC
            if op > dst_len - w:
                return EOVER
            out.append(d[pos:pos + op])
            pos += op
            w += op
    if w != dst_len:
        return ESHORT
    return b"".join(out)


# ---------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------
COPY_LENGTHS = (1, 15, 16, 17, 255, 256, 257, 0x10000)


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def all_valid():
    """[(name, base, delta, result)].  Every copy length of COPY_LENGTHS at every base offset residue
    mod 16 (one item each) and, inside the item, at every dst residue mod 16 (sixteen copies, padded apart
    by inserts); an item's own place in its arena shifts all sixteen alike, so they stay all sixteen."""
    rng = np.random.default_rng(5)
    out = []
    for L in COPY_LENGTHS:
        for b in range(16):
            base = _rand(rng, b + L + 37)
            ops, w = [], 0
            for r in range(16):
                pad = (r - w) % 16
                if pad:
                    ops.append(("i", _rand(rng, pad)))
                    w += pad
                ops.append(("c", b + (r % 3) * 16 if b + (r % 3) * 16 + L <= len(base) else b, L))
                w += L
            delta, res = encode(base, ops)
            out.append(("copy%d@%d" % (L, b), base, delta, res))
    base = _rand(rng, 500)
    for name, ops in (
        ("insert1", [("i", b"x")]),
        ("insert127", [("i", _rand(rng, 127))]),
        ("insert127+copy", [("i", _rand(rng, 127)), ("c", 3, 200), ("i", _rand(rng, 127))]),
        ("whole", [("c", 0, 500)]),
        ("ops300", [("c", (7 * k) % 500, 1) if k % 2 else ("i", bytes([k & 0xFF])) for k in range(300)]),
        ("reorder", [("c", 250, 250), ("c", 0, 250)]),
        ("overlap-sources", [("c", 10, 100), ("c", 50, 100), ("c", 10, 100)]),
    ):
        delta, res = encode(base, ops)
        out.append((name, base, delta, res))
    delta, res = encode(base, [("c", 5, 33), ("i", b"abc")], all_bytes=True)
    out.append(("all-arg-bytes", base, delta, res))
    out.append(("empty-result", base, header(500, 0), b""))
    out.append(("empty-both", b"", header(0, 0), b""))
    delta, res = encode(b"", [("i", b"made of nothing"), ("i", _rand(rng, 100))])
    out.append(("empty-base-inserts", b"", delta, res))
    # an offset that needs its fourth byte, in range: the base is 16 MiB and a little
    big = bytes(1 << 24) + _rand(rng, 64)
    delta, res = encode(big, [("i", b"far:"), ("c", (1 << 24) + 16, 40), ("c", (1 << 24) - 8, 24)])
    assert delta[len(header(len(big), len(res))) + 5] & 0x08
    out.append(("offset-4-bytes", big, delta, res))
    for name, base, delta, res in out:
        assert apply(base, delta) == res, name
    return out


def crafted_invalid():
    """[(name, base, delta, dst_len, code)]: at least one per code 1..8"""
    base = bytes(range(200))
    h = header(200, 50)
    out = [
        ("empty-delta", base, b"", 50, EHEADER),
        ("one-varint", base, varint(200), 50, EHEADER),
        ("varint-truncated", base, varint(200) + b"\x80", 50, EHEADER),
        ("varint-11-bytes", base, b"\xff" * 10 + b"\x01" + varint(50), 50, EHEADER),
        ("base-size-off-by-one", base, header(201, 50) + copy_op(0, 50), 50, EBASE),
        ("base-size-zero", base, header(0, 50) + insert_op(b"x" * 50), 50, EBASE),
        ("result-size-larger", base, header(200, 51) + copy_op(0, 50), 50, ESIZE),
        ("result-size-smaller", base, header(200, 49) + copy_op(0, 49), 50, ESIZE),
        ("opcode-0", base, h + copy_op(0, 20) + b"\x00" + copy_op(0, 30), 50, EOP),
        ("opcode-0-first", base, h + b"\x00", 50, EOP),
        ("copy-args-missing", base, h + copy_op(0, 20) + bytes([0x80 | 0x01 | 0x10]) + b"\x05", 50, ETRUNC),
        ("copy-no-args-at-all", base, h + bytes([0x80 | 0x0F | 0x70]), 50, ETRUNC),
        ("insert-literals-missing", base, h + bytes([40]) + b"y" * 39, 50, ETRUNC),
        ("copy-past-base", base, h + copy_op(160, 41) + insert_op(b"z" * 9), 50, ECOPY),
        ("copy-offset-behind-base", base, h + copy_op(201, 1) + insert_op(b"z" * 49), 50, ECOPY),
        ("copy-offset-huge", base, h + copy_op(0xFFFFFFF0, 50), 50, ECOPY),
        ("copy-size-0-is-65536", base, header(200, 0x10000) + bytes([0x80]), 0x10000, ECOPY),
        ("copy-over", base, h + copy_op(0, 30) + copy_op(0, 21), 50, EOVER),
        ("insert-over", base, h + copy_op(0, 30) + insert_op(b"q" * 21), 50, EOVER),
        ("short", base, h + copy_op(0, 30) + insert_op(b"q" * 19), 50, ESHORT),
        ("no-ops", base, h, 50, ESHORT),
    ]
    for name, b, d, dl, code in out:
        assert apply(b, d, dl) == code, (name, apply(b, d, dl))
    return out


def mutations(n=2000, seed=7):
    """[(base, delta, dst_len)]: single bit flips and truncations of the valid deltas with small bases"""
    rng = np.random.default_rng(seed)
    pool = [(b, d, len(r)) for _, b, d, r in all_valid() if len(b) < 4096]
    out = []
    for k in range(n):
        b, d, dl = pool[int(rng.integers(len(pool)))]
        if k % 4 == 3:
            out.append((b, d[:int(rng.integers(len(d)))], dl))
        else:
            bit = int(rng.integers(8 * len(d)))
            m = bytearray(d)
            m[bit >> 3] ^= 1 << (bit & 7)
            out.append((b, bytes(m), dl))
    return out


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, np.uint64)
    np.cumsum(np.asarray(lengths, np.uint64), out=off[1:])
    return off


# ---------------------------------------------------------------------------------------------
# packs
# ---------------------------------------------------------------------------------------------
TYPE_NUM = {"commit": 1, "tree": 2, "blob": 3, "ofs": 6, "ref": 7}


def oid_of(kind, content):
    return hashlib.sha1(b"%s %d\0" % (kind.encode(), len(content)) + content).digest()


def _entry_head(type_num, size):
    head = [(type_num << 4) | (size & 15)]
    size >>= 4
    while size:
        head[-1] |= 0x80
        head.append(size & 0x7F)
        size >>= 7
    return bytes(head)


def _ofs_varint(rel):
    out = [rel & 0x7F]
    rel >>= 7
    while rel:
        rel -= 1
        out.append(0x80 | (rel & 0x7F))
        rel >>= 7
    return bytes(reversed(out))


def build_pack(entries):
    """entries: dicts with ``kind`` "blob" | "tree" (``content``), "ofs" (``base``: index of an earlier
    entry, ``delta``) or "ref" (``base_oid``, ``delta``); optional ``stream`` (the zlib stream instead of
    zlib.compress of the payload), ``size`` (the entry header's size instead of the payload's length).
    -> (pack bytes, [entry offset], [crc32 of the entry's bytes])"""
    body = bytearray(b"PACK" + struct.pack(">II", 2, len(entries)))
    offs, crcs = [], []
    for e in entries:
        at = len(body)
        payload = e["content"] if e["kind"] in ("blob", "tree") else e["delta"]
        raw = _entry_head(TYPE_NUM[e["kind"]], e.get("size", len(payload)))
        if e["kind"] == "ofs":
            raw += _ofs_varint(at - offs[e["base"]])
        elif e["kind"] == "ref":
            raw += e["base_oid"]
        raw += e.get("stream") or zlib.compress(payload)
        body += raw
        offs.append(at)
        crcs.append(zlib.crc32(raw))
    body += hashlib.sha1(body).digest()
    return bytes(body), offs, crcs


def resolve(entries, extern=None):
    """[(type name, content) or None where the chain does not apply] per entry.  extern: {oid: (type,
    content)} of objects outside the pack (REF_DELTA bases)"""
    done = [None] * len(entries)
    by_oid = dict(extern or {})
    for _ in range(len(entries) + 1):
        for k, e in enumerate(entries):
            if done[k] is not None:
                continue
            if e["kind"] in ("blob", "tree"):
                done[k] = (e["kind"], e["content"])
            else:
                base = done[e["base"]] if e["kind"] == "ofs" else by_oid.get(e["base_oid"])
                if base is None:
                    continue
                res = apply(base[1], e["delta"])
                if isinstance(res, int):
                    continue
                done[k] = (base[0], res)
            by_oid[oid_of(*done[k])] = done[k]
    return done


def write_idx(path, oids, offs, crcs, pack_sha):
    """an idx v2 for the pack (offsets below 2 GiB)"""
    order = sorted(range(len(oids)), key=lambda k: oids[k])
    fan = [0] * 256
    for o in oids:
        fan[o[0]] += 1
    for k in range(1, 256):
        fan[k] += fan[k - 1]
    body = b"\377tOc" + struct.pack(">I", 2) + struct.pack(">256I", *fan)
    body += b"".join(oids[k] for k in order)
    body += b"".join(struct.pack(">I", crcs[k]) for k in order)
    body += b"".join(struct.pack(">I", offs[k]) for k in order)
    body += pack_sha
    with open(path, "wb") as f:
        f.write(body + hashlib.sha1(body).digest())


def write_pack(gitdir, entries, index="git", oids=None, extern=None):
    """the pack written under gitdir, indexed by ``git index-pack`` or (index="own": packs git refuses,
    thin packs) by write_idx with ``oids`` ([20-byte id per entry]; None: the resolved objects' ids, a
    made-up id where the chain does not apply).  -> (pack path, [entry offset], [oid per entry])"""
    body, offs, crcs = build_pack(entries)
    name = hashlib.sha1(body).hexdigest()
    path = os.path.join(gitdir, "objects", "pack", "pack-%s.pack" % name)
    with open(path, "wb") as f:
        f.write(body)
    if oids is None:
        done = resolve(entries, extern)
        oids = [oid_of(*d) if d is not None else hashlib.sha1(b"unresolved %d %s" % (k, name.encode())).digest()
                for k, d in enumerate(done)]
    if index == "git":
        subprocess.run(["git", "--git-dir", gitdir, "index-pack", path], check=True, capture_output=True)
    else:
        write_idx(path[:-5] + ".idx", oids, offs, crcs, body[-20:])
    return path, offs, oids


def init_bare(path):
    subprocess.run(["git", "init", "-q", "--bare", path], check=True)
    return path


def oid_array(oids):
    return np.frombuffer(b"".join(oids), np.uint8).reshape(-1, 20).copy()


# ---------------------------------------------------------------------------------------------
# repositories written by git (fast-import --depth=0, then repacked into delta chains)
# ---------------------------------------------------------------------------------------------
def fast_import(gitdir, stream, depth0=True):
    cmd = ["git", "-c", "fastimport.unpackLimit=0", "fast-import", "--quiet"] + (["--depth=0"] if depth0 else [])
    subprocess.run(cmd, input=stream, env=dict(os.environ, GIT_DIR=gitdir), check=True)


def repack(gitdir, depth=50, window=50):
    subprocess.run(["git", "--git-dir", gitdir, "repack", "-adfq", "--depth=%d" % depth, "--window=%d" % window], check=True)


def verify_pack(gitdir):
    """{oid bytes: (chain depth (0: not a delta), offset in the pack, base oid or None)} of every blob in
    the repository's packs, from ``git verify-pack -v``"""
    out = {}
    pdir = os.path.join(gitdir, "objects", "pack")
    for f in sorted(os.listdir(pdir)):
        if not f.endswith(".idx"):
            continue
        txt = subprocess.run(["git", "verify-pack", "-v", os.path.join(pdir, f)], check=True, capture_output=True).stdout.decode()
        for line in txt.splitlines():
            p = line.split()
            if len(p) >= 5 and len(p[0]) == 40 and p[1] == "blob":
                out[bytes.fromhex(p[0])] = (int(p[5]), int(p[4]), bytes.fromhex(p[6])) if len(p) >= 7 else (0, int(p[4]), None)
    return out


def versioned_features(n_features=150, n_versions=12, seed=21):
    """[[blob of feature f at version v]]: each version edits one field or 8 geometry bytes of the one before"""
    rng = np.random.default_rng(seed)
    legend = hashlib.sha1(b"legend").digest()
    out = []
    for f in range(n_features):
        geom = bytearray(b"GP\x00\x03" + _rand(rng, int(rng.integers(120, 400))))
        fields = [b"name-%d" % f, b"class-%d" % (f % 7), _rand(rng, 24), b"survey %d of the district" % f]
        vers = []
        for v in range(n_versions):
            if v:
                if rng.integers(2):
                    at = int(rng.integers(4, len(geom) - 8))
                    geom[at:at + 8] = _rand(rng, 8)
                else:
                    k = int(rng.integers(len(fields)))
                    fields[k] = b"v%d-" % v + _rand(rng, int(rng.integers(4, 30)))
            blob = b"\x92\xc4\x14" + legend + b"\x95" + b"\xc5" + struct.pack(">H", len(geom)) + bytes(geom)
            for x in fields:
                blob += b"\xc4" + bytes([len(x)]) + x
            vers.append(blob)
        out.append(vers)
    return out


def import_versions(gitdir, feats, path_of=lambda f: "f/%d" % f):
    """one commit per version on main, every feature at its path; one fast-import --depth=0"""
    lines, mark = [], 0
    nv = len(feats[0])
    for v in range(nv):
        marks = []
        for f, vers in enumerate(feats):
            mark += 1
            marks.append(mark)
            lines.append(b"blob\nmark :%d\ndata %d\n" % (mark, len(vers[v])) + vers[v] + b"\n")
        lines.append(b"commit refs/heads/main\ncommitter t <t@t> %d +0000\ndata 2\nv%d\n" % (1600000000 + v, v % 10))
        for f, mk in enumerate(marks):
            lines.append(b"M 100644 :%d %s\n" % (mk, path_of(f).encode()))
        lines.append(b"\n")
    fast_import(gitdir, b"".join(lines))


def six_kind_blobs(inf_max):
    """about 1,200 blobs of six kinds, the empty blob and one of inf_max + 1 bytes (the corpus of
    test_gpu_read_batch_device.py, made again here)"""
    rng = np.random.default_rng(11)
    legend = hashlib.sha1(b"legend").digest()
    out = [b"", bytes(rng.integers(0, 256, inf_max + 1, dtype=np.uint8))]
    for k in range(300):
        out.append(b"\x92\xc4\x14" + legend + b"\x93" + rng.integers(0, 256, 12, dtype=np.uint8).tobytes() + b"name-%d" % k)
    for k in range(300):
        out.append(b"\x92\xc4\x14" + legend + b"GP\x00\x03" + bytes(rng.integers(0, 256, 300, dtype=np.uint8)) + b"polygon %d" % k)
    for k in range(250):
        out.append((b"row %d of the survey; " % k) * int(rng.integers(2, 60)))
    for k in range(150):
        out.append(b"z%d" % k + bytes(int(rng.integers(1, 5000))) + b"end")
    for n in (1, 65_535, 65_536, 70_000):
        out.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
    for k in range(200):
        out.append(b"%d:" % k + bytes(rng.integers(97, 101, int(rng.integers(10, 900)), dtype=np.uint8)))
    assert len(set(out)) == len(out)
    return out


def import_blobs(gitdir, blobs, branch="main"):
    lines = [b"blob\nmark :%d\ndata %d\n" % (k + 1, len(b)) + b + b"\n" for k, b in enumerate(blobs)]
    lines.append(b"commit refs/heads/%s\ncommitter t <t@t> 1600000000 +0000\ndata 1\nx\n" % branch.encode())
    lines += [b"M 100644 :%d f/%d\n" % (k + 1, k) for k in range(len(blobs))]
    lines.append(b"\n")
    fast_import(gitdir, b"".join(lines))


# ---------------------------------------------------------------------------------------------
# datasets (for field_diff): the points fixture's two versions, and versioned features as a table
# ---------------------------------------------------------------------------------------------
def points_repo(gitdir):
    """the points fixture's two versions on refs/heads/c0 and c1 (what test_gpu_dropin_device_inflate.py
    diffs, made again here), written by fast-import --depth=0.  -> dataset path"""
    import json

    from fixtures import load

    fx = load("repo_points")
    init_bare(gitdir)
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
    fast_import(gitdir, b"".join(lines))
    return ds


VERSIONED_DS = "nz_points"


def versioned_dataset(gitdir, n_features=150, n_versions=12, seed=31):
    """a points table of n_features rows committed n_versions times on refs/heads/v0 .. v<n-1>: each
    version edits one field of every feature — the t50_fid int, or 8 bytes of the geometry's x — so every
    feature is an update between any two versions.  fast-import --depth=0.  -> dataset path"""
    import json

    from kart_amd import synth
    from kart_amd.schema import Legend

    init_bare(gitdir)
    rng = np.random.default_rng(seed)
    legend = Legend(["c-fid"], [c["id"] for c in synth.POINT_SCHEMA[1:]])
    lh = legend.hexhash()
    inner = f"{VERSIONED_DS}/.table-dataset"
    meta = {f"{inner}/meta/schema.json": json.dumps(synth.POINT_SCHEMA).encode(),
            f"{inner}/meta/path-structure.json": json.dumps({"scheme": "int", "branches": 64, "levels": 4,
                                                             "encoding": "base64"}).encode(),
            f"{inner}/meta/legend/{lh}": legend.dumps(),
            f"{inner}/meta/crs/EPSG:4326.wkt": b'GEOGCS["WGS 84",AUTHORITY["EPSG","4326"]]',
            ".kart.repostructure.version": b"3\n"}
    pks = np.arange(1, n_features + 1, dtype=np.int64)
    arena, off = synth.int_pk_paths(pks)
    paths = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(n_features)]
    data, boff = synth.point_blobs(pks, np.zeros(n_features, np.uint64), lh)
    blobs = [bytearray(data[int(boff[i]):int(boff[i + 1])].tobytes()) for i in range(n_features)]
    lines = []
    for v in range(n_versions):
        lines.append(b"commit refs/heads/v%d\ncommitter t <t@t> %d +0000\ndata 1\nx\n" % (v, 1600000000 + v))
        if v:
            lines.append(b"from refs/heads/v%d\n" % (v - 1))
            for b in blobs:  # (synth.point_blobs' layout: x at 60..68 as a little-endian double, t50_fid at 77..81)
                if rng.integers(2):
                    b[77:81] = _rand(rng, 4)
                else:
                    b[60:66] = _rand(rng, 6)  # (the mantissa's low bytes: x stays a finite number near where it was)
        else:
            for p, d in meta.items():
                lines.append(b"M 100644 inline %s\ndata %d\n%s\n" % (p.encode(), len(d), d))
        for p, b in zip(paths, blobs):
            lines.append(b"M 100644 inline %s/feature/%s\ndata %d\n%s\n" % (inner.encode(), p, len(b), bytes(b)))
        lines.append(b"\n")
    fast_import(gitdir, b"".join(lines))
    return VERSIONED_DS
