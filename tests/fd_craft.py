"""Hand-built feature blobs for the field-diff tests: every legal msgpack encoding of a value,
canonical or not, laid out at chosen positions inside a blob, and the plain Python restatement
(``oracle.py_feature`` + ``py_changed_fields``) of what the diff of two such blobs is.

A feature blob is ``92 <str(40) legend hex> <array of non-pk values>``.  Nothing here reads a
fixture: every set is generated, deterministic, and small.
"""
import functools
import math
import struct

import msgpack
import numpy as np

from kart_amd.schema import Column, FieldMaps, Legend, Schema
from oracle import oracle as O

# ------------------------------------------------------------------------------------------
# encoders: one function per msgpack header form


def _be(v, w):
    return int(v).to_bytes(w, "big")


def int_forms(v):
    """every legal encoding of the integer v: {form name: bytes}"""
    out = {}
    if 0 <= v <= 0x7F:
        out["fix"] = bytes([v])
    if -32 <= v < 0:
        out["fix"] = bytes([v & 0xFF])
    for t, w in ((0xCC, 1), (0xCD, 2), (0xCE, 4), (0xCF, 8)):
        if 0 <= v < 1 << (8 * w):
            out[f"u{8 * w}"] = bytes([t]) + _be(v, w)
    for t, w in ((0xD0, 1), (0xD1, 2), (0xD2, 4), (0xD3, 8)):
        if -(1 << (8 * w - 1)) <= v < 1 << (8 * w - 1):
            out[f"i{8 * w}"] = bytes([t]) + (v & ((1 << (8 * w)) - 1)).to_bytes(w, "big")
    return out


def float_forms(x):
    """float64 always; float32 too when x survives the round trip (NaN included)"""
    out = {"f64": b"\xcb" + struct.pack(">d", x)}
    try:
        y = struct.unpack(">f", struct.pack(">f", x))[0]
    except OverflowError:
        return out
    if y == x or (math.isnan(x) and math.isnan(y)):
        out["f32"] = b"\xca" + struct.pack(">f", x)
    return out


def str_forms(b):
    """b: the UTF-8 payload bytes"""
    n = len(b)
    out = {}
    if n < 32:
        out["fix"] = bytes([0xA0 | n]) + b
    if n < 1 << 8:
        out["s8"] = b"\xd9" + _be(n, 1) + b
    if n < 1 << 16:
        out["s16"] = b"\xda" + _be(n, 2) + b
    out["s32"] = b"\xdb" + _be(n, 4) + b
    return out


def bin_forms(b):
    n = len(b)
    out = {}
    if n < 1 << 8:
        out["b8"] = b"\xc4" + _be(n, 1) + b
    if n < 1 << 16:
        out["b16"] = b"\xc5" + _be(n, 2) + b
    out["b32"] = b"\xc6" + _be(n, 4) + b
    return out


def ext_forms(code, b):
    n = len(b)
    c = bytes([code & 0xFF])
    out = {}
    if n in (1, 2, 4, 8, 16):
        out["fix"] = bytes([0xD4 + n.bit_length() - 1]) + c + b
    if n < 1 << 8:
        out["e8"] = b"\xc7" + _be(n, 1) + c + b
    if n < 1 << 16:
        out["e16"] = b"\xc8" + _be(n, 2) + c + b
    out["e32"] = b"\xc9" + _be(n, 4) + c + b
    return out


NIL, TRUE, FALSE = b"\xc0", b"\xc3", b"\xc2"
G = ord("G")


def s_total(total, fill=b"p"):
    """a str value whose whole encoding is ``total`` bytes (>= 1): the padding values"""
    assert 1 <= total < 258
    if total <= 32:
        return bytes([0xA0 | (total - 1)]) + fill * (total - 1)
    return b"\xd9" + bytes([total - 2]) + fill * (total - 2)


def geom(n, seed=0):
    """an ext 'G' payload of n >= 2 bytes: 'GP' and a deterministic tail"""
    rng = np.random.default_rng(1000 + seed)
    return b"GP" + rng.integers(0, 256, n - 2, dtype=np.uint8).tobytes()


def rbytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------
# blobs and arenas


def legend_header(hexs, form="s8"):
    h = hexs.encode("ascii")
    assert len(h) == 40
    return {"s8": b"\xd9\x28", "s16": b"\xda\x00\x28", "s32": b"\xdb\x00\x00\x00\x28"}[form] + h


def array_header(n, form=None):
    if form is None:
        form = "fix" if n < 16 else "a16" if n < 1 << 16 else "a32"
    if form == "fix":
        assert n < 16
        return bytes([0x90 | n])
    if form == "a16":
        return b"\xdc" + _be(n, 2)
    return b"\xdd" + _be(n, 4)


def blob(legend_hex, values, legend_form="s8", array_form=None, count=None):
    """values: encoded msgpack values; count: the array header's count when it is to differ from
    len(values)"""
    n = len(values) if count is None else count
    return b"\x92" + legend_header(legend_hex, legend_form) + array_header(n, array_form) + b"".join(values)


def arena(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    if blobs:
        off[1:] = np.cumsum([len(b) for b in blobs])
    data = np.frombuffer(b"".join(blobs), np.uint8).copy() if blobs else np.zeros(0, np.uint8)
    return data, off


# ------------------------------------------------------------------------------------------
# schemas and legends

PK = Column("pk-id", "fid", "integer", 0)


def schema_of(ids, pk_last=False):
    """columns named as their ids, the int pk 'fid' first (or last)"""
    cols = [Column(i, i, "blob") for i in ids]
    return Schema(cols + [PK] if pk_last else [PK] + cols)


def legend_of(ids):
    lg = Legend((PK.id,), tuple(ids))
    return lg.hexhash(), lg


class Set:
    """one crafted set: blobs per side, the schemas and legends they are read under, and the
    tables (FieldMaps) kd_fielddiff consumes"""

    def __init__(self, name, olds, news, legends, old_schema, new_schema=None, nested=(), big=False):
        assert len(olds) == len(news)
        self.name = name + ("_big" if big else "")
        self.nested = frozenset(nested)  # rows holding a nested container: Python decodes them, the engine refuses
        self.olds, self.news = list(olds), list(news)
        self.legends = dict(legends)
        if big:  # legends no blob names: they only grow the tables past what LDS holds (k_fielddiff_g)
            self.legends.update(bulk_legends())
        self.old_schema = old_schema
        self.new_schema = new_schema or old_schema
        self.maps = FieldMaps(self.old_schema, self.legends, self.new_schema, self.legends)
        self.old_arena = arena(self.olds)
        self.new_arena = arena(self.news)

    def __len__(self):
        return len(self.olds)

    @functools.cached_property
    def expected(self):
        return expect(self.olds, self.news, self.legends, (self.old_schema, self.new_schema))

    @functools.cached_property
    def oracle(self):
        return O.fielddiff(*self.old_arena, *self.new_arena, None, self.maps)

    def table_bytes(self):
        return table_bytes(self.maps)


SMALL_TABLE, BIG_TABLE = 2048, 24 * 1024  # wide margins around the 16 KiB selector of k_fielddiff_g


def table_bytes(m):
    """size of the packed device tables of a FieldMaps (what picks k_fielddiff_g above 16 KiB): the
    layout of fielddiff_device's one packed upload in kd_fielddiff.hip (o_lo .. o_end), restated — a
    change of that layout has to be repeated here"""
    al = lambda x: (x + 15) & ~15  # noqa: E731
    nlo, nln, nk = max(1, len(m.old_hashes)), max(1, len(m.new_hashes)), m.n_keys
    maxv = max(1, int(m.map_old.max()) + 1)
    t = 0
    for part in (nlo * 40, nln * 40, nlo * nk * 2, nln * nk * 2, m.words * 8, nlo * nln * 2, nlo * maxv * 2, nlo * 4):
        t = al(t + part)
    return t


@functools.lru_cache(maxsize=None)
def bulk_legends(n=320):
    """n one-column legends of columns no schema holds: 40 B of legend hex each per side"""
    return dict(legend_of([f"bulk{j}"]) for j in range(n))


def _legend_hex_of(b):
    return msgpack.unpackb(b, raw=False, ext_hook=lambda c, d: None)[0]


# what the reference's decode raises on a crafted row: msgpack's own errors (ExtraData, FormatError,
# incomplete input and UnicodeDecodeError are ValueErrors), the ext hook's ValueError, the unpacking
# of something that is not [legend, values], an unknown legend, Legend's value-count assertion
PY_RAISES = (ValueError, msgpack.exceptions.UnpackException, KeyError, AssertionError)


def expect(olds, news, legends, schemas):
    """per update the changed names by Python's own decode and ==, or None where Python raises
    (malformed msgpack, unknown legend, a value count that is not the legend's)"""
    out = []
    so, sn = schemas
    for ob, nb in zip(olds, news):
        try:
            old = O.py_feature(ob, [1], legends[_legend_hex_of(ob)], so)
            new = O.py_feature(nb, [1], legends[_legend_hex_of(nb)], sn)
            out.append(O.py_changed_fields(old, new))
        except PY_RAISES:
            out.append(None)
    return out


# ------------------------------------------------------------------------------------------
# the value matrix of the semantics set


def value_matrix():
    """[(label, bytes)]: every header form of ints, floats, nil / bools, strs, bins and exts whose
    pairwise == is worth asking: equal values in different encodings, neighbours, int == float"""
    out = []
    ints = [0, 1, 2, 127, 128, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 53,
            2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, -1, -32, -33, -128, -2 ** 63]
    for v in ints:
        out += [(f"int {v} {k}", b) for k, b in int_forms(v).items()]
    floats = [0.0, -0.0, 1.0, -1.0, 0.5, 255.0, 2.0 ** 31, 2.0 ** 53, 2.0 ** 63, -2.0 ** 63, 2.0 ** 64, 0.1, 1e300,
              math.inf, -math.inf, math.nan]
    for x in floats:
        out += [(f"float {x!r} {k}", b) for k, b in float_forms(x).items()]
    out += [("nil", NIL), ("true", TRUE), ("false", FALSE)]
    strs = [b"", b"a", b"GP", "é".encode(), b"abcdefghij", b"abcdefghijk", b"abcdefghijkl" + b"m" * 19, b"s" * 32]
    for s in strs:
        out += [(f"str {len(s)} {k}", b) for k, b in str_forms(s).items()]
    bins = [b"", b"a", b"GP", b"GP\x00\x01", b"abcdefghij", b"GP" + b"\x07" * 14, b"abcdefghijkl" + b"m" * 19,
            b"s" * 32]
    for s in bins:
        out += [(f"bin {len(s)} {k}", b) for k, b in bin_forms(s).items()]
    for code, pay in ((G, b""), (G, b"GP"), (G, b"GP\x00\x01"), (G, b"GP" + b"\x07" * 6), (G, b"GP" + b"\x07" * 14),
                      (G, b"GP" + b"\x07" * 18), (5, b"GP" + b"\x07" * 6), (5, b""), (5, b"a"), (5, b"GP\x00\x01"), (-1, b"GP\x00\x01"), (5, b"GP" + b"\x07" * 18)):
        out += [(f"ext {code} {len(pay)} {k}", b) for k, b in ext_forms(code, pay).items()]
    return out


# ------------------------------------------------------------------------------------------
# the crafted sets (each built once per process; every test and every kernel parametrisation
# shares the Set, its Python expectation and its oracle result)

# a front padding that pushes what follows out of both head windows (128 B for the small shape, 80 B
# for the large one, from the blob's 16-B-aligned start) and a back padding longer than both tail
# windows (48 / 64 B)
FRONT_OUT, BACK_OUT = 150, 100


@functools.lru_cache(maxsize=None)
def semantics_set(big=False):
    """the cross product of value_matrix() as the middle value of three"""
    hx, lg = legend_of(["a", "b", "c"])
    vm = value_matrix()
    olds, news = [], []
    one, z = b"\x01", b"\xa1z"
    enc = [blob(hx, [one, b, z]) for _, b in vm]
    for x in enc:
        for y in enc:
            olds.append(x)
            news.append(y)
    return Set("semantics", olds, news, {hx: lg}, schema_of(["a", "b", "c"]), big=big)


def _pos_legends():
    ids = {(p, q): (["p"] if p else []) + ["v"] + (["q"] if q else []) for p in (0, 1) for q in (0, 1)}
    return {k: legend_of(v) for k, v in ids.items()}


def _flip(b, i):
    return b[:i] + bytes([b[i] ^ 0x40]) + b[i + 1:]


@functools.lru_cache(maxsize=None)
def position_set():
    """six value kinds at front paddings 0-160 B and back paddings {0, 3, 47, 64, 90} B, equal and
    different, the new side's front padding 0-15 B longer than the old side's"""
    legs = _pos_legends()
    kinds = [
        ("fixint", b"\x05", b"\x06"),
        ("u64", b"\xcf" + _be(2 ** 63 + 5, 8), None),
        ("f64", b"\xcb" + struct.pack(">d", 1234.5678), None),
        ("str20", str_forms(b"abcdefghijklmnopqrst")["s8"], None),
        ("bin40", bin_forms(rbytes(40, 5))["b8"], None),
        ("ext61", ext_forms(G, geom(61))["e8"], None),
    ]
    olds, news = [], []
    n = 0
    for ki, (_, val, other) in enumerate(kinds):
        for front in range(0, 161):
            for back in (0, 3, 47, 64, 90):
                for differ in (0, 1):
                    n += 1
                    skew = (front * 7 + back + 3 * ki + 5 * differ) % 16
                    # the differing byte: the last one, or (odd rows of the byte kinds) one 18 B before it
                    nv = val
                    if differ:
                        nv = other or _flip(val, len(val) - 1 if n % 2 == 0 or len(val) < 20 else len(val) - 18)
                    hx, _ = legs[(1 if front else 0, 1 if back else 0)]
                    hy, _ = legs[(1 if front + skew else 0, 1 if back else 0)]
                    q = [s_total(back, b"q")] if back else []
                    olds.append(blob(hx, ([s_total(front)] if front else []) + [val] + q))
                    news.append(blob(hy, ([s_total(front + skew)] if front + skew else []) + [nv] + q))
    return Set("position", olds, news, {h: l for h, l in legs.values()}, schema_of(["p", "v", "q"]))


PAYLOAD_LENGTHS = [13, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025]
PAYLOAD_LONG = [65535, 65536, 70000]


def _bin(b, wide=False):
    f = bin_forms(b)
    return f["b32"] if wide or "b16" not in f else f["b16"] if "b8" not in f else f["b8"]


@functools.lru_cache(maxsize=None)
def payload_set():
    """bin payloads outside both windows: each length equal / first byte / last byte / middle byte /
    only a neighbouring byte outside the payload different, at every relative skew 0-15.  The byte
    just before a payload is its own length byte, so the nearest byte before it that can differ
    without changing the value is the last byte of the value in front; the byte just after it is
    the next value's first byte.  Schema p, v, n, q: n is the neighbour behind the payload."""
    hx, lg = legend_of(["p", "v", "n", "q"])
    olds, news = [], []

    def row(n, variant, skew, seed):
        pay = rbytes(n, seed)
        new = pay
        p_old, p_new = s_total(FRONT_OUT), s_total(FRONT_OUT + skew)
        nb_old = nb_new = b"\x11"
        if variant == 1:
            new = _flip(pay, 0)
        elif variant == 2:
            new = _flip(pay, n - 1)
        elif variant == 3:
            new = _flip(pay, n // 2)
        elif variant == 4:  # the neighbours differ, the payload does not
            p_new = _flip(p_new, len(p_new) - 1)
            nb_new = b"\x12"
        # (every other length / variant: the new side in the bin32 header, the same length in another width)
        olds.append(blob(hx, [p_old, _bin(pay), nb_old, s_total(BACK_OUT, b"q")]))
        news.append(blob(hx, [p_new, _bin(new, wide=(n + variant) % 2 == 1), nb_new, s_total(BACK_OUT, b"q")]))

    seed = 0
    for n in PAYLOAD_LENGTHS:
        for variant in range(5):
            for skew in range(16):
                seed += 1
                row(n, variant, skew, seed)
    for n in PAYLOAD_LONG:
        row(n, 0, 3, 2 * n)
        row(n, 2, 9, 2 * n + 2)
    return Set("payload", olds, news, {hx: lg}, schema_of(["p", "v", "n", "q"]))


@functools.lru_cache(maxsize=None)
def queue_set():
    """every update carries three payloads outside the windows (48, 64 and 80 B): a round of 32 or
    64 updates queues more compares than the round's queue holds"""
    ids = ["p", "v1", "v2", "v3", "q"]
    hx, lg = legend_of(ids)
    olds, news = [], []
    for u in range(256):
        pays = [rbytes(n, 31 * u + i) for i, n in enumerate((48, 64, 80))]
        newp = list(pays)
        for i in range(3):
            if (u >> i) & 1:
                newp[i] = _flip(pays[i], (u * 7 + i) % len(pays[i]))
        skew = u % 16
        olds.append(blob(hx, [s_total(FRONT_OUT)] + [_bin(p) for p in pays] + [s_total(BACK_OUT, b"q")]))
        news.append(blob(hx, [s_total(FRONT_OUT + skew)] + [_bin(p) for p in newp] + [s_total(BACK_OUT, b"q")]))
    return Set("queue", olds, news, {hx: lg}, schema_of(ids))


@functools.lru_cache(maxsize=None)
def wide_set(n_cols, big=False):
    """n_cols value columns (union keys 0 .. n_cols-1, the pk last) under one legend: small values
    everywhere, 64-B payloads at the keys around the mask-word and queue-key limits, array headers
    dc and (non-canonically) dd, and one failing row whose last key was already set"""
    ids = [f"k{i}" for i in range(n_cols)]
    hx, lg = legend_of(ids)
    long_keys = sorted({k for k in (0, 63, 64, 255, 256, 299) if k < n_cols} | {n_cols - 1})
    olds, news = [], []
    rng = np.random.default_rng(n_cols)

    def values(u, change):
        vals = []
        for k in range(n_cols):
            if k in long_keys:
                pay = rbytes(64, 1000 * u + k)
                vals.append(_bin(_flip(pay, (u + k) % 64) if k in change else pay))
            else:
                vals.append(bytes([(k + (1 if k in change else 0)) & 0x7F]))
        return vals

    for u in range(48):
        if u < len(long_keys):
            change = {long_keys[u]}
        elif u < 2 * len(long_keys):
            change = set(long_keys) - {long_keys[u - len(long_keys)]}
        else:
            change = set(rng.choice(n_cols, size=int(rng.integers(0, 6)), replace=False).tolist())
        form = "a32" if u % 5 == 0 else "a16"
        olds.append(blob(hx, values(u, set()), array_form="a16"))
        b = blob(hx, values(u, change), array_form=form)
        if u == 20:  # the last key differs (its bit is set), then a byte trails: status 4, mask clear
            b = blob(hx, values(u, {0, n_cols - 1}), array_form=form) + b"\x00"
        if u == 22:  # the last value is missing on both sides after others differed: status 1, mask clear
            olds[-1] = blob(hx, values(u, set())[:-1], array_form="a16")
            b = blob(hx, values(u, {0, n_cols - 2})[:-1], array_form=form)
        if u == 24:  # missing on one side
            b = blob(hx, values(u, {0, n_cols - 2})[:-1], array_form=form)
        if u == 26:  # missing on both sides and a trailing byte: status 4 wins
            olds[-1] = blob(hx, values(u, set())[:-1], array_form="a16")
            b = blob(hx, values(u, {n_cols - 2})[:-1], array_form=form) + b"\xc0"
        if u == 28:  # a malformed last value behind a differing key of the last mask word
            b = blob(hx, values(u, {n_cols - 2})[:-1] + [b"\xc1"], array_form=form)
        news.append(b)
    return Set(f"wide{n_cols}", olds, news, {hx: lg}, schema_of(ids, pk_last=True), big=big)


@functools.lru_cache(maxsize=None)
def legends_set(n_cols, n_leg, same_schema=False):
    """cross-legend pairs: n_leg legends per side that reorder and drop columns, an old and a new
    schema that each lack some of the other's columns — map codes -1 (not in the schema), -2 (not
    in the legend) and -3 (the pk) beside value indices — every (old legend, new legend) pair twice.  A key
    missing from one schema sends every pair down the general path; with same_schema both sides
    read one schema, and the same-legend pairs take the lockstep path"""
    ids = [f"c{i}" for i in range(n_cols)]
    rng = np.random.default_rng(100 * n_cols + n_leg)
    legs = []
    for j in range(n_leg):
        cols = list(ids)
        if j % 3 == 1:
            cols = cols[::-1]
        elif j % 3 == 2:
            cols = [cols[i] for i in rng.permutation(n_cols)]
        if j >= 2:  # drop a few columns
            drop = set(rng.choice(n_cols, size=max(1, n_cols // 8), replace=False).tolist())
            cols = [c for c in cols if int(c[1:]) not in drop]
        legs.append(legend_of(cols) + (cols,))
    # the old schema lacks the last columns, the new one the first: union = old, then new-only
    cut = max(1, n_cols // 10)
    old_schema, new_schema = schema_of(ids[:-cut]), schema_of(ids[cut:])
    if same_schema:
        old_schema = new_schema = schema_of(ids)
    olds, news = [], []
    u = 0
    for a in range(n_leg):
        for b in range(n_leg):
            for rep in range(2):
                u += 1
                base = {c: bytes([(int(c[1:]) * 3 + u) & 0x7F]) for c in ids}
                for c in rng.choice(n_cols, size=3, replace=False):
                    base[ids[c]] = _bin(rbytes(40, u * 7 + int(c)))
                new = dict(base)
                if rep:
                    for c in rng.choice(n_cols, size=min(n_cols, 4), replace=False):
                        c = ids[c]
                        new[c] = _flip(new[c], len(new[c]) - 1)
                olds.append(blob(legs[a][0], [base[c] for c in legs[a][2]]))
                news.append(blob(legs[b][0], [new[c] for c in legs[b][2]]))
    return Set(f"legends{n_cols}x{n_leg}{'s' if same_schema else ''}", olds, news, {h: l for h, l, _ in legs}, old_schema, new_schema)


@functools.lru_cache(maxsize=None)
def headers_set(big=False):
    """the three legend header forms and the three array header forms on either side, an unknown
    legend (status 2), a first byte that is not 92, blobs of 0, 43 and 44 bytes"""
    hx, lg = legend_of(["a", "b", "c"])
    he, le = legend_of([])
    unknown = "0123456789abcdef0123456789abcdef01234567"
    vals = [b"\x01", b"\xa3abc", _bin(rbytes(40, 9))]
    olds, news = [], []
    forms = [(lf, af) for lf in ("s8", "s16", "s32") for af in ("fix", "a16", "a32")]
    for i, (lf, af) in enumerate(forms):
        for j, (mf, bf) in enumerate(forms):
            nv = list(vals)
            if (i + j) % 2:
                nv[(i + j) % 3] = b"\x02"
            olds.append(blob(hx, vals, lf, af))
            news.append(blob(hx, nv, mf, bf))
    good = blob(hx, vals)
    empty = blob(he, [])  # 44 bytes: a legend without value columns
    assert len(empty) == 44
    odd = [
        (blob(unknown, vals), good), (good, blob(unknown, vals)),            # status 2
        (b"\x93" + good[1:] + b"\xc0", good), (good, b"\x91" + good[1:]),  # not a 2-array
        (b"", good), (good, b""), (b"", b""),
        (empty[:43], empty), (empty, empty[:43]),                            # 43 bytes: no array header
        (empty, empty), (empty, good), (good, empty),
        (blob(he, [], "s16"), empty), (blob(he, [], "s8", "a32"), blob(he, [], "s32", "a16")),
    ]
    for o, n in odd:
        olds += [good, o, good]
        news += [good, n, good]
    return Set("headers", olds, news, {hx: lg, he: le}, schema_of(["a", "b", "c"]), big=big)


@functools.lru_cache(maxsize=None)
def maxvals_set(big=False):
    """4,096 nils (the most values a blob may hold) and 4,097 (status 3), under a legend of 4,096
    columns of which the schema keeps the first three: the value-to-key table follows the largest
    value index a schema column maps, so the tables stay small"""
    ids = [f"n{i}" for i in range(4096)]
    hx, lg = legend_of(ids)
    b96, b97 = blob(hx, [NIL] * 4096), blob(hx, [NIL] * 4097)
    c96 = blob(hx, [NIL, b"\x07"] + [NIL] * 4093 + [b"\x09"], array_form="a32")
    olds = [b96, b96, b97, b96, b97, b96]
    news = [b96, c96, b96, b97, b97, b96]
    return Set("maxvals", olds, news, {hx: lg}, schema_of(["n0", "n1", "n2"]), big=big)


def _malformed_rows(hx):
    """(old, new) pairs Python raises on or the engine documents as refused: schema g, a, b"""
    g = ext_forms(G, geom(300))["e16"]          # longer than either head window: its compare is queued
    g2 = ext_forms(G, _flip(geom(300), 200))["e16"]
    a, b = b"\x05", b"\xa3abc"
    good = blob(hx, [g, a, b])
    bads = {
        "nested": b"\x91\x01", "c1": b"\xc1", "badgeom": ext_forms(G, b"XYZ1")["fix"],
        "badgeom8": ext_forms(G, b"G")["e8"], "map": b"\x80",
    }
    rows, nested = [], set()
    for name, bad in bads.items():
        if name in ("nested", "map"):  # Python decodes a nested container; the engine refuses it (status 4)
            nested |= set(range(len(rows), len(rows) + 4))
        rows.append((good, blob(hx, [bad, a, b])))            # the failing value first
        rows.append((blob(hx, [g, a, bad]), good))            # last
        rows.append((good, blob(hx, [g2, a, bad])))           # after a queued payload that differs
        rows.append((blob(hx, [g, bad, b]), blob(hx, [g2, a, b])))
    rows.append((good, good + b"\x00"))                        # trailing byte
    rows.append((good + b"\xc0", good))
    rows.append((good, blob(hx, [g2, b"\x06", b]) + b"\x00"))  # ... after bits were set
    rows.append((good, good[:-1]))                             # truncated in the last value
    rows.append((good[:200], good))                            # truncated in the payload
    rows.append((good, blob(hx, [g2, a, b"\xd9\x05abc"])))     # str8 longer than the blob
    short = blob(hx, [g, a])
    short2 = blob(hx, [g2, b"\x06"])
    rows.append((short, short))                                # value count short of the legend, both sides
    rows.append((short, short2))                               # ... with differences before the missing value
    rows.append((short, good))                                 # short on one side
    rows.append((good, short2))
    rows.append((blob(hx, [g]), blob(hx, [g])))
    rows.append((blob(hx, []), blob(hx, [])))
    rows.append((blob(hx, [g, a], count=3), good))             # the header promises a value that is not there
    rows.append((short, good + b"\x00"))                       # status 4 wins over status 1
    rows.append((short + b"\x00", short2 + b"\x00"))
    return rows, nested, good, blob(hx, [g2, b"\x06", b])


@functools.lru_cache(maxsize=None)
def malformed_set(big=False):
    """every malformed row between good rows (equal and differing) of the same round"""
    hx, lg = legend_of(["g", "a", "b"])
    rows, nested, good, good2 = _malformed_rows(hx)
    olds, news = [], []
    for o, n in rows:
        olds += [good, o, good]
        news += [good2, n, good]
    return Set("malformed", olds, news, {hx: lg}, schema_of(["g", "a", "b"]), nested={3 * i + 1 for i in nested},
               big=big)


@functools.lru_cache(maxsize=None)
def divergence_set(big=False):
    """where Python raises and the engine answers: more values than the legend has (both sides,
    one side), invalid UTF-8 in a str.  Kept apart from every Python-checked set."""
    hx, lg = legend_of(["g", "a", "b"])
    g = ext_forms(G, geom(300))["e16"]
    good = blob(hx, [g, b"\x05", b"\xa3abc"])
    more = blob(hx, [g, b"\x05", b"\xa3abc", b"\x09"])
    more2 = blob(hx, [g, b"\x06", b"\xa3abc", b"\x0a", NIL])
    bad8 = blob(hx, [g, b"\x05", b"\xa3a\xffc"])
    bad8b = blob(hx, [g, b"\x05", b"\xa3a\xfec"])
    olds = [more, more, good, more2, bad8, bad8, good]
    news = [more, more2, more, good, bad8, bad8b, bad8]
    want = [[], ["a"], [], ["a"], [], ["b"], ["b"]]
    return Set("divergence", olds, news, {hx: lg}, schema_of(["g", "a", "b"]), big=big), want


@functools.lru_cache(maxsize=None)
def arena_end_set(residue):
    """an arena whose last blob ends at the arena's end with a payload as its last value; the old
    arena's length is ``residue`` mod 16, the new one's five more"""
    hx, lg = legend_of(["p", "v"])
    olds, news = [], []
    for u in range(8):
        pay = rbytes(40 + u, 50 + u + residue)
        olds.append(blob(hx, [s_total(1 + u), _bin(pay)]))
        news.append(blob(hx, [s_total(3 + 2 * u), _bin(_flip(pay, len(pay) - 1) if u % 2 else pay)]))

    def fit(blobs, want, first_pad):
        # the first blob's padding grows until the arena's length has the wanted residue
        total = sum(len(b) for b in blobs)
        grow = (want - total) % 16
        pay = rbytes(40, 50 + residue)
        blobs[0] = blob(hx, [s_total(first_pad + grow), _bin(pay)])
        assert sum(len(b) for b in blobs) % 16 == want % 16

    fit(olds, residue, 1)
    fit(news, residue + 5, 3)
    return Set(f"arena_end{residue}", olds, news, {hx: lg}, schema_of(["p", "v"]))


TILE, TILE_BYTES = 32, 16384


@functools.lru_cache(maxsize=None)
def tiles_set():
    """tiles of 32 back-to-back updates whose old span reaches 16,384 B + {0, +-1, +-15, +-16, +-17}
    inside a header, inside a value, or exactly at a blob's end; the new side's blobs are longer,
    so its span crosses in an earlier update.  Every tile is a multiple of 16 B long on both
    sides, so each starts on a 16-B boundary of its arena."""
    ids = ["p", "v", "q"]
    hx, lg = legend_of(ids)
    olds, news = [], []

    def mk(p_total, pay, q_total):
        return blob(hx, [s_total(p_total), _bin(pay), s_total(q_total, b"q")])

    PAY = 600
    base_len = len(mk(20, b"x" * PAY, 20))  # 44 + 20 + 603 + 20
    t = 0
    for delta in (0, 1, -1, 15, -15, 16, -16, 17, -17):
        for where in ("header", "value", "end"):
            t += 1
            # blob k of the tile holds the crossing; the blobs in front of it sum to `lead`
            k = 21 + t % 3
            at = {"header": 20, "value": 200, "end": 0}[where]
            tile_o, tile_n = [], []
            for u in range(TILE):
                pay = rbytes(PAY, 77 * t + u)
                npay = _flip(pay, (13 * u + t) % PAY) if u % 3 == 0 else pay
                tile_o.append([20, pay, 20])
                tile_n.append([20 + 16 + u % 7, npay, 20 + t % 9])
            # stretch the first blobs' q padding so that the crossing lands where it should
            target = TILE_BYTES + delta
            lead, n_lead = target - at, k  # blobs 0..k-1 sum to lead: blob k starts `at` bytes before the crossing
            extra = lead - n_lead * base_len
            assert 0 <= extra <= n_lead * 200, (extra, k)
            for u in range(n_lead):
                add = min(200, extra)
                tile_o[u][2] += add
                extra -= add
            ob = [mk(*x) for x in tile_o]
            nb = [mk(*x) for x in tile_n]
            assert sum(len(b) for b in ob[:n_lead]) == lead
            # round both tiles up to 16 B through the last blob's q padding
            for blobs, spec in ((ob, tile_o), (nb, tile_n)):
                spec[-1][2] += (-sum(len(b) for b in blobs)) % 16
                blobs[-1] = mk(*spec[-1])
                assert sum(len(b) for b in blobs) % 16 == 0
            olds += ob
            news += nb
    return Set("tiles", olds, news, {hx: lg}, schema_of(ids))
