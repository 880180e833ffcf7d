"""Crafted inputs of the key packer (kd_keypack.h on the CPU, kd_pack_keys_device on the GPU) and a Python
reference of its rules built on base64, msgpack and kart_amd.walkkey.

An item is (entry bytes, expected key, expected status); the three groups — KD_KEY_INT entries, base-64
hash paths of 4 levels and hex hash paths of 2 — are what `groups()` returns, each with its (key_mode,
levels, hex).  `mutations()` are seeded byte mutations whose expected values are the host packer's.
"""
import base64
import json
import os

import msgpack
import numpy as np

from kart_amd import _native as N
from kart_amd import walkkey

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHABET = set(walkkey.B64)
INT, HASH64, HASHHEX = (N.KD_KEY_INT, 4, 0), (N.KD_KEY_HASH, 4, 0), (N.KD_KEY_HASH, 2, 1)
_WIDTH = {0xcc: 1, 0xcd: 2, 0xce: 4, 0xcf: 8, 0xd0: 1, 0xd1: 2, 0xd2: 4, 0xd3: 8}


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
def ref_int(entry):
    """(key, status) of one KD_KEY_INT entry by the rules of kd_keypack.h"""
    name = entry[entry.rfind(b"/") + 1:]
    if len(name) > 24:
        return 0, 1
    text = name.split(b"=")[0]
    if any(c not in ALPHABET for c in text):
        return 0, 1
    nbytes = len(text) * 6 // 8
    data = base64.urlsafe_b64decode(text + b"A" * (-len(text) % 4))[:nbytes]  # (left-over bits dropped)
    if nbytes > 16 or nbytes < 2 or data[0] != 0x91:
        return 0, 1
    t = data[1]
    if not (t <= 0x7f or t >= 0xe0 or t in _WIDTH):
        return 0, 1
    if nbytes != 2 + _WIDTH.get(t, 0):
        return 0, 1
    pk = msgpack.unpackb(data[1:])
    if pk >= 1 << 63:
        return 0, 2
    return walkkey.pk_to_int_key(pk), 0


def fnv1a64(b):
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & ((1 << 64) - 1)
    return h


def ref_hash(entry, levels, hex_):
    bucket, pos, bits = 0, 0, 0
    for _ in range(levels):
        for _ in range(2 if hex_ else 1):
            if pos >= len(entry):
                return 0, 1
            ch = entry[pos]
            pos += 1
            if hex_:
                if ch not in b"0123456789abcdef":
                    return 0, 1
                bucket, bits = bucket << 4 | int(chr(ch), 16), bits + 4
            else:
                if ch not in ALPHABET:
                    return 0, 1
                bucket, bits = bucket << 6 | int(walkkey.RANK[walkkey.B64.index(ch)]), bits + 6
        if pos >= len(entry) or entry[pos] != ord("/"):
            return 0, 1
        pos += 1
    return (bucket << (64 - bits) | fnv1a64(entry[pos:]) >> bits) & ((1 << 64) - 1), 0


def ref(entry, cfg):
    return ref_int(entry) if cfg[0] == N.KD_KEY_INT else ref_hash(entry, cfg[1], cfg[2])


# ---------------------------------------------------------------------------------------------
# the crafted entries
# ---------------------------------------------------------------------------------------------
def _b64(raw):
    return base64.urlsafe_b64encode(raw)


def _kats():
    with open(os.path.join(GOLDEN, "paths.json")) as f:
        return json.load(f)


def int_valid():
    """valid KD_KEY_INT entries with the pk each encodes"""
    out = [(p.encode(), int(pk)) for pk, p in _kats()["int"]]
    pks = [s + j for s in walkkey.CLASS_BLOCK for j in range(64)]
    pks += [-(1 << 63), (1 << 63) - 1, 1 << 30, -(1 << 30), (1 << 30) - 1, -(1 << 30) - 1] + list(range(-64, 0))
    out += [(b"A/A/A/A/" + walkkey.filename(pk).encode(), pk) for pk in pks]
    out += [(walkkey.filename(pk).encode(), pk) for pk in (0, 77, -5, 1 << 40)]  # a bare filename
    # lax forms the host packer accepts: any width for any value, nothing looked at behind '=', no padding
    out += [(b"x/" + _b64(b"\x91\xcf" + (5).to_bytes(8, "big")), 5), (b"x/" + _b64(b"\x91\xd3" + b"\xff" * 8), -1),
            (b"x/" + _b64(b"\x91\xcd\x00\x07"), 7), (b"x/" + _b64(b"\x91\xd1\x00\x07"), 7),
            (b"q/kQA=!!?", 0),(b"q/kQA", 0), (b"q/kQB", 0), (b"q/kQA=A", 0), (b"//kQE=", 1)]
    return out


def int_refused():
    """(name of the rule, entry, status)"""
    big = _b64(b"\x91\xcf" + (1 << 63).to_bytes(8, "big"))
    return [
        ("empty entry", b"", 1), ("empty name", b"A/A/A/A/", 1), ("name of 25 bytes", b"A/" + b"kQA=" + b"=" * 21, 1),
        ("25 bytes and no slash", b"k" * 25, 1), ("byte outside the alphabet", b"A/kQ!=", 1),
        ("byte outside the alphabet, standard base64", b"A/kc+A", 1), ("space", b"A/kQ A", 1),
        ("17 decoded bytes", b"A/" + _b64(b"\x91" + b"\x00" * 16)[:23], 1),
        ("18 decoded bytes", b"A/" + _b64(b"\x91" + b"\x00" * 17), 1),
        ("one decoded byte", b"A/kQ==", 1), ("no decoded byte", b"A/k", 1), ("only padding", b"A/====", 1),
        ("first byte 0x92", b"A/" + _b64(b"\x92\x00"), 1), ("first byte 0x90", b"A/" + _b64(b"\x90\x00"), 1),
        ("type nil", b"A/" + _b64(b"\x91\xc0"), 1), ("type float", b"A/" + _b64(b"\x91\xca\x00\x00\x00\x00"), 1),
        ("type str", b"A/" + _b64(b"\x91\xa1a"), 1), ("type bin", b"A/" + _b64(b"\x91\xc4\x01a"), 1),
        ("type fixext", b"A/" + _b64(b"\x91\xd4\x00\x00"), 1), ("type array", b"A/" + _b64(b"\x91\x91\x00"), 1),
        ("uint16 cut short", b"A/" + _b64(b"\x91\xcd\x01"), 1), ("uint16 too long", b"A/" + _b64(b"\x91\xcd\x01\x02\x03"), 1),
        ("fixint with a tail", b"A/" + _b64(b"\x91\x05\x00"), 1), ("int64 cut short", b"A/" + _b64(b"\x91\xd3" + b"\x80" * 7), 1),
        ("uint64 2^63", b"A/" + big, 2), ("uint64 2^64 - 1", b"A/" + _b64(b"\x91\xcf" + b"\xff" * 8), 2),
    ]


def hash_valid(cfg):
    """valid hash paths of this structure: the reference's KATs and filenames of every staged length"""
    _, levels, hex_ = cfg
    out = [p.encode() for _, p in _kats()["legacy" if hex_ else "hash"]]
    lead = b"3f/a0/" if hex_ else b"-/_/A/z/"
    rng = np.random.default_rng(41)
    for ln in (0, 1, 15, 16, 17, 255, 1000):
        out.append(lead + bytes(rng.integers(0, 256, ln, dtype=np.uint8)))
    out += [(b"00/00/" if hex_ else b"A/A/A/A/") + b"kaA=", (b"ff/ff/" if hex_ else b"z/z/z/z/") + b"a/b/c"]
    return out


def hash_refused(cfg):
    _, levels, hex_ = cfg
    if hex_:
        return [("uppercase hex", b"3F/a0/kaA=", 1), ("uppercase hex, second digit", b"3f/aB/kaA=", 1),
                ("missing slash", b"3fa0/kaA=", 1), ("missing last slash", b"3f/a0", 1), ("short path", b"3f/a", 1),
                ("one digit", b"3", 1), ("empty", b"", 1), ("not hex", b"3g/a0/x", 1), ("three digits", b"3f0/a0/x", 1)]
    return [("missing slash", b"AB/C/D/x", 1), ("missing last slash", b"A/B/C/D", 1), ("short path", b"A/B/C", 1),
            ("one digit", b"A", 1), ("empty", b"", 1), ("not base64", b"A/B/+/D/x", 1), ("padding as digit", b"A/B/=/D/x", 1),
            ("two digits", b"A/B/C/DD/x", 1)]


def truncations(valid):
    """every valid entry cut at every byte"""
    return [e[:k] for e in valid for k in range(len(e))]


def group(cfg):
    """[(entry, key, status)] of one structure: valid entries, refusals between them, every truncation"""
    if cfg[0] == N.KD_KEY_INT:
        good = [(e, walkkey.pk_to_int_key(pk), 0) for e, pk in int_valid()]
        for e, k, s in good:
            assert ref_int(e) == (k, s), e
        bad = [(e, 0, st) for _, e, st in int_refused()]
        valid = [e for e, _ in int_valid()]
    else:
        valid = hash_valid(cfg)
        good = [(e, *ref(e, cfg)) for e in valid]
        assert all(s == 0 for _, _, s in good)
        bad = [(e, 0, st) for _, e, st in hash_refused(cfg)]
    for e, k, s in bad:
        assert ref(e, cfg) == (k, s), e
    items = []
    for j, g in enumerate(good):  # a refusal after every third good entry
        items.append(g)
        if j % 3 == 2 and bad:
            items.append(bad[(j // 3) % len(bad)])
    items += bad
    short = sorted(set(valid), key=len)[:40] if cfg[0] == N.KD_KEY_HASH else valid
    items += [(e, *ref(e, cfg)) for e in truncations([v for v in short if len(v) <= 64])]
    return items


def mutations(cfg, count=2000, seed=5):
    """seeded mutations of valid entries: bytes replaced, inserted or removed"""
    rng = np.random.default_rng(seed + cfg[1] + cfg[2])
    valid = [e for e, _ in int_valid()] if cfg[0] == N.KD_KEY_INT else [e for e in hash_valid(cfg) if len(e) <= 300]
    pool = b"/=-_AZaz09kQ\x00\xff+ fF"
    out = []
    for _ in range(count):
        e = bytearray(valid[int(rng.integers(0, len(valid)))])
        for _ in range(int(rng.integers(1, 4))):
            op, at = int(rng.integers(0, 3)), int(rng.integers(0, len(e) + 1))
            c = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.7 else int(rng.integers(0, 256))
            if op == 0 and at < len(e):
                e[at] = c
            elif op == 1:
                e.insert(at, c)
            elif at < len(e):
                del e[at]
        out.append(bytes(e))
    return out


def arena(entries):
    off = np.zeros(len(entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in entries])
    return np.frombuffer(b"".join(entries) + b"\0", np.uint8)[:int(off[-1])], off


def host_pack(entries, cfg, data=None, off=None):
    """(keys, status) of the host packer (kd_pack_int_keys / kd_pack_hash_keys)"""
    if data is None:
        data, off = arena(entries)
    n = len(off) - 1
    keys, status = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint8)
    pad = np.zeros(16, np.uint8)
    L = N.lib()
    if cfg[0] == N.KD_KEY_INT:
        bad = L.kd_pack_int_keys(N.ptr(data) if data.size else N.ptr(pad), N.ptr(off), n, N.ptr(keys), N.ptr(status))
    else:
        bad = L.kd_pack_hash_keys(N.ptr(data) if data.size else N.ptr(pad), N.ptr(off), n, cfg[1], cfg[2], N.ptr(keys),
                                  N.ptr(status))
    assert bad == int(np.count_nonzero(status[:n]))
    return keys[:n], status[:n]
