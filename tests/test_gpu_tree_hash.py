"""kd_tree_hash on the GPU against the hashlib reference (tests/tree_ref.py): ids, status, bodies and
body offsets of crafted tree batches — SHA-1 padding and header edges, run sizes around the wave,
block and ranking bounds, a long tree beside short ones, byte values, name alignment, ranking, the
order rules, the device form chained over two levels — and the recorded feature-tree ids of
tests/golden/tree_ids.json through treebuild.feature_tree."""
import json
import os

import numpy as np
import pytest

import tree_ref as R
from fixtures import GOLDEN, load
from kart_amd import _native as N
from kart_amd import treebuild as TB

pytestmark = pytest.mark.gpu
REF = R.RefEngine()

with open(os.path.join(GOLDEN, "tree_ids.json")) as f:
    TREE_IDS = json.load(f)
SIDES = [(fx, side) for fx, sides in TREE_IDS.items() for side in sides]


def pack(trees, lead=0):
    """[[(name, oid)]] -> names, name_off, oids, seg (``lead`` unused bytes in front of the names)"""
    ents = [e for t in trees for e in t]
    names, off = R.pack_names([n for n, _ in ents])
    if lead:
        names, off = np.concatenate([np.full(lead, 0x2F, np.uint8), names]), off + np.uint64(lead)
    oids = np.frombuffer(b"".join(o for _, o in ents), np.uint8).reshape(-1, 20) if ents else np.zeros((0, 20), np.uint8)
    seg = np.zeros(len(trees) + 1, np.uint64)
    seg[1:] = np.cumsum([len(t) for t in trees])
    return names, off, oids, seg


def check(engine, trees, kind, rank=False, lead=0):
    args = pack(trees, lead)
    ids, st, body, boff = engine.tree_hash(*args, kind, rank=rank, bodies=True)
    wids, wst, wbody, wboff = REF.tree_hash(*args, kind, rank=rank, bodies=True)
    assert np.array_equal(st, wst), np.nonzero(st != wst)[0][:10]
    assert np.array_equal(boff, wboff)
    assert np.array_equal(body, wbody)
    bad = np.nonzero(np.any(ids != wids, axis=1))[0]
    assert bad.size == 0, (bad[:10], [len(trees[t]) for t in bad[:10]])
    ids2, st2 = engine.tree_hash(*args, kind, rank=rank)  # without bodies: the same ids
    assert np.array_equal(ids2, wids) and np.array_equal(st2, wst)
    return wids, wst


def oid_of(rng):
    return rng.integers(0, 256, 20, dtype=np.uint8).tobytes()


def run_of(rng, k, tail=10):
    """k entries with distinct names, ascending under both order rules"""
    return [(b"%04d" % j + bytes(rng.integers(0x61, 0x7B, int(rng.integers(0, tail + 1)), dtype=np.uint8)), oid_of(rng))
            for j in range(k)]


def tree_of_body_len(rng, want, kind):
    """a tree whose body is exactly ``want`` bytes long"""
    fixed = (6 if kind == R.TREE else 7) + 21
    lens, left = [], want
    while left > 2 * (fixed + 120):
        lens.append(100)
        left -= fixed + 100
    first = (left - 2 * fixed) // 2
    lens += [first, left - 2 * fixed - first]
    assert all(3 <= x <= 255 for x in lens)
    t = [(b"%03d" % j + b"x" * (ln - 3), oid_of(rng)) for j, ln in enumerate(lens)]
    assert len(R.tree_body(t, kind)) == want
    return t


@pytest.mark.parametrize("kind", [R.BLOB, R.TREE])
def test_padding_and_header_edges(engine, kind):
    """single-entry trees of name length 1..200: every residue of the message length mod 64 (55, 56, 63
    and 0 among them) and the header's step from 2 to 3 digits; bodies of 998..1001 and 9998..10001
    bytes: its steps to 4 and 5 digits"""
    rng = np.random.default_rng(3)
    trees = [[(b"n" * ln, oid_of(rng))] for ln in range(1, 201)]
    fixed = (6 if kind == R.TREE else 7) + 21
    msg = {(len(b"tree %d\0" % (fixed + ln)) + fixed + ln) % 64 for ln in range(1, 201)}
    assert msg == set(range(64)) and fixed + 1 < 100 <= fixed + 200
    trees += [tree_of_body_len(rng, b, kind) for b in (998, 999, 1000, 1001, 9998, 9999, 10000, 10001)]
    check(engine, trees, kind)


def test_run_sizes(engine):
    """runs of 0, 1, 2, 63, 64, 65, 511, 512 and 513 entries, empty runs first, in the middle and last,
    a run that starts at entry 255 (the last entry of the first 256-entry block), 314 trees"""
    rng = np.random.default_rng(4)
    sizes = [0, 1, 2, 63, 64, 65, 60, 5, 511, 0, 512, 513, 3] + [int(x) for x in rng.integers(1, 4, 300)] + [0]
    assert sum(sizes[:7]) == 255 and len(sizes) % 64 and len(sizes) > 256
    trees = [run_of(rng, k) for k in sizes]
    for kind in (R.BLOB, R.TREE):
        ids, st = check(engine, trees, kind)
        assert not st.any() and ids[0].tobytes().hex() == R.EMPTY_TREE == ids[-1].tobytes().hex()


def test_long_tree_beside_small_ones(engine):
    rng = np.random.default_rng(5)
    long = [(b"%06d" % j + bytes(rng.integers(0x61, 0x7B, 34, dtype=np.uint8)), oid_of(rng)) for j in range(6000)]
    small = [run_of(rng, int(k)) for k in rng.integers(0, 5, 1000)]
    ids, st = check(engine, small[:500] + [long] + small[500:], R.BLOB)
    assert not st.any()


def test_byte_values(engine):
    rng = np.random.default_rng(6)
    hi = [bytes([0x80 + j, 0xFF, 0xC3, 0xA9][: 1 + j % 4]) + bytes([0x80 + j]) for j in range(100)]
    trees = [[(n, b"\0" * 20) for n in sorted(hi)], [(n, b"\xff" * 20) for n in sorted(hi)],
             [(bytes([c]), oid_of(rng)) for c in range(1, 256) if c != 0x2F]]
    for kind in (R.BLOB, R.TREE):
        ids, st = check(engine, trees, kind)
        assert not st.any()


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_name_alignment(engine, lead):
    """name lengths 1, 2, 3, ...: the names start at every offset mod 4 of the arena, whatever its lead"""
    rng = np.random.default_rng(7)
    trees = [[(b"%02d" % j + b"y" * ((j + t) % 7), oid_of(rng)) for j in range(t % 9)] for t in range(80)]
    starts = pack(trees, lead)[1][:-1]
    assert set((starts % np.uint64(4)).tolist()) == {0, 1, 2, 3}
    check(engine, trees, R.BLOB, lead=lead)
    check(engine, trees, R.TREE, lead=lead)


def test_ranking(engine):
    rng = np.random.default_rng(8)
    sizes = [512, 0, 1, 2, 64, 300, 512, 7] + [int(x) for x in rng.integers(1, 6, 100)]
    sorted_trees = []
    for k in sizes:  # names of mixed length with common prefixes: a, a-, a0, ab ...
        names = set()
        while len(names) < k:
            names.add(bytes(rng.choice(np.frombuffer(b"ab-0\xc3", np.uint8), int(rng.integers(1, 9)))))
        sorted_trees.append([(n, oid_of(rng)) for n in sorted(names)])
    shuffled = [[t[i] for i in rng.permutation(len(t))] for t in sorted_trees]
    want, st = check(engine, sorted_trees, R.BLOB)
    got, st2 = check(engine, shuffled, R.BLOB, rank=True)
    assert np.array_equal(got, want) and not st.any() and not st2.any()
    # a duplicate name: status 2 for that tree only
    dup = [list(t) for t in shuffled]
    dup[4][10] = (dup[4][40][0], dup[4][10][1])
    ids, st3 = check(engine, dup, R.BLOB, rank=True)
    assert st3.tolist() == [2 if t == 4 else 0 for t in range(len(dup))]
    assert np.array_equal(np.delete(ids, 4, 0), np.delete(want, 4, 0)) and not ids[4].any()
    # 513 entries under the flag, and the flag with tree entries
    with pytest.raises(N.Unsupported):
        engine.tree_hash(*pack([run_of(rng, 3), run_of(rng, 513)]), R.BLOB, rank=True)
    with pytest.raises(N.KdError) as ei:
        engine.tree_hash(*pack([run_of(rng, 3)]), R.TREE, rank=True)
    assert ei.value.code == N.KD_EINVAL
    ids, st = engine.tree_hash(*pack([run_of(rng, 513)]), R.BLOB)  # without the flag any length goes
    assert st.tolist() == [0]


def test_order_check_and_names(engine):
    rng = np.random.default_rng(9)
    trees = [run_of(rng, 5) for _ in range(9)]
    trees[3][1], trees[3][2] = trees[3][2], trees[3][1]
    trees[5] = [(b"a", oid_of(rng)), (b"a-", oid_of(rng))]
    trees[6] = [(b"a-", oid_of(rng)), (b"a", oid_of(rng))]
    trees[7] = [(b"same", oid_of(rng)), (b"same", oid_of(rng))]
    ids, st = check(engine, trees, R.BLOB)
    assert st.tolist() == [0, 0, 0, 1, 0, 0, 1, 1, 0]
    ids, st = check(engine, trees, R.TREE)
    assert st.tolist() == [0, 0, 0, 1, 0, 1, 0, 1, 0]
    bad = [run_of(rng, 4), [(b"p/q", oid_of(rng))], [(b"a", oid_of(rng)), (b"", oid_of(rng))], [(b"z" * 256, oid_of(rng))],
           [(b"z" * 255, oid_of(rng))], [(b"nu\0l", oid_of(rng))], run_of(rng, 2)]
    for kind in (R.BLOB, R.TREE):
        ids, st = check(engine, bad, kind)
        assert st.tolist() == [0, 3, 3, 3, 0, 3, 0]
    ids, st = check(engine, bad[:5], R.BLOB, rank=True)
    assert st.tolist() == [0, 3, 3, 3, 0]


def test_device_form_chains_levels(engine):
    """inputs and outputs in DevBufs; the second call reads the first call's tree_oid buffer as its
    oid array, nothing downloaded in between; a body_cap one byte short is KD_EINVAL"""
    from kart_amd.device import DevBuf

    rng = np.random.default_rng(10)
    leaves = [run_of(rng, int(k)) for k in rng.integers(1, 9, 70)]
    args = pack(leaves)
    wids, wst, wbody, wboff = REF.tree_hash(*args, R.BLOB, bodies=True)
    dev = [DevBuf.from_numpy(engine, a.reshape(-1)) for a in args]
    ids, st, body, boff = engine.tree_hash(*dev, R.BLOB, bodies=True)
    assert all(isinstance(x, DevBuf) for x in (ids, st, body, boff))
    # level 2: 70 directories "00".."69" in three trees, their ids still on the device
    dnames, doff = R.pack_names([b"%02d" % j for j in range(70)])
    dseg = np.array([0, 1, 64, 70], np.uint64)
    ids2, st2 = engine.tree_hash(dnames, doff, ids, dseg, R.TREE)
    want2, wst2 = REF.tree_hash(dnames, doff, wids, dseg, R.TREE)
    assert np.array_equal(ids2.download(np.uint8, 60).reshape(3, 20), want2)
    assert not st2.download(np.uint8, 3).any() and not wst2.any()
    assert np.array_equal(ids.download(np.uint8, 20 * 70).reshape(70, 20), wids)
    assert np.array_equal(st.download(np.uint8, 70), wst)
    assert np.array_equal(boff.download(np.uint64, 71), wboff)
    assert np.array_equal(body.download(np.uint8, wbody.size), wbody)
    need = int(wboff[-1])
    with pytest.raises(N.KdError) as ei:
        engine.tree_hash(*dev, R.BLOB, bodies=True, body_cap=need - 1)
    assert ei.value.code == N.KD_EINVAL
    with pytest.raises(N.KdError) as ei:
        engine.tree_hash(*args, R.BLOB, bodies=True, body_cap=need - 1)
    assert ei.value.code == N.KD_EINVAL
    exact = engine.tree_hash(*args, R.BLOB, bodies=True, body_cap=need)
    assert np.array_equal(exact[2], wbody) and np.array_equal(exact[0], wids)


@pytest.mark.parametrize("fx_name,side", SIDES)
def test_recorded_feature_tree_ids(engine, fx_name, side):
    fx = load(fx_name)
    paths, off = fx.a[f"{side}_names"], fx.a[f"{side}_name_off"].astype(np.uint64)
    oids, enc = fx.oids(side), fx.encoding(side)
    ft = TB.feature_tree(engine, paths, off, oids, enc, bodies=True)
    assert ft.root.hex() == TREE_IDS[fx_name][side]
    for ids, body, boff in ft.objects:  # every object's body hashes to its id
        for t in range(0, ids.shape[0], max(1, ids.shape[0] // 16)):
            assert R.object_id(body[int(boff[t]):int(boff[t + 1])].tobytes()) == ids[t].tobytes()
    if enc.scheme != "int":  # a hash-key side from key order: grouped by leaf tree, ranked inside
        order = np.asarray(fx.packed(side).order, np.int64)
        kp, ko = TB.gather_rows(paths, off, order)
        kp, ko, kid = TB.group_by_directory(kp, ko, oids[order], enc)
        assert TB.feature_tree(engine, kp, ko, kid, enc, rank=True).root.hex() == TREE_IDS[fx_name][side]
