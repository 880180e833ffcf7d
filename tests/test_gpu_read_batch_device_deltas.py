"""ObjectDB.read_batch_device(..., deltas=True) against ObjectDB.read_batch: the same data, off and
status for every input — delta chains rebuilt on the GPU level by level, everything else as before.

The repositories are written by git (fast-import --depth=0, then ``repack -adf --depth=50 --window=50``)
or by hand (tests/delta_craft.py) where git would not write what is tested.  Expected counters come from
``git verify-pack -v`` or from how the pack was made, never from the code under test.
"""
import hashlib
import subprocess
import zlib

import numpy as np
import pytest

import delta_craft as C
from kart_amd import _native as N
from kart_amd.odb import ObjectDB

pytestmark = pytest.mark.gpu

EIGHT = ("device", "host", "compressed", "fixups", "deltas", "links", "depth", "scratch")


def _same(engine, db, oids):
    data, off, status = db.read_batch(oids)
    dev, dstatus, stats = db.read_batch_device(engine, oids, deltas=True)
    ddata, doff = dev.download()
    assert tuple(stats) == EIGHT
    assert np.array_equal(dstatus, status)
    assert np.array_equal(doff, off)
    assert np.array_equal(ddata, data)
    assert stats["device"] + stats["deltas"] + stats["host"] + stats["fixups"] == len(oids)
    return stats, (data.tobytes(), off, status)


def _blobs_of(read, k):
    raw, off, _ = read
    return raw[int(off[k]):int(off[k + 1])]


@pytest.fixture(scope="module")
def versioned(tmp_path_factory):
    """150 features x 12 versions at the same paths, repacked into delta chains"""
    feats = C.versioned_features()
    gitdir = C.init_bare(str(tmp_path_factory.mktemp("dlv") / "v.git"))
    C.import_versions(gitdir, feats)
    C.repack(gitdir)
    blobs = [b for vers in feats for b in vers]
    assert len(set(blobs)) == len(blobs) == 1800
    vp = C.verify_pack(gitdir)
    oids = [C.oid_of("blob", b) for b in blobs]
    assert all(o in vp for o in oids)
    return gitdir, blobs, oids, vp


def _chain_closure(vp, oids):
    """the unique delta entries on the chains of `oids` (verify-pack's base links)"""
    seen = set()
    for o in oids:
        while vp[o][2] is not None and o not in seen:
            seen.add(o)
            o = vp[o][2]
    return seen


def test_versioned_features_in_pack_order_and_shuffled(engine, versioned):
    gitdir, blobs, oids, vp = versioned
    n_delta = sum(vp[o][0] > 0 for o in oids)
    deepest = max(vp[o][0] for o in oids)
    assert n_delta >= 1000 and deepest >= 4, (n_delta, deepest)
    db = ObjectDB(gitdir)
    try:
        order = sorted(range(len(oids)), key=lambda k: vp[oids[k]][1])
        rng = np.random.default_rng(2)
        for pick in (order, rng.permutation(len(oids)).tolist()):
            stats, read = _same(engine, db, C.oid_array([oids[k] for k in pick]))
            assert not read[2].any()
            assert [_blobs_of(read, j) for j in range(len(pick))] == [blobs[k] for k in pick]
            assert stats["deltas"] == n_delta and stats["device"] == len(oids) - n_delta
            assert stats["host"] == 0 and stats["fixups"] == 0
            assert stats["depth"] == deepest and stats["links"] == n_delta
            assert stats["scratch"] > 0 and stats["compressed"] > 0
    finally:
        db.close()


def test_only_the_chain_tips_requested(engine, versioned):
    """intermediate versions and bases nobody asked for live in workspace: more links than requests"""
    gitdir, blobs, oids, vp = versioned
    bases = {vp[o][2] for o in oids if vp[o][2] is not None}
    tips = [o for o in oids if vp[o][0] > 0 and o not in bases]
    assert tips
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(tips))
        by_oid = dict(zip(oids, blobs))
        assert [_blobs_of(read, j) for j in range(len(tips))] == [by_oid[o] for o in tips]
        assert stats["deltas"] == len(tips) and stats["device"] == 0 and stats["host"] == 0 and stats["fixups"] == 0
        assert stats["links"] == len(_chain_closure(vp, tips)) > stats["deltas"]
        assert stats["depth"] == max(vp[o][0] for o in tips)
    finally:
        db.close()


def test_request_shapes(engine, versioned):
    gitdir, blobs, oids, vp = versioned
    by_oid = dict(zip(oids, blobs))
    d = next(o for o in oids if vp[o][0] >= 3)
    b = vp[d][2]
    tree = bytes.fromhex(subprocess.run(["git", "--git-dir", gitdir, "rev-parse", "main^{tree}"], check=True,
                                        capture_output=True).stdout.decode().strip())
    missing = hashlib.sha1(b"no such object").digest()
    db = ObjectDB(gitdir)
    try:
        for pair in ([d, b], [b, d]):  # a delta and its own base, in both orders
            stats, read = _same(engine, db, C.oid_array(pair))
            assert [_blobs_of(read, 0), _blobs_of(read, 1)] == [by_oid[pair[0]], by_oid[pair[1]]]
            assert stats["deltas"] == 2 and stats["links"] == vp[d][0] and stats["depth"] == vp[d][0]
        stats, read = _same(engine, db, C.oid_array([d, d, d]))  # the same delta three times
        assert [_blobs_of(read, k) for k in range(3)] == [by_oid[d]] * 3
        assert stats["deltas"] == 3 and stats["links"] == vp[d][0]
        stats, read = _same(engine, db, C.oid_array([d, missing, tree, b, d]))
        assert read[2].tolist() == [0, 1, 2, 0, 0]
        assert stats["deltas"] == 3 and stats["host"] == 2
        dev, st, stats = db.read_batch_device(engine, np.zeros((0, 20), np.uint8), deltas=True)  # n = 0
        assert dev.n == 0 and st.size == 0 and stats == dict.fromkeys(EIGHT, 0)
        assert dev.download()[1].tolist() == [0]
    finally:
        db.close()


def test_deltas_off_is_the_four_counter_read(engine, versioned):
    gitdir, blobs, oids, vp = versioned
    db = ObjectDB(gitdir)
    try:
        ids = C.oid_array(oids[:200])
        data, off, status = db.read_batch(ids)
        for kw in ({}, {"deltas": False}):
            dev, dstatus, stats = db.read_batch_device(engine, ids, **kw)
            ddata, doff = dev.download()
            assert np.array_equal(doff, off) and np.array_equal(ddata, data) and np.array_equal(dstatus, status)
            assert tuple(stats) == EIGHT[:4]
            n_plain = sum(vp[o][0] == 0 for o in oids[:200])
            assert stats["device"] == n_plain and stats["host"] == 200 - n_plain and stats["fixups"] == 0
    finally:
        db.close()


def test_six_kind_corpus_repacked(engine, tmp_path):
    """oversized blobs, 65,536-byte blobs, zero runs and empty blobs next to deltas"""
    blobs = C.six_kind_blobs(N.KD_INF_MAX)
    gitdir = C.init_bare(str(tmp_path / "six.git"))
    C.import_blobs(gitdir, blobs)
    C.repack(gitdir)
    vp = C.verify_pack(gitdir)
    oids = [C.oid_of("blob", b) for b in blobs]
    size = dict(zip(oids, map(len, blobs)))

    def on_device(o):  # the whole chain within KD_INF_MAX (verify-pack names every base)
        while o is not None:
            if size[o] > N.KD_INF_MAX:
                return False
            o = vp[o][2]
        return True

    n_delta = sum(vp[o][0] > 0 and on_device(o) for o in oids)
    n_plain = sum(vp[o][0] == 0 and on_device(o) for o in oids)
    assert n_delta > 0
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids))
        assert [_blobs_of(read, k) for k in range(len(blobs))] == blobs
        assert stats["deltas"] == n_delta and stats["device"] == n_plain and stats["fixups"] == 0
        assert stats["host"] == len(oids) - n_delta - n_plain >= 1
    finally:
        db.close()


# ---------------------------------------------------------------------------------------------
# hand-made packs
# ---------------------------------------------------------------------------------------------
def _text(k, n=300):
    return (b"feature %d: " % k) + bytes(np.random.default_rng(100 + k).integers(97, 123, n, dtype=np.uint8))


def _edit(prev, k):
    """(delta, result): the previous version with 8 bytes replaced"""
    at = 20 + 7 * (k % 30)
    return C.encode(prev, [("c", 0, at), ("i", b"<edit%03d>" % (k % 1000)), ("c", at + 8, len(prev) - at - 8)])


def test_ref_delta_with_its_base_in_the_same_pack(engine, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "r.git"))
    base = _text(1)
    d1, r1 = _edit(base, 1)
    d2, r2 = _edit(r1, 2)
    entries = [{"kind": "ref", "base_oid": C.oid_of("blob", r1), "delta": d2},  # (the base behind its delta: REF_DELTA may)
               {"kind": "blob", "content": base},
               {"kind": "ref", "base_oid": C.oid_of("blob", base), "delta": d1}]
    _, _, oids = C.write_pack(gitdir, entries, index="git")
    assert oids == [C.oid_of("blob", r2), C.oid_of("blob", base), C.oid_of("blob", r1)]
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids))
        assert [_blobs_of(read, k) for k in range(3)] == [r2, base, r1]
        assert (stats["device"], stats["deltas"], stats["links"], stats["depth"], stats["host"], stats["fixups"]) == (1, 2, 2, 2, 0, 0)
    finally:
        db.close()


def test_ref_delta_with_its_base_in_another_pack_is_host_class(engine, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "x.git"))
    base = _text(2)
    d1, r1 = _edit(base, 1)
    d2, r2 = _edit(r1, 2)
    C.write_pack(gitdir, [{"kind": "blob", "content": base}], index="git")
    _, _, oids = C.write_pack(gitdir, [{"kind": "ref", "base_oid": C.oid_of("blob", base), "delta": d1},
                                       {"kind": "ofs", "base": 0, "delta": d2}],
                              index="own", extern={C.oid_of("blob", base): ("blob", base)})
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids + [C.oid_of("blob", base)]))
        assert [_blobs_of(read, k) for k in range(3)] == [r1, r2, base]
        assert (stats["device"], stats["deltas"], stats["host"], stats["fixups"]) == (1, 0, 2, 0)
    finally:
        db.close()


def test_chain_over_a_tree_is_status_2(engine, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "t.git"))
    tree = b"100644 a\0" + hashlib.sha1(b"a").digest() + b"100644 b\0" + hashlib.sha1(b"b").digest()
    delta, res = C.encode(tree, [("c", 0, 29)])
    blob = _text(3)
    _, _, oids = C.write_pack(gitdir, [{"kind": "tree", "content": tree}, {"kind": "ofs", "base": 0, "delta": delta},
                                       {"kind": "blob", "content": blob}], index="own")
    assert oids[1] == C.oid_of("tree", res)
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids))
        assert read[2].tolist() == [2, 2, 0] and _blobs_of(read, 2) == blob
        assert (stats["device"], stats["deltas"], stats["host"]) == (1, 0, 2)
    finally:
        db.close()


def test_result_above_the_device_limit_is_host_class(engine, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "big.git"))
    base = bytes(np.random.default_rng(4).integers(0, 256, 200 << 10, dtype=np.uint8))
    ops = [("c", k << 16, 1 << 16) for k in range(3)] + [("c", 3 << 16, 8 << 10), ("c", 0, 1 << 16), ("c", 1 << 16, 36 << 10)]
    big_delta, big = C.encode(base, ops)
    assert len(big) == 300 << 10 and len(base) <= N.KD_INF_MAX < len(big)
    d1, r1 = C.encode(base, [("c", 100, 5000)])
    _, _, oids = C.write_pack(gitdir, [{"kind": "blob", "content": base}, {"kind": "ofs", "base": 0, "delta": big_delta},
                                       {"kind": "ofs", "base": 0, "delta": d1}], index="git")
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids))
        assert [_blobs_of(read, k) for k in range(3)] == [base, big, r1]
        assert (stats["device"], stats["deltas"], stats["host"], stats["fixups"]) == (1, 1, 1, 0)
    finally:
        db.close()


def test_chain_deeper_than_the_limit(engine, tmp_path):
    """66 links: levels 1..64 are rebuilt on the device, the two below them read on the host"""
    gitdir = C.init_bare(str(tmp_path / "deep.git"))
    cur = _text(5)
    entries, want = [{"kind": "blob", "content": cur}], [cur]
    for k in range(N.KD_DL_MAX_DEPTH + 2):
        delta, cur = _edit(cur, k)
        entries.append({"kind": "ofs", "base": k, "delta": delta})
        want.append(cur)
    assert len(set(want)) == len(want)
    _, _, oids = C.write_pack(gitdir, entries, index="git")
    db = ObjectDB(gitdir)
    try:
        stats, read = _same(engine, db, C.oid_array(oids))
        assert [_blobs_of(read, k) for k in range(len(want))] == want
        assert (stats["device"], stats["deltas"], stats["host"], stats["fixups"]) == (1, N.KD_DL_MAX_DEPTH, 2, 0)
        assert stats["depth"] == N.KD_DL_MAX_DEPTH == stats["links"]
    finally:
        db.close()


@pytest.mark.parametrize("damage", ["zlib-stream", "copy-past-base"])
def test_a_failed_middle_link_fails_what_is_below_it_only(engine, tmp_path, damage):
    """base <- d1 <- d2 (damaged) <- d3, and a sibling of d1 on the same base: d2 and d3 get the host
    route's status and length 0, everything else — the sibling included — its bytes"""
    gitdir = C.init_bare(str(tmp_path / "mid.git"))
    base = _text(6)
    d1, r1 = _edit(base, 1)
    sib, rs = _edit(base, 9)
    filler = bytes(np.random.default_rng(8).integers(0, 256, 120, dtype=np.uint8))
    d2, r2 = C.encode(r1, [("c", 0, 40), ("i", filler), ("c", 40, len(r1) - 40)])
    d3, r3 = _edit(r2, 3)
    e2 = {"kind": "ofs", "base": 1, "delta": d2}
    if damage == "zlib-stream":
        stream = bytearray(zlib.compress(d2))
        stream[len(stream) // 2] ^= 0x10
        e2["stream"] = bytes(stream)
        with pytest.raises(zlib.error):
            zlib.decompress(e2["stream"])
    else:
        e2["delta"] = C.header(len(r1), len(r2)) + C.copy_op(len(r1) - 10, 50) + C.insert_op(b"x" * 100)
        assert C.apply(r1, e2["delta"]) == C.ECOPY
    other = _text(7)
    entries = [{"kind": "blob", "content": base}, {"kind": "ofs", "base": 0, "delta": d1}, e2,
               {"kind": "ofs", "base": 2, "delta": d3}, {"kind": "ofs", "base": 0, "delta": sib}, {"kind": "blob", "content": other}]
    oids = [C.oid_of("blob", x) for x in (base, r1, r2, r3, rs, other)]
    C.write_pack(gitdir, entries, index="own", oids=oids)
    db = ObjectDB(gitdir)
    try:
        ask = [oids[k] for k in (5, 3, 4, 2, 1, 0)]
        stats, read = _same(engine, db, C.oid_array(ask))
        assert read[2].tolist() == [0, 2, 0, 2, 0, 0]
        assert [_blobs_of(read, k) for k in range(6)] == [other, b"", rs, b"", r1, base]
        assert (stats["device"], stats["deltas"], stats["host"], stats["fixups"]) == (2, 2, 2, 0)
    finally:
        db.close()
