"""The batched device read's plan (kd_odb_plan.cpp) on the CPU under AddressSanitizer and UBSan (no GPU).

One stand-alone program (tests/odb_plan_host_check.cpp) is built with the sanitizers from kd_odb.cpp and
kd_odb_plan.cpp and run as a program, once per case.  For a repository and a list of ids it makes the plan
with KD_RBD_DELTAS and without, checks the plan's own invariants (every range inside its allocation, the
written ranges disjoint, bases below their deltas, the status indices, the source spans, the copies' homes),
then carries the plan out on the host in heap blocks of exactly the planned sizes — zlib for the two
inflate launches, kd_delta.h level by level, the copies — so a wrong offset is a sanitizer report, not a
GPU fault.  Here its output is compared with the crafted content and with Reader::read of the same ids.

A planner that called everything host class would pass all that, so the counts of delta-class requests,
items and depth must equal what ``git verify-pack -v`` or the crafted entry list says, exactly (as
tests/test_gpu_read_batch_device_deltas.py derives them).
"""
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import delta_craft as C
from kart_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kart_amd", "csrc")
HOST, STREAM, DELTA = 0, 1, 2
COUNTERS = ("device", "host", "compressed", "fixups", "deltas", "links", "depth", "scratch")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("odb_plan_host")
    exe = str(tmp / "odb_plan_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wshadow", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "odb_plan_host_check.cpp"), os.path.join(CSRC, "kd_odb.cpp"),
                    os.path.join(CSRC, "kd_odb_plan.cpp"), "-o", exe, "-lz", "-ldl", "-pthread"], check=True)
    count = [0]

    def run(gitdir, oids):
        """-> (with KD_RBD_DELTAS, without, Reader::read): the first two (counters, passes, [(class, status,
        bytes)]), the third [(result, type, bytes)]"""
        count[0] += 1
        ids, out = str(tmp / ("ids%d.bin" % count[0])), str(tmp / ("out%d.bin" % count[0]))
        with open(ids, "wb") as f:
            f.write(b"".join(oids))
        r = subprocess.run([exe, gitdir, ids, out], capture_output=True, text=True)
        assert r.returncode == 0, f"odb_plan_host_check failed ({r.returncode}):\n{r.stderr[-4000:]}"
        raw = open(out, "rb").read()
        at = 0

        def rows():
            nonlocal at
            got = []
            for _ in oids:
                a, b, ln = struct.unpack_from("<BBQ", raw, at)
                got.append((a, b, raw[at + 10:at + 10 + ln]))
                at += 10 + ln
            return got

        sections = []
        for _ in range(2):
            head = struct.unpack_from("<9Q", raw, at)
            at += 72
            sections.append((dict(zip(COUNTERS, head[:8])), head[8], rows()))
        reader = rows()
        assert at == len(raw)
        return sections[0], sections[1], reader

    return run


def _agree(on, off, reader, want):
    """both plans give what Reader::read gives, and that is `want`: [blob bytes | 1 missing | 2 not a
    readable blob] per id"""
    for (st, _, rows) in (on, off):
        assert st["device"] + st["deltas"] + st["host"] + st["fixups"] == len(want)
        for k, ((_, status, data), (rc, typ, rdata), w) in enumerate(zip(rows, reader, want)):
            if isinstance(w, int):
                assert status == w and data == b"", (k, status)
                assert rc == w if w == 1 else (rc == 2 or typ != 3), (k, rc, typ)
            else:
                assert (status, data) == (0, w), (k, status)
                assert (rc, typ, rdata) == (0, 3, w), (k, rc, typ)
    assert all(c in (HOST, STREAM) for c, _, _ in off[2]) and off[0]["deltas"] == off[0]["links"] == off[0]["scratch"] == 0


def _classes(section):
    return [c for c, _, _ in section[2]]


def _four(section):
    st = section[0]
    return st["device"], st["deltas"], st["host"], st["fixups"]


# ---------------------------------------------------------------------------------------------
# written by git: 150 features x 12 versions, repacked into delta chains
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def versioned(tmp_path_factory):
    feats = C.versioned_features()
    gitdir = C.init_bare(str(tmp_path_factory.mktemp("planv") / "v.git"))
    C.import_versions(gitdir, feats)
    C.repack(gitdir)
    blobs = [b for vers in feats for b in vers]
    assert len(set(blobs)) == len(blobs) == 1800
    vp = C.verify_pack(gitdir)
    oids = [C.oid_of("blob", b) for b in blobs]
    assert all(o in vp for o in oids)
    return gitdir, dict(zip(oids, blobs)), oids, vp


def _chain_closure(vp, oids):
    """the unique delta entries on the chains of `oids` (verify-pack's base links)"""
    seen = set()
    for o in oids:
        while vp[o][2] is not None and o not in seen:
            seen.add(o)
            o = vp[o][2]
    return seen


def _versioned_case(check, versioned, ask, want=None):
    """the counters and classes verify-pack gives for the packed blobs among `ask`"""
    gitdir, by_oid, _, vp = versioned
    on, off, reader = check(gitdir, ask)
    _agree(on, off, reader, want or [by_oid[o] for o in ask])
    known = [o for o in ask if o in vp]
    n_delta = sum(vp[o][0] > 0 for o in known)
    assert _classes(on) == [(DELTA if vp[o][0] else STREAM) if o in vp else HOST for o in ask]
    assert _classes(off) == [STREAM if o in vp and not vp[o][0] else HOST for o in ask]
    assert _four(on) == (len(known) - n_delta, n_delta, len(ask) - len(known), 0)
    assert _four(off) == (len(known) - n_delta, 0, len(ask) - len(known) + n_delta, 0)
    assert on[0]["links"] == len(_chain_closure(vp, known))
    assert on[0]["depth"] == max([vp[o][0] for o in known] or [0])
    assert on[1] == off[1] == 1
    return on, off


def test_all_ids_in_pack_order_and_shuffled(check, versioned):
    _, _, oids, vp = versioned
    n_delta = sum(vp[o][0] > 0 for o in oids)
    assert n_delta >= 1000 and max(vp[o][0] for o in oids) >= 4
    order = sorted(oids, key=lambda o: vp[o][1])
    shuffled = [oids[k] for k in np.random.default_rng(2).permutation(len(oids))]
    for ask in (order, shuffled):
        on, _ = _versioned_case(check, versioned, ask)
        assert on[0]["links"] == n_delta and on[0]["scratch"] > 0 and on[0]["compressed"] > 0


def test_only_the_chain_tips(check, versioned):
    """intermediate versions and bases nobody asked for live in workspace: more links than requests"""
    _, _, oids, vp = versioned
    bases = {vp[o][2] for o in oids if vp[o][2] is not None}
    tips = [o for o in oids if vp[o][0] > 0 and o not in bases]
    assert tips
    on, _ = _versioned_case(check, versioned, tips)
    assert on[0]["links"] > on[0]["deltas"] == len(tips) and on[0]["device"] == 0


def test_request_shapes(check, versioned):
    gitdir, by_oid, oids, vp = versioned
    d = next(o for o in oids if vp[o][0] >= 3)
    b = vp[d][2]
    root = b
    while vp[root][2] is not None:
        root = vp[root][2]
    assert vp[b][0] >= 2 and vp[root][0] == 0
    on, _ = _versioned_case(check, versioned, [d, d, d])  # one id three times: one item, two copies
    assert on[0]["deltas"] == 3 and on[0]["links"] == vp[d][0]
    for ask in ([d, b], [b, d], [d, b, root], [root, b, d], [b, root, d, b]):  # a delta, an intermediate link, its base
        on, _ = _versioned_case(check, versioned, ask)
        assert on[0]["links"] == on[0]["depth"] == vp[d][0]
    tree = bytes.fromhex(subprocess.run(["git", "--git-dir", gitdir, "rev-parse", "main^{tree}"], check=True,
                                        capture_output=True).stdout.decode().strip())
    missing = hashlib.sha1(b"no such object").digest()
    on, _ = _versioned_case(check, versioned, [d, missing, tree, b, d], want=[by_oid[d], 1, 2, by_oid[b], by_oid[d]])
    assert on[0]["deltas"] == 3 and on[0]["host"] == 2
    on, off, reader = check(gitdir, [])  # n = 0
    assert on[0] == off[0] == dict.fromkeys(COUNTERS, 0) and reader == []


# ---------------------------------------------------------------------------------------------
# hand-made packs
# ---------------------------------------------------------------------------------------------
def _text(k, n=300):
    return (b"feature %d: " % k) + bytes(np.random.default_rng(100 + k).integers(97, 123, n, dtype=np.uint8))


def _edit(prev, k):
    """(delta, result): the previous version with 8 bytes replaced"""
    at = 20 + 7 * (k % 30)
    return C.encode(prev, [("c", 0, at), ("i", b"<edit%03d>" % (k % 1000)), ("c", at + 8, len(prev) - at - 8)])


def test_ref_delta_with_its_base_in_the_same_pack(check, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "r.git"))
    base = _text(1)
    d1, r1 = _edit(base, 1)
    d2, r2 = _edit(r1, 2)
    entries = [{"kind": "ref", "base_oid": C.oid_of("blob", r1), "delta": d2},  # (the base behind its delta: REF_DELTA may)
               {"kind": "blob", "content": base},
               {"kind": "ref", "base_oid": C.oid_of("blob", base), "delta": d1}]
    _, _, oids = C.write_pack(gitdir, entries, index="git")
    on, off, reader = check(gitdir, oids)
    _agree(on, off, reader, [r2, base, r1])
    assert _classes(on) == [DELTA, STREAM, DELTA] and _classes(off) == [HOST, STREAM, HOST]
    assert _four(on) == (1, 2, 0, 0) and (on[0]["links"], on[0]["depth"]) == (2, 2)


def test_ref_delta_with_its_base_in_another_pack_is_host_class(check, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "x.git"))
    base = _text(2)
    d1, r1 = _edit(base, 1)
    d2, r2 = _edit(r1, 2)
    C.write_pack(gitdir, [{"kind": "blob", "content": base}], index="git")
    _, _, oids = C.write_pack(gitdir, [{"kind": "ref", "base_oid": C.oid_of("blob", base), "delta": d1},
                                       {"kind": "ofs", "base": 0, "delta": d2}],
                              index="own", extern={C.oid_of("blob", base): ("blob", base)})
    on, off, reader = check(gitdir, oids + [C.oid_of("blob", base)])
    _agree(on, off, reader, [r1, r2, base])
    assert _classes(on) == [HOST, HOST, STREAM]
    assert _four(on) == (1, 0, 2, 0) and (on[0]["links"], on[0]["depth"]) == (0, 0)


def test_chain_over_a_tree_is_status_2(check, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "t.git"))
    tree = b"100644 a\0" + hashlib.sha1(b"a").digest() + b"100644 b\0" + hashlib.sha1(b"b").digest()
    delta, res = C.encode(tree, [("c", 0, 29)])
    blob = _text(3)
    _, _, oids = C.write_pack(gitdir, [{"kind": "tree", "content": tree}, {"kind": "ofs", "base": 0, "delta": delta},
                                       {"kind": "blob", "content": blob}], index="own")
    assert oids[1] == C.oid_of("tree", res)
    on, off, reader = check(gitdir, oids)
    _agree(on, off, reader, [2, 2, blob])
    assert _classes(on) == [HOST, HOST, STREAM] and _four(on) == (1, 0, 2, 0)


def test_result_above_the_device_limit_is_host_class(check, tmp_path):
    gitdir = C.init_bare(str(tmp_path / "big.git"))
    base = bytes(np.random.default_rng(4).integers(0, 256, 200 << 10, dtype=np.uint8))
    ops = [("c", k << 16, 1 << 16) for k in range(3)] + [("c", 3 << 16, 8 << 10), ("c", 0, 1 << 16), ("c", 1 << 16, 36 << 10)]
    big_delta, big = C.encode(base, ops)
    assert len(big) == 300 << 10 and len(base) <= N.KD_INF_MAX < len(big)
    d1, r1 = C.encode(base, [("c", 100, 5000)])
    _, _, oids = C.write_pack(gitdir, [{"kind": "blob", "content": base}, {"kind": "ofs", "base": 0, "delta": big_delta},
                                       {"kind": "ofs", "base": 0, "delta": d1}], index="git")
    on, off, reader = check(gitdir, oids)
    _agree(on, off, reader, [base, big, r1])
    assert _classes(on) == [STREAM, HOST, DELTA]
    assert _four(on) == (1, 1, 1, 0) and (on[0]["links"], on[0]["depth"]) == (1, 1)


def test_chain_deeper_than_the_limit(check, tmp_path):
    """66 links: levels 1..64 are delta class, the two below them host class"""
    gitdir = C.init_bare(str(tmp_path / "deep.git"))
    cur = _text(5)
    entries, want = [{"kind": "blob", "content": cur}], [cur]
    for k in range(N.KD_DL_MAX_DEPTH + 2):
        delta, cur = _edit(cur, k)
        entries.append({"kind": "ofs", "base": k, "delta": delta})
        want.append(cur)
    assert len(set(want)) == len(want) == 67
    _, _, oids = C.write_pack(gitdir, entries, index="git")
    on, off, reader = check(gitdir, oids)
    _agree(on, off, reader, want)
    assert _classes(on) == [STREAM] + [DELTA] * N.KD_DL_MAX_DEPTH + [HOST] * 2
    assert _four(on) == (1, N.KD_DL_MAX_DEPTH, 2, 0)
    assert on[0]["depth"] == N.KD_DL_MAX_DEPTH == on[0]["links"]


@pytest.mark.parametrize("damage", ["zlib-stream", "copy-past-base"])
def test_a_failed_middle_link_fails_what_is_below_it_only(check, tmp_path, damage):
    """base <- d1 <- d2 (damaged) <- d3, and a sibling of d1 on the same base: d2 and d3 fail in the first
    pass's levels and on the host, and are host-class failures of the second; everything else — the sibling
    included — gets its bytes"""
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
    on, off, reader = check(gitdir, [oids[k] for k in (5, 3, 4, 2, 1, 0)])
    _agree(on, off, reader, [other, 2, rs, 2, r1, base])
    assert _classes(on) == [STREAM, HOST, DELTA, HOST, DELTA, STREAM]
    assert _four(on) == (2, 2, 2, 0) and (on[0]["links"], on[0]["depth"]) == (2, 1)
    assert (on[1], off[1]) == (2, 1)


def test_two_ref_deltas_naming_each_other(check, tmp_path):
    """a cycle git would never write: both are host class (the planner does not loop), the Reader calls
    both corrupt"""
    gitdir = C.init_bare(str(tmp_path / "cyc.git"))
    a, b, plain = _text(10), _text(11), _text(12)
    da, _ = C.encode(b, [("c", 0, 100), ("i", b"from b")])
    db, _ = C.encode(a, [("c", 0, 100), ("i", b"from a")])
    oids = [C.oid_of("blob", x) for x in (a, b, plain)]
    entries = [{"kind": "ref", "base_oid": oids[1], "delta": da}, {"kind": "ref", "base_oid": oids[0], "delta": db},
               {"kind": "blob", "content": plain}]
    C.write_pack(gitdir, entries, index="own", oids=oids)
    on, off, reader = check(gitdir, oids)
    _agree(on, off, reader, [2, 2, plain])
    assert _classes(on) == [HOST, HOST, STREAM]
    assert _four(on) == (1, 0, 2, 0) and (on[0]["links"], on[0]["depth"]) == (0, 0) and on[1] == 1
