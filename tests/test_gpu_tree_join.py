"""kd_tree_join_batch against the Python reference of tree_craft.py: exact outputs, canaries behind every
output array and count.

Most cases run the device form on buffers of this test's own (DevBuf), each output sized exactly to what
the reference keeps and followed by CAN bytes of 0xA5 in HBM, so a store outside a task's own ranges
shows.  The host form (Engine.tree_join) is compared on the same inputs.
"""
import os
import re

import numpy as np
import pytest

import tree_craft as C
from kart_amd import _native as N
from kart_amd.device import DevBuf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAN = 64
FILL = 0xA5


# ---------------------------------------------------------------------------------------------
# running one call
# ---------------------------------------------------------------------------------------------
def _canaried(engine, nbytes):
    b = DevBuf(engine, nbytes + CAN)
    b.upload(np.full(nbytes + CAN, FILL, np.uint8))
    return b


def _body(buf, nbytes, what):
    raw = buf.download(np.uint8, nbytes + CAN)
    assert (raw[nbytes:] == FILL).all(), f"canary behind {what} overwritten"
    return raw[:nbytes]


def run_device(engine, data, off, tasks, pfx, pfx_off, k, compare, caps):
    """one device-form call; returns ([(paths, path_off, oids, modes)], count, status, totals) with every
    array downloaded whole (cap entries) after its canary was checked"""
    off = np.ascontiguousarray(off, np.uint64)
    pfx_off = np.ascontiguousarray(pfx_off, np.uint64)
    tasks = np.ascontiguousarray(tasks, np.uint32).reshape(-1, k)
    nt, ntrees = tasks.shape[0], off.shape[0] - 1
    d_data = data if isinstance(data, DevBuf) else DevBuf.from_numpy(engine, np.concatenate([data, np.zeros(16, np.uint8)]))
    d_pfx = DevBuf.from_numpy(engine, np.concatenate([np.ascontiguousarray(pfx, np.uint8), np.zeros(16, np.uint8)]))
    d_off, d_poff, d_tasks = (DevBuf.from_numpy(engine, x) for x in (off, pfx_off, tasks))
    outs, bufs = (N.KdTjOut * k)(), []
    for r in range(k):
        cn, cb = caps[r]
        sizes = (8 * (cn + 1), 4 * cn, 20 * cn, cb)
        b = [_canaried(engine, s) for s in sizes]
        bufs.append((b, sizes))
        outs[r].cap_n, outs[r].cap_bytes = cn, cb
        outs[r].path_off, outs[r].mode, outs[r].oid, outs[r].path = (x.ptr for x in b)
    d_count, d_status, d_tot = _canaried(engine, 4 * nt * k), _canaried(engine, nt), _canaried(engine, 16 * k)
    c0, c1 = compare if compare is not None else (N.KD_WALK_ALL, N.KD_WALK_ALL)
    N.check(engine.L.kd_tree_join_batch(engine.ctx, d_data.ptr, d_off.ptr, ntrees, d_tasks.ptr, d_pfx.ptr, d_poff.ptr, nt, k,
                                        c0, c1, outs, d_count.ptr, d_status.ptr, d_tot.ptr, N.KD_MEM_DEVICE),
            "kd_tree_join_batch")
    engine.sync()
    res = []
    for r, (b, sizes) in enumerate(bufs):
        po, mo, oo, pa = (_body(x, s, f"root {r} array {j}") for j, (x, s) in enumerate(zip(b, sizes)))
        res.append((pa, po.view(np.uint64), oo.reshape(-1, 20), mo.view(np.uint32)))
    count = _body(d_count, 4 * nt * k, "count").view(np.uint32).reshape(nt, k)
    status = _body(d_status, nt, "status")
    totals = _body(d_tot, 16 * k, "totals").view(np.uint64).reshape(k, 2)
    return res, count, status, totals


def _same(got, want, k):
    """got (arrays of cap entries) == want (the reference), root by root"""
    (g_outs, g_count, g_status, *g_tot), (w_outs, w_count, w_status) = got, want
    assert np.array_equal(g_status, w_status)
    assert np.array_equal(g_count, w_count)
    for r in range(k):
        wp, wo, wi, wm = w_outs[r]
        gp, go, gi, gm = g_outs[r]
        n, nb = len(wm), len(wp)
        if g_tot:
            assert g_tot[0][r].tolist() == [n, nb]
        assert np.array_equal(go[:n + 1], wo), f"root {r}: path_off"
        assert np.array_equal(gm[:n], wm), f"root {r}: modes"
        assert np.array_equal(gi[:n], wi), f"root {r}: oids"
        assert np.array_equal(gp[:nb], wp), f"root {r}: paths"


def check(engine, trees, tasks, prefixes, k, compare, host=True):
    """the device form with exact capacities and the host form, both against the reference"""
    want = C.join_batch(trees, tasks, prefixes, k, compare)
    data, off = C.arena(trees)
    pfx, pfx_off = C.arena(prefixes)
    caps = [(len(want[0][r][3]), len(want[0][r][0])) for r in range(k)]
    _same(run_device(engine, data, off, tasks, pfx, pfx_off, k, compare, caps), want, k)
    if host:
        _same(engine.tree_join(data, off, np.array(tasks, np.uint32), pfx, pfx_off, k, compare), want, k)
    return want


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
edited, mixed, compares, PREFIXES = C.edited, C.mixed, C.compares, C.PREFIXES


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def _const(path, name):
    text = open(os.path.join(ROOT, "kart_amd", "csrc", path)).read()
    m = re.search(r"constexpr int %s = (\d+);" % name, text)
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def test_seam_constants_are_the_source_s():
    """the sizes the cases below are built around: one task per lane and TJ_NT lanes per workgroup, the
    scan's GF_SPT * 1024 counts per round; the kernels load and store bytes, so there is no load chunk"""
    assert _const("kd_treewalk.hip", "TJ_NT") == 64
    assert _const("kd_treewalk.hip", "TJ_KMAX") == 3
    assert _const("kd_geomfilter.hip", "GF_SPT") == 8
    text = open(os.path.join(ROOT, "kart_amd", "csrc", "kd_treewalk.hip")).read()
    assert "u32x4" not in text and "uint4" not in text  # (no wide access whose chunk would be a seam)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_task_shape_and_compare(engine, k):
    trees, tasks, prefixes = mixed(k)
    for cmp_ in compares(k):
        outs, count, status = check(engine, trees, tasks, prefixes, k, cmp_)
        assert not status.any()
        if cmp_ is None:
            assert count.sum() == sum(len(C.parse(trees[i])[1]) for task in tasks for i in task if i != C.NONE)
        else:
            assert 0 < count.sum() < sum(len(C.parse(trees[i])[1]) for task in tasks for i in task if i != C.NONE)


def test_entry_count_seams(engine):
    rng = np.random.default_rng(2)
    trees, tasks = [], []
    for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
        a = C.rand_tree(rng, n, 1, 20)
        b = edited(rng, a, 0.08)
        trees += [C.mk(a), C.mk(b)]
        tasks.append([len(trees) - 2, len(trees) - 1])
    check(engine, trees, tasks, [b"x"] * len(tasks), 2, (0, 1))
    check(engine, trees, tasks, [b""] * len(tasks), 2, None, host=False)


def test_tree_start_offsets(engine):
    """trees at every start offset mod 16 (fillers between them that no task names), entries of every
    length so that they straddle every 16-byte line"""
    rng = np.random.default_rng(3)
    trees, tasks, at = [], [], 0
    for s in range(32):
        fill = (s - at) % 16 or 16
        trees.append(b"\xee" * fill)
        at += fill
        assert at % 16 == s % 16
        a = [(0o100644, b"n" * ln + b"%02d" % ln, bytes(rng.integers(0, 256, 20, dtype=np.uint8))) for ln in range(1, 18)]
        a.sort(key=lambda e: e[1])
        b = edited(rng, a, 0.3)
        trees += [C.mk(a), C.mk(b)]
        at += len(trees[-2]) + len(trees[-1])
        tasks.append([len(trees) - 2, len(trees) - 1])
    check(engine, trees, tasks, [b"p%d" % t for t in range(len(tasks))], 2, (0, 1))


@pytest.mark.parametrize("nt", [1, 63, 64, 65, 129, 1400])
def test_task_counts(engine, nt):
    """workgroup seams (64 tasks each) and, at 1,400 tasks of three roots, a count array of 8,401 words:
    the scan's second round"""
    rng = np.random.default_rng(nt)
    pool = [C.rand_tree(rng, int(rng.integers(0, 6)), 1, 8) for _ in range(40)]
    trees = [C.mk(p) for p in pool] + [C.mk(edited(rng, p, 0.4)) for p in pool]
    k = 3
    tasks = [[int(rng.integers(0, len(trees))) if rng.random() < 0.85 else C.NONE for _ in range(k)] for _ in range(nt)]
    prefixes = [PREFIXES[int(rng.integers(0, 4))] for _ in range(nt)]
    check(engine, trees, tasks, prefixes, k, (1, 2), host=nt in (1, 65, 1400))


def test_prune_outcomes(engine):
    o1, o2, o3 = C.oid_of(1), C.oid_of(2), C.oid_of(3)
    a = C.mk([(0o100644, b"exec", o1), (0o100644, b"moved-from", o2), (0o100644, b"same", o3), (0o100644, b"third-differs", o1)])
    b = C.mk([(0o100755, b"exec", o1), (0o100644, b"moved-to", o2), (0o100644, b"same", o3), (0o100644, b"third-differs", o1)])
    c = C.mk([(0o100644, b"only-third", o3), (0o100644, b"same", o3), (0o100644, b"third-differs", o2)])
    outs, count, status = check(engine, [a, b, c], [[0, 1, 2]], [b"d"], 3, (0, 1))
    names = [[bytes(p[int(o[i]):int(o[i + 1])]) for i in range(len(m))] for p, o, _, m in outs]
    # mode 100644 vs 100755 with an equal OID: kept; the same OID under two names: both kept; identical in
    # the compared roots: dropped in the third root too, whatever it holds; absent in both: dropped
    assert names == [[b"d/exec", b"d/moved-from"], [b"d/exec", b"d/moved-to"], []]
    assert outs[0][3].tolist() == [0o100644, 0o100644] and outs[1][3].tolist() == [0o100755, 0o100644]
    # OIDs that differ in one byte only, the first or the last: kept
    first, last = bytes([o1[0] ^ 1]) + o1[1:], o1[:19] + bytes([o1[19] ^ 0x80])
    d = C.mk([(0o100644, b"first-byte", o1), (0o100644, b"last-byte", o1), (0o100644, b"same", o1)])
    e = C.mk([(0o100644, b"first-byte", first), (0o100644, b"last-byte", last), (0o100644, b"same", o1)])
    outs, _, _ = check(engine, [d, e], [[0, 1]], [b""], 2, (0, 1))
    assert [o[1].tolist() for o in outs] == [[0, 10, 19]] * 2 and outs[1][2].tobytes() == first + last
    outs, _, _ = check(engine, [a, b, c], [[0, 1, 2]], [b""], 3, (0, 2))
    assert [len(o[3]) for o in outs] == [3, 2, 2]  # `same` agrees in 0 and 2, `moved-to` is in neither: gone from root 1 as well


def test_every_refusal_between_good_tasks(engine):
    rng = np.random.default_rng(4)
    good = [C.rand_tree(rng, 6, 1, 10) for _ in range(3)]
    trees = [C.mk(g) for g in good] + [C.mk(edited(rng, g, 0.5)) for g in good]
    tasks, codes = [], []
    for j, (name, bad, code) in enumerate(C.crafted_invalid()):
        trees.append(bad)
        tasks += [[j % 3, 3 + j % 3], [len(trees) - 1, 3] if j % 2 else [0, len(trees) - 1], [1, 4]]
        codes += [0, code, 0]
    for cmp_ in (None, (0, 1)):
        outs, count, status = check(engine, trees, tasks, [b"r"] * len(tasks), 2, cmp_)
        assert status.tolist() == codes
        assert not count[np.array(codes) != 0].any() and count[np.array(codes) == 0].any(axis=1).all()


def test_tree_index_out_of_range(engine):
    rng = np.random.default_rng(6)
    trees = [C.mk(C.rand_tree(rng, 4, 1, 6)) for _ in range(4)]
    tasks = [[0, 1], [2, 9], [4, 0], [2, 3]]
    want = C.join_batch(trees, [tasks[0], [C.NONE, C.NONE], [C.NONE, C.NONE], tasks[3]], [b"q"] * 4, 2, (0, 1))
    want[2][1] = want[2][2] = N.KD_TJ_ERANGE
    data, off = C.arena(trees)
    pfx, pfx_off = C.arena([b"q"] * 4)
    caps = [(len(want[0][r][3]), len(want[0][r][0])) for r in range(2)]
    _same(run_device(engine, data, off, tasks, pfx, pfx_off, 2, (0, 1), caps), want, 2)
    _same(engine.tree_join(data, off, np.array(tasks, np.uint32), pfx, pfx_off, 2, (0, 1)), want, 2)


def test_arena_offsets_beyond_4g(engine):
    """a sparse arena: real trees below 64 KiB, across 2^32 and above it, a 4 GiB filler nobody names
    between them (HBM that is allocated and never touched)"""
    rng = np.random.default_rng(8)
    real = [C.mk(x) for a in (C.rand_tree(rng, 30, 1, 20) for _ in range(3)) for x in (a, edited(rng, a, 0.2))]
    G = 1 << 32
    place = [100, 100 + len(real[0]) + 3, G - 37, G - 37 + len(real[2]) + 5, G + (1 << 20) + 9, 0]
    place[5] = place[4] + len(real[4])
    total = place[5] + len(real[5])
    off, trees, where, at = [0], [], [], 0
    for j, t in enumerate(real):
        if place[j] > at:
            off.append(place[j])  # a filler
            trees.append(None)
        off.append(place[j] + len(t))
        where.append(len(trees))
        trees.append(t)
        at = place[j] + len(t)
    tasks = [[where[0], where[1]], [where[2], where[3]], [where[4], where[5]]]
    assert off[-1] == total and max(off) > G
    buf = DevBuf(engine, total + 16)
    for j, t in enumerate(real):
        buf.upload(np.frombuffer(t, np.uint8), offset=place[j])
    prefixes = [b"hi/%d" % t for t in range(len(tasks))]
    want = C.join_batch([t if t is not None else b"" for t in trees], tasks, prefixes, 2, (0, 1))
    pfx, pfx_off = C.arena(prefixes)
    caps = [(len(want[0][r][3]), len(want[0][r][0])) for r in range(2)]
    got = run_device(engine, buf, np.array(off, np.uint64), tasks, pfx, pfx_off, 2, (0, 1), caps)
    _same(got, want, 2)
    assert not got[2].any() and got[1].all()


def test_capacity(engine):
    """the device form refuses a task whose ranges pass a capacity and writes nothing of it; the host form
    returns KD_EINVAL"""
    rng = np.random.default_rng(9)
    trees = [C.mk(C.rand_tree(rng, 5, 2, 6)) for _ in range(4)]
    tasks = [[0], [1], [2], [3]]
    want = C.join_batch(trees, tasks, [b""] * 4, 1, None)
    data, off = C.arena(trees)
    pfx, pfx_off = C.arena([b""] * 4)
    n, nb = len(want[0][0][3]), len(want[0][0][0])
    outs, count, status, totals = run_device(engine, data, off, tasks, pfx, pfx_off, 1, None, [(n - 1, nb)])
    assert status.tolist() == [0, 0, 0, N.KD_TJ_ECAP] and totals[0].tolist() == [n, nb]
    assert count[:, 0].tolist() == [5, 5, 5, 0]
    assert np.array_equal(outs[0][3][:15], want[0][0][3][:15]) and np.array_equal(outs[0][1][:16], want[0][0][1][:16])
    out = (N.KdTjOut * 1)()
    po, mo, oo, pa = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32), np.zeros(20 * n, np.uint8), np.full(nb, FILL, np.uint8)
    out[0].cap_n, out[0].cap_bytes = n, nb - 1
    out[0].path_off, out[0].mode, out[0].oid, out[0].path = (x.ctypes.data for x in (po, mo, oo, pa))
    cnt, st = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    tk = np.array(tasks, np.uint32)
    rc = engine.L.kd_tree_join_batch(engine.ctx, N.ptr(data), N.ptr(off), 4, N.ptr(tk), N.ptr(pfx),
                                     N.ptr(pfx_off), 4, 1, -1, -1, out, N.ptr(cnt), N.ptr(st), None, N.KD_MEM_HOST)
    assert rc == N.KD_EINVAL and (pa == FILL).all()


def test_no_tasks_and_bad_arguments(engine):
    outs, count, status = engine.tree_join(np.zeros(0, np.uint8), [0], np.zeros((0, 2), np.uint32), np.zeros(0, np.uint8), [0], 2)
    assert count.shape == (0, 2) and status.size == 0
    assert all(o[1].tolist() == [0] and o[0].size == 0 for o in outs)
    with pytest.raises(N.KdError):
        engine.tree_join(np.zeros(0, np.uint8), [0], np.zeros((0, 2), np.uint32), np.zeros(0, np.uint8), [0], 2, compare=(1, 1))
    with pytest.raises(N.KdError):
        engine.tree_join(np.zeros(0, np.uint8), [0], np.zeros((0, 4), np.uint32), np.zeros(0, np.uint8), [0], 4)
