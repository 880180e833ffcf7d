"""kd_find_renames on crafted arrays: deletes and inserts paired by blob OID on the GPU equal the
reference's two-dict loop (tests/renames_ref.py), through Engine.find_renames (host lists) and the
device-count form (capacity above the count, poison records in the tail)."""
import ctypes

import numpy as np
import pytest

from renames_ref import NONE, renames_ref_arrays

pytestmark = pytest.mark.gpu

CAP_MIN = 1024


def table_cap(n_del):
    """the documented table size: the smallest power of two >= max(1024, 2 * deletes)"""
    c = CAP_MIN
    while c < 2 * n_del:
        c *= 2
    return c


def home_slot(oid, cap):
    """the documented home slot: the little-endian u64 of OID bytes 8..15, masked with cap - 1"""
    return int.from_bytes(bytes(oid[8:16]), "little") & (cap - 1)


def oid_with(tag=None, home=None, tail=None, rng=None):
    """a 20-byte OID with chosen bytes 0..3 (tag), 8..15 (the home-slot word) and 16..19"""
    o = rng.integers(0, 256, 20, dtype=np.uint8) if rng is not None else np.zeros(20, np.uint8)
    if tag is not None:
        o[0:4] = np.frombuffer(int(tag).to_bytes(4, "little"), np.uint8)
    if home is not None:
        o[8:16] = np.frombuffer(int(home).to_bytes(8, "little"), np.uint8)
    if tail is not None:
        o[16:20] = np.frombuffer(int(tail).to_bytes(4, "little"), np.uint8)
    return o


def build(kinds, oids, rng=None):
    """kinds [n] (0 update, 1 delete, 2 insert) and oids [n, 20] (a delta's OID; ignored for updates)
    -> (oid_a, oid_b, delta): every record names an entry of its own on each side it has"""
    kinds = np.asarray(kinds, np.int64)
    oids = np.asarray(oids, np.uint8).reshape(-1, 20)
    n = kinds.shape[0]
    has_a, has_b = kinds != 2, kinds != 1
    delta = np.full((n, 2), NONE, np.uint32)
    delta[has_a, 0] = np.arange(int(has_a.sum()), dtype=np.uint32)
    delta[has_b, 1] = np.arange(int(has_b.sum()), dtype=np.uint32)
    oid_a = np.ascontiguousarray(oids[has_a])
    oid_b = np.ascontiguousarray(oids[has_b])
    upd_b = kinds[has_b] == 0
    oid_b[upd_b] ^= 0x5A  # (an update's two blobs differ)
    return oid_a, oid_b, delta


class Side:
    """what Engine.find_renames reads of a PackedSide"""

    walk_rows = False

    def __init__(self, oid):
        from kart_amd import _native as N

        self.oid = np.ascontiguousarray(oid, np.uint8).reshape(-1, 20)
        self.n = int(self.oid.shape[0])
        self.key = np.arange(self.n, dtype=np.uint64)
        self.key_mode = N.KD_KEY_INT

    def kd_side(self):
        from kart_amd import _native as N

        s = N.KdSide()
        s.n = self.n
        s.key, s.oid = N.ptr(self.key), N.ptr(self.oid)
        s.mem, s.key_mode = N.KD_MEM_HOST, self.key_mode
        return s


def device_form(engine, oid_a, oid_b, delta, orders=None, extra=777):
    """the device-count form: everything in HBM, the list's capacity above the count, the tail
    holding records that would pair (and index far outside the sides) if they were read"""
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    n = int(delta.shape[0])
    cap = n + extra
    full = np.empty((cap, 2), np.uint32)
    full[:n] = delta
    full[n::2] = (0, NONE)
    full[n + 1::2] = (NONE, 0)
    full[cap - 3:] = ((0xFFFFFFF0, NONE), (NONE, 0xFFFFFFF0), (7, 7))
    bufs = [DevBuf.from_numpy(engine, x.reshape(-1) if x.size else np.zeros(20, np.uint8)) for x in (oid_a, oid_b)]
    sides = []
    for o, b in zip((oid_a, oid_b), bufs):
        s = N.KdSide()
        s.n, s.oid, s.mem, s.key_mode = int(o.shape[0]), b.ptr, N.KD_MEM_DEVICE, N.KD_KEY_INT
        sides.append(s)
    d_ord = [None, None]
    if orders is not None:
        d_ord = [DevBuf.from_numpy(engine, np.ascontiguousarray(o, np.uint32) if o.size else np.zeros(1, np.uint32))
                 for o in orders]
    d_delta = DevBuf.from_numpy(engine, full.reshape(-1))
    d_n = DevBuf.from_numpy(engine, np.array([n], np.uint64))
    d_ren, d_k = DevBuf(engine, 8 * (cap // 2 + 1)), DevBuf(engine, 8)
    N.check(engine.L.kd_memset(engine.ctx, d_ren.ptr, 0xEE, d_ren.nbytes), "kd_memset")
    N.check(engine.L.kd_find_renames(engine.ctx, ctypes.byref(sides[0]), ctypes.byref(sides[1]),
                                     d_ord[0].ptr if d_ord[0] else None, d_ord[1].ptr if d_ord[1] else None,
                                     d_delta.ptr, cap, d_n.ptr, N.KD_MEM_DEVICE, d_ren.ptr, d_k.ptr, N.KD_MEM_DEVICE),
            "kd_find_renames")
    k = int(d_k.download(np.uint64, 1)[0])
    assert k <= n // 2
    # nothing is written behind the pairs
    assert (d_ren.download(np.uint8, d_ren.nbytes - 8 * k, offset=8 * k) == 0xEE).all()
    return d_ren.download(np.uint32, 2 * k).reshape(k, 2)


def check(engine, oid_a, oid_b, delta):
    """both forms against the reference loop; returns the pairs"""
    want = renames_ref_arrays(delta, oid_a, oid_b)
    host = engine.find_renames(Side(oid_a), Side(oid_b), delta)
    assert host.dtype == np.uint32 and np.array_equal(host, want)
    dev = device_form(engine, oid_a, oid_b, delta)
    assert np.array_equal(dev, want)
    return want


def random_case(n, seed):
    """n deltas, a third of them updates; the rest drawn from OID groups of 1..5 deletes, of which
    about 30 % also have 1..5 inserts, and insert-only groups; record order shuffled"""
    rng = np.random.default_rng(seed)
    n_upd = n // 3
    kinds, gid = [], []
    g = 0
    left = n - n_upd
    while left > 0:
        r = rng.random()
        md = int(rng.integers(1, 6)) if r < 0.6 else 0
        mi = int(rng.integers(1, 6)) if (r >= 0.6 or rng.random() < 0.3) else 0
        md = min(md, left)
        mi = min(mi, left - md)
        kinds += [1] * md + [2] * mi
        gid += [g] * (md + mi)
        left -= md + mi
        g += 1
    kinds = np.array(kinds + [0] * n_upd, np.int64)
    gid = np.array(gid + list(range(g, g + n_upd)), np.int64)
    pool = rng.integers(0, 256, (g + n_upd, 20), dtype=np.uint8)
    p = rng.permutation(n)
    return build(kinds[p], pool[gid[p]])


@pytest.fixture(scope="module")
def random_12291():
    return random_case(3 * 4096 + 3, 11)


def test_nothing_to_pair(engine):
    rng = np.random.default_rng(1)
    o = rng.integers(0, 256, (50, 20), dtype=np.uint8)
    z = np.zeros((0, 20), np.uint8)
    none = np.zeros((0, 2), np.uint32)
    assert engine.find_renames(Side(z), Side(z), none).shape == (0, 2)
    # the device-count form with a count of 0 over a capacity full of records that would pair
    assert device_form(engine, z, z, none).shape == (0, 2)
    assert device_form(engine, o, o, none).shape == (0, 2)
    assert device_form(engine, o, o, np.array([[0, NONE]], np.uint32)).shape == (0, 2)  # (a count of 1)
    for kind in (2, 1, 0):  # inserts only, deletes only, updates only (the same OIDs throughout)
        a, b, d = build([kind] * 50, o)
        assert check(engine, a, b, d).shape == (0, 2)
    # one delete + one insert with differing OIDs
    a, b, d = build([1, 2], o[:2])
    assert check(engine, a, b, d).shape == (0, 2)


def test_one_pair(engine):
    rng = np.random.default_rng(2)
    o = rng.integers(0, 256, 20, dtype=np.uint8)
    for kinds in ((1, 2), (2, 1)):
        a, b, d = build(kinds, [o, o])
        got = check(engine, a, b, d)
        assert got.tolist() == [[kinds.index(1), kinds.index(2)]]


def test_random_three_blocks(engine, random_12291):
    a, b, d = random_12291
    got = check(engine, a, b, d)
    # (the case is what it says: about 30 % of the deletes have an insert of their OID)
    ins = {b[j].tobytes() for j in d[(d[:, 0] == NONE) & (d[:, 1] != NONE), 1]}
    dels = [a[i].tobytes() for i in d[(d[:, 0] != NONE) & (d[:, 1] == NONE), 0]]
    assert 0.2 < sum(x in ins for x in dels) / len(dels) < 0.4 and got.shape[0] > 300
    assert np.all(np.diff(got[:, 0].astype(np.int64)) > 0)


def test_random_300k(engine):
    a, b, d = random_case(300_000, 12)
    assert check(engine, a, b, d).shape[0] > 5_000


def test_count_scan_second_pass(engine):
    """a list of 4,097 blocks: its 8,194 block counts take the scan kernel's loop past its first 8,192
    (the inserts' prefixes of the last blocks depend on the carry).  Deletes and inserts sit at both
    ends, every record between is an update of entry 0 (the pass never looks at an update's entry), and
    the expected pairs come from the reference loop over the records that are not updates"""
    from renames_ref import renames_ref

    rng = np.random.default_rng(15)
    n, m = 4097 * 4096 - 5, 300
    ends = np.concatenate([np.arange(m), np.arange(n - m, n)])
    kinds = rng.integers(1, 3, 2 * m)
    oids = rng.integers(0, 256, (2 * m, 20), dtype=np.uint8)[rng.integers(0, m, 2 * m)]  # (about half the OIDs recur)
    oid_a, oid_b, small = build(kinds, oids)
    delta = np.zeros((n, 2), np.uint32)
    delta[ends] = small
    want = np.asarray(renames_ref([("delete" if k == 1 else "insert", o.tobytes()) for k, o in zip(kinds, oids)]),
                      np.int64).reshape(-1, 2)
    want = ends[want].astype(np.uint32)
    assert want.shape[0] > 50 and (want[:, 0] > n - m).any() and (want[:, 1] > n - m).any()
    assert np.array_equal(device_form(engine, oid_a, oid_b, delta), want)


def test_one_oid_many_copies(engine):
    o = np.random.default_rng(3).integers(0, 256, 20, dtype=np.uint8)
    kinds = np.array([1, 2] * 3000)
    a, b, d = build(kinds, np.tile(o, (6000, 1)))
    assert check(engine, a, b, d).tolist() == [[5998, 5999]]


def test_same_tag_same_home_slot(engine):
    """64 distinct OIDs equal in bytes 0..15: a tag match alone must not end the probe"""
    rng = np.random.default_rng(4)
    head = rng.integers(0, 256, 16, dtype=np.uint8)
    oids = np.tile(np.concatenate([head, np.zeros(4, np.uint8)]), (64, 1))
    oids[:, 16:] = rng.permutation(1 << 16)[:64].astype("<u4").view(np.uint8).reshape(64, 4)
    assert len({x.tobytes() for x in oids}) == 64
    kinds = np.array([1] * 64 + [2] * 64)
    ins = rng.permutation(64)
    ins[:10] = ins[10:20]  # (some OIDs inserted twice, some never)
    a, b, d = build(kinds, np.concatenate([oids, oids[ins]]))
    got = check(engine, a, b, d)
    assert got.shape[0] == len(set(ins.tolist()))


def test_equal_first_eight_bytes(engine):
    rng = np.random.default_rng(5)
    oids = rng.integers(0, 256, (300, 20), dtype=np.uint8)
    oids[:, :8] = oids[0, :8]
    kinds = np.array([1] * 300 + [2] * 300)
    p = rng.permutation(600)
    a, b, d = build(kinds[p], np.concatenate([oids, oids[rng.permutation(300)]])[p])
    assert check(engine, a, b, d).shape[0] == 300


def test_zero_and_ff_oids(engine):
    rng = np.random.default_rng(6)
    z, f = np.zeros(20, np.uint8), np.full(20, 0xFF, np.uint8)
    x = rng.integers(0, 256, 20, dtype=np.uint8)
    kinds = [1, 1, 2, 0, 2, 1, 2, 2, 1]
    oids = [z, f, f, x, z, x, z, x, z]
    a, b, d = build(kinds, oids)
    assert check(engine, a, b, d).tolist() == [[1, 2], [5, 7], [8, 6]]


def test_probe_chain_wraps(engine):
    """40 distinct OIDs whose home slot is cap - 1 (40 deletes: cap = 1024): all but the first claim
    slots 0, 1, ... past the table's end"""
    rng = np.random.default_rng(7)
    cap = table_cap(40)
    assert cap == 1024
    oids = np.stack([oid_with(home=(cap - 1) | (k << 10), rng=rng) for k in range(40)])
    assert {home_slot(o, cap) for o in oids} == {cap - 1} and len({o.tobytes() for o in oids}) == 40
    kinds = np.array([1] * 40 + [2] * 30)
    a, b, d = build(kinds, np.concatenate([oids, oids[rng.permutation(40)[:30]]]))
    assert check(engine, a, b, d).shape[0] == 30


def test_long_probe_chain(engine):
    """2,000 distinct OIDs sharing one home slot"""
    rng = np.random.default_rng(8)
    cap = table_cap(2000)
    oids = np.stack([oid_with(home=77 | (k << 12), rng=rng) for k in range(2000)])
    assert cap == 4096 and {home_slot(o, cap) for o in oids} == {77}
    kinds = np.array([1] * 2000 + [2] * 2000)
    p = rng.permutation(4000)
    a, b, d = build(kinds[p], np.concatenate([oids, oids[rng.permutation(2000)]])[p])
    assert check(engine, a, b, d).shape[0] == 2000


def test_pair_across_blocks(engine):
    rng = np.random.default_rng(9)
    n = 2 * 4096 + 5
    oids = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    oids[n - 1] = oids[0]
    for first, last in ((1, 2), (2, 1)):
        kinds = np.zeros(n, np.int64)
        kinds[0], kinds[n - 1] = first, last
        a, b, d = build(kinds, oids)
        want = [[0, n - 1]] if first == 1 else [[n - 1, 0]]
        assert check(engine, a, b, d).tolist() == want


def test_permuted_form(engine, random_12291):
    """OIDs in shuffled row order read through base_order / target_order: the materialised form's pairs"""
    a, b, d = random_12291
    want = renames_ref_arrays(d, a, b)
    rng = np.random.default_rng(10)
    rows, orders = [], []
    for o in (a, b):
        p = rng.permutation(o.shape[0])  # row p[i] holds sorted entry i
        w = np.empty_like(o)
        w[p] = o
        rows.append(w)
        orders.append(p.astype(np.uint32))
    assert np.array_equal(device_form(engine, rows[0], rows[1], d, orders=orders), want)


def test_permuted_pipeline(engine):
    """DiffPipeline.renames() after a step, plain and through the sort orders (unsorted=): one answer,
    the reference loop's over the step's own delta list"""
    from kart_amd import synth
    from kart_amd.device import DiffPipeline
    from kart_amd.schema import FieldMaps

    # a tenth of the untouched features re-keyed: one delete + one insert of one OID each
    L, k = synth.renumber_pks(synth.points_layer(20_000, seed=5), 0.1)
    T = L.target
    assert k > 1000
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    rng = np.random.default_rng(13)
    got = []
    for unsorted in (None, (rng.permutation(L.base.n), rng.permutation(T.n))):
        pipe = DiffPipeline(engine, L.base, T, L.base_blobs, L.target_blobs, maps, unsorted=unsorted)
        pipe.step()
        ren = pipe.renames()
        engine.sync()
        counts, delta, *_ = pipe.results()
        want = renames_ref_arrays(delta, L.base.oid, T.oid)
        assert np.array_equal(ren, want) and ren.shape[0] == k
        got.append(ren)
    assert np.array_equal(got[0], got[1])


def test_swapped_columns(engine, random_12291):
    """a reversed diff: sides and columns exchanged pair the same deltas with the roles exchanged"""
    a, b, d = random_12291
    fwd = check(engine, a, b, d)
    rev = check(engine, b, a, np.ascontiguousarray(d[:, ::-1]))
    assert {(int(x), int(y)) for x, y in fwd} == {(int(y), int(x)) for x, y in rev}


def test_deterministic(engine, random_12291):
    a, b, d = random_12291
    r1 = device_form(engine, a, b, d)
    r2 = device_form(engine, a, b, d)
    assert r1.tobytes() == r2.tobytes()
    h1 = engine.find_renames(Side(a), Side(b), d)
    assert h1.tobytes() == r1.tobytes()


@pytest.mark.parametrize("n_delta", [0, 1])
def test_short_list_raw_call(engine, n_delta):
    """kd_find_renames itself with a list of 0 or 1 records (Engine.find_renames answers those without
    calling it): *n_ren = 0 in host memory and in device memory, ren untouched"""
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    o = np.random.default_rng(14).integers(0, 256, (4, 20), dtype=np.uint8)
    sa, sb = Side(o).kd_side(), Side(o).kd_side()
    d = np.array([[0, NONE], [NONE, 0]], np.uint32)  # (the second record would pair with the first)
    ren = np.full((2, 2), 0xEEEEEEEE, np.uint32)
    k = ctypes.c_uint64(99)
    N.check(engine.L.kd_find_renames(engine.ctx, ctypes.byref(sa), ctypes.byref(sb), None, None,
                                     N.ptr(d) if n_delta else None, n_delta, None, N.KD_MEM_HOST, N.ptr(ren),
                                     ctypes.byref(k), N.KD_MEM_HOST), "kd_find_renames")
    assert k.value == 0 and (ren == 0xEEEEEEEE).all()
    # device list and outputs, with and without a device count
    d_delta = DevBuf.from_numpy(engine, d.reshape(-1))
    d_cnt = DevBuf.from_numpy(engine, np.array([n_delta], np.uint64))
    for d_n in (None, d_cnt.ptr):
        d_ren, d_k = DevBuf.from_numpy(engine, ren.reshape(-1)), DevBuf.from_numpy(engine, np.array([99], np.uint64))
        N.check(engine.L.kd_find_renames(engine.ctx, ctypes.byref(sa), ctypes.byref(sb), None, None, d_delta.ptr,
                                         n_delta, d_n, N.KD_MEM_DEVICE, d_ren.ptr, d_k.ptr, N.KD_MEM_DEVICE),
                "kd_find_renames")
        assert int(d_k.download(np.uint64, 1)[0]) == 0
        assert (d_ren.download(np.uint32, 4) == 0xEEEEEEEE).all()


def test_bad_arguments(engine):
    from kart_amd import _native as N

    o = np.zeros((4, 20), np.uint8)
    sa, sb = Side(o).kd_side(), Side(o).kd_side()
    d = np.array([[0, NONE], [NONE, 0]], np.uint32)
    ren = np.zeros((2, 2), np.uint32)
    k = ctypes.c_uint64()
    order = np.arange(4, dtype=np.uint32)
    L = engine.L
    call = lambda *x: L.kd_find_renames(engine.ctx, *x)  # noqa: E731
    assert call(ctypes.byref(sa), ctypes.byref(sb), N.ptr(order), None, N.ptr(d), 2, None, N.KD_MEM_HOST, N.ptr(ren),
                ctypes.byref(k), N.KD_MEM_HOST) == N.KD_EINVAL  # one order without the other
    assert call(ctypes.byref(sa), ctypes.byref(sb), None, None, N.ptr(d), 2**32 - 1, None, N.KD_MEM_HOST, N.ptr(ren),
                ctypes.byref(k), N.KD_MEM_HOST) == N.KD_EINVAL
    assert call(ctypes.byref(sa), ctypes.byref(sb), None, None, None, 2, None, N.KD_MEM_HOST, N.ptr(ren),
                ctypes.byref(k), N.KD_MEM_HOST) == N.KD_EINVAL
    assert call(ctypes.byref(sa), None, None, None, N.ptr(d), 2, None, N.KD_MEM_HOST, N.ptr(ren), ctypes.byref(k),
                N.KD_MEM_HOST) == N.KD_EINVAL
    assert call(ctypes.byref(sa), ctypes.byref(sb), None, None, N.ptr(d), 2, None, N.KD_MEM_HOST, N.ptr(ren), None,
                N.KD_MEM_HOST) == N.KD_EINVAL
