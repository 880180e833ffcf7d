"""-m gpu: the ordered join's update list, which k_place2 derives from the staged delta list (the
join stages no update list of its own): records, both key lists and the pk order built from them
against the oracle and numpy, at the shapes where the derived rank or the placement can go wrong,
and with nothing written beyond the counts (canaries)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

from kart_amd import _native as N

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CANARY = 0xA5
W = 1 << 30  # one pk wrap: the int key orders bucket (pk // 64 mod 2^24) above wrap (pk >> 30)


def _side(pks, rng):
    from kart_amd import packing, walkkey

    keys = np.sort(walkkey.int_keys(np.asarray(pks, np.int64)))
    return packing.PackedSide(keys, rng.integers(0, 256, size=(keys.size, 20), dtype=np.uint8), 0, np.arange(keys.size))


def _sides(pa, pb, equal, seed=5):
    """two int sides as tests/test_gpu_walk.py::_int_side builds them; equal(pks) -> bool per shared pk:
    that pair carries the same OID (no delta); every other shared pk is an update"""
    from kart_amd import walkkey

    rng = np.random.default_rng(seed)
    A, B = _side(pa, rng), _side(pb, rng)
    _, ia, ib = np.intersect1d(A.key, B.key, assume_unique=True, return_indices=True)
    eq = np.asarray(equal(walkkey.int_keys_to_pks(A.key[ia])), bool) if ia.size else np.zeros(0, bool)
    B.oid[ib[eq]] = A.oid[ia[eq]]
    return A, B


def _case(name):
    """(pks of base, pks of target, equal-OID rule)"""
    ar = lambda a, b, s=1: np.arange(a, b, s, dtype=np.int64)
    none, every = (lambda p: np.zeros(p.size, bool)), (lambda p: np.ones(p.size, bool))
    most = lambda p: (p * 2654435761 >> 7) % 10 != 0  # ~10 % updates
    e = np.zeros(0, np.int64)
    if name == "both_empty":
        return e, e, none
    if name == "base_empty":
        return e, ar(0, 3000), none
    if name == "target_empty":
        return ar(-100, 2900), e, none
    if name == "one_equal":
        return ar(77, 78), ar(77, 78), every
    if name == "one_differs":
        return ar(77, 78), ar(77, 78), none
    if name == "tile_1024":  # base.n + target.n = one full tile
        return ar(0, 512), ar(256, 768), most
    if name == "tile_1025":  # a second tile of one item
        return ar(0, 513), ar(256, 768), most
    if name in ("tiles_65", "tiles_129"):  # the placement's 64-tile group boundaries
        n = (int(name[6:]) * 1024 - 100) // 2
        return ar(0, n), ar(n // 2, n // 2 + n), most
    if name == "disjoint":  # every item a delta: 1024 staged records per tile, all 16 chunks, no update
        return ar(0, 8192, 2), ar(1, 8192, 2), none
    if name == "all_updates":  # the derived update rank runs across chunks
        return ar(0, 5000), ar(0, 5000), none
    if name == "identical":  # no delta
        return ar(0, 5000), ar(0, 5000), every
    if name == "leaf_cut":  # 118 items in the first leaf tree: every later tile boundary cuts one, deltas on both sides
        return ar(0, 2000), ar(10, 2000), none
    if name == "interleaved":  # updates and one-sided records mixed inside a wave's 64 records: update rank != delta rank
        a, b = ar(0, 4000), ar(0, 4000)
        return a[a % 3 != 0], b[b % 5 != 0], (lambda p: p % 2 == 0)
    if name == "negative":
        return ar(-70000, -5000, 3), ar(-80000, -20000, 2), most
    if name == "straddle_zero":
        return ar(-3000, 3000), ar(-2500, 3500), most
    if name == "wraps":  # key order (bucket, then wrap) and pk order disagree
        a = np.concatenate([ar(k * W - 300, k * W + 300) for k in (-1, 0, 1)])
        b = np.concatenate([ar(k * W - 200, k * W + 400) for k in (-1, 0, 1)])
        return a, b, (lambda p: p % 3 == 0)
    raise KeyError(name)


CASES = ["both_empty", "base_empty", "target_empty", "one_equal", "one_differs", "tile_1024", "tile_1025", "tiles_65",
         "tiles_129", "disjoint", "all_updates", "identical", "leaf_cut", "interleaved", "negative", "straddle_zero",
         "wraps"]


class _Run:
    """one kd_diff2_device_ex call over canary-filled outputs; every buffer downloaded whole"""

    def __init__(self, engine, A, B, with_upd=True, keys=True, ukeys=True, orders=False):
        from kart_amd.device import DevBuf, DevSide

        L, ctx = engine.L, engine.ctx
        self.dA, self.dB = DevSide(engine, A), DevSide(engine, B)
        sa, sb = self.dA.kd_side(), self.dB.kd_side()
        self.sa, self.sb = sa, sb
        cap = A.n + B.n + 1
        self.cap = cap
        self.buf = {k: DevBuf(engine, 8 * cap) for k in ("delta", "upd", "dkey", "ukey")}
        for b in self.buf.values():
            N.check(L.kd_memset(ctx, b.ptr, CANARY, b.nbytes), "kd_memset")
        self.c = DevBuf(engine, 64)
        self.c.zero()
        oa = ob = None
        if orders:  # identity orders: the late-materialised (PERM) join on the same rows
            oa = DevBuf.from_numpy(engine, np.arange(max(A.n, 1), dtype=np.uint32))
            ob = DevBuf.from_numpy(engine, np.arange(max(B.n, 1), dtype=np.uint32))
        N.check(L.kd_diff2_device_ex(ctx, ctypes.byref(sa), ctypes.byref(sb), oa.ptr if oa else None,
                                     ob.ptr if ob else None, 0, self.buf["delta"].ptr,
                                     self.buf["upd"].ptr if with_upd else None, self.buf["dkey"].ptr if keys else None,
                                     self.buf["ukey"].ptr if keys and ukeys and with_upd else None, self.c.ptr,
                                     self.c.ptr + 32), "kd_diff2_device_ex")
        engine.sync()
        self.counts = self.c.download(np.uint64, 8)
        self.raw = {k: b.download(np.uint8, b.nbytes) for k, b in self.buf.items()}

    def arr(self, name, dtype, n):
        """the first n 8-byte elements, after checking that nothing beyond them was touched"""
        raw = self.raw[name]
        assert (raw[n * 8:] == CANARY).all(), f"{name}: written beyond its {n} elements"
        return raw[: n * 8].view(dtype)


def _record_keys(A, B, rec):
    ka = A.key if A.n else np.zeros(1, np.uint64)
    kb = B.key if B.n else np.zeros(1, np.uint64)
    return np.where(rec[:, 0] != NONE, ka[np.minimum(rec[:, 0], ka.size - 1)], kb[np.minimum(rec[:, 1], kb.size - 1)])


def _check(run, A, B, with_upd=True, keys=True, ukeys=True):
    od, oc = O.classify2(A.key, A.oid, B.key, B.oid)
    cnt = run.counts
    assert cnt[4] == 0
    assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (oc["inserts"], oc["updates"], oc["deletes"])
    nd, nu = int(cnt[3]), int(cnt[1])
    assert np.array_equal(run.arr("delta", np.uint32, nd).reshape(nd, 2), od)
    want_upd = od[(od[:, 0] != NONE) & (od[:, 1] != NONE)]
    assert nu == want_upd.shape[0]
    upd = run.arr("upd", np.uint32, nu if with_upd else 0).reshape(-1, 2)
    if with_upd:
        assert np.array_equal(upd, want_upd)
    assert np.array_equal(run.arr("dkey", np.uint64, nd if keys else 0), _record_keys(A, B, od) if keys else [])
    has_uk = keys and ukeys and with_upd
    assert np.array_equal(run.arr("ukey", np.uint64, nu if has_uk else 0), _record_keys(A, B, want_upd) if has_uk else [])
    return od, want_upd


def _options(engine, request, **opts):
    old = {k: engine.get_option(k) for k in opts}
    request.addfinalizer(lambda: [engine.set_option(k, v) for k, v in old.items()])
    for k, v in opts.items():
        engine.set_option(k, v)


@pytest.mark.parametrize("oid_lds", [False, True], ids=["plain", "oidlds"])
@pytest.mark.parametrize("case", CASES)
def test_gpu_derived_updates_vs_oracle(engine, request, case, oid_lds):
    """records, derived update list, both key lists and the pk order of both lists (kd_delta_pk_order
    over the key lists: a stable argsort of the records' pks), with the join's plain and OIDs-in-LDS
    instantiations; canaries intact"""
    from kart_amd import walkkey
    from kart_amd.device import DevBuf

    A, B = _sides(*_case(case))
    _options(engine, request, j2_oidlds_min=0 if oid_lds else 1 << 26)
    run = _Run(engine, A, B)
    od, upd = _check(run, A, B)
    pks_all = walkkey.int_keys_to_pks(np.concatenate([A.key, B.key]))
    lo, hi = (int(pks_all.min()), int(pks_all.max())) if pks_all.size else (0, 0)
    for rec, name, keyname, slot in ((od, "delta", "dkey", 24), (upd, "upd", "ukey", 8)):
        n = rec.shape[0]
        pk, perm = DevBuf(engine, 8 * run.cap), DevBuf(engine, 4 * run.cap)
        for b in (pk, perm):
            N.check(engine.L.kd_memset(engine.ctx, b.ptr, CANARY, b.nbytes), "kd_memset")
        N.check(engine.L.kd_delta_pk_order(engine.ctx, ctypes.byref(run.sa), ctypes.byref(run.sb), run.buf[name].ptr,
                                           run.buf[keyname].ptr, run.cap, run.c.ptr + slot, lo, hi, pk.ptr, perm.ptr),
                "kd_delta_pk_order")
        engine.sync()
        pks = walkkey.int_keys_to_pks(_record_keys(A, B, rec))
        want = np.argsort(pks, kind="stable")
        got_pk, got_perm = pk.download(np.uint8, pk.nbytes), perm.download(np.uint8, perm.nbytes)
        assert np.array_equal(got_perm[: 4 * n].view(np.uint32), want.astype(np.uint32))
        assert np.array_equal(got_pk[: 8 * n].view(np.int64), pks[want])
        assert (got_perm[4 * n:] == CANARY).all() and (got_pk[8 * n:] == CANARY).all()


@pytest.mark.parametrize("oid_lds", [False, True], ids=["plain", "oidlds"])
@pytest.mark.parametrize("form", ["no_upd", "no_keys", "delta_keys_only"])
def test_gpu_derived_updates_optional_outputs(engine, request, form, oid_lds):
    """d_upd == NULL, no key lists, delta keys without update keys: what is asked for is right, and
    nothing is written through an absent list"""
    A, B = _sides(*_case("interleaved"))
    _options(engine, request, j2_oidlds_min=0 if oid_lds else 1 << 26)
    kw = {"no_upd": dict(with_upd=False), "no_keys": dict(keys=False), "delta_keys_only": dict(ukeys=False)}[form]
    _check(_Run(engine, A, B, **kw), A, B, **kw)


def test_gpu_derived_updates_through_orders(engine):
    """the late-materialised join (OIDs read through the sides' orders) stages and places the same way"""
    A, B = _sides(*_case("tiles_65"))
    _check(_Run(engine, A, B, orders=True), A, B)


@pytest.mark.parametrize("layer", ["points", "polygons"])
def test_gpu_derived_updates_pipeline(engine, layer):
    """DiffPipeline for three steps: records, field diff and both pk orders against the oracle"""
    from kart_amd import synth, walkkey
    from kart_amd.device import DiffPipeline
    from kart_amd.schema import FieldMaps

    L = synth.points_layer(20_000, seed=41) if layer == "points" else synth.polygons_layer(20_000, seed=42)
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    pipe = DiffPipeline(engine, L.base, L.target, L.base_blobs, L.target_blobs, maps)
    assert pipe.pk_order
    for _ in range(3):
        pipe.step()
    engine.sync()
    counts, delta, upd, masks, status = pipe.results()
    od, oc = O.classify2(L.base.key, L.base.oid, L.target.key, L.target.oid)
    assert np.array_equal(delta, od)
    assert np.array_equal(upd, od[(od[:, 0] != NONE) & (od[:, 1] != NONE)])
    om, ost = O.fielddiff(*L.base_blobs, *L.target_blobs, upd, maps)
    assert np.array_equal(masks, om) and np.array_equal(status, ost)
    d_pk, d_perm, u_pk, u_perm = pipe.pk_results()
    for rec, pk_out, perm_out in ((delta, d_pk, d_perm), (upd, u_pk, u_perm)):
        pks = walkkey.int_keys_to_pks(_record_keys(L.base, L.target, rec))
        want = np.argsort(pks, kind="stable")
        assert np.array_equal(perm_out, want.astype(np.uint32)) and np.array_equal(pk_out, pks[want])
