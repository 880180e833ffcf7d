"""-m gpu: the walk-order path — joins straight on the sides as the tree walk lists them, the deltas
radix-sorted into pk order (kd_delta_pk_order), the hash sides' per-bucket sort
(kd_sort_segmented_into) and the late-materialised three-way merge — against numpy, the oracle and the
reference's own sorted_items order (tests/golden)."""
import ctypes
import os
import re

import numpy as np
import pytest

from fixtures import DIFF_FIXTURES, load, pk_of
from oracle import oracle as O

from kart_amd import _native as N

pytestmark = pytest.mark.gpu


def _int_side(pks, rng):
    from kart_amd import packing, walkkey

    keys = np.sort(walkkey.int_keys(np.asarray(pks, np.int64)))
    return packing.PackedSide(keys, rng.integers(0, 256, size=(keys.size, 20), dtype=np.uint8), 0, np.arange(keys.size))


@pytest.mark.parametrize("case", ["small", "neg", "wide", "one", "empty_base", "dense", "spread", "range_1e9"])
def test_gpu_delta_pk_order_vs_numpy(engine, case):
    """records of two int sides -> pks ascending + record index: any pk range (a few bits, the whole
    signed 64-bit range: 64-bit compact keys, 8 passes), a single pk, an empty side"""
    from kart_amd import walkkey

    rng = np.random.default_rng(len(case))
    if case == "small":
        pa, pb = np.arange(0, 3000), np.arange(1500, 4000)
    elif case == "neg":
        pa, pb = np.arange(-70000, 5000, 3), np.arange(-80000, -20000, 2)
    elif case == "wide":
        u = np.unique(rng.integers(-2**63, 2**63 - 1, 60000, dtype=np.int64))
        pa, pb = u[:40000], u[20000:]
    elif case == "one":
        pa, pb = np.array([77]), np.array([77])
    elif case == "empty_base":
        pa, pb = np.zeros(0, np.int64), np.arange(5, 50000)
    elif case == "spread":  # bitmap path, hundreds of scan chunks (the one-round-trip tail scan)
        u = np.unique(rng.integers(0, 200_000_000, 1_200_000, dtype=np.int64))
        pa, pb = u[: 2 * u.size // 3], u[u.size // 3:]
    elif case == "range_1e9":  # bitmap path, 5,723 scan chunks: still one trip of the chunk totals' scan (8,192 chunks;
        # its second trip is test_order_crafted.py's test_gpu_bitmap_two_trips)
        u = np.unique(rng.integers(0, 1_500_000_000, 600_000, dtype=np.int64))
        pa, pb = u[: 2 * u.size // 3], u[u.size // 3:]
    else:
        pa, pb = np.arange(0, 2_000_000), np.arange(1_000_000, 3_000_000)
    A, B = _int_side(pa, rng), _int_side(pb, rng)
    if case == "one":
        B.oid[0] ^= 1
    ka, kb = A.key, B.key
    # the union as classify2 would list it (key order), every pair a record
    allk = np.union1d(ka, kb)
    ia = np.searchsorted(ka, allk)
    ib = np.searchsorted(kb, allk)
    has_a = (ia < ka.size) & (ka[np.minimum(ia, max(ka.size - 1, 0))] == allk) if ka.size else np.zeros(allk.size, bool)
    has_b = (ib < kb.size) & (kb[np.minimum(ib, max(kb.size - 1, 0))] == allk) if kb.size else np.zeros(allk.size, bool)
    rec = np.stack([np.where(has_a, ia, 0xFFFFFFFF), np.where(has_b, ib, 0xFFFFFFFF)], 1).astype(np.uint32)
    pk, perm = engine.delta_pk_order(A, B, rec)
    pks = walkkey.int_keys_to_pks(allk)
    want = np.argsort(pks, kind="stable")
    assert np.array_equal(perm, want.astype(np.uint32)) and np.array_equal(pk, pks[want])


@pytest.mark.parametrize("name", [n for n in DIFF_FIXTURES])
def test_gpu_pk_order_equals_reference_sorted_items(engine, name):
    """The reference's own DeltaDiff.sorted_items order (the golden delta lists were written in it) ==
    classify2's deltas put in pk order on the GPU, for every int-PK diff of the reference repos"""
    from checks import delta_set, golden_set  # noqa: F401

    fx = load(name)
    for case in fx.cases("diff2"):
        A, B = fx.packed(case["base"]), fx.packed(case["target"])
        if A.key_mode != 0 or not case["deltas"]:
            continue
        r = engine.diff2(A, B)
        pk, perm = engine.delta_pk_order(A, B, r.delta)
        got = []
        for p, i in zip(pk.tolist(), perm.tolist()):
            a, b = r.delta[i]
            got.append(("insert" if a == 0xFFFFFFFF else "delete" if b == 0xFFFFFFFF else "update", p))
        want = [(d["type"], pk_of(d["old_pk"]) if d["old_pk"] is not None else pk_of(d["new_pk"])) for d in case["deltas"]]
        assert got == want, (name, case["base"], case["target"])


def _seg_sort(engine, keys, seg_bits=24, max_seg=0):
    from kart_amd.device import DevBuf

    n = keys.size
    dk = DevBuf.from_numpy(engine, keys if n else np.zeros(1, np.uint64))
    ko, order, err = DevBuf(engine, 8 * max(n, 1)), DevBuf(engine, 4 * max(n, 1)), DevBuf(engine, 8)
    err.zero()
    N.check(engine.L.kd_sort_segmented_into(engine.ctx, dk.ptr, ko.ptr, order.ptr, n, seg_bits, max_seg, err.ptr),
            "kd_sort_segmented_into")
    return ko.download(np.uint64, n), order.download(np.uint32, n), int(err.download(np.uint32, 1)[0])


@pytest.mark.parametrize("n", [1, 2, 1000, 400_000, 3_000_000])
def test_gpu_segmented_sort_c4_walk_order(engine, n):
    """the C4 string-PK sides in git tree order: buckets ascend, entries inside a bucket in filename
    order; the per-bucket sort equals a full stable argsort of the keys"""
    from kart_amd import synth

    from kart_amd import packing

    M = synth.table3_layers(max(n, 10), seed=3, walk=True)
    for S in (M.ancestor, M.ours, M.theirs):
        keys = S.key[:n]
        ref = np.argsort(keys, kind="stable")
        # the full halo, and the small one the host's scan allows (seg_max <= 128)
        for max_seg in (0, packing.keys_scan(keys, S.key_mode).seg_max):
            k, order, err = _seg_sort(engine, keys, max_seg=max_seg)
            assert err == 0
            assert np.array_equal(order, ref.astype(np.uint32)) and np.array_equal(k, keys[ref])


@pytest.mark.parametrize("run", [60, 200, 500])
def test_gpu_segmented_sort_long_runs(engine, run):
    """runs of 60 / 200 / 500 entries crossing tile boundaries: exact with the full halo; with a
    hint of 128 a longer run that crosses a tile edge is flagged (err 4), never mis-sorted"""
    rng = np.random.default_rng(run)
    nb = 40_000 // run
    b = np.repeat(np.arange(nb, dtype=np.uint64), run)
    keys = (b << np.uint64(40)) | rng.permutation(b.size).astype(np.uint64)
    ref = np.argsort(keys, kind="stable")
    k, order, err = _seg_sort(engine, keys, max_seg=0)
    assert err == 0 and np.array_equal(order, ref.astype(np.uint32)) and np.array_equal(k, keys[ref])
    k, order, err = _seg_sort(engine, keys, max_seg=128)
    if run <= 128:
        assert err == 0 and np.array_equal(order, ref.astype(np.uint32))
    else:
        assert err & 4


def test_gpu_segmented_sort_flags(engine):
    """duplicate keys and descending bucket bits set err 1; a bucket of more than 512 entries err 4"""
    rng = np.random.default_rng(5)
    base = np.sort(rng.integers(0, 2**63, 5000, dtype=np.uint64))
    dup = base.copy()
    dup[100] = dup[101]
    assert _seg_sort(engine, dup)[2] & 1
    desc = base.copy()
    desc[10], desc[4000] = desc[4000], desc[10]
    assert _seg_sort(engine, desc, seg_bits=24)[2] & 1
    big = (np.uint64(7) << np.uint64(40)) | rng.permutation(2000).astype(np.uint64)
    assert _seg_sort(engine, big)[2] & 4
    ok = (np.uint64(7) << np.uint64(40)) | rng.permutation(500).astype(np.uint64)
    k, order, err = _seg_sort(engine, ok)
    assert err == 0 and np.array_equal(k, np.sort(ok))


@pytest.mark.parametrize("n", [1000, 400_000, pytest.param(50_000_000, marks=pytest.mark.timeout(900))])
def test_gpu_merge3_segmented_c4_walk_order(engine, n):
    """C4 from the sides as the tree walk lists them: three per-bucket sorts, then the three-way merge
    reading OIDs and filenames through the orders (kd_merge3_device_perm) — conflicts and merge deltas
    bit-exact with the oracle on the key-sorted sides; 50M rows = C4 at its stated size"""
    from kart_amd import packing, synth
    from kart_amd.device import MergePipeline

    M = synth.table3_layers(n, seed=n, walk=True)
    pipe = MergePipeline(engine, M.ancestor, M.ours, M.theirs, segmented=True)
    for _ in range(2):
        pipe.step()
    engine.sync()
    n_clean, conf, md = pipe.results()
    srt = []
    for S, order in zip((M.ancestor, M.ours, M.theirs), pipe.orders()):
        ref = np.argsort(S.key, kind="stable")
        assert np.array_equal(order, ref.astype(np.uint32))
        srt.append((S.key[ref], S.oid[ref]))
    oc, om, ocl = O.classify3(*srt[0], *srt[1], *srt[2])
    assert np.array_equal(conf, oc.reshape(-1, 3)) and np.array_equal(md, om.reshape(-1, 2)) and n_clean == ocl
    assert conf.shape[0] == M.n_conflict
    del packing


@pytest.mark.parametrize("n,flags", [(1000, 0), (300_000, 0), (300_000, 1), (2_000_000, 0)])
def test_gpu_diff2_ex_record_keys(engine, n, flags):
    """kd_diff2_device_ex writes every delta's and update's join key beside it (the key the pk order
    reads): equal to the side key the record points at, in both compaction modes"""
    from kart_amd import synth
    from kart_amd.device import DevBuf, DevSide

    L = synth.points_layer(n, seed=31)
    A, B = DevSide(engine, L.base), DevSide(engine, L.target)
    sa, sb = A.kd_side(), B.kd_side()
    cap = L.base.n + L.target.n + 1
    d, u, dk, uk, c = (DevBuf(engine, 8 * cap) for _ in range(5))
    c.zero()
    N.check(engine.L.kd_diff2_device_ex(engine.ctx, ctypes.byref(sa), ctypes.byref(sb), None, None, flags, d.ptr, u.ptr,
                                        dk.ptr, uk.ptr, c.ptr, c.ptr + 32), "kd_diff2_device_ex")
    cnt = c.download(np.uint64, 8)
    assert cnt[4] == 0
    nd, nu = int(cnt[3]), int(cnt[1])
    for rec, keys, m in ((d, dk, nd), (u, uk, nu)):
        r = rec.download(np.uint32, 2 * m).reshape(m, 2)
        k = keys.download(np.uint64, m)
        want = np.where(r[:, 0] != 0xFFFFFFFF, L.base.key[np.minimum(r[:, 0], L.base.n - 1)],
                        L.target.key[np.minimum(r[:, 1], L.target.n - 1)])
        assert np.array_equal(k, want)


@pytest.mark.parametrize("flags", [0, 1])
def test_gpu_diff2_ex_delta_keys_only(engine, flags):
    """each key list is optional on its own: delta keys with the update list but no update
    keys writes the delta keys and leaves the update list correct (no store through the NULL list)"""
    from kart_amd import synth
    from kart_amd.device import DevBuf, DevSide

    L = synth.points_layer(300_000, seed=32)
    A, B = DevSide(engine, L.base), DevSide(engine, L.target)
    sa, sb = A.kd_side(), B.kd_side()
    cap = L.base.n + L.target.n + 1
    d, u, dk, c = (DevBuf(engine, 8 * cap) for _ in range(4))
    c.zero()
    N.check(engine.L.kd_diff2_device_ex(engine.ctx, ctypes.byref(sa), ctypes.byref(sb), None, None, flags, d.ptr, u.ptr,
                                        dk.ptr, None, c.ptr, c.ptr + 32), "kd_diff2_device_ex")
    cnt = c.download(np.uint64, 8)
    assert cnt[4] == 0
    nd, nu = int(cnt[3]), int(cnt[1])
    od, oc = O.classify2(L.base.key, L.base.oid, L.target.key, L.target.oid)
    r = d.download(np.uint32, 2 * nd).reshape(nd, 2)
    ru = u.download(np.uint32, 2 * nu).reshape(nu, 2)
    key = lambda x: sorted(map(tuple, x.tolist()))
    assert key(r) == key(od) and nu == oc["updates"]
    k = dk.download(np.uint64, nd)
    want = np.where(r[:, 0] != 0xFFFFFFFF, L.base.key[np.minimum(r[:, 0], L.base.n - 1)],
                    L.target.key[np.minimum(r[:, 1], L.target.n - 1)])
    assert np.array_equal(k, want)
    assert set(map(tuple, ru.tolist())) <= set(map(tuple, r.tolist()))


# the A/B switches of kartdiff.h's option table that change which join kernel runs:
# every one bit-exact with the oracle on the C4 layer (sorted and walk-order forms) and, for the
# two-way join's OID staging, on the C3 polygon layer
OPTION_SETS = {
    "two_step": {"merge3_join": 0},             # classify2 + k_resolve3
    "oidlds": {"j2_oidlds_min": 0},             # k_join2 stages OIDs in LDS at every size
}
OPTION_DEFAULTS = {"merge3_join": 1, "j2_oidlds_min": 1 << 26}


@pytest.mark.parametrize("opts", sorted(OPTION_SETS))
def test_gpu_option_paths_vs_oracle(engine, request, opts):
    from kart_amd import synth
    from kart_amd.device import DiffPipeline, MergePipeline
    from kart_amd.schema import FieldMaps

    for k, v in OPTION_SETS[opts].items():
        engine.set_option(k, v)
    request.addfinalizer(lambda: [engine.set_option(k, OPTION_DEFAULTS[k]) for k in OPTION_SETS[opts]])
    key = lambda rows: sorted(map(tuple, np.asarray(rows).tolist()))
    # three-way: the sorted form, then the walk-order form (per-bucket sorts, OIDs / names through the orders)
    M = synth.table3_layers(300_000, seed=31)
    oc, om, ocl = O.classify3(M.ancestor.key, M.ancestor.oid, M.ours.key, M.ours.oid, M.theirs.key, M.theirs.oid)
    pipe = MergePipeline(engine, M.ancestor, M.ours, M.theirs)
    pipe.step()
    engine.sync()
    n_clean, conf, md = pipe.results()
    assert key(conf) == key(oc) and key(md) == key(om) and n_clean == ocl
    W = synth.table3_layers(300_000, seed=32, walk=True)
    wp = MergePipeline(engine, W.ancestor, W.ours, W.theirs, segmented=True)
    wp.step()
    engine.sync()
    n_clean, conf, md = wp.results()
    srt = []
    for S, order in zip((W.ancestor, W.ours, W.theirs), wp.orders()):
        srt.append((S.key[order], S.oid[order]))
    oc, om, ocl = O.classify3(*srt[0], *srt[1], *srt[2])
    assert key(conf) == key(oc) and key(md) == key(om) and n_clean == ocl
    # two-way on the polygon layer
    L = synth.polygons_layer(1_000_000, seed=33)
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    dp = DiffPipeline(engine, L.base, L.target, L.base_blobs, L.target_blobs, maps)
    dp.step()
    engine.sync()
    counts, delta, upd, masks, status = dp.results()
    od, _ = O.classify2(L.base.key, L.base.oid, L.target.key, L.target.oid)
    assert np.array_equal(delta, od)
    om2, ost = O.fielddiff(*L.base_blobs, *L.target_blobs, upd, maps)
    assert np.array_equal(masks, om2) and np.array_equal(status, ost)


def _header_options():
    """(name, KD_* variable) of every `name [KD_NAME]` line of kartdiff.h's comment on kd_set_option"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "kartdiff.h")).read()
    comment = text[text.index("/* Tuning options of a context"):text.index("int kd_set_option(")]
    return re.findall(r"^ \*\s+(\w+)\s+\[(KD_\w+)\]", comment, re.M)


def _declared_defaults():
    """the default kd_opts declares for each of its fields (kd_internal.h)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "kart_amd", "csrc", "kd_internal.h")).read()
    body = re.search(r"^struct kd_opts \{\n(.*?)^\};", text, re.M | re.S).group(1)
    out = {}
    for name, value in re.findall(r"^\s*(?:int|int64_t|uint64_t)\s+(\w+)\s*=\s*([^;]+);", body, re.M):
        assert re.fullmatch(r"[-\d\s<ul]+", value), value  # integer literals and shifts only
        out[name] = eval(re.sub(r"(\d)(?:ull|ul|u|ll)\b", r"\1", value))
    return out


def test_gpu_option_table_matches_header(monkeypatch):
    """the option comment of kartdiff.h, kd_opts and the library's option table name the same options
    with the same defaults, and a retired or unknown option is KD_EINVAL"""
    from kart_amd.engine import Engine

    listed = _header_options()
    defaults = _declared_defaults()
    assert len(listed) >= 10 and len({n for n, _ in listed}) == len(listed)
    for name, env in listed:
        assert env == "KD_" + name.upper()
        monkeypatch.delenv(env, raising=False)  # kd_init would seed the option from it
    with Engine(0) as eng:  # a fresh context: nothing has set an option on it
        for name, _ in listed:
            assert eng.get_option(name) == defaults[name], name
        for name in ("merge3_split", "j3_ol", "j3_v", "j2r", "no_such_option"):
            with pytest.raises(N.KdError) as e:
                eng.set_option(name, 1)
            assert e.value.code == N.KD_EINVAL, name
            with pytest.raises(N.KdError) as e:
                eng.get_option(name)
            assert e.value.code == N.KD_EINVAL, name
