"""-m gpu: what runs in front of kd_diff2_step's field diff.

Partition: k_partition2's two-level guided search on sides whose splits lie far from the
proportional guess (blocks of one-sided keys, disjoint sides, an empty or one-entry side), at every
size where its shape changes (1024-item tiles, 32-tile groups) — records, derived updates, counts
and both key lists against the oracle.  (A coarse table of true splits for the top-level guess was
measured and is not in the tree; these are the cases it had to pass.)

Count (``step_count``): the field diff of update-order arenas queued directly behind the join, its
update count the sum of the join's partial counters (tile t adds to counter t % 64), k_gscan2 on the
side stream in its one-wave form — every output of the step bit for bit against the separate calls."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

from oracle import oracle as O

from kart_amd import _native as N
from test_gpu_join2_walk import S, TILE, _mk
from test_gpu_place2_updates import _Run, _check, _options

pytestmark = pytest.mark.gpu

G = 32 * TILE  # entries of both sides in one k_partition2 group
NONE = 0xFFFFFFFF
SLOTS = 64     # partial update counters
CANARY = 0xA5

SIZES = {
    "one_tile": 1000,
    "one_group": G,
    "one_group_plus_1": G + 1,      # 2 groups, the second a one-entry tile
    "three_groups": 2 * G + 5,
    "four_groups": 4 * G,           # a multiple of the group size
    "five_groups": 4 * G + 1,       # the last group a one-entry tile
    "eleven_ragged": 10 * G + 20123,
}
PART_CASES = ["inserts_behind", "deletes_front", "both_blocks", "a_below_b", "b_below_a", "identical", "a_empty",
              "b_empty", "a_single", "b_single"]


def _part_keys(case, n):
    """(base keys, target keys) with n entries together (identical sides: n rounded up to even)"""
    ar = lambda a, b: S * np.arange(a, b, dtype=np.int64)
    if case in ("inserts_behind", "deletes_front"):  # one block of one-sided keys beyond every shared key
        a = (n - n // 5) // 2
        k = n - 2 * a
        if case == "inserts_behind":
            return ar(0, a), np.concatenate([ar(0, a), S * a + np.arange(k)])
        return np.concatenate([np.arange(k), k + ar(1, a + 1)]), k + ar(1, a + 1)
    if case == "both_blocks":  # deletes in front and inserts behind: the drift turns twice
        dels = n // 6
        a = (n - dels - n // 5) // 2
        ins = n - dels - 2 * a
        shared = dels + ar(1, a + 1)
        return np.concatenate([np.arange(dels), shared]), np.concatenate([shared, shared[-1] + 1 + np.arange(ins)])
    if case in ("a_below_b", "b_below_a"):
        lo, hi = ar(0, n // 2), ar(n // 2, n)
        return (lo, hi) if case == "a_below_b" else (hi, lo)
    if case == "identical":
        return ar(0, (n + 1) // 2), ar(0, (n + 1) // 2)
    if case in ("a_empty", "b_empty"):
        e, full = np.zeros(0, np.int64), ar(0, n)
        return (e, full) if case == "a_empty" else (full, e)
    if case in ("a_single", "b_single"):  # one entry, a key the other side does not hold, in its middle
        one, full = np.array([S * (n // 2) + 5], np.int64), ar(0, n - 1)
        return (one, full) if case == "a_single" else (full, one)
    raise KeyError(case)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", PART_CASES)
def test_gpu_partition_guess_vs_oracle(engine, request, case, size):
    ka, kb = _part_keys(case, SIZES[size])
    assert ka.size + kb.size in (SIZES[size], SIZES[size] + 1)
    A, B = _mk(ka, kb)
    _check(_Run(engine, A, B), A, B)  # (asserts the error flag is 0)


def test_gpu_partition_single_matching_entry(engine, request):
    """a one-entry side whose key the other side holds"""
    ka, kb = np.array([S * 70000], np.int64), S * np.arange(0, 4 * G, dtype=np.int64)
    for A, B in (_mk(ka, kb), _mk(kb, ka)):
        _check(_Run(engine, A, B), A, B)


def test_gpu_partition_three_way_unchanged(engine, request):
    """the three-way join's launch of k_partition2 (30k-row sides: 5 groups of its 384-item tiles), with deletes in
    front on one side and inserts behind on the other, against the oracle"""
    from kart_amd import packing

    rng = np.random.default_rng(17)
    m, k = 30000, 6000
    keys = np.concatenate([1 + np.arange(k), S * np.arange(1, m + 1), S * (m + 1) + np.arange(k)]).astype(np.uint64)
    oids = rng.integers(0, 256, size=(keys.size, 20), dtype=np.uint8)
    front, back = np.arange(keys.size) < k, np.arange(keys.size) >= k + m

    def side(sel, oid):
        return packing.PackedSide(keys[sel], np.ascontiguousarray(oid[sel]), 0, np.arange(int(sel.sum())))

    oO = oids.copy(); oO[rng.random(keys.size) < 0.1, 0] ^= 1
    oT = oids.copy(); oT[rng.random(keys.size) < 0.1, 1] ^= 1
    A = side(~back & (rng.random(keys.size) > 0.05), oids)
    O_ = side(~front & ~back & (rng.random(keys.size) > 0.05), oO)   # ours: the front block deleted
    T = side(~front & (rng.random(keys.size) > 0.05), oT)            # theirs: that too, and the back block inserted
    oc, om, ocl = O.classify3(A.key, A.oid, O_.key, O_.oid, T.key, T.oid)
    assert oc.size and om.size
    r3 = engine.merge3(A, O_, T)
    assert np.array_equal(np.asarray(r3.conflict).reshape(-1, 3), oc.reshape(-1, 3))
    assert np.array_equal(np.asarray(r3.mdelta).reshape(-1, 2), om.reshape(-1, 2)) and r3.n_clean == ocl


# ---- the update count from the join -------------------------------------------------------------

COUNT_SIDES = ["no_update", "no_delta", "one_update_last_tile", "many_tiles", "one_slot"]


@functools.lru_cache(maxsize=None)
def _layer(inserts=True):
    """72k points, 5 % updates: 140 join tiles, updates in every one of them (the inserts fill the last tiles:
    without them the last tile holds updates too)"""
    from kart_amd import synth
    from kart_amd.schema import FieldMaps

    L = synth.points_layer(72_000, frac_update=0.05, frac_insert=0.01 if inserts else 0.0, seed=23)
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    od, _ = O.classify2(L.base.key, L.base.oid, L.target.key, L.target.oid)
    upd = od[(od[:, 0] != NONE) & (od[:, 1] != NONE)].astype(np.int64)
    pos = upd[:, 0] + upd[:, 1]  # the pair's items are union items pos and pos + 1
    whole = pos % TILE != TILE - 1  # (both in one tile)
    return L, maps, upd, pos // TILE, whole


@functools.lru_cache(maxsize=None)
def _sides(name):
    """(base, target, base blobs, target blobs, maps, update list): the layer with the updates outside `keep`
    undone (the target entry takes the base's OID, so the join no longer lists it)"""
    L, maps, upd, tile, whole = _layer(name != "one_update_last_tile")
    ntiles = (L.base.n + L.target.n + TILE - 1) // TILE
    assert ntiles > 2 * SLOTS + 5 and np.unique(tile).size > SLOTS
    if name == "no_delta":
        return L.base, L.base, L.base_blobs, L.base_blobs, maps, upd[:0]
    if name == "many_tiles":
        keep = np.ones(upd.shape[0], bool)
    elif name == "no_update":
        keep = np.zeros(upd.shape[0], bool)
    elif name == "one_update_last_tile":
        keep = np.zeros(upd.shape[0], bool)
        keep[np.flatnonzero(whole & (tile == ntiles - 1))[-1]] = True
    elif name == "one_slot":  # tiles 5, 69 and 133: counter 5 alone
        keep = whole & (tile % SLOTS == 5)
        assert np.unique(tile[keep]).size == 3
    elif name == "first_half":  # (a prefix of many_tiles' updates: the same arena indices)
        keep = np.arange(upd.shape[0]) < upd.shape[0] // 2
    else:
        raise KeyError(name)
    oid = L.target.oid.copy()
    oid[upd[~keep, 1]] = L.base.oid[upd[~keep, 0]]
    return L.base, dataclasses.replace(L.target, oid=oid), L.base_blobs, L.target_blobs, maps, upd[keep]


@functools.lru_cache(maxsize=None)
def _big_maps():
    """the layer's maps with 320 more legends that no blob names (fd_craft.bulk_legends): packed tables
    above the 16 KiB the windowed kernels hold in LDS, so the field diff is k_fielddiff_g"""
    import fd_craft as F
    from kart_amd.schema import FieldMaps

    L = _layer()[0]
    legends = {**L.legends, **F.bulk_legends()}
    return FieldMaps(L.schema, legends, L.schema, legends)


def _pipeline(engine, name, arenas=True, big=False):
    from kart_amd.device import DiffPipeline

    base, target, bb, tb, maps, upd = _sides(name)
    pipe = DiffPipeline(engine, base, target, bb, tb, _big_maps() if big else maps)
    assert pipe.pk_order
    if arenas:  # update i's blobs at arena index i
        pipe.use_update_arenas(upd)
    for b in (pipe.delta, pipe.upd, pipe.masks, pipe.status, pipe.d_pk, pipe.d_perm, pipe.dkey, pipe.ukey, pipe.u_pk,
              pipe.u_perm):
        N.check(engine.L.kd_memset(engine.ctx, b.ptr, CANARY, b.nbytes), "kd_memset")
    return pipe


def _separate_calls(pipe, arenas):
    """the step as separate entry points on the pipeline's buffers (no sync)"""
    L, ctx = pipe.eng.L, pipe.eng.ctx
    c = pipe.counts.ptr
    N.check(L.kd_diff2_device_ex(ctx, ctypes.byref(pipe._sa), ctypes.byref(pipe._sb), None, None, 0, pipe.delta.ptr,
                                 pipe.upd.ptr, pipe.dkey.ptr, pipe.ukey.ptr, c, c + 32), "kd_diff2_device_ex")
    ob, nb = (pipe._ob_u, pipe._nb_u) if arenas else (pipe._ob, pipe._nb)
    N.check(L.kd_fielddiff(ctx, ctypes.byref(ob), ctypes.byref(nb), None if arenas else pipe.upd.ptr, pipe.cap_upd,
                           ctypes.cast(c + 8, N.c_u64p), N.KD_MEM_DEVICE, ctypes.byref(pipe._km), pipe.masks.ptr,
                           pipe.status.ptr, N.KD_MEM_DEVICE), "kd_fielddiff")
    lo, hi = pipe.pk_range
    N.check(L.kd_delta_pk_order(ctx, ctypes.byref(pipe._sa), ctypes.byref(pipe._sb), pipe.delta.ptr, pipe.dkey.ptr,
                                pipe.cap, c + 24, lo, hi, pipe.d_pk.ptr, pipe.d_perm.ptr), "kd_delta_pk_order")
    N.check(L.kd_delta_pk_order(ctx, ctypes.byref(pipe._sa), ctypes.byref(pipe._sb), pipe.upd.ptr, pipe.ukey.ptr,
                                pipe.cap_upd, c + 8, lo, hi, pipe.u_pk.ptr, pipe.u_perm.ptr), "kd_delta_pk_order")


def _download(pipe):
    """(after a sync) counts and error word; every list up to its count; masks and status whole"""
    c = pipe.counts.download(np.uint64, 8)
    nd, nu = int(c[3]), int(c[1])
    out = {"counts": c,
           "delta": pipe.delta.download(np.uint32, 2 * nd), "dkey": pipe.dkey.download(np.uint64, nd),
           "upd": pipe.upd.download(np.uint32, 2 * nu), "ukey": pipe.ukey.download(np.uint64, nu),
           "d_pk": pipe.d_pk.download(np.int64, nd), "d_perm": pipe.d_perm.download(np.uint32, nd),
           "u_pk": pipe.u_pk.download(np.int64, nu), "u_perm": pipe.u_perm.download(np.uint32, nu),
           "masks": pipe.masks.download(np.uint8, pipe.masks.nbytes),
           "status": pipe.status.download(np.uint8, pipe.status.nbytes)}
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, arenas, big=False):
    """the separate calls' outputs, checked against the oracle's records (once per form, never modified)"""
    eng = _reference.engine
    pipe = _pipeline(eng, name, arenas, big)
    _separate_calls(pipe, arenas)
    eng.sync()
    out = _download(pipe)
    base, target = _sides(name)[:2]
    od, oc = O.classify2(base.key, base.oid, target.key, target.oid)
    assert out["counts"][4] == 0
    assert [int(x) for x in out["counts"][:4]] == [oc["inserts"], oc["updates"], oc["deletes"], od.shape[0]]
    assert np.array_equal(out["delta"].reshape(-1, 2), od)
    for v in out.values():
        v.setflags(write=False)
    return out


def _assert_equal(got, ref):
    assert got.keys() == ref.keys()
    for k in ref:
        # (masks and status whole: canaries beyond the update count — a field diff that took a
        # larger count would have written there)
        assert np.array_equal(got[k], ref[k]), k


@pytest.fixture(autouse=True)
def _ref_engine(engine):
    _reference.engine = engine


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("count", [0, 1])
@pytest.mark.parametrize("name", COUNT_SIDES)
def test_gpu_step_count_equals_separate_calls(engine, request, name, count, overlap):
    ref = _reference(name, True)
    nu = int(ref["counts"][1])
    assert {"no_update": nu == 0, "no_delta": not ref["counts"][:4].any(), "one_update_last_tile": nu == 1,
            "many_tiles": nu > 1000, "one_slot": 3 <= nu < 200}[name]
    if name != "no_delta":
        assert int(ref["counts"][3]) > nu
    _options(engine, request, step_overlap_min=0, step_count=count, step_overlap=overlap)
    pipe = _pipeline(engine, name)
    pipe.step()
    engine.sync()
    _assert_equal(_download(pipe), ref)


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("count", [0, 1])
def test_gpu_step_count_back_to_back(engine, request, count, overlap):
    """two steps on one pipeline with no host sync between them, the target's OIDs replaced in between so that
    the second step finds the first half of the updates (the same arena indices): its field diff must see
    counters zeroed after the first step's field diff read them, and nothing of the first step's count"""
    ref1, ref2 = _reference("many_tiles", True), _reference("first_half", True)
    nu1, nu2 = int(ref1["counts"][1]), int(ref2["counts"][1])
    assert 0 < nu2 < nu1
    _options(engine, request, step_overlap_min=0, step_count=count, step_overlap=overlap)
    pipe = _pipeline(engine, "many_tiles")
    oid2 = _sides("first_half")[1].oid
    engine.sync()
    pipe.step()
    pipe.B.oid.upload(oid2.reshape(-1), sync=False)  # (on the context's stream: after the first step)
    pipe.step()
    engine.sync()
    got = _download(pipe)
    words = pipe.maps.words
    # the first step's results still lie beyond the second's counts: its masks and status were right
    want = dict(ref2)
    want["masks"] = ref1["masks"].copy()
    want["masks"][: nu2 * words * 8] = ref2["masks"][: nu2 * words * 8]
    want["status"] = ref1["status"].copy()
    want["status"][:nu2] = ref2["status"][:nu2]
    _assert_equal(got, want)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("count", [0, 1])
def test_gpu_step_count_pairs_form(engine, request, count, overlap):
    """a field diff given pairs reads the placed update list: k_gscan2 and k_place2 stay in front of it"""
    ref = _reference("many_tiles", False)
    _options(engine, request, step_overlap_min=0, step_count=count, step_overlap=overlap)
    pipe = _pipeline(engine, "many_tiles", arenas=False)
    pipe.step()
    engine.sync()
    _assert_equal(_download(pipe), ref)


def test_gpu_step_count_big_tables(engine, request):
    """k_fielddiff_g, the kernel for tables too large for LDS, sums the partial counters too: many_tiles
    (updates in more than 64 join tiles, so every one of the 64 counters holds a part of the count) under
    maps of 24 KiB and more — every output of the step equals the separate calls run with the same maps,
    and masks and status equal the small-table reference (legends nobody names change no result)"""
    import fd_craft as F

    small, big = _sides("many_tiles")[4], _big_maps()
    assert F.table_bytes(small) <= 16 * 1024 and F.table_bytes(big) >= F.BIG_TABLE
    assert big.words == small.words and big.keys == small.keys
    tile = _layer()[3]
    assert np.unique(tile % SLOTS).size == SLOTS
    ref_small, ref = _reference("many_tiles", True), _reference("many_tiles", True, True)
    assert int(ref["counts"][1]) > 1000
    assert np.array_equal(ref["masks"], ref_small["masks"]) and np.array_equal(ref["status"], ref_small["status"])
    _options(engine, request, step_overlap_min=0, step_count=1, step_overlap=1)
    pipe = _pipeline(engine, "many_tiles", big=True)
    assert pipe.masks.nbytes == ref_small["masks"].size
    pipe.step()
    engine.sync()
    _assert_equal(_download(pipe), ref)


@pytest.mark.parametrize("kern", ["stream", "walk"])
def test_gpu_step_count_other_field_diff_kernels(engine, request, kern):
    """the streamed and the walked field diff kernels sum the partial counters too"""
    ref = _reference("many_tiles", True)
    _options(engine, request, step_overlap_min=0, step_count=1, step_overlap=1, fd_stream=int(kern == "stream"),
             fd_walk=int(kern == "walk"))
    pipe = _pipeline(engine, "many_tiles")
    pipe.step()
    engine.sync()
    _assert_equal(_download(pipe), ref)
