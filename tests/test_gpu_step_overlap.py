"""-m gpu: kd_diff2_step, the whole step behind one call, against the separate entry points run in
sequence (kd_diff2_device_ex + kd_fielddiff + 2 x kd_delta_pk_order, which the rest of the suite pins
to the oracle): every output bit for bit, with both schedules (``step_overlap`` 0: one stream; 1 / 2:
the placement and the pk order on the side stream beside the field diff), both arena forms, back to
back without a host sync, and with nothing written beyond the counts (canaries)."""
import ctypes
import functools

import numpy as np
import pytest

from kart_amd import _native as N

pytestmark = pytest.mark.gpu

CANARY = 0xA5
LISTS = ("delta", "upd", "dkey", "ukey", "d_pk", "d_perm", "u_pk", "u_perm")
ELEM = {"delta": 8, "upd": 8, "dkey": 8, "ukey": 8, "d_pk": 8, "d_perm": 4, "u_pk": 8, "u_perm": 4}


class _Shape:
    """two sides, their blobs and the field maps"""

    def __init__(self, base, target, base_blobs, target_blobs, maps):
        self.base, self.target, self.base_blobs, self.target_blobs, self.maps = base, target, base_blobs, target_blobs, maps


@functools.lru_cache(maxsize=None)
def _shape(name):
    from kart_amd import packing, synth
    from kart_amd.schema import FieldMaps

    if name in ("points", "points_b", "same", "empty"):
        # points: 586 join tiles = 10 placement groups; 4,688 mask blocks = more than one scan chunk
        # at either chunk size (4096 / 1024)
        L = synth.points_layer(120_000, seed=12) if name == "points_b" else synth.points_layer(300_000, seed=11)
    elif name == "polygons":  # the field diff's long-blob window shape
        L = synth.polygons_layer(20_000, seed=13)
    else:
        raise KeyError(name)
    maps = FieldMaps(L.schema, L.legends, L.schema, L.legends)
    if name == "same":  # a side against itself: no deltas, zero updates
        return _Shape(L.base, L.base, L.base_blobs, L.base_blobs, maps)
    if name == "empty":
        e = packing.PackedSide(np.zeros(0, np.uint64), np.zeros((0, 20), np.uint8), 0, np.zeros(0, np.int64))
        blobs = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        return _Shape(e, e, blobs, blobs, maps)
    return _Shape(L.base, L.target, L.base_blobs, L.target_blobs, maps)


@functools.lru_cache(maxsize=None)
def _update_arenas(name):
    """the updates' blobs in update order (host): what a field diff without pairs reads"""
    from oracle import oracle as O

    S = _shape(name)
    od, _ = O.classify2(S.base.key, S.base.oid, S.target.key, S.target.oid)
    upd = od[(od[:, 0] != 0xFFFFFFFF) & (od[:, 1] != 0xFFFFFFFF)]
    out = []
    for side, (data, off) in ((0, S.base_blobs), (1, S.target_blobs)):
        idx = upd[:, side].astype(np.int64)
        start = off[idx].astype(np.int64)
        lens = off[idx + 1].astype(np.int64) - start
        noff = np.zeros(idx.size + 1, np.uint64)
        np.cumsum(lens, out=noff[1:])
        pos = np.repeat(start - noff[:-1].astype(np.int64), lens) + np.arange(int(noff[-1]), dtype=np.int64)
        out.append((np.ascontiguousarray(data[pos]), noff))
    return out


def _pk_range(S):
    from kart_amd import walkkey

    pks = walkkey.int_keys_to_pks(np.concatenate([S.base.key, S.target.key]))
    return (int(pks.min()), int(pks.max())) if pks.size else (0, 0)


class _Run:
    """device inputs and canary-filled outputs of one shape; ``reference()`` queues the separate
    calls, ``step()`` the one call — neither synchronises"""

    def __init__(self, engine, name, arenas, pk=True):
        from kart_amd.device import DevBlobs, DevBuf, DevSide

        S = _shape(name)
        self.eng, self.S, self.pk = engine, S, pk
        self.dA, self.dB = DevSide(engine, S.base), DevSide(engine, S.target)
        self.sa, self.sb = self.dA.kd_side(), self.dB.kd_side()
        blobs = _update_arenas(name) if arenas else (S.base_blobs, S.target_blobs)
        self.OB, self.NB = DevBlobs(engine, *blobs[0]), DevBlobs(engine, *blobs[1])
        self.ob, self.nb = self.OB.kd_blobs(), self.NB.kd_blobs()
        self.arenas = arenas
        self.km = S.maps.kd_maps()
        self.words = S.maps.words
        self.cap = S.base.n + S.target.n + 1
        self.cap_upd = min(S.base.n, S.target.n)
        self.lo, self.hi = _pk_range(S)
        self.buf = {k: DevBuf(engine, ELEM[k] * self.cap) for k in LISTS}
        self.buf["masks"] = DevBuf(engine, 8 * self.cap * self.words)
        self.buf["status"] = DevBuf(engine, self.cap)
        self.c = DevBuf(engine, 64)
        self.reset()

    def reset(self):
        L, ctx = self.eng.L, self.eng.ctx
        for b in self.buf.values():
            N.check(L.kd_memset(ctx, b.ptr, CANARY, b.nbytes), "kd_memset")
        self.c.zero()

    def reference(self):
        L, ctx, b = self.eng.L, self.eng.ctx, self.buf
        N.check(L.kd_diff2_device_ex(ctx, ctypes.byref(self.sa), ctypes.byref(self.sb), None, None, 0, b["delta"].ptr,
                                     b["upd"].ptr, b["dkey"].ptr, b["ukey"].ptr, self.c.ptr, self.c.ptr + 32),
                "kd_diff2_device_ex")
        N.check(L.kd_fielddiff(ctx, ctypes.byref(self.ob), ctypes.byref(self.nb), None if self.arenas else b["upd"].ptr,
                               self.cap_upd, ctypes.cast(self.c.ptr + 8, N.c_u64p), N.KD_MEM_DEVICE,
                               ctypes.byref(self.km), b["masks"].ptr, b["status"].ptr, N.KD_MEM_DEVICE), "kd_fielddiff")
        if self.pk:
            self.pk_order_deltas()
            N.check(L.kd_delta_pk_order(ctx, ctypes.byref(self.sa), ctypes.byref(self.sb), b["upd"].ptr, b["ukey"].ptr,
                                        self.cap_upd, self.c.ptr + 8, self.lo, self.hi, b["u_pk"].ptr, b["u_perm"].ptr),
                    "kd_delta_pk_order")

    def pk_order_deltas(self):
        L, ctx, b = self.eng.L, self.eng.ctx, self.buf
        N.check(L.kd_delta_pk_order(ctx, ctypes.byref(self.sa), ctypes.byref(self.sb), b["delta"].ptr, b["dkey"].ptr,
                                    self.cap, self.c.ptr + 24, self.lo, self.hi, b["d_pk"].ptr, b["d_perm"].ptr),
                "kd_delta_pk_order")

    def step_args(self):
        b = self.buf
        st = N.KdStep()
        st.base, st.target = ctypes.pointer(self.sa), ctypes.pointer(self.sb)
        st.d_delta, st.d_upd, st.d_delta_key, st.d_upd_key = b["delta"].ptr, b["upd"].ptr, b["dkey"].ptr, b["ukey"].ptr
        st.d_counts, st.d_err = self.c.ptr, self.c.ptr + 32
        st.old_blobs, st.new_blobs = ctypes.pointer(self.ob), ctypes.pointer(self.nb)
        if not self.arenas:
            st.d_pairs = b["upd"].ptr
        st.upd_cap = self.cap_upd
        st.maps = ctypes.pointer(self.km)
        st.d_masks, st.d_status = b["masks"].ptr, b["status"].ptr
        st.pk_lo, st.pk_hi, st.delta_cap = self.lo, self.hi, self.cap
        if self.pk:
            st.d_delta_pk, st.d_delta_perm = b["d_pk"].ptr, b["d_perm"].ptr
            st.d_upd_pk, st.d_upd_perm = b["u_pk"].ptr, b["u_perm"].ptr
        return st

    def step(self):
        N.check(self.eng.L.kd_diff2_step(self.eng.ctx, ctypes.byref(self.step_args())), "kd_diff2_step")

    def download(self):
        """(after a sync) counts and every buffer whole"""
        out = {k: b.download(np.uint8, b.nbytes) for k, b in self.buf.items()}
        out["counts"] = self.c.download(np.uint64, 8)
        return out


@functools.lru_cache(maxsize=None)
def _reference(name, arenas, pk):
    """the separate calls' outputs (computed once per form on the session's engine, never modified)"""
    run = _Run(_reference.engine, name, arenas, pk)
    run.reference()
    _reference.engine.sync()
    out = run.download()
    for v in out.values():
        v.setflags(write=False)
    return out


def _assert_equal(got, ref, pk=True):
    """counts; records, keys, pk outputs, masks and status up to their counts, bit for bit; the
    canaries beyond the counts untouched; (and whatever else a buffer holds is the reference's too)"""
    assert np.array_equal(got["counts"], ref["counts"]), (got["counts"], ref["counts"])
    assert got["counts"][4] == 0
    nd, nu = int(ref["counts"][3]), int(ref["counts"][1])
    for k in LISTS:
        n = (nd if k in ("delta", "dkey", "d_pk", "d_perm") else nu) * ELEM[k]
        if not pk and k in ("d_pk", "d_perm", "u_pk", "u_perm"):
            n = 0  # pk outputs omitted: never written
        assert np.array_equal(got[k][:n], ref[k][:n]), k
        assert (got[k][n:] == CANARY).all(), f"{k}: written beyond its count"
    words = got["masks"].size // got["status"].size // 8
    assert np.array_equal(got["masks"][: nu * words * 8], ref["masks"][: nu * words * 8])
    assert np.array_equal(got["status"][:nu], ref["status"][:nu])
    for k in ("masks", "status"):
        assert np.array_equal(got[k], ref[k]), f"{k}: differs beyond the update count"


def _options(engine, request, **opts):
    opts.setdefault("step_overlap_min", 0)  # (the schedule asked for, whatever the sides' size)
    old = {k: engine.get_option(k) for k in opts}
    request.addfinalizer(lambda: [engine.set_option(k, v) for k, v in old.items()])
    for k, v in opts.items():
        engine.set_option(k, v)


@pytest.fixture(autouse=True)
def _ref_engine(engine):
    _reference.engine = engine


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("arenas", [True, False], ids=["arenas", "pairs"])
@pytest.mark.parametrize("name", ["points", "polygons", "same", "empty"])
def test_gpu_step_equals_separate_calls(engine, request, name, arenas, overlap):
    ref = _reference(name, arenas, True)
    if name == "points":
        assert int(ref["counts"][3]) > 0 and int(ref["counts"][1]) > 0
    if name in ("same", "empty"):
        assert not ref["counts"][:4].any()
    _options(engine, request, step_overlap=overlap)
    run = _Run(engine, name, arenas)
    run.step()
    engine.sync()
    _assert_equal(run.download(), ref)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("arenas", [True, False], ids=["arenas", "pairs"])
def test_gpu_step_without_pk_outputs(engine, request, arenas, overlap):
    """NULL pk outputs: no pk order, nothing written through them"""
    _options(engine, request, step_overlap=overlap)
    run = _Run(engine, "points", arenas, pk=False)
    run.step()
    engine.sync()
    _assert_equal(run.download(), _reference("points", arenas, True), pk=False)


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("wave", [0, 1])
def test_gpu_step_scan_forms(engine, request, overlap, wave):
    """the pk order's block-wide and LDS-free scans on either schedule"""
    _options(engine, request, step_overlap=overlap, pkm_wave=wave)
    run = _Run(engine, "points", True)
    run.step()
    engine.sync()
    _assert_equal(run.download(), _reference("points", True, True))


@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("arenas", [True, False], ids=["arenas", "pairs"])
@pytest.mark.parametrize("seq", ["same", "alternated"])
def test_gpu_step_back_to_back(engine, request, seq, arenas, overlap):
    """three steps without a host sync between them (the next step's partition, join and mark reuse
    the scratch this step's side work reads), then a plain kd_delta_pk_order with no sync before it"""
    names = ["points", "points", "points"] if seq == "same" else ["points", "points_b", "points"]
    refs = {n: _reference(n, arenas, True) for n in set(names)}
    _options(engine, request, step_overlap=overlap)
    runs = {n: _Run(engine, n, arenas) for n in set(names)}
    engine.sync()
    for n in names:
        runs[n].step()
    last = runs[names[-1]]
    N.check(engine.L.kd_memset(engine.ctx, last.buf["d_pk"].ptr, CANARY, last.buf["d_pk"].nbytes), "kd_memset")
    N.check(engine.L.kd_memset(engine.ctx, last.buf["d_perm"].ptr, CANARY, last.buf["d_perm"].nbytes), "kd_memset")
    last.pk_order_deltas()
    engine.sync()
    for n, run in runs.items():
        _assert_equal(run.download(), refs[n])


def test_gpu_step_profiled_launches(engine, request):
    """per-kernel events cover the side stream's kernels: one k_place2 and two of each pk-order
    kernel per step, with the results unchanged"""
    _options(engine, request, step_overlap=1)
    request.addfinalizer(lambda: (engine.prof_enable(False), engine.prof_reset()))
    engine.prof_select(None)
    engine.prof_enable(True)
    engine.prof_reset()
    run = _Run(engine, "points", True)
    run.step()
    engine.sync()
    want = {"k_partition2": 1, "k_join2": 1, "k_gscan2": 1, "k_place2": 1, "k_fielddiff": 1, "k_pkm_mark": 2,
            "k_pkm_scan": 2, "k_pkm_cscan": 2, "k_pkm_place": 2}
    got = {k: engine.prof_get(k) for k in want}
    assert {k: v[0] for k, v in got.items()} == want
    assert all(v[1] > 0 for v in got.values())
    engine.prof_enable(False)
    _assert_equal(run.download(), _reference("points", True, True))
