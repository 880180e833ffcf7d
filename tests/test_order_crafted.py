"""The order kernels of kd_sort.hip on crafted edges (tests/order_craft.py): kd_delta_pk_order's bitmap
placement and radix sort, kd_diff2_step's LDS-free scans, kd_sort_side_into / kd_sort_side, and the
host bookkeeping of the two mask buffers — every output exact against numpy's sort of the crafted pks
(or keys), canaries beyond the counts untouched, the intended path checked by launch counts.

The CPU part pins the kernel constants the crafted seams depend on to the source text and asserts that
every case reaches the path it states."""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import order_craft as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
PAD = 64  # elements kept beyond every output's capacity: canaries too

BITMAP = OC.bitmap_cases()
RADIX = OC.radix_cases()
STEP = OC.step_cases()
BOOK = OC.book_cases()
BIG = {"msgpack": OC.msgpack_case, "span31": OC.span31_case}
DUPS = OC.dup_cases()


def _ids(cases):
    return [c.name for c in cases]


@functools.lru_cache(maxsize=None)
def _crafted(group, name):
    case = next(c for c in {"bitmap": BITMAP, "radix": RADIX}[group] if c.name == name)
    m = OC.materialise(case)
    for a in vars(m).values():
        a.setflags(write=False)
    return case, m


# ================================================================================================
# CPU part
# ================================================================================================
def _source():
    return open(os.path.join(ROOT, "kart_amd", "csrc", "kd_sort.hip")).read()


def test_constants_match_source():
    """the constants order_craft.py states equal the #define / constexpr lines of kd_sort.hip, and the
    Makefile overrides none of them"""
    text = _source()

    def define(name):
        return int(re.search(r"^#define %s (\d+)\b" % name, text, re.M).group(1))

    def const(name):
        return int(re.search(r"^constexpr int (?:[^;]*?\b)?%s = (\d+)\s*[,;]" % name, text, re.M).group(1))

    assert const("PKM_NT") == OC.PKM_NT
    assert define("KD_PKM_IPT") == OC.PKM_IPT and re.search(r"\bPKM_IPT = KD_PKM_IPT\b", text)
    assert re.search(r"\bPKM_CH = PKM_NT \* PKM_IPT;", text) and OC.PKM_CH == OC.PKM_NT * OC.PKM_IPT
    assert re.search(r"^constexpr int PKM_CHW = 64 \* PKM_IPT;", text, re.M) and OC.PKM_CHW == 64 * OC.PKM_IPT
    assert const("PKC_PT") == OC.PKC_PT and const("PKC_WPT") == OC.PKC_WPT
    assert define("KD_RS_RB") == OC.RS_RB and re.search(r"^constexpr int RS_RB = KD_RS_RB;", text, re.M)
    assert define("KD_RS_NT") == OC.RS_NT and re.search(r"^constexpr int RS_NT = KD_RS_NT;", text, re.M)
    assert define("KD_RS_IPT32") == OC.IPT32 and define("KD_RS_IPT64") == OC.IPT64
    assert re.search(r"IPT = sizeof\(CK\) == 4 \? KD_RS_IPT32 : KD_RS_IPT64;", text)
    assert const("RS_HIST_NT") * const("RS_HIST_IPT") == OC.RS_HIST_CHUNK
    assert define("KD_RS_LBW") == OC.RS_LBW and const("RS_MAXRUNS") == OC.RS_MAXRUNS
    # the chunk-total scans: 1024 threads x PKC_PT and 64 lanes x PKC_WPT chunks per trip
    assert re.search(r"__launch_bounds__\(1024\) void k_pkm_cscan\(", text) and "base += 1024 * PKC_PT" in text
    assert re.search(r"__launch_bounds__\(64\) void k_pkm_cscan_w\(", text) and "base += 64 * PKC_WPT" in text
    assert (OC.CSCAN_TRIP, OC.CSCAN_W_TRIP, OC.TILE32, OC.TILE64) == (8192, 2048, 8192, 4096)
    internal = open(os.path.join(ROOT, "kart_amd", "csrc", "kd_internal.h")).read()
    assert re.search(r"pkm_max_blocks = 1ull << 26;", internal) and OC.PKM_MAX_BLOCKS == 1 << 26
    mk = open(os.path.join(ROOT, "kart_amd", "csrc", "Makefile")).read()
    assert not re.search(r"-DKD_RS_|-DKD_PKM_", mk)


@pytest.mark.parametrize("case", BITMAP + [f() for f in BIG.values()], ids=_ids(BITMAP) + list(BIG))
def test_bitmap_cases_reach_their_path(case):
    """the stated blocks, chunks and chunk-total trips follow from the constants, the default takes
    the bitmap, and the builders' invariants hold"""
    e = case.expect
    assert e["path"] == "bitmap" and OC.takes_bitmap(case.lo, case.hi)
    assert OC.bitmap_geometry(case.lo, case.hi) == {"nb": e["nb"], "nch": e["nch"], "trips": e["trips"]}
    assert case.cap <= 70_000
    OC.check_crafted(case, OC.materialise(case))


def test_bitmap_cases_cover_the_seams():
    by = {c.name: c for c in BITMAP}
    assert {c.expect["nb"] for c in BITMAP} >= {1, 15, 16, 17, 4095, 4096, 4097, 8193}
    assert any(c.expect["nb"] % OC.PKM_IPT for c in BITMAP)  # the last thread's masks partly in range
    for name in ("nb16", "nb17", "nb4097", "loose"):
        c = by[name]
        assert c.lo < 0 < c.hi and np.isin(np.arange(-64, 0), c.pks).all(), name  # the block [-64, -1], full
    for nb in (15, 17, 4095, 4097, 8193):  # pk_lo = 64k + 63, pk_hi = 64m, both records
        c = by[f"nb{nb}"]
        assert c.lo % 64 == 63 and c.hi % 64 == 0 and c.lo in c.pks and c.hi in c.pks
    c = by["loose"]  # a whole empty chunk on both ends
    assert (c.pks.min() >> 6) - (c.lo >> 6) >= OC.PKM_CH and (c.hi >> 6) - (c.pks.max() >> 6) >= OC.PKM_CH
    assert np.all(np.diff(by["asc"].pks) > 0) and np.all(np.diff(by["desc"].pks) < 0)
    blk = by["aba"].pks[:64] >> 6  # one wave: block A in two runs
    runs = blk[np.concatenate([[True], blk[1:] != blk[:-1]])]
    assert runs.size > np.unique(runs).size
    blk = by["run_63_0"].pks >> 6
    assert len(set(blk[62:67].tolist())) == 1 and blk[61] != blk[62] and blk[67] != blk[66]
    blk = by["run_64"].pks >> 6
    assert len(set(blk[:64].tolist())) == 1 and len(set(blk[64:128].tolist())) == 1 and blk[63] != blk[64]
    assert {by[f"n{n}"].n for n in (1, 63, 64, 65, 255, 256, 257)} == {1, 63, 64, 65, 255, 256, 257}
    assert by["dn_below"].n < by["dn_below"].cap and by["dn_above"].dn > by["dn_above"].cap
    assert by["dn_zero"].n == 0 < by["dn_zero"].cap
    # the poisoned tail would shift ranks: most of its pks lie below the head's largest
    c = by["dn_below"]
    assert (c.tail < c.pks.max()).sum() > c.tail.size // 2
    m = OC.msgpack_case()
    assert set(OC.MSGPACK_EDGES) <= set(m.pks.tolist())
    s = OC.span31_case()
    assert s.hi - s.lo == 2**31 + 2**20
    ch = np.unique(((s.pks >> 6) - (s.lo >> 6)) // OC.PKM_CH)
    assert {0, 8191, 8192, 8195, 8196} <= set(ch.tolist())  # both sides of the trip seam, and the last chunk


@pytest.mark.parametrize("case", RADIX, ids=_ids(RADIX))
def test_radix_cases_reach_their_path(case):
    e = case.expect
    assert e["path"] == "radix"
    assert OC.radix_geometry(case.lo, case.hi) == {k: e[k] for k in ("bits", "npass", "width", "ck")}
    assert e["npass"] * e["width"] >= max(e["bits"], 1) and e["width"] <= OC.RS_RB
    assert case.cap <= 70_000
    OC.check_crafted(case, OC.materialise(case))


def test_radix_cases_cover_the_widths():
    by = {c.name: c for c in RADIX}
    assert {c.expect["bits"] for c in RADIX} >= {0, 1, 9, 10, 18, 19, 27, 28, 32, 33, 36, 37, 45, 46, 63, 64}
    assert {by[n].lo for n in ("one_min", "one_max")} == {OC.I64_MIN, OC.I64_MAX}
    assert by["w64_cross"].lo < 0 < by["w64_cross"].hi
    n32 = {c.n for c in RADIX if c.expect["ck"] == 32}
    n64 = {c.n for c in RADIX if c.expect["ck"] == 64}
    assert n32 >= {8191, 8192, 8193, 2 * 8192 + 1} and n64 >= {4095, 4096, 4097}
    # 9-bit digits on 64-bit keys with 4 to 7 passes
    assert {c.expect["npass"] for c in RADIX if c.expect["ck"] == 64 and c.expect["width"] == 9} >= {4, 5, 7}
    for name, digit in (("hot_digit", 1), ("hot_digit64", 2)):
        c = by[name]
        d = ((c.pks - c.lo) >> (9 * digit)) & 511
        vals, cnt = np.unique(d, return_counts=True)
        assert vals.size == 2 and cnt.min() == 1  # all records but one share the digit
        assert OC.radix_tiles(c)[1] >= 6 > OC.RS_LBW + 1
    for name in ("dn_below", "dn_below64"):
        tc, tn = OC.radix_tiles(by[name])
        assert tc >= tn + 5 and by[name].n < by[name].cap
    assert by["dn_zero"].n == 0 < by["dn_zero"].cap


@pytest.mark.parametrize("case", STEP, ids=_ids(STEP))
def test_step_cases_reach_their_path(case):
    e = case.expect
    assert e["path"] == "bitmap_wave" and OC.takes_bitmap(case.lo, case.hi)
    assert OC.bitmap_geometry(case.lo, case.hi, wave=True) == {"nb": e["nb"], "nch": e["nch"], "trips": e["trips"]}
    assert case.pks.size <= 35_000
    OC.check_step(case, OC.materialise_step(case))


def test_step_cases_cover_the_seams():
    assert [c.expect["nb"] for c in STEP[:3]] == [1023, 1024, 1025]
    assert {c.expect["nch"] for c in STEP} >= {1, 2, 3, 4, 5, 2051}
    s = STEP[-1]
    assert s.hi - s.lo + 1 == 2**27 + 2**17 - 62 and s.expect["trips"] == 2  # (bounds 64k + 63 .. 64m)
    ch = np.unique(((s.pks >> 6) - (s.lo >> 6)) // OC.PKM_CHW)
    assert {0, 2047, 2048, 2050} <= set(ch.tolist())


def test_dup_cases_take_passes():
    for name, keys in DUPS.items():
        vary, bits, npass = OC.sort_plan(keys)
        assert npass >= 1 and np.unique(keys).size < keys.size <= 70_000, name
    assert OC.sort_plan(DUPS["two_values"])[1:] == (1, 1)
    assert np.unique(DUPS["513_values"]).size == 513 and OC.sort_plan(DUPS["513_values"])[2] == 2
    assert OC.sort_plan(DUPS["doubled_wide"])[1] > 32
    k = DUPS["copies_lanes_waves_tiles"]
    pos = np.nonzero(k == k[40])[0]
    assert {0, 1, 63, 64, 65}.issubset(pos.tolist()) and np.unique(pos // OC.TILE32).size == 4


def test_book_cases_are_disjoint():
    seen = np.zeros(0, np.int64)
    for form, case in BOOK:
        assert not np.intersect1d(seen, case.pks).size and case.pks.size > 100 and case.lo == 0
        seen = np.union1d(seen, case.pks)
        if form == "step":
            OC.check_step(case, OC.materialise_step(case))
        else:
            OC.check_crafted(case, OC.materialise(case))
    nbs = [c.expect.get("nb") for f, c in BOOK if f == "bitmap"]
    assert nbs[:4] == [20_000, 100, 50_000, 50_000]  # large, small, larger than the first, the same again
    assert [f for f, _ in BOOK].count("radix") == 1 and [f for f, _ in BOOK].count("step") == 1


# ================================================================================================
# GPU part
# ================================================================================================
PK_KERNELS = ("k_pkm_mark", "k_pkm_scan", "k_pkm_cscan", "k_pkm_place", "k_dpk_keys", "k_sort_scan", "k_sort_pass")


@contextlib.contextmanager
def _profiled(eng):
    eng.prof_select(None)
    eng.prof_enable(True)
    eng.prof_reset()
    try:
        yield
    finally:
        eng.prof_enable(False)
        eng.prof_reset()


def _launches(eng, names=PK_KERNELS):
    return {k: eng.prof_get(k)[0] for k in names}


def _bitmap_launches(calls=1):
    return dict({k: 0 for k in PK_KERNELS}, k_pkm_mark=calls, k_pkm_scan=calls, k_pkm_cscan=calls, k_pkm_place=calls)


def _radix_launches(npass):
    return dict({k: 0 for k in PK_KERNELS}, k_dpk_keys=1, k_sort_scan=1, k_sort_pass=npass)


def _options(eng, request, **opts):
    old = {k: eng.get_option(k) for k in opts}
    request.addfinalizer(lambda: [eng.set_option(k, v) for k, v in old.items()])
    for k, v in opts.items():
        eng.set_option(k, v)


class _Keys:
    """what DevSide(keys_only=True) reads of a side"""

    def __init__(self, key):
        self.key, self.n, self.key_mode = key, int(key.size), 0


def _fill(eng, buf):
    from kart_amd import _native as N

    N.check(eng.L.kd_memset(eng.ctx, buf.ptr, CANARY, buf.nbytes), "kd_memset")


class _PkCall:
    """device inputs and canary-filled outputs of one kd_delta_pk_order call; run() does not synchronise"""

    def __init__(self, eng, case, m):
        from kart_amd.device import DevBuf, DevSide

        self.eng, self.case, self.m = eng, case, m
        self.A, self.B = DevSide(eng, _Keys(m.key_a), keys_only=True), DevSide(eng, _Keys(m.key_b), keys_only=True)
        self.sa, self.sb = self.A.kd_side(), self.B.kd_side()
        self.rec = DevBuf.from_numpy(eng, m.rec.reshape(-1))
        self.rkey = DevBuf.from_numpy(eng, m.rkey)
        self.dn = DevBuf.from_numpy(eng, np.array([case.dn], np.uint64))
        self.pk, self.perm = DevBuf(eng, 8 * (case.cap + PAD)), DevBuf(eng, 4 * (case.cap + PAD))

    def run(self, keys):
        from kart_amd import _native as N

        _fill(self.eng, self.pk)
        _fill(self.eng, self.perm)
        c = self.case
        N.check(self.eng.L.kd_delta_pk_order(self.eng.ctx, ctypes.byref(self.sa), ctypes.byref(self.sb), self.rec.ptr,
                                             self.rkey.ptr if keys else None, c.cap, self.dn.ptr, c.lo, c.hi, self.pk.ptr,
                                             self.perm.ptr), "kd_delta_pk_order")

    def check(self):
        """(after a sync) pk and perm equal the reference up to the count; canaries beyond"""
        n = self.case.n
        pk, perm = self.pk.download(np.uint8, self.pk.nbytes), self.perm.download(np.uint8, self.perm.nbytes)
        got_pk, got_perm = pk[:8 * n].view(np.int64), perm[:4 * n].view(np.uint32)
        assert np.array_equal(got_perm, self.m.want_perm), (self.case.name, "perm")
        assert np.array_equal(got_pk, self.m.want_pk), (self.case.name, "pk")
        assert (pk[8 * n:] == CANARY).all() and (perm[4 * n:] == CANARY).all(), (self.case.name, "written beyond the count")
        return pk, perm


def _both_key_forms(eng, case, m, want):
    """the call with the records' keys given and with d_keys NULL (gathered from the sides): each exact,
    each on the intended path, the two equal"""
    call = _PkCall(eng, case, m)
    outs = []
    for keys in (True, False):
        with _profiled(eng):
            call.run(keys)
            eng.sync()
            assert _launches(eng) == want, (case.name, keys)
        outs.append(call.check())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids(BITMAP))
def test_gpu_bitmap_crafted(engine, name):
    """1. bitmap placement through kd_delta_pk_order (k_pkm_mark's run merge, k_pkm_scan's vector and
    tail paths, k_pkm_place; device counts at, below, above the capacity and zero)"""
    case, m = _crafted("bitmap", name)
    assert engine.get_option("pkm_max_blocks") == OC.PKM_MAX_BLOCKS
    _both_key_forms(engine, case, m, _bitmap_launches())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BIG))
def test_gpu_bitmap_two_trips(name):
    """the chunk totals' scan past one trip of 8,192 chunks (k_pkm_cscan's carry): the msgpack width
    limits over [-2**31, 2**31 - 1] (16,384 chunks) and a span of 2**31 + 2**20 pks (8,197 chunks), on
    a context of their own so the session's does not keep the 0.7 to 1.5 GB of scratch"""
    from kart_amd.engine import Engine

    case = BIG[name]()
    m = OC.materialise(case)
    with Engine(0) as eng:
        _both_key_forms(eng, case, m, _bitmap_launches())


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids(RADIX))
def test_gpu_radix_crafted(engine, request, name):
    """3. the radix pk order (pkm_max_blocks = 0): k_dpk_keys and k_sort_pass on 32-bit and 64-bit
    compact keys at every pass count, tile seams, a hot digit's look-back, device counts"""
    case, m = _crafted("radix", name)
    _options(engine, request, pkm_max_blocks=0)
    _both_key_forms(engine, case, m, _radix_launches(case.expect["npass"]))


# ---- 2. kd_diff2_step, LDS-free scans ------------------------------------------------------------
STEP_LISTS = {"delta": 8, "upd": 8, "dkey": 8, "ukey": 8, "d_pk": 8, "d_perm": 4, "u_pk": 8, "u_perm": 4}


class _StepRun:
    """two crafted sides in HBM and canary-filled outputs of a kd_diff2_step without a field diff"""

    def __init__(self, eng, case, s):
        from kart_amd import packing
        from kart_amd.device import DevBuf, DevSide

        self.eng, self.case, self.s = eng, case, s
        mk = lambda k, o: packing.PackedSide(k, o, 0, np.arange(k.size))
        self.A, self.B = DevSide(eng, mk(s.key_a, s.oid_a)), DevSide(eng, mk(s.key_b, s.oid_b))
        self.sa, self.sb = self.A.kd_side(), self.B.kd_side()
        self.cap = s.key_a.size + s.key_b.size + 1
        self.cap_upd = min(s.key_a.size, s.key_b.size)
        self.buf = {k: DevBuf(eng, e * (self.cap + PAD)) for k, e in STEP_LISTS.items()}
        self.c = DevBuf(eng, 64)

    def step(self):
        from kart_amd import _native as N

        for b in self.buf.values():
            _fill(self.eng, b)
        self.c.zero()
        b = self.buf
        st = N.KdStep()
        st.base, st.target = ctypes.pointer(self.sa), ctypes.pointer(self.sb)
        st.d_delta, st.d_upd, st.d_delta_key, st.d_upd_key = b["delta"].ptr, b["upd"].ptr, b["dkey"].ptr, b["ukey"].ptr
        st.d_counts, st.d_err = self.c.ptr, self.c.ptr + 32
        st.upd_cap = self.cap_upd
        st.pk_lo, st.pk_hi, st.delta_cap = self.case.lo, self.case.hi, self.cap
        st.d_delta_pk, st.d_delta_perm = b["d_pk"].ptr, b["d_perm"].ptr
        st.d_upd_pk, st.d_upd_perm = b["u_pk"].ptr, b["u_perm"].ptr
        N.check(self.eng.L.kd_diff2_step(self.eng.ctx, ctypes.byref(st)), "kd_diff2_step")

    def download(self):
        out = {k: b.download(np.uint8, b.nbytes) for k, b in self.buf.items()}
        out["counts"] = self.c.download(np.uint64, 8)
        return out

    def check(self, got):
        """the join's records are the crafted ones; delta and update pk outputs equal the reference of
        the records' crafted pks; canaries beyond the counts"""
        s, kinds, pks = self.s, np.asarray(self.case.kinds), self.case.pks
        c = got["counts"]
        assert c[4] == 0 and (int(c[0]), int(c[1]), int(c[2])) == (s.counts["inserts"], s.counts["updates"], s.counts["deletes"])
        nd, nu = int(c[3]), int(c[1])
        assert nd == int((kinds != OC.SAME).sum())
        for rec_k, pk_k, perm_k, n, want_set in (("delta", "d_pk", "d_perm", nd, pks[kinds != OC.SAME]),
                                                 ("upd", "u_pk", "u_perm", nu, pks[kinds == OC.UPDATE])):
            rec = got[rec_k][:8 * n].view(np.uint32).reshape(n, 2)
            ia, ib = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
            assert np.all((ia < s.pk_a.size) | (ia == OC.NONE)) and np.all((ib < s.pk_b.size) | (ib == OC.NONE))
            rec_pk = np.where(ia != OC.NONE, s.pk_a[np.minimum(ia, s.pk_a.size - 1)], s.pk_b[np.minimum(ib, s.pk_b.size - 1)])
            assert np.array_equal(np.sort(rec_pk), want_set), rec_k
            want_pk, want_perm = OC.reference(rec_pk, n)
            assert np.array_equal(got[perm_k][:4 * n].view(np.uint32), want_perm), perm_k
            assert np.array_equal(got[pk_k][:8 * n].view(np.int64), want_pk), pk_k
            assert (got[pk_k][8 * n:] == CANARY).all() and (got[perm_k][4 * n:] == CANARY).all(), f"{pk_k}: beyond the count"


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("name", _ids(STEP))
def test_gpu_step_wave_scans_crafted(engine, request, name, overlap):
    """2. k_pkm_scan<true> and k_pkm_cscan_w behind kd_diff2_step (pkm_wave = 1, no field diff): chunks
    of 1,024 masks at their seams, three to five chunks (four waves per scan block), 2,051 chunks (the
    chunk totals' second trip); exact, and bit for bit what pkm_wave = 0 gives"""
    case = next(c for c in STEP if c.name == name)
    s = OC.materialise_step(case)
    _options(engine, request, pkm_wave=1, step_overlap=overlap, step_overlap_min=0)
    run = _StepRun(engine, case, s)
    with _profiled(engine):
        run.step()
        engine.sync()
        assert _launches(engine) == _bitmap_launches(2)
    got = run.download()
    run.check(got)
    engine.set_option("pkm_wave", 0)
    run.step()
    engine.sync()
    ref = run.download()
    run.check(ref)
    for k in got:
        assert np.array_equal(got[k], ref[k]), f"{k}: pkm_wave 1 differs from pkm_wave 0"


# ---- 4. side sorts ----------------------------------------------------------------------------------
def _info(keys):
    from kart_amd import _native as N

    info = N.KdKeysInfo()
    info.vary = int(np.bitwise_or.reduce(keys ^ keys[0]))
    info.key0 = int(keys[0])
    return info


def _oids(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 20), dtype=np.uint8)


def _sort_into(eng, keys, oids, koff=0, ooff=0, info=False):
    """kd_sort_side_into with the keys read at a 16-byte-aligned address + koff and the OIDs written at
    one + ooff: views into larger DevBufs.  Returns (sorted keys, OIDs, order, dup) after checking the
    canaries around every output."""
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    n = keys.size
    kin = DevBuf(eng, 8 * n + 16)
    oin = DevBuf.from_numpy(eng, oids.reshape(-1))
    kout, oout, order, dup = DevBuf(eng, 8 * (n + PAD)), DevBuf(eng, 20 * (n + PAD) + 16), DevBuf(eng, 4 * (n + PAD)), DevBuf(eng, 16)
    for b in (kin, kout, oout, order, dup):
        assert b.ptr % 16 == 0
        _fill(eng, b)
    kin.upload(keys, offset=koff)
    N.check(eng.L.kd_sort_side_into(eng.ctx, kin.ptr + koff, oin.ptr, kout.ptr, oout.ptr + ooff, order.ptr, n, dup.ptr,
                                    ctypes.byref(_info(keys)) if info else None), "kd_sort_side_into")
    eng.sync()
    k, o, r = kout.download(np.uint8, kout.nbytes), oout.download(np.uint8, oout.nbytes), order.download(np.uint8, order.nbytes)
    assert (k[8 * n:] == CANARY).all() and (r[4 * n:] == CANARY).all()
    assert (o[:ooff] == CANARY).all() and (o[ooff + 20 * n:] == CANARY).all()
    d = dup.download(np.uint8, 16)
    assert (d[4:] == CANARY).all()
    return k[:8 * n].view(np.uint64), o[ooff:ooff + 20 * n].reshape(n, 20), r[:4 * n].view(np.uint32), int(d[:4].view(np.uint32)[0])


SORT_KERNELS = ("k_rs_bits", "k_sort_hist", "k_sort_scan", "k_sort_pass", "k_gather_oid", "k_check_sorted", "k_iota")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DUPS))
def test_gpu_sort_side_duplicates_stable(engine, name):
    """duplicate keys that take radix passes: order and OIDs equal numpy's stable argsort (equal keys
    keep their input order through every pass's ranking and look-back), d_dup is set"""
    keys = DUPS[name]
    oids = _oids(keys.size, 7)
    want_order, want_keys = OC.stable_reference(keys)
    npass = OC.sort_plan(keys)[2]
    for info in (False, True):
        with _profiled(engine):
            k, o, order, dup = _sort_into(engine, keys, oids, info=info)
            got = _launches(engine, SORT_KERNELS)
        assert got == {"k_rs_bits": 0 if info else 1, "k_sort_hist": 1, "k_sort_scan": 1, "k_sort_pass": npass,
                       "k_gather_oid": 1, "k_check_sorted": 1, "k_iota": 0}
        assert np.array_equal(order, want_order), "not stable"
        assert np.array_equal(k, want_keys) and np.array_equal(o, oids[want_order]) and dup == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 4097])
def test_gpu_sort_side_unaligned_pointers(engine, n):
    """keys at a 16-byte-aligned address + 8 (k_rs_bits' and k_sort_hist's scalar loads) and the OID
    output at one + 4 (k_gather_oid's dword stores), against the same sort with aligned pointers, with
    and without the host's key info"""
    rng = np.random.default_rng(n)
    keys = rng.permutation(1 << 20)[:n].astype(np.uint64) << np.uint64(13)  # distinct: 20 varying bits
    oids = _oids(n, n)
    want_order, want_keys = OC.stable_reference(keys)
    for info in (False, True):
        control = _sort_into(engine, keys, oids, 0, 0, info)
        for koff, ooff in ((8, 0), (0, 4), (8, 4)):
            got = _sort_into(engine, keys, oids, koff, ooff, info)
            for a, b in zip(got, control):
                assert np.array_equal(a, b), (koff, ooff, info)
        k, o, order, dup = control
        assert np.array_equal(order, want_order) and np.array_equal(k, want_keys)
        assert np.array_equal(o, oids[want_order]) and dup == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dups", [False, True], ids=["distinct", "duplicates"])
def test_gpu_sort_side_in_place_single_pass(engine, dups):
    """kd_sort_side in place with one pass (at most 9 varying bits): the pass reads a copy of the
    caller's keys (rs.kin), the OIDs are gathered in place, h_dup reports duplicates"""
    from kart_amd import _native as N
    from kart_amd.device import DevBuf

    rng = np.random.default_rng(9)
    vals = (np.uint64(3) << np.uint64(50)) | (rng.permutation(512).astype(np.uint64) << np.uint64(4))
    keys = np.ascontiguousarray(rng.permutation(np.repeat(vals, 33)) if dups else vals[:300])  # (three tiles / one)
    assert OC.sort_plan(keys)[2] == 1 and (keys.size > 2 * OC.TILE32) == dups
    n = keys.size
    oids = _oids(n, 11)
    want_order, want_keys = OC.stable_reference(keys)
    dk, do, order = DevBuf(engine, 8 * (n + PAD)), DevBuf(engine, 20 * (n + PAD)), DevBuf(engine, 4 * (n + PAD))
    for b in (dk, do, order):
        _fill(engine, b)
    dk.upload(keys)
    do.upload(oids.reshape(-1))
    h_dup = ctypes.c_uint32(7)
    with _profiled(engine):
        N.check(engine.L.kd_sort_side(engine.ctx, dk.ptr, do.ptr, order.ptr, n, ctypes.addressof(h_dup)), "kd_sort_side")
        engine.sync()
        assert _launches(engine, ("k_sort_pass", "k_rs_bits", "k_gather_oid")) == {"k_sort_pass": 1, "k_rs_bits": 1, "k_gather_oid": 1}
    k, o, r = dk.download(np.uint8, dk.nbytes), do.download(np.uint8, do.nbytes), order.download(np.uint8, order.nbytes)
    assert np.array_equal(r[:4 * n].view(np.uint32), want_order) and np.array_equal(k[:8 * n].view(np.uint64), want_keys)
    assert np.array_equal(o[:20 * n].reshape(n, 20), oids[want_order]) and h_dup.value == (1 if dups else 0)
    assert (k[8 * n:] == CANARY).all() and (o[20 * n:] == CANARY).all() and (r[4 * n:] == CANARY).all()


# ---- 5. mask bookkeeping ------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mask_bookkeeping_sequence():
    """one fresh context, no host sync between the calls: bitmap calls of a large range, a small one, a
    larger one (both mask buffers regrow) and the same again, a radix call and a wave-form step in
    between — pkm_cur / pkm_zero_ptr / pkm_zero_nb must leave every call's masks zero where it marks,
    or a stale bit shifts its ranks.  Each call's outputs equal its own reference after one sync."""
    from kart_amd.engine import Engine

    with Engine(0) as eng:
        eng.set_option("step_overlap_min", 0)
        calls = []
        for form, case in BOOK:
            if form == "step":
                calls.append((form, _StepRun(eng, case, OC.materialise_step(case))))
            else:
                calls.append((form, _PkCall(eng, case, OC.materialise(case))))
        eng.sync()
        for i, (form, call) in enumerate(calls):
            if form == "step":
                eng.set_option("pkm_wave", 1)
                call.step()
            else:
                eng.set_option("pkm_max_blocks", 0 if form == "radix" else OC.PKM_MAX_BLOCKS)
                call.run(keys=bool(i & 1))
        eng.sync()
        for form, call in calls:
            if form == "step":
                call.check(call.download())
            else:
                call.check()
        del calls, call
