"""-m gpu: the join tile's work out of LDS under the j2_walk option — the guided split search (a
verified bracket of half-width W around the proportional guess, the blind search when a wave's
bracket fails), the unguarded walk of full waves, and k_join2's straight-line complete order
check — against the oracle, bit for bit: records, counts and both key lists.
Every case runs with j2_walk 0 and 1 and with the OIDs read from HBM and from LDS."""
import numpy as np
import pytest

from oracle import oracle as O

from kart_amd import _native as N
from test_gpu_place2_updates import _Run, _case, _check, _options, _sides

pytestmark = pytest.mark.gpu

W = 8        # KD_J2_GW: the bracket is [g - W, g + W - 1]
TILE = 1024  # items of a tile; a thread walks 4, a wave 256
S = 10000    # spacing of the shared keys: room for a run of one-sided keys between two of them
CONFIGS = [(walk, oidlds) for walk in (0, 1) for oidlds in (0, 1 << 26)]


def _mk(ka, kb, upd_every=3, seed=11):
    """two int-key sides over the given ascending keys; shared keys carry equal OIDs except every
    upd_every-th (by key), which is an update"""
    from kart_amd import packing

    rng = np.random.default_rng(seed)
    ka, kb = np.asarray(ka, np.uint64), np.asarray(kb, np.uint64)
    A = packing.PackedSide(ka, rng.integers(0, 256, size=(ka.size, 20), dtype=np.uint8), 0, np.arange(ka.size))
    B = packing.PackedSide(kb, rng.integers(0, 256, size=(kb.size, 20), dtype=np.uint8), 0, np.arange(kb.size))
    _, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    eq = (ka[ia] // np.uint64(S)) % np.uint64(upd_every) != 0
    B.oid[ib[eq]] = A.oid[ia[eq]]
    return A, B


def _both_ways(engine, request, A, B, orders=False):
    for walk, oidlds in CONFIGS:
        _options(engine, request, j2_walk=walk, j2_oidlds_min=oidlds)
        _check(_Run(engine, A, B, orders=orders), A, B)


def _drift(A, B):
    """per tile, per thread: the merge-path split of the thread's diagonal (ties: A first) minus the
    proportional guess round(dd * na / (na + nb)) — what the bracket has to hold"""
    keys = np.concatenate([A.key, B.key])
    side = np.concatenate([np.zeros(A.n, np.int64), np.ones(B.n, np.int64)])
    cum = np.concatenate([[0], np.cumsum(side[np.lexsort((side, keys))] == 0)])
    out = []
    for d0 in range(0, A.n + B.n, TILE):
        n = min(TILE, A.n + B.n - d0)
        dd = np.minimum(np.arange(TILE // 4) * 4, n)
        out.append((cum[d0 + dd] - cum[d0]) - np.floor(dd * (cum[d0 + n] - cum[d0]) / n + 0.5))
    return out


def _with_run(shared, at, k, in_target):
    """shared keys S * i on both sides and k consecutive keys more on one side just before shared key `at`"""
    s = S * np.arange(shared, dtype=np.int64)
    side = np.sort(np.concatenate([s, S * at - k + np.arange(k)]))
    return (s, side) if in_target else (side, s)


RUNS = [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 2 * W + 2, 2 * W + 4, 4 * W]


@pytest.mark.parametrize("in_target", [True, False], ids=["inserts", "deletes"])
def test_gpu_bracket_edges(engine, request, in_target):
    """a run of k one-sided keys just before a thread's diagonal, early in a tile (wave 0), in wave 1
    and late in the tile: a split drifts from its guess by about k / 2 just after the run and less
    further on, so over the k's some lanes lie inside, on and outside the bracket's edge, and some
    waves hold passing and failing lanes together"""
    seen, mixed = set(), False
    for k in RUNS:
        for t0 in (12, 70, 200):
            A, B = _mk(*_with_run(1500, 2 * t0, k, in_target))
            for d in _drift(A, B):
                seen |= set(d.astype(int).tolist())
                out = (d < -W) | (d > W - 1)
                mixed |= any(out[w:w + 64].any() and not out[w:w + 64].all() for w in range(0, d.size, 64))
            _both_ways(engine, request, A, B)
    edge = {-W - 1, -W, -W + 1} if in_target else {W - 2, W - 1, W}
    assert edge <= seen and mixed, "the cases no longer reach the bracket's edge"


@pytest.mark.parametrize("in_target", [True, False], ids=["inserts", "deletes"])
def test_gpu_far_off_guess(engine, request, in_target):
    """3,000 consecutive one-sided keys in the middle of 6,000 shared ones: tiles with na = 0 or
    nb = 0, and around them tiles whose splits lie far from the guess"""
    s, side = _with_run(6000, 3000, 3000, True)
    A, B = _mk(s, side) if in_target else _mk(side, s)
    _both_ways(engine, request, A, B)


@pytest.mark.parametrize("case", ["both_empty", "base_empty", "target_empty", "one_equal", "one_differs", "negative",
                                  "wraps"])
def test_gpu_walk_tiny_and_wrapping(engine, request, case):
    """empty and one-entry sides; negative and wrap-crossing pks"""
    A, B = _sides(*_case(case))
    _both_ways(engine, request, A, B)


@pytest.mark.parametrize("first", ["insert", "delete"])
def test_gpu_walk_ties_straddle(engine, request, first):
    """one one-sided key ahead of 1,500 shared ones: every matched pair lies on items (2i + 1, 2i + 2)
    and so straddles each thread boundary (items 4t - 1 | 4t), the wave boundary at item 256 and the
    tile boundary at item 1024, where the lookahead entry completes the pair"""
    s = S * np.arange(1, 1501, dtype=np.int64)
    one = np.concatenate([[1], s])
    A, B = _mk(s, one, upd_every=2) if first == "insert" else _mk(one, s, upd_every=2)
    _both_ways(engine, request, A, B)


@pytest.mark.parametrize("rem", [1, 3, 4, 5, 255, 257, 1023])
def test_gpu_walk_partial_last_tile(engine, request, rem):
    """(nA + nB) mod 1024 = rem: the guarded walk of the last wave and the order check's ragged end"""
    e = 2 + rem % 2
    m = (TILE + rem - e) // 2
    s = S * np.arange(m, dtype=np.int64)
    extra = np.array([5, S * (m // 2) + 5, S * m + 5][:e], np.int64)
    A, B = _mk(s, np.sort(np.concatenate([s, extra])))
    assert (A.n + B.n) % TILE == rem
    _both_ways(engine, request, A, B)
    _both_ways(engine, request, B, A)


def test_gpu_walk_through_orders(engine, request):
    """the late-materialised join (identity orders) takes the same search and walk"""
    A, B = _mk(*_with_run(1500, 140, 2 * W + 2, True))
    _both_ways(engine, request, A, B, orders=True)


def test_gpu_walk_hash_keys(engine, request):
    """hash keys with filenames: the two-way join and the three-way join (which shares the tile's
    search and walk) against the oracle under both settings"""
    from test_gpu_parity import _hash_sides

    rng = np.random.default_rng(3)
    keys, names, oids, side = _hash_sides(rng, 3000, [24])
    m = keys.size
    selA, selO, selT = (rng.random(m) > 0.1 for _ in range(3))
    oO = oids.copy(); oO[rng.random(m) < 0.1, 0] ^= 1
    oT = oids.copy(); oT[rng.random(m) < 0.1, 1] ^= 1
    A, O_, T = side(selA, oids, names), side(selO, oO, names), side(selT, oT, names)
    od, _ = O.classify2(A.key, A.oid, O_.key, O_.oid)
    oc, om, ocl = O.classify3(A.key, A.oid, O_.key, O_.oid, T.key, T.oid)
    for walk in (0, 1):
        _options(engine, request, j2_walk=walk)
        assert np.array_equal(engine.diff2(A, O_).delta, od)
        r3 = engine.merge3(A, O_, T)
        assert np.array_equal(np.asarray(r3.conflict).reshape(-1, 3), oc.reshape(-1, 3))
        assert np.array_equal(np.asarray(r3.mdelta).reshape(-1, 2), om.reshape(-1, 2)) and r3.n_clean == ocl


def _tile_split(ka, kb, d):
    """the merge-path split of diagonal d (ties: A first) by its definition, and whether the predicate
    is monotone there (one crossing), so that any search finds the same split"""
    lo, hi = max(d - kb.size, 0), min(d, ka.size)
    p = np.array([ka[i] > kb[d - 1 - i] for i in range(lo, hi)] + [True])
    return lo + int(np.argmax(p)), bool((np.diff(p.astype(int)) >= 0).all())


@pytest.mark.parametrize("kind", ["equal", "descending"])
@pytest.mark.parametrize("in_target", [False, True], ids=["base", "target"])
def test_gpu_walk_rejects_unsorted(engine, request, kind, in_target):
    """one adjacent pair of one side equal or descending — inside a thread's run of the order check
    (key 41), at a run boundary (40), at a wave boundary (256), as the first key of the second tile
    against its lookbehind key (512), as a side's last entry — is rejected under every setting.  The
    other side holds 512 keys below and 988 above all of the faulty side's, so tile 0 is those 512
    and the faulty side's first 512 whatever the pair at 511 | 512 looks like: asserted from the split"""
    from kart_amd import packing

    n = 1500
    other = np.concatenate([1 + np.arange(512), (1 << 40) + np.arange(n - 512)]).astype(np.uint64)
    for x in (40, 41, 256, 512, n - 1):
        bad = (1 << 20) + 10 * np.arange(n, dtype=np.uint64)
        bad[x] = bad[x - 1] - np.uint64(0 if kind == "equal" else 1)
        ka, kb = (other, bad) if in_target else (bad, other)
        i0, monotone = _tile_split(ka, kb, TILE)
        assert monotone and (i0, TILE - i0) == (512, 512)  # key 512 of either side is tile 1's first
        oid = np.zeros((n, 20), np.uint8)
        A, B = (packing.PackedSide(v, oid, 0, np.arange(n)) for v in (ka, kb))
        for walk, oidlds in CONFIGS:
            _options(engine, request, j2_walk=walk, j2_oidlds_min=oidlds)
            with pytest.raises(N.Unsupported):
                engine.diff2(A, B)


def _walk_alone_rejects(ka, kb):
    """host model of one tile's (the whole input's, na + nb <= 1024) guided split search and walk
    with the walk's own order compares only: True if they flag the input"""
    na, nb, n = ka.size, kb.size, ka.size + kb.size
    A = lambda i: int(ka[i]) if 0 <= i < na else 0
    B = lambda j: int(kb[j]) if 0 <= j < nb else 0

    def rounds(r, dd, lo, hi):
        for _ in range(r):
            w = hi - lo
            s = (w + 3) >> 2
            p1, p2, p3 = lo + s - 1, lo + 2 * s - 1, lo + 3 * s - 1
            hm = hi - 1 if w > 0 else lo
            q1, q2, q3 = max(p1, lo), min(p2, hm), min(p3, hm)
            b1 = A(q1) > B(dd - 1 - q1)
            b2 = p2 >= hi or A(q2) > B(dd - 1 - q2)
            b3 = p3 >= hi or A(q3) > B(dd - 1 - q3)
            nlo, nhi = p3 + 1, hi
            if b3: nlo, nhi = p2 + 1, min(p3, hi)
            if b2: nlo, nhi = p1 + 1, min(p2, hi)
            if b1: nlo, nhi = lo, p1
            if w > 0: lo, hi = nlo, nhi
        return lo

    flagged = False
    for wave in range(4):
        lanes = []
        for t in range(64 * wave, 64 * wave + 64):
            dd = min(4 * t, n)
            lo, hi = max(dd - nb, 0), min(dd, na)
            g = min(max(dd * na // n if (2 * dd * na) % (2 * n) < n else dd * na // n + 1, lo), hi)  # round half up
            L, H = max(g - W, lo), min(g + W - 1, hi)
            hm = hi - 1 if hi > lo else lo
            xl, xh = (L - 1 if L > lo else lo), min(H, hm)
            ok = (L <= lo or not A(xl) > B(dd - 1 - xl)) and (H >= hi or A(xh) > B(dd - 1 - xh))
            lanes.append((dd, lo, hi, L, H, ok))
        guided = all(l[5] for l in lanes)
        for dd, lo, hi, L, H, _ in lanes:
            ia = rounds(2, dd, L, H) if guided else rounds(5, dd, lo, hi)
            jb = dd - ia
            ap_ok, bp_ok, ap, bp = ia > 0, jb > 0, A(ia - 1), B(jb - 1)
            for _ in range(min(dd + 4, n) - dd):
                ka_, kb_ = A(min(ia, max(na - 1, 0))), B(min(jb, max(nb - 1, 0)))
                ta = jb >= nb or (ia < na and ka_ <= kb_)
                flagged |= (ap_ok and ap >= ka_) if ta else (bp_ok and bp >= kb_)
                if ta: ap, ap_ok, ia = ka_, True, ia + 1
                else: bp, bp_ok, jb = kb_, True, jb + 1
    return flagged


def test_gpu_complete_check_catches_what_the_walk_skips(engine, request):
    """one key of the base displaced far upwards: the thread that meets it takes target keys for the
    rest of its items, the next thread's split lies past its successor, and so the walk consumes
    neither key of the descending pair behind it (the host model of search + walk does not flag the
    input).  Only the complete order check rejects it: the straight-line one under j2_walk = 1,
    the loops under 0, with the OIDs in LDS (k_join2's large-join form) and from HBM"""
    from kart_amd import packing

    n, p = 400, 100
    k = 10 * np.arange(n, dtype=np.uint64)
    bad = k.copy()
    bad[p] = np.uint64(1 << 40)
    assert not _walk_alone_rejects(bad, k), "the walk alone now rejects this input: the case no longer isolates the check"
    assert _walk_alone_rejects(np.concatenate([k[:p], k[p - 1:-1]]), k)  # (the model does see a pair the walk consumes)
    oid = np.zeros((n, 20), np.uint8)
    A, B = (packing.PackedSide(v, oid, 0, np.arange(n)) for v in (bad, k))
    for walk, oidlds in CONFIGS:
        _options(engine, request, j2_walk=walk, j2_oidlds_min=oidlds)
        with pytest.raises(N.Unsupported):
            engine.diff2(A, B)
