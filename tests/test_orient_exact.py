"""kd_orient2d_exact_batch: the exact sign of the orientation determinant (kd_exact.h, the predicate
behind KD_GF_EXACT) on the host, held against refine_exact.orient (Fractions) on ~100k triples: zero
determinants on a lattice, heavy cancellation at projected-metre magnitudes, near misses the FP64
static bound cannot certify, random doubles over 400 binades, and both sides of the range guard."""
import math

import numpy as np
import pytest

import refine_exact as X
from kart_amd import _native as N

LO, HI = 2.0 ** -485, 2.0 ** 510  # the guard: a non-zero coordinate v is admissible when LO <= |v| < HI


def exact_batch(abc):
    abc = np.ascontiguousarray(abc, np.float64).reshape(-1, 6)
    out = np.full(abc.shape[0], 99, np.int8)
    N.check(N.lib().kd_orient2d_exact_batch(N.ptr(abc), abc.shape[0], N.ptr(out)), "kd_orient2d_exact_batch")
    return out


def fractions(abc):
    return np.array([X.orient(t[0:2], t[2:4], t[4:6]) for t in np.asarray(abc, np.float64).reshape(-1, 6)], np.int8)


def static_filter_certifies(abc):
    """the FP64 bound of kd_georefine.hip's gr_orient, evaluated the same way (numpy does not fuse)"""
    ax, ay, bx, by, cx, cy = np.asarray(abc, np.float64).reshape(-1, 6).T
    eps = 2.0 ** -53
    t1, t2 = (ax - cx) * (by - cy), (ay - cy) * (bx - cx)
    s = np.abs(t1) + np.abs(t2)
    return (s >= 1e-290) & np.isfinite(s) & (np.abs(t1 - t2) > (3.0 + 16.0 * eps) * eps * s)


def lattice(rng, n):
    """n triples of small-integer points: half of them random in [0, 12]^2, half three points of one
    lattice line through such a point (coordinates in [-12, 24])"""
    rnd = rng.integers(0, 13, (n // 2, 6))
    a = rng.integers(0, 13, (n - n // 2, 2))
    d = rng.integers(-3, 4, (n - n // 2, 2))
    k = rng.integers(-4, 5, (n - n // 2, 2))
    col = np.concatenate([a, a + d * k[:, :1], a + d * k[:, 1:]], 1)
    return np.concatenate([rnd, col]).astype(np.float64)


def test_binding_and_header_list_the_exact_entry():
    assert "kd_orient2d_exact_batch" in N.SIGNATURES and hasattr(N.lib(), "kd_orient2d_exact_batch")
    assert N.KD_GF_EXACT == 0x4 and N.KD_GF_EXACT & (N.KD_GF_RECT | N.KD_GF_DELTA_HEADS) == 0
    assert exact_batch(np.zeros((0, 6))).shape == (0,)
    assert exact_batch([[0, 0, 1, 0, 0, 1], [0, 0, 0, 1, 1, 0], [0, 0, 1, 1, 2, 2]]).tolist() == [1, -1, 0]


@pytest.mark.parametrize("scaled", [False, True])
def test_lattice_zero_determinants(scaled):
    """small-integer lattice points, and the same lattice scaled by 2^-10 and shifted to
    (1570000.25, 5180000.5) (still exactly representable): at least a quarter of the determinants
    are exactly zero, and every sign equals the Fractions'"""
    abc = lattice(np.random.default_rng(20261020), 30000)
    if scaled:
        abc = abc * 2.0 ** -10 + np.array([1570000.25, 5180000.5] * 3)
    z0 = X.ZEROS[0]
    want = fractions(abc)
    zeros = X.ZEROS[0] - z0
    assert zeros * 4 >= abc.shape[0] and zeros == int((want == 0).sum())
    got = exact_batch(abc)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert (want == 1).sum() > 3000 and (want == -1).sum() > 3000


def test_one_ulp_off_a_line():
    """c = a + t (b - a) with a = p + L d, b = p - M d and p, d, L, M of few bits, so that c = p is on
    the line exactly; then c.x or c.y moves by one ulp of a coordinate ~2^-10 while |a - c| ~ 1: the
    determinant (~2^-62) is far inside the static bound (~2^-52), and it is not zero"""
    rng = np.random.default_rng(7)
    n = 20000
    p = rng.integers(-2048, 2049, (n, 2)) * 2.0 ** -21
    p[p == 0] = 2.0 ** -21
    d = rng.integers(1, 64, (n, 2)) / 64.0 * rng.choice([-1.0, 1.0], (n, 2))
    L, M = rng.integers(1, 5, (n, 1)) / 2.0, rng.integers(1, 5, (n, 1)) / 2.0
    a, b = p + L * d, p - M * d
    c = p.copy()
    which = rng.integers(0, 2, n)
    up = rng.integers(0, 2, n).astype(bool)
    moved = np.nextafter(c[np.arange(n), which], np.where(up, np.inf, -np.inf))
    on_line = np.concatenate([a, b, c], 1)
    c[np.arange(n), which] = moved
    abc = np.concatenate([a, b, c], 1)
    assert (fractions(on_line[:500]) == 0).all()  # (the construction is exact)
    want = fractions(abc)
    assert (want != 0).all()
    assert static_filter_certifies(abc).mean() < 0.01
    got = exact_batch(abc)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_random_doubles_over_400_binades():
    rng = np.random.default_rng(11)
    n = 20000
    abc = rng.uniform(1.0, 2.0, (n, 6)) * 2.0 ** rng.integers(-200, 201, (n, 6)) * rng.choice([-1.0, 1.0], (n, 6))
    # a share with one common exponent per triple, where the terms compete
    abc[: n // 2] = rng.uniform(-1.0, 1.0, (n // 2, 6)) * 2.0 ** rng.integers(-200, 201, (n // 2, 1))
    got = exact_batch(abc)
    assert np.array_equal(got, fractions(abc))
    assert set(got.tolist()) == {-1, 1}


def test_range_guard():
    """a non-zero coordinate is admissible when 2^-485 <= |v| < 2^510: just inside the sign is the
    Fractions', just outside (and for subnormals, infinities and NaN) the answer is 2"""
    rng = np.random.default_rng(3)
    base = np.array([1.5, -2.25, 3.0, 0.5, -0.75, 1.25])
    inside = [LO, math.nextafter(HI, 0.0)]
    outside = [math.nextafter(LO, 0.0), HI, 5e-324, 1e-310, 1e-200, 1e200, 1e300, math.inf, math.nan]
    ins, outs = [], []
    for pos in range(6):
        for sign in (1.0, -1.0):
            for v, dst in [(v, ins) for v in inside] + [(v, outs) for v in outside]:
                t = base.copy()
                t[pos] = sign * v
                dst.append(t)
    # every operand at an end of the window: random mantissas, and lattices (zero determinants) there
    lat = lattice(rng, 2000)
    ins = np.concatenate([np.array(ins), rng.uniform(1.0, 2.0, (2000, 6)) * LO * rng.choice([-1.0, 1.0], (2000, 6)),
                          rng.uniform(0.5, 1.0, (2000, 6)) * math.nextafter(HI, 0.0) * rng.choice([-1.0, 1.0], (2000, 6)),
                          lat * LO, lat * 2.0 ** 505, np.zeros((1, 6))])
    assert ((np.abs(ins) >= LO) | (ins == 0)).all() and (np.abs(ins) < HI).all()
    want = fractions(ins)
    got = exact_batch(ins)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert (want == 0).sum() > 500
    assert exact_batch(np.array(outs)).tolist() == [2] * len(outs)
