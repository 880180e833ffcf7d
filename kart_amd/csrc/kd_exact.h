// kd_exact.h — the exact sign of the orientation determinant of three points given as doubles,
// shared by the host (kd_orient2d_exact_batch) and the device (kd_georefine.hip's exact kernels).
//
// det = (ax-cx)(by-cy) - (ay-cy)(bx-cx) expands over the raw coordinates (cx*cy cancels) to
//   ax*by - ax*cy - cx*by - ay*bx + ay*cx + cy*bx.
// A double is a rational, so det is one; its sign is taken without rounding by floating-point
// expansion arithmetic (Shewchuk, "Adaptive Precision Floating-Point Arithmetic and Fast Robust
// Geometric Predicates", 1997): each product as p + e with p = fl(x*y) and e = fma(x, y, -p), the
// twelve components summed into a non-overlapping expansion with the error-free two_sum
// (Grow-Expansion, Theorem 10), whose most significant non-zero component carries the sign.  The
// library is built with -ffp-contract=off: the one fused operation is the explicit fma.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KD_XHD __host__ __device__ inline
#else
#define KD_XHD inline
#endif

namespace kd {

constexpr int KD_ORIENT_RANGE = 2;  // kd_orient2d_exact: an operand outside the range guard

// s + e = a + b exactly (Knuth; no assumption about the magnitudes)
KD_XHD void x_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// p + e = a * b exactly, given that neither p overflows nor e underflows (the range guard)
KD_XHD void x_two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    e = __builtin_fma(a, b, -p);
}

// The range guard.  A non-zero coordinate v = m * 2^(E-52) (m an integer below 2^53, 2^E <= |v|).
//   Low end: x*y is an integer multiple of 2^(Ex+Ey-104), and so is the rounding error e of
//   two_prod; e is a double (and the fma returns it) only if that unit is no smaller than the
//   smallest subnormal 2^-1074: Ex + Ey >= -970, which holds for every pair when E >= -485.
//   (Sums never underflow: two_sum's operations are exact or round to a representable multiple of
//   the same unit.)
//   High end: with |v| < 2^510 a product is below 2^1020, and every partial sum the expansion
//   forms is bounded by the sum of the six products' magnitudes, below 6 * 2^1020 < 2^1023: nothing
//   overflows.
// So a coordinate is admissible when it is zero or 2^-485 <= |v| < 2^510; degrees and projected
// metres lie hundreds of binades inside.  NaN and infinities fail the comparison.
KD_XHD bool x_in_range(double v) {
    const double m = fabs(v);
    return m == 0.0 || (m >= 0x1p-485 && m < 0x1p510);
}

// sign of det((a - c), (b - c)) over the raw coordinates: -1, 0, +1, or KD_ORIENT_RANGE when a
// coordinate is outside the guard (the caller then cannot tell)
KD_XHD int kd_orient2d_exact(double ax, double ay, double bx, double by, double cx, double cy) {
    if (!(x_in_range(ax) && x_in_range(ay) && x_in_range(bx) && x_in_range(by) && x_in_range(cx) && x_in_range(cy)))
        return KD_ORIENT_RANGE;
    double h[12];
    x_two_prod(ax, by, h[1], h[0]);
    x_two_prod(-ax, cy, h[3], h[2]);
    x_two_prod(-cx, by, h[5], h[4]);
    x_two_prod(-ay, bx, h[7], h[6]);
    x_two_prod(ay, cx, h[9], h[8]);
    x_two_prod(cy, bx, h[11], h[10]);
    // Grow-Expansion, component by component: h[0..m) is a non-overlapping expansion (zeros
    // allowed), h[m] joins it
#pragma unroll
    for (int m = 1; m < 12; m++) {
        double q = h[m];
#pragma unroll
        for (int i = 0; i < m; i++) x_two_sum(q, h[i], q, h[i]);
        h[m] = q;
    }
#pragma unroll
    for (int i = 11; i >= 0; i--)
        if (h[i] != 0.0) return h[i] > 0.0 ? 1 : -1;
    return 0;
}

}  // namespace kd
