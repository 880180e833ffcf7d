// kd_georefine.hip — the exact stage of the spatially filtered diff: for every side kd_geom_filter left
// 1 CANDIDATE (its envelope overlaps the filter's), the WKB behind the GPKG header is decoded from the
// blob arena and Intersects(feature, filter polygon) decided where FP64 can prove the answer.
//
// Reference (file:line under /root/reference):
//   SpatialFilter.matches .................. kart/spatial_filter/__init__.py:534-590 (the prepared
//       filter geometry's Intersects after the envelope check)
//   the filter geometry is a POLYGON or MULTIPOLYGON . kart/spatial_filter/__init__.py:261
//
// Filter region: the even-odd interior of all its rings, boundary included.  Intersects(F, P) holds
// when (a) a vertex of F lies in P, (b) a segment of F meets a boundary segment of P, or (c) F is
// areal and the first vertex of a ring of P lies in F.  Everything reduces to exact comparisons of
// doubles and the sign of det = (ax-cx)(by-cy) - (ay-cy)(bx-cx), which counts only when
// |det| > (3 + 16 eps) eps (|(ax-cx)(by-cy)| + |(ay-cy)(bx-cx)|), eps = 2^-53 (Shewchuk's static
// bound; the library is built with -ffp-contract=off).  A witness gives 2 MATCHING; no witness and
// nothing undecided 0 NON_MATCHING; anything else — every touching configuration among them — stays
// 1 CANDIDATE (unless KD_GF_EXACT is set, below).  Unsupported or malformed WKB (type >= 7, EWKB flags, counts past the value, a
// non-finite coordinate) stays 1 as well.  No byte outside the GPKG value is read.
//
// Kernels: k_gr_list sorts the candidate sides into two work lists by their WKB type (each block
// into slots of its own, the blocks' counts scanned afterwards: no contended atomic anywhere);
// k_gr_points takes points and small multipoints, one lane per side, the filter's edges read
// wave-uniformly from LDS tiles; k_gr_wave takes everything else, one wave per side: the side's
// vertices are fetched 64 at a time (lane i the i-th 16-B coordinate pair) into LDS, the lanes spread
// over the filter edges of a tile or over the chunk's segments, whichever has more, and a filter
// edge whose box misses the feature's envelope is skipped before any determinant.  The kept list is
// then rebuilt from the codes (gf_rekeep).
//
// KD_GF_EXACT adds a second pass between the workers and the statistics.  k_gr_points and k_gr_wave
// are the EXACT = false instantiations of the two worker templates and run as without the flag;
// k_gr_relist then lists the sides whose code is still 1, and k_gr_points_x / k_gr_wave_x — the
// EXACT = true instantiations: same walkers, tiles and chunking — decide them with the determinant's
// exact sign (kd_exact.h) wherever the static bound fails, so that a touching configuration becomes a
// witness and only an operand outside that header's range guard leaves a side 1.  Their list may be
// empty: they read its device-side count and return.
#include <algorithm>
#include <cmath>

#include "kd_exact.h"
#include "kd_geom.h"

namespace kd {

constexpr int GR_TILE = 128;  // filter edges per LDS tile (4 x 8 B each: 4 KB, so LDS does not bound k_gr_wave's residency)
constexpr int GR_LB = 4096;   // deltas per k_gr_list block: its sides' slots in the work list are its own
constexpr int GR_CH = 63;     // feature segments per chunk (64 vertices)
constexpr u32 GR_MAXPT = 64;  // most points of a multipoint k_gr_points takes (one mask bit each)

struct GrArgs {
    const kd_geom_head* head[2];
    u64 nhead[2];
    int dense;  // heads in delta order (KD_GF_DELTA_HEADS): side s of delta d at head[s][d]
    const u8* data[2];
    const u64* off[2];
    u64 nblob[2];
    const uint2* pairs;
    u64 cap;
    const u64* d_n;
    u8* match;
    // the filter: edges as four arrays of nep doubles (ax, ay, bx, by), then the rings' first
    // vertices (qx [nr], qy [nr])
    const double* fe;
    u32 ne, nep, nr;
    double f0, f1, f2, f3;  // its envelope (min-x, max-x, min-y, max-y)
    // the work list: k_gr_list's block b owns slots [2 * GR_LB * b, 2 * GR_LB * (b + 1)) — its point
    // sides from the front, its wave sides from the back — so no list position is taken by a global
    // atomic (15,000 candidates among 2M deltas: one contended counter cost 170 us).  bcnt [2 * nblk]:
    // the blocks' point counts, then their wave counts; scanned in place (exclusive, the total in
    // *tot) before the workers run, which find a work item's block by bisection
    u32* list;
    u32* bcnt;
    const u64* tot;
    u32 nblk;
    // outcome counts per block of k_gr_list, k_gr_points and k_gr_wave (4 each, in that order of
    // kernels): summed into stats by k_gr_stats, again without contended atomics
    u32* part;
    u32 np_list, np_pts, np_wave;
    unsigned long long* stats;  // [4]: decided true, decided false, undecided, unsupported
};

// work item i of a list (pre: the scanned counts of its nblk blocks, off: what the scan counted in
// front of the list) -> the block that holds it and its rank there
__device__ __forceinline__ void gr_item(const u32* pre, u32 nblk, u32 off, u32 i, u32& blk, u32& rank) {
    u32 lo = 0, hi = nblk;  // the last block with pre[b] - off <= i
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (pre[mid] - off <= i) lo = mid;
        else hi = mid;
    }
    blk = lo;
    rank = i - (pre[lo] - off);
}

// ---- certified predicates ----
// EXACT = false: FP64 behind Shewchuk's static bound, "cannot tell" where it fails (the fast
// kernels).  EXACT = true: the same bound first — whatever it certifies gets the same answer — and
// the exact sign from kd_exact.h where it fails; "cannot tell" is then left to operands outside that
// header's range guard.
constexpr int GR_UNK = KD_ORIENT_RANGE;  // gr_orient<true>: cannot tell

// sign of det((a - c), (b - c)).  EXACT = false: +1 / -1 when certain, 0 when not.  EXACT = true:
// +1 / -1 / 0 all certain, GR_UNK when not
template <bool EXACT>
__device__ __forceinline__ int gr_orient(double ax, double ay, double bx, double by, double cx, double cy) {
    constexpr double eps = 1.1102230246251565e-16;  // 2^-53
    constexpr double K = (3.0 + 16.0 * eps) * eps;
    const double t1 = (ax - cx) * (by - cy), t2 = (ay - cy) * (bx - cx);
    const double det = t1 - t2, s = fabs(t1) + fabs(t2);
    if constexpr (!EXACT) {
        if (!(s >= 1e-290 && s < __builtin_huge_val())) return 0;  // tiny, overflowed or NaN
        if (!(fabs(det) > K * s)) return 0;
        return det > 0 ? 1 : -1;
    } else {
        if (s >= 1e-290 && s < __builtin_huge_val() && fabs(det) > K * s) return det > 0 ? 1 : -1;
        return kd_orient2d_exact(ax, ay, bx, by, cx, cy);
    }
}

// one edge (a, b) of a region's boundary against the point (x, y): crossing parity of the ray to
// the right (par), "cannot tell" (und) and, EXACT only, "on the edge" (on: a witness).
// (a.y > y) != (b.y > y) is exact; a point equal to an end of the edge, on a horizontal edge's span
// or (EXACT) with an exact-zero orientation inside the edge's y-range is on the boundary:
// undecided without EXACT, `on` with it.  The three cases cover every point of the edge, so where no
// edge reports `on` the point is on none and the half-open parity is right.
template <bool EXACT>
__device__ __forceinline__ void gr_pt_edge(double ax, double ay, double bx, double by, double x, double y, u32& par,
                                           u32& und, u32& on) {
    if ((ax == x && ay == y) || (bx == x && by == y)) { (EXACT ? on : und) = 1; return; }
    const bool ua = ay > y, ub = by > y;
    if (ua != ub) {
        if (fmax(ax, bx) < x) return;              // wholly to the left: no crossing
        if (fmin(ax, bx) > x) { par ^= 1; return; }  // wholly to the right: one crossing
        const int o = gr_orient<EXACT>(ax, ay, bx, by, x, y);
        if constexpr (EXACT) {
            if (o == GR_UNK) und = 1;
            else if (o == 0) on = 1;
            else par ^= (u32)((o > 0) == ub);
        } else {
            if (o == 0) und = 1;
            else par ^= (u32)((o > 0) == ub);  // an upward edge is crossed when the point is to its left
        }
    } else if (ay == y && by == y && x >= fmin(ax, bx) && x <= fmax(ax, bx)) {
        (EXACT ? on : und) = 1;
    }
}

// segments (a, b) and (c, d): 0 they do not meet, 2 they meet (EXACT = false: cross properly),
// 1 cannot tell.  EXACT: with the closed boxes overlapping, o1 * o2 <= 0 and o3 * o4 <= 0 means
// they share a point — collinear segments whose boxes overlap do, an end on the other's line
// between its ends does — so 1 is left to an operand out of range.
template <bool EXACT>
__device__ __forceinline__ int gr_seg(double ax, double ay, double bx, double by, double cx, double cy, double dx,
                                      double dy) {
    if (fmax(ax, bx) < fmin(cx, dx) || fmax(cx, dx) < fmin(ax, bx) || fmax(ay, by) < fmin(cy, dy) ||
        fmax(cy, dy) < fmin(ay, by))
        return 0;
    if constexpr (!EXACT) {
        const int o1 = gr_orient<false>(ax, ay, bx, by, cx, cy), o2 = gr_orient<false>(ax, ay, bx, by, dx, dy);
        if (o1 && o1 == o2) return 0;
        const int o3 = gr_orient<false>(cx, cy, dx, dy, ax, ay), o4 = gr_orient<false>(cx, cy, dx, dy, bx, by);
        if (o3 && o3 == o4) return 0;
        return (o1 && o2 && o3 && o4) ? 2 : 1;
    } else {
        // (one call site for the four signs: the expansion code is long)
        int o[2] = {0, 0};
        bool unk = false;
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            const double px = k ? cx : ax, py = k ? cy : ay, qx = k ? dx : bx, qy = k ? dy : by;
            int prod = 1;
#pragma unroll 1
            for (int j = 0; j < 2; j++) {
                const double rx = k ? (j ? bx : ax) : (j ? dx : cx), ry = k ? (j ? by : ay) : (j ? dy : cy);
                const int v = gr_orient<true>(px, py, qx, qy, rx, ry);
                if (v == GR_UNK) { unk = true; prod = 0; }
                else prod *= v;
            }
            o[k] = prod;  // o1 * o2, then o3 * o4 (0 with an unknown among them)
        }
        if (o[0] > 0 || o[1] > 0) return 0;  // (both signs certain, equal and non-zero)
        return unk ? 1 : 2;
    }
}

// ---- locating and walking the WKB ----
// the WKB of side s of delta d (behind the GPKG header): 1 found, 0 a side the refine leaves alone
// (absent, no geometry head), -1 unsupported (out of range, malformed GPKG header)
__device__ __forceinline__ int gr_locate(const GrArgs& a, u64 d, int s, const u8*& w, u32& wlen) {
    const uint2 pr = a.pairs[d];
    const u32 bi = s ? pr.y : pr.x;
    if (bi == KD_NONE) return 0;
    const u64 hi = a.dense ? d : (u64)bi;
    if (hi >= a.nhead[s] || (u64)bi >= a.nblob[s]) return -1;
    const kd_geom_head* h = a.head[s] + hi;
    const u32 glen = h->glen, gs = h->goff_status;
    if ((gs >> 24) != KD_GH_GEOM) return 0;
    const u64 o = a.off[s][bi], e = a.off[s][bi + 1];
    const u64 goff = gs & 0xFFFFFFu;
    if (e < o || goff + glen > e - o) return -1;
    const u8* g = a.data[s] + o + goff;
    if (glen < 8 || g[0] != 'G' || g[1] != 'P' || g[2] != 0) return -1;
    const u8 f = g[3];
    const int et = (f >> 1) & 7;
    if ((f & 0x20) || et > 4) return -1;
    const u32 hs = 8 + (u32)env_size(et);
    if (glen < hs) return -1;
    w = g + hs;
    wlen = glen - hs;
    return 1;
}

// ISO WKB type -> base type 1..6 and the coordinate stride (XY 16, Z / M 24, ZM 32); anything else
// (type 7 and above, EWKB flag bits) is refused
__device__ __forceinline__ bool gr_type(u32 t, u32& base, u32& stride) {
    const u32 dim = t / 1000;
    base = t % 1000;
    if (dim > 3 || base < 1 || base > 6) return false;
    stride = dim == 0 ? 16u : dim == 3 ? 32u : 24u;
    return true;
}

// a run of vertices: a point (kind 0), a linestring (1) or a polygon's ring (2, of polygon `poly`)
struct GrRun {
    u32 off, cnt, stride, kind, poly;
    bool le;
};

// The walk over a geometry's runs in storage order.  W: the walk runs in every lane of a wave on
// the same bytes, its values kept wave-uniform.  Every read is checked against the value's length.
struct GrWalk {
    const u8* w;
    u32 len, p, parts, rings, sub, stride, poly, base;
    bool le, bad;
};

template <bool W>
__device__ __forceinline__ u32 gr_uni(u32 v) {
    if constexpr (W) return (u32)__builtin_amdgcn_readfirstlane((int)v);
    else return v;
}

template <bool W>
__device__ __forceinline__ void gr_walk_init(GrWalk& k, const u8* w, u32 len) {
    k.w = w;
    k.len = len;
    k.p = 0;
    k.parts = k.rings = k.sub = k.stride = k.base = 0;
    k.poly = 0xFFFFFFFFu;
    k.le = false;
    k.bad = true;
    if (len < 5 || w[0] > 1) return;
    const bool le = w[0] == 1;
    u32 base, st;
    if (!gr_type(gr_uni<W>(ld_u32(w + 1, le)), base, st)) return;
    k.base = base;
    if (base <= 3) {  // a single geometry: its header is read again as the one part
        k.parts = 1;
        k.sub = base;
    } else {
        if (len < 9) return;
        k.parts = gr_uni<W>(ld_u32(w + 5, le));
        k.sub = base - 3;
        k.p = 9;
    }
    k.bad = false;
}

// the next run; false at the end, or with k.bad set on malformed input
template <bool W>
__device__ __forceinline__ bool gr_next(GrWalk& k, GrRun& r) {
    for (;;) {
        if (k.rings) {
            if (k.len - k.p < 4) { k.bad = true; return false; }
            const u32 cnt = gr_uni<W>(ld_u32(k.w + k.p, k.le));
            k.p += 4;
            if ((u64)cnt * k.stride > (u64)(k.len - k.p)) { k.bad = true; return false; }
            r.off = k.p; r.cnt = cnt; r.stride = k.stride; r.kind = 2; r.poly = k.poly; r.le = k.le;
            k.p += cnt * k.stride;
            k.rings--;
            return true;
        }
        if (!k.parts) return false;
        k.parts--;
        if (k.len - k.p < 5 || k.w[k.p] > 1) { k.bad = true; return false; }
        k.le = k.w[k.p] == 1;
        u32 base, st;
        if (!gr_type(gr_uni<W>(ld_u32(k.w + k.p + 1, k.le)), base, st) || base != k.sub) { k.bad = true; return false; }
        k.stride = st;
        k.p += 5;
        if (k.sub == 1) {
            if (k.len - k.p < st) { k.bad = true; return false; }
            r.off = k.p; r.cnt = 1; r.stride = st; r.kind = 0; r.poly = 0; r.le = k.le;
            k.p += st;
            return true;
        }
        if (k.len - k.p < 4) { k.bad = true; return false; }
        const u32 cnt = gr_uni<W>(ld_u32(k.w + k.p, k.le));
        k.p += 4;
        if (k.sub == 2) {
            if ((u64)cnt * st > (u64)(k.len - k.p)) { k.bad = true; return false; }
            r.off = k.p; r.cnt = cnt; r.stride = st; r.kind = 1; r.poly = 0; r.le = k.le;
            k.p += cnt * st;
            return true;
        }
        k.rings = cnt;  // a polygon: its rings follow (each checked as it is read)
        k.poly++;
    }
}

__device__ __forceinline__ bool gr_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// ---- the work lists ----
// one lane per delta, GR_LB deltas per block: the sides with code 1 and a geometry head go to the
// block's point slots (points, multipoints of up to GR_MAXPT points) or its wave slots; a side whose
// value cannot be located or whose WKB header is refused is counted unsupported and keeps its 1
__global__ __launch_bounds__(256) void k_gr_list(GrArgs a) {
    __shared__ u32 s_c[4];               // point sides, wave sides, unsupported, candidates
    __shared__ u16 s_cand[2 * GR_LB];    // the block's candidate sides (2 * delta in the block + side)
    const u64 n = a.d_n ? min(*a.d_n, a.cap) : a.cap;
    const int tid = threadIdx.x;
    if (tid < 4) s_c[tid] = 0;
    __syncthreads();
    const u64 t0 = (u64)blockIdx.x * GR_LB;
    u32* const slots = a.list + 2 * t0;
    if (t0 < n) {  // block-uniform
        // the candidates from the codes alone (all loads in flight together), then each candidate's
        // geometry located by a lane of its own: the chain of dependent loads behind a candidate
        // (pair, head, offsets, GPKG header, WKB header) is waited for once per block, not once per round
        u32 mm[GR_LB / 256];
#pragma unroll
        for (int r = 0; r < GR_LB / 256; r++) {
            const u64 d = t0 + (u64)r * 256 + tid;
            mm[r] = d < n ? (u32) * (const u16*)(a.match + 2 * d) : 0u;
        }
#pragma unroll
        for (int r = 0; r < GR_LB / 256; r++) {
            const u32 m = mm[r], x = (u32)(r * 256 + tid) * 2;
            if ((m & 0xff) == 1) s_cand[atomicAdd(&s_c[3], 1u)] = (u16)x;
            if ((m >> 8) == 1) s_cand[atomicAdd(&s_c[3], 1u)] = (u16)(x + 1);
        }
        __syncthreads();
        const u32 nc = s_c[3];
        for (u32 i = tid; i < nc; i += 256) {
            const u32 x = s_cand[i];
            const u64 d = t0 + (x >> 1);
            const int sd = x & 1;
            const u8* w;
            u32 wlen;
            const int rc = gr_locate(a, d, sd, w, wlen);
            int cls = rc < 0 ? 2 : -1;  // 0 point list, 1 wave list, 2 unsupported
            if (rc > 0) {
                cls = 2;
                if (wlen >= 5 && w[0] <= 1) {
                    const bool le = w[0] == 1;
                    u32 base, st;
                    if (gr_type(ld_u32(w + 1, le), base, st))
                        cls = base == 1 || (base == 4 && wlen >= 9 && ld_u32(w + 5, le) <= GR_MAXPT) ? 0 : 1;
                }
            }
            if (cls >= 0) {
                const u32 k = atomicAdd(&s_c[cls], 1u);  // (LDS: the block's own counters)
                if (cls < 2) slots[cls ? 2 * GR_LB - 1 - k : k] = (u32)(2 * d + sd);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.bcnt[blockIdx.x] = s_c[0];
        a.bcnt[a.nblk + blockIdx.x] = s_c[1];
        u32* p = a.part + 4 * blockIdx.x;
        p[0] = p[1] = p[2] = 0;
        p[3] = s_c[2];
    }
}

// the sides the fast kernels left 1, listed again for the exact kernels (KD_GF_EXACT): block b reads
// k_gr_list's block b — its counts from the scanned bcnt — and keeps the sides whose code is still 1
// in the same slots of list2, counted in bcnt2 (scanned afterwards like bcnt).  Those are the
// undecided sides and, rarely, sides the fast kernels refused deep in the WKB; the exact kernels
// refuse the latter again.  The code byte is the status the fast kernels hand over: they write
// nothing more than without the flag.
__global__ __launch_bounds__(256) void k_gr_relist(GrArgs a, u32* list2, u32* bcnt2) {
    __shared__ u32 s_c[2];
    const int tid = threadIdx.x;
    const u32 b = blockIdx.x;
    if (tid < 2) s_c[tid] = 0;
    __syncthreads();
    const u32 np = a.bcnt[b + 1] - a.bcnt[b];  // (bcnt[nblk], the first wave prefix, is every point side)
    const u32 nw = (b + 1 < a.nblk ? a.bcnt[a.nblk + b + 1] : (u32)*a.tot) - a.bcnt[a.nblk + b];
    const u32* const src = a.list + 2ull * GR_LB * b;
    u32* const dst = list2 + 2ull * GR_LB * b;
    if (np <= 2 * GR_LB && nw <= 2 * GR_LB - np) {  // (what k_gr_list can have written)
        for (u32 i = tid; i < np; i += 256) {
            const u32 sid = src[i];
            if (a.match[sid] == 1) dst[atomicAdd(&s_c[0], 1u)] = sid;  // (LDS: the block's own counters)
        }
        for (u32 i = tid; i < nw; i += 256) {
            const u32 sid = src[2 * GR_LB - 1 - i];
            if (a.match[sid] == 1) dst[2 * GR_LB - 1 - atomicAdd(&s_c[1], 1u)] = sid;
        }
    }
    __syncthreads();
    if (tid == 0) {
        bcnt2[b] = s_c[0];
        bcnt2[a.nblk + b] = s_c[1];
    }
}

// the outcome counts of every block summed into stats[4] (one block).  EXACT (KD_GF_EXACT): the part
// slots of the exact kernels follow the others, as many as the fast workers have; the fast kernels'
// undecided and unsupported sides are then exactly what the exact kernels took and count again under
// their final outcome, so only the fast kernels' decided counts are read
template <bool EXACT>
__global__ __launch_bounds__(1024) void k_gr_stats(GrArgs a) {
    __shared__ unsigned long long s_s[16][4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const u32 np = a.np_list + a.np_pts + a.np_wave;
    unsigned long long v[4] = {0, 0, 0, 0};
    if constexpr (!EXACT) {
#pragma unroll 4
        for (u32 i = tid; i < np; i += 1024) {
            const u32x4 x = ((const u32x4*)a.part)[i];
            v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
        }
    } else {
#pragma unroll 4
        for (u32 i = tid; i < np + a.np_pts + a.np_wave; i += 1024) {
            const u32x4 x = ((const u32x4*)a.part)[i];
            const bool handed = i >= a.np_list && i < np;
            v[0] += x.x; v[1] += x.y;
            if (!handed) { v[2] += x.z; v[3] += x.w; }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int o = 32; o; o >>= 1) v[c] += __shfl_xor(v[c], o);
        if (lane == 0) s_s[wid][c] = v[c];
    }
    __syncthreads();
    if (tid < 4) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; w++) t += s_s[w][tid];
        a.stats[tid] = t;
    }
}

// one wave's LDS traffic kept in program order (the hardware runs a wave's LDS instructions in
// order; this keeps the compiler from moving them): what k_gr_wave's waves, each on a side of its own
// with LDS arrays of its own, use where a block would use a barrier
template <bool WAVE>
__device__ __forceinline__ void gr_sync() {
    if constexpr (WAVE) __builtin_amdgcn_wave_barrier();
    else __syncthreads();
}

// the filter's tile t in LDS (uniform over the NT threads that share the arrays: a block, or with
// NT = 64 one wave; `cur` the tile the arrays hold): its edge count
template <int NT>
__device__ __forceinline__ u32 gr_stage(const GrArgs& a, double (*s_e)[GR_TILE], u32 t, int& cur, int tid) {
    const u32 e0 = t * GR_TILE, m = min((u32)GR_TILE, a.ne - e0);
    if ((int)t != cur) {
        gr_sync<NT == 64>();  // the readers of the tile before
        for (u32 i = tid; i < m; i += NT) {
#pragma unroll
            for (int q = 0; q < 4; q++) s_e[q][i] = a.fe[(u64)q * a.nep + e0 + i];
        }
        gr_sync<NT == 64>();
        cur = (int)t;
    }
    return m;
}

// ---- points and small multipoints: one lane per side ----
template <bool EXACT>
__global__ __launch_bounds__(256) void k_gr_points_t(GrArgs a) {
    __shared__ double s_e[4][GR_TILE];
    __shared__ u32 s_st[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const u32 nitem = a.bcnt[a.nblk];  // (the scan's count in front of the wave counts: every point side)
    const u32 ntile = (a.ne + GR_TILE - 1) / GR_TILE;
    int cur = -1;
    if (tid < 4) s_st[tid] = 0;
    __syncthreads();
    for (u32 base = blockIdx.x * 256u; base < nitem; base += gridDim.x * 256u) {  // block-uniform
        const u32 it = base + tid;
        const bool valid = it < nitem;
        u64 d = 0;
        int s = 0;
        const u8* w = nullptr;
        u32 wlen = 0;
        bool bad = false;
        if (valid) {
            u32 blk, rank;
            gr_item(a.bcnt, a.nblk, 0, it, blk, rank);
            const u32 sid = a.list[2ull * GR_LB * blk + rank];
            d = sid >> 1;
            s = sid & 1;
            bad = gr_locate(a, d, s, w, wlen) <= 0;
        }
        u64 parm = 0, undm = 0, onm = 0;  // per point of the side: crossing parity, undecided, on the boundary (EXACT)
        for (u32 t = 0; t < ntile; t++) {
            const u32 m = gr_stage<256>(a, s_e, t, cur, tid);
            if (!valid || bad) continue;
            GrWalk k;
            gr_walk_init<false>(k, w, wlen);
            GrRun r;
            u32 j = 0;
            while (!k.bad && gr_next<false>(k, r)) {
                if (r.kind != 0 || j >= GR_MAXPT) { bad = true; break; }
                const double x = ld_f64(w + r.off, r.le), y = ld_f64(w + r.off + 8, r.le);
                if (!gr_finite(x) || !gr_finite(y)) { bad = true; break; }
                if (x >= a.f0 && x <= a.f1 && y >= a.f2 && y <= a.f3) {  // (outside the envelope: outside)
                    u32 par = 0, und = 0, on = 0;
                    for (u32 e = 0; e < m; e++) gr_pt_edge<EXACT>(s_e[0][e], s_e[1][e], s_e[2][e], s_e[3][e], x, y, par, und, on);
                    parm ^= (u64)par << j;
                    undm |= (u64)und << j;
                    if constexpr (EXACT) onm |= (u64)on << j;
                }
                j++;
            }
            bad |= k.bad;
        }
        int st = -1;  // 0 true, 1 false, 2 undecided, 3 unsupported
        if (valid) {
            if (bad) st = 3;
            else {
                if constexpr (EXACT) st = (onm | (parm & ~undm)) ? 0 : undm ? 2 : 1;
                else st = (parm & ~undm) ? 0 : undm ? 2 : 1;
                if (st != 2) a.match[2 * d + s] = st == 0 ? 2 : 0;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const u64 b = __ballot(st == c);
            if (b && lane == 0) atomicAdd(&s_st[c], (u32)__popcll(b));
        }
    }
    __syncthreads();
    if (tid < 4) a.part[4 * (a.np_list + blockIdx.x) + tid] = s_st[tid];
}
template __global__ void k_gr_points_t<false>(GrArgs);
// the exact pass over the sides k_gr_relist listed (a.list / a.bcnt / a.tot / a.part are its own)
template __global__ void k_gr_points_t<true>(GrArgs);

// ---- lineal and areal geometries (and large multipoints): one wave per side ----
__device__ __forceinline__ double gr_min64(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double gr_max64(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// vertices [s0, s0 + ns] of a run into the wave's LDS chunk (lane i the i-th; a ring wraps to its
// first vertex)
__device__ __forceinline__ void gr_chunk(const u8* w, const GrRun& r, u32 s0, u32 ns, double* s_vx, double* s_vy, int lane) {
    gr_sync<true>();  // the chunk before has been read
    if ((u32)lane <= ns) {
        u32 i = s0 + lane;
        if (i >= r.cnt) i -= r.cnt;
        const u8* p = w + r.off + (u64)i * r.stride;
        s_vx[lane] = ld_f64(p, r.le);
        s_vy[lane] = ld_f64(p + 8, r.le);
    }
    gr_sync<true>();
}

constexpr int GR_WPB = 4;  // waves per block, each working alone (no block barrier in the kernel)
constexpr u32 GR_RC = 4;   // runs of a geometry remembered from the first walk (most have one or two)
template <bool EXACT>
__global__ __launch_bounds__(64 * GR_WPB) void k_gr_wave_t(GrArgs a) {
    __shared__ double s_ew[GR_WPB][4][GR_TILE];
    __shared__ double s_vw[GR_WPB][2][64];
    __shared__ u32 s_rw[GR_WPB][GR_RC][6];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u32(*const s_run)[6] = s_rw[wid];
    double(*const s_e)[GR_TILE] = s_ew[wid];
    double *const s_vx = s_vw[wid][0], *const s_vy = s_vw[wid][1];
    const u32 npts = a.bcnt[a.nblk];
    const u32 nitem = (u32)(*a.tot - npts);
    const u32 ntile = (a.ne + GR_TILE - 1) / GR_TILE;
    const double inf = __builtin_huge_val();
    int cur = -1;
    u32 cst[4] = {0, 0, 0, 0};
    for (u32 it = blockIdx.x * GR_WPB + wid; it < nitem; it += gridDim.x * GR_WPB) {  // wave-uniform
        u32 blk, rank;
        gr_item(a.bcnt + a.nblk, a.nblk, npts, it, blk, rank);
        const u32 sid = a.list[2ull * GR_LB * blk + 2 * GR_LB - 1 - rank];
        const u64 d = sid >> 1;
        const int s = sid & 1;
        const u8* w;
        u32 wlen;
        GrWalk k;
        GrRun r;
        int st = 3;
        bool wit = false, und = false;
        if (gr_locate(a, d, s, w, wlen) > 0) {
            // pass A: every count and coordinate checked, the envelope of the vertices
            // (the runs it finds are kept in LDS: with up to GR_RC of them the later walks read no
            // header again — every header is a load the next one waits for)
            gr_walk_init<true>(k, w, wlen);
            double mnx = inf, mxx = -inf, mny = inf, mxy = -inf;
            bool bad = false;
            u32 nrun = 0, ri = 0;
            while (!k.bad && gr_next<true>(k, r)) {
                if (nrun < GR_RC && lane == 0) {
                    u32* q = s_run[nrun];
                    q[0] = r.off; q[1] = r.cnt; q[2] = r.stride; q[3] = r.kind; q[4] = r.poly; q[5] = r.le;
                }
                nrun++;
                for (u32 v0 = 0; v0 < r.cnt; v0 += 64) {
                    const u32 i = v0 + lane;
                    if (i < r.cnt) {
                        const u8* p = w + r.off + (u64)i * r.stride;
                        const double x = ld_f64(p, r.le), y = ld_f64(p + 8, r.le);
                        bad |= !gr_finite(x) || !gr_finite(y);
                        mnx = fmin(mnx, x); mxx = fmax(mxx, x); mny = fmin(mny, y); mxy = fmax(mxy, y);
                    }
                }
            }
            gr_sync<true>();
            const bool cached = nrun <= GR_RC;
            auto rewind = [&] {
                ri = 0;
                if (!cached) gr_walk_init<true>(k, w, wlen);
            };
            auto next = [&]() -> bool {
                if (!cached) return gr_next<true>(k, r);
                if (ri >= nrun) return false;
                const u32* q = s_run[ri++];
                r.off = gr_uni<true>(q[0]); r.cnt = gr_uni<true>(q[1]); r.stride = gr_uni<true>(q[2]);
                r.kind = gr_uni<true>(q[3]); r.poly = gr_uni<true>(q[4]); r.le = gr_uni<true>(q[5]) != 0;
                return true;
            };
            if (!k.bad && !__any(bad)) {
                st = 0;
                const u32 gbase = k.base;
                mnx = gr_min64(mnx); mxx = gr_max64(mxx); mny = gr_min64(mny); mxy = gr_max64(mxy);
                // (no vertex, or an envelope apart from the filter's: nothing can meet)
                const bool apart = !(mnx <= a.f1 && mxx >= a.f0 && mny <= a.f3 && mxy >= a.f2);
                // (b) segments of F against the boundary of P
                if (!apart) {
                    rewind();
                    while (!wit && next()) {
                        if (r.kind == 0 || r.cnt == 0) continue;
                        const u32 nseg = r.kind == 2 ? r.cnt : r.cnt - 1;  // (a ring closes onto its first vertex)
                        for (u32 s0 = 0; s0 < nseg && !wit; s0 += GR_CH) {
                            const u32 ns = min((u32)GR_CH, nseg - s0);
                            gr_chunk(w, r, s0, ns, s_vx, s_vy, lane);
                            bool lw = false, lu = false;
                            for (u32 t = 0; t < ntile; t++) {
                                const u32 m = gr_stage<64>(a, s_e, t, cur, lane);
                                if ((m + 63) / 64 * ns <= m) {  // lanes over the tile's edges
                                    for (u32 e = lane; e < m; e += 64) {
                                        const double ax = s_e[0][e], ay = s_e[1][e], bx = s_e[2][e], by = s_e[3][e];
                                        if (fmax(ax, bx) < mnx || fmin(ax, bx) > mxx || fmax(ay, by) < mny || fmin(ay, by) > mxy)
                                            continue;
                                        for (u32 j = 0; j < ns; j++) {
                                            const int q = gr_seg<EXACT>(ax, ay, bx, by, s_vx[j], s_vy[j], s_vx[j + 1], s_vy[j + 1]);
                                            lw |= q == 2;
                                            lu |= q == 1;
                                        }
                                    }
                                } else if ((u32)lane < ns) {  // lanes over the chunk's segments
                                    const double cx = s_vx[lane], cy = s_vy[lane], dx = s_vx[lane + 1], dy = s_vy[lane + 1];
                                    for (u32 e = 0; e < m; e++) {
                                        const double ax = s_e[0][e], ay = s_e[1][e], bx = s_e[2][e], by = s_e[3][e];
                                        if (fmax(ax, bx) < mnx || fmin(ax, bx) > mxx || fmax(ay, by) < mny || fmin(ay, by) > mxy)
                                            continue;
                                        const int q = gr_seg<EXACT>(ax, ay, bx, by, cx, cy, dx, dy);
                                        lw |= q == 2;
                                        lu |= q == 1;
                                    }
                                }
                            }
                            wit = __any(lw);
                            und |= __any(lu) != 0;
                        }
                    }
                }
                // (a) vertices of F in P: with every pair of (b) refuted a run lies wholly inside or
                // wholly outside P, so its first vertex speaks for it; otherwise every vertex is tried
                if (!apart && !wit) {
                    rewind();
                    while (!wit && next()) {
                        const u32 npt = und ? r.cnt : min(r.cnt, 1u);
                        for (u32 i = 0; i < npt && !wit; i++) {
                            const u8* p = w + r.off + (u64)i * r.stride;
                            const double x = ld_f64(p, r.le), y = ld_f64(p + 8, r.le);
                            if (!(x >= a.f0 && x <= a.f1 && y >= a.f2 && y <= a.f3)) continue;
                            u32 par = 0, pu = 0, on = 0;
                            for (u32 t = 0; t < ntile; t++) {
                                const u32 m = gr_stage<64>(a, s_e, t, cur, lane);
                                for (u32 e = lane; e < m; e += 64) gr_pt_edge<EXACT>(s_e[0][e], s_e[1][e], s_e[2][e], s_e[3][e], x, y, par, pu, on);
                            }
                            if (EXACT && __any(on)) wit = true;  // (on the boundary: certain whatever else is not)
                            else if (__any(pu)) und = true;
                            else if (__popcll(__ballot(par)) & 1) wit = true;
                        }
                    }
                }
                // (c) F areal: the first vertex of a ring of P in one of F's polygons
                if (!apart && !wit && (gbase == 3 || gbase == 6)) {
                    for (u32 rq = 0; rq < a.nr && !wit; rq++) {
                        const double qx = a.fe[4ull * a.nep + rq], qy = a.fe[4ull * a.nep + a.nr + rq];
                        if (!(qx >= mnx && qx <= mxx && qy >= mny && qy <= mxy)) continue;
                        rewind();
                        u32 par = 0, pu = 0, on = 0, poly = 0xFFFFFFFFu;
                        auto fin = [&] {
                            if (EXACT && __any(on)) wit = true;  // (the ring's first vertex on F's boundary)
                            else if (__any(pu)) und = true;
                            else if (__popcll(__ballot(par)) & 1) wit = true;
                            par = pu = on = 0;
                        };
                        while (next()) {
                            if (r.poly != poly) {
                                if (poly != 0xFFFFFFFFu) fin();
                                poly = r.poly;
                                if (wit) break;
                            }
                            for (u32 s0 = 0; s0 < r.cnt; s0 += GR_CH) {
                                const u32 ns = min((u32)GR_CH, r.cnt - s0);
                                gr_chunk(w, r, s0, ns, s_vx, s_vy, lane);
                                if ((u32)lane < ns) gr_pt_edge<EXACT>(s_vx[lane], s_vy[lane], s_vx[lane + 1], s_vy[lane + 1], qx, qy, par, pu, on);
                            }
                        }
                        if (poly != 0xFFFFFFFFu && !wit) fin();
                    }
                }
                st = wit ? 0 : und ? 2 : 1;
            }
        }
        if (lane == 0 && (st == 0 || st == 1)) a.match[2 * d + s] = st == 0 ? 2 : 0;
#pragma unroll
        for (int c = 0; c < 4; c++) cst[c] += st == c;
    }
    if (lane < 4) a.part[4 * (a.np_list + a.np_pts + blockIdx.x * GR_WPB + wid) + lane] = lane == 0 ? cst[0] : lane == 1 ? cst[1] : lane == 2 ? cst[2] : cst[3];
}
template __global__ void k_gr_wave_t<false>(GrArgs);
template __global__ void k_gr_wave_t<true>(GrArgs);

// FNV-1a over the filter's bytes (the key of its device copy)
static u64 gr_hash(const void* p, size_t n, u64 h) {
    const u8* b = (const u8*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

// the filter's device copy (slot "gr.filter"), written again only when the filter changed
static int gr_filter(kd_ctx* ctx, const kd_filter_poly* f, GrArgs& a) {
    const u64 nv = f->n_vert, nr = f->n_ring;
    KD_CHECK(nr >= 1 && nv >= 2 && f->xy && f->ring_off, "kd_geom_refine: empty filter");
    if (nv > (1ull << 20)) {
        set_error("kd_geom_refine: a filter of %llu vertices (at most 2^20)", (unsigned long long)nv);
        return KD_EUNSUPPORTED;
    }
    KD_CHECK(f->ring_off[0] == 0 && f->ring_off[nr] == nv, "kd_geom_refine: ring_off must run from 0 to n_vert");
    double env[4] = {f->xy[0], f->xy[0], f->xy[1], f->xy[1]};
    for (u64 r = 0; r < nr; r++) {
        const u64 b = f->ring_off[r], e = f->ring_off[r + 1];
        KD_CHECK(b < e && e <= nv && e - b >= 2, "kd_geom_refine: ring %llu is empty", (unsigned long long)r);
        KD_CHECK(f->xy[2 * b] == f->xy[2 * (e - 1)] && f->xy[2 * b + 1] == f->xy[2 * (e - 1) + 1],
                 "kd_geom_refine: ring %llu is not closed", (unsigned long long)r);
    }
    for (u64 i = 0; i < nv; i++) {
        const double x = f->xy[2 * i], y = f->xy[2 * i + 1];
        KD_CHECK(std::isfinite(x) && std::isfinite(y), "kd_geom_refine: filter vertex %llu is not finite", (unsigned long long)i);
        env[0] = std::min(env[0], x); env[1] = std::max(env[1], x);
        env[2] = std::min(env[2], y); env[3] = std::max(env[3], y);
    }
    const u64 ne = nv - nr, nep = (ne + 63) / 64 * 64;
    a.ne = (u32)ne;
    a.nep = (u32)nep;
    a.nr = (u32)nr;
    a.f0 = env[0]; a.f1 = env[1]; a.f2 = env[2]; a.f3 = env[3];
    const size_t bytes = (4 * nep + 2 * nr) * sizeof(double);
    void* dev;
    int rc;
    if ((rc = ensure(ctx, "gr.filter", bytes, &dev))) return rc;
    a.fe = (const double*)dev;
    u64 h = gr_hash(f->xy, nv * 16, 0xcbf29ce484222325ull);
    h = gr_hash(f->ring_off, (nr + 1) * 8, h);
    if (ctx->gr_dev == dev && ctx->gr_ptr == (const void*)f->xy && ctx->gr_nv == nv && ctx->gr_nr == nr && ctx->gr_hash == h)
        return KD_OK;
    std::vector<double> buf(4 * nep + 2 * nr, 0.0);
    u64 e = 0;
    for (u64 r = 0; r < nr; r++) {
        const u64 b = f->ring_off[r], en = f->ring_off[r + 1];
        for (u64 i = b; i + 1 < en; i++, e++) {
            buf[e] = f->xy[2 * i];
            buf[nep + e] = f->xy[2 * i + 1];
            buf[2 * nep + e] = f->xy[2 * i + 2];
            buf[3 * nep + e] = f->xy[2 * i + 3];
        }
        buf[4 * nep + r] = f->xy[2 * b];
        buf[4 * nep + nr + r] = f->xy[2 * b + 1];
    }
    KD_HIP(hipMemcpyAsync(dev, buf.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));  // (buf leaves scope)
    ctx->gr_dev = dev;
    ctx->gr_ptr = f->xy;
    ctx->gr_nv = nv;
    ctx->gr_nr = nr;
    ctx->gr_hash = h;
    return KD_OK;
}

}  // namespace kd

using namespace kd;

extern "C" int kd_orient2d_exact_batch(const double* abc, uint64_t n, int8_t* out) {
    KD_CHECK(n == 0 || (abc && out), "kd_orient2d_exact_batch: NULL argument");
    for (u64 i = 0; i < n; i++) {
        const double* p = abc + 6 * i;
        out[i] = (int8_t)kd_orient2d_exact(p[0], p[1], p[2], p[3], p[4], p[5]);
    }
    return KD_OK;
}

extern "C" int kd_geom_refine(kd_ctx* ctx, const kd_filter_poly* filter, const kd_geom_head* heads_old, uint64_t n_old,
                              const kd_geom_head* heads_new, uint64_t n_new, uint32_t heads_mem, const kd_blobs* old_blobs,
                              const kd_blobs* new_blobs, const uint32_t* pairs, uint64_t n, const uint64_t* d_n,
                              uint32_t pairs_mem, uint32_t flags, uint8_t* match, uint32_t* keep, uint64_t* n_keep,
                              uint64_t* stats, uint32_t out_mem) {
    KD_CHECK(ctx && filter && match && keep && n_keep && stats, "kd_geom_refine: NULL argument");
    if (!heads_old && !heads_new) {
        set_error("kd_geom_refine: needs geometry heads (locating the geometry from legends is not built)");
        return KD_EUNSUPPORTED;
    }
    KD_CHECK((n_old == 0 || heads_old) && (n_new == 0 || heads_new), "kd_geom_refine: heads NULL");
    KD_CHECK(old_blobs && new_blobs, "kd_geom_refine: needs both blob arenas");
    KD_CHECK(n == 0 || pairs, "kd_geom_refine: pairs NULL");
    KD_CHECK(d_n == nullptr || (out_mem == KD_MEM_DEVICE && pairs_mem == KD_MEM_DEVICE),
             "kd_geom_refine: a device count needs device pairs and outputs");
    KD_CHECK(n < (1ull << 31), "kd_geom_refine: too many deltas");
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    GrArgs a{};
    if ((rc = gr_filter(ctx, filter, a))) return rc;
    const bool host_out = out_mem == KD_MEM_HOST;
    // the scan's total (u64) at 0, stats[4] (u64) at 16, the second scan's total (u64) at 48
    void* dc;
    if ((rc = ensure(ctx, "gr.cnt", 64, &dc))) return rc;
    unsigned long long* dstats = host_out ? (unsigned long long*)((char*)dc + 16) : (unsigned long long*)stats;
    void* t_nk;
    if ((rc = ensure(ctx, "gr.nk", 8, &t_nk))) return rc;
    u64* const nk_dst = host_out ? (u64*)t_nk : n_keep;
    if (n == 0) {
        KD_HIP(hipMemsetAsync(nk_dst, 0, 8, ctx->stream));
        if (!host_out) KD_HIP(hipMemsetAsync(stats, 0, 32, ctx->stream));
        if (host_out) {
            KD_HIP(hipStreamSynchronize(ctx->stream));
            *n_keep = 0;
            stats[0] = stats[1] = stats[2] = stats[3] = 0;
        }
        return KD_OK;
    }
    const kd_geom_head* hs[2] = {heads_old, heads_new};
    const u64 nh[2] = {n_old, n_new};
    const kd_blobs* bl[2] = {old_blobs, new_blobs};
    const char* htag[2] = {"gh.o", "gh.n"};
    const char* tag[2][2] = {{"gf.od", "gf.oo"}, {"gf.nd", "gf.no"}};
    const bool dh = (flags & KD_GF_DELTA_HEADS) != 0;
    for (int s = 0; s < 2; s++) {
        const void *dhd, *dd, *doff;
        if ((rc = stage_in(ctx, htag[s], nh[s] ? (const void*)hs[s] : nullptr, nh[s] * sizeof(kd_geom_head), heads_mem, &dhd)))
            return rc;
        a.head[s] = (const kd_geom_head*)dhd;
        a.nhead[s] = nh[s];
        const kd_blobs* B = bl[s];
        KD_CHECK(B->off && (B->n == 0 || B->data), "kd_geom_refine: arena %d NULL", s);
        KD_CHECK(dh || B->n == nh[s], "kd_geom_refine: arena %d holds %llu blobs, %llu heads", s, (unsigned long long)B->n,
                 (unsigned long long)nh[s]);
        const u64 bytes = B->mem == KD_MEM_HOST ? (B->n ? B->off[B->n] : 0) : 0;
        if ((rc = stage_in(ctx, tag[s][1], B->off, (B->n + 1) * 8, B->mem, &doff))) return rc;
        if ((rc = stage_in(ctx, tag[s][0], B->data, bytes ? bytes : 1, B->mem, &dd))) return rc;
        a.data[s] = (const u8*)dd;
        a.off[s] = (const u64*)doff;
        a.nblob[s] = B->n;
    }
    a.dense = dh ? 1 : 0;
    if (dh) KD_CHECK(nh[0] >= n && nh[1] >= n, "kd_geom_refine: KD_GF_DELTA_HEADS needs a head slot per delta and side");
    const void* dp;
    if ((rc = stage_in(ctx, "gf.pairs", pairs, n * 8, pairs_mem, &dp))) return rc;
    a.pairs = (const uint2*)dp;
    a.cap = n;
    a.d_n = d_n;
    u8* dm = match;
    u32* dk = keep;
    if (host_out) {
        void *x, *y;
        if ((rc = ensure(ctx, "gf.match", 2 * n + 2, &x)) || (rc = ensure(ctx, "gf.keep", 4 * n + 4, &y))) return rc;
        dm = (u8*)x;
        dk = (u32*)y;
        if ((rc = stage_h2d(ctx, dm, match, 2 * n))) return rc;
    }
    KD_CHECK(((u64)dm & 1) == 0, "kd_geom_refine: match must be 2-byte aligned");
    a.match = dm;
    const u64 cu = (u64)ctx->n_cu;
    const u64 nblk = (n + GR_LB - 1) / GR_LB;
    const unsigned g_pts = (unsigned)std::max<u64>(1, std::min<u64>((2 * n + 255) / 256, cu * 4));
    const int occ = occupancy(ctx, (const void*)k_gr_wave_t<false>, 64 * GR_WPB, 0);
    const unsigned g_wave = (unsigned)std::max<u64>(1, std::min<u64>((2 * n + GR_WPB - 1) / GR_WPB, cu * (u64)occ));
    // KD_GF_EXACT: a second pass over the sides the fast kernels leave 1, with a work list, block
    // counts and part slots of its own behind theirs; the same grids (a block whose share of the
    // list is empty — every block when nothing was left — reads the device-side count and returns)
    const bool exact = (flags & KD_GF_EXACT) != 0;
    const u64 np_x = exact ? g_pts + (u64)g_wave * GR_WPB : 0;
    void *dl, *db, *dpart;
    if ((rc = ensure(ctx, "gr.list", 8 * GR_LB * nblk * (exact ? 2 : 1), &dl)) ||
        (rc = ensure(ctx, "gr.bcnt", (8 * nblk + 16) * (exact ? 2 : 1), &db)) ||
        (rc = ensure(ctx, "gr.part", 16 * (nblk + g_pts + (u64)g_wave * GR_WPB + np_x), &dpart)))
        return rc;
    a.list = (u32*)dl;
    a.bcnt = (u32*)db;
    a.tot = (const u64*)dc;
    a.nblk = (u32)nblk;
    a.part = (u32*)dpart;
    a.np_list = (u32)nblk;
    a.np_pts = g_pts;
    a.np_wave = g_wave * GR_WPB;
    a.stats = dstats;
    if ((rc = launch(ctx, "k_gr_list", [&] { hipLaunchKernelGGL(k_gr_list, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, a); })))
        return rc;
    if ((rc = gf_scan(ctx, (u32*)db, (u32)(2 * nblk), (u64*)dc))) return rc;
    if ((rc = launch(ctx, "k_gr_points", [&] { hipLaunchKernelGGL(k_gr_points_t<false>, dim3(g_pts), dim3(256), 0, ctx->stream, a); })))
        return rc;
    if ((rc = launch(ctx, "k_gr_wave", [&] { hipLaunchKernelGGL(k_gr_wave_t<false>, dim3(g_wave), dim3(64 * GR_WPB), 0, ctx->stream, a); })))
        return rc;
    if (exact) {
        GrArgs x = a;
        x.list = a.list + 2 * GR_LB * nblk;
        x.bcnt = a.bcnt + 2 * nblk + 4;
        x.tot = (const u64*)((char*)dc + 48);
        x.part = a.part + 4 * ((u64)a.np_pts + a.np_wave);  // (its workers' slots follow the fast ones)
        if ((rc = launch(ctx, "k_gr_relist", [&] {
                 hipLaunchKernelGGL(k_gr_relist, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, a, x.list, x.bcnt);
             })))
            return rc;
        if ((rc = gf_scan(ctx, x.bcnt, (u32)(2 * nblk), (u64*)((char*)dc + 48)))) return rc;
        if ((rc = launch(ctx, "k_gr_points_x", [&] { hipLaunchKernelGGL(k_gr_points_t<true>, dim3(g_pts), dim3(256), 0, ctx->stream, x); })))
            return rc;
        if ((rc = launch(ctx, "k_gr_wave_x", [&] { hipLaunchKernelGGL(k_gr_wave_t<true>, dim3(g_wave), dim3(64 * GR_WPB), 0, ctx->stream, x); })))
            return rc;
    }
    if ((rc = launch(ctx, "k_gr_stats", [&] {
             if (exact) hipLaunchKernelGGL(k_gr_stats<true>, dim3(1), dim3(1024), 0, ctx->stream, a);
             else hipLaunchKernelGGL(k_gr_stats<false>, dim3(1), dim3(1024), 0, ctx->stream, a);
         })))
        return rc;
    if ((rc = gf_rekeep(ctx, dm, n, d_n, dk, nk_dst))) return rc;
    if (!host_out) return KD_OK;
    u64 nk = 0;
    unsigned long long hst[4];
    KD_HIP(hipMemcpyAsync(&nk, t_nk, 8, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipMemcpyAsync(hst, dstats, 32, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipMemcpyAsync(match, dm, 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    if (nk) KD_HIP(hipMemcpyAsync(keep, dk, 4 * nk, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    *n_keep = nk;
    for (int i = 0; i < 4; i++) stats[i] = hst[i];
    return prof_flush(ctx);
}
