// kd_keypack.hip — join keys and the side scan on the device (kd_pack_keys_device): a path arena, its
// offsets and nothing else become keys, statuses and one kd_keypack_info, all in HBM.
//
// k_kp_pack<MODE, IPT>: one tile of T = 256 * IPT consecutive entries per 256-thread workgroup.  The
// tile's bytes [off[i0], off[i0 + T]) are one contiguous span of the arena; when it fits the LDS budget
// it is staged with aligned 16-byte coalesced loads — only chunks that hold at least one byte of the
// span, which lies inside [off[0], off[n]): k_join2's page argument, an aligned chunk never crosses a
// page — and every lane decodes its entries from LDS (kd_keypack.h, the host packer's decoder).  When it
// does not fit (long hash filenames) the tile's lanes decode from HBM, each reading the bytes of its own
// entries only.  Lane t owns entries i0 + r * 256 + t: offsets, keys (8 bytes per lane) and statuses are
// coalesced.  An entry is refused (status 1, nothing read) when off[i + 1] < off[i] or when it does not
// lie inside [off[0], off[n]] — for ascending offsets the second never happens.
//
// The same kernel writes the tile's partial of the side scan: kd_keys_scan's Part (kd_ctx.hip) as a
// monoid, plus what a seam needs.  The ordered fields come from the keys in LDS, each lane folding IPT
// consecutive ones, then a wave reduction by shuffles and the four waves in order; no global atomic.
// k_kp_fold combines partials in tile order (each lane a contiguous run, then the same reduction);
// beyond KP_FOLD_DIRECT tiles a first level folds KP_FOLD_CHUNK partials per workgroup.  Every step
// is a fixed-shape fold of an associative combine: the result is a pure function of the inputs.
#include "kd_internal.h"
#include "kd_keypack.h"
#include "kd_walkkey.h"

using namespace kd;

namespace {

constexpr int KP_NT = 256;
constexpr int KP_LDS = 30720;            // the largest staged span (bytes)
constexpr u64 KP_FOLD_DIRECT = 4096;     // partials one workgroup folds directly
constexpr u64 KP_FOLD_CHUNK = 4096;      // partials per first-level workgroup beyond that

// the scan of a run of keys (len == 0: the identity)
struct KpPart {
    u64 first, last;  // first and last key
    u64 vary;         // OR of key ^ first
    i64 lo, hi;       // pk range (KD_KEY_INT)
    u64 b0, b1;       // first and last bucket (key >> 40)
    u64 pre, suf, mx; // the first, the last and the longest bucket run
    u64 len;
    u64 bad, first_bad;
    u32 asc, basc;    // keys strictly ascending / buckets never descending inside
    u64 hbm;          // tiles that decoded from HBM
};

__device__ __forceinline__ KpPart kp_identity() {
    KpPart p;
    p.first = p.last = p.vary = 0;
    p.lo = INT64_MAX;
    p.hi = INT64_MIN;
    p.b0 = p.b1 = p.pre = p.suf = p.mx = p.len = 0;
    p.bad = 0;
    p.first_bad = UINT64_MAX;
    p.asc = p.basc = 1;
    p.hbm = 0;
    return p;
}

// the scan of L followed by R (kd_keys_scan's combine: a seam is ascending when last(L) < first(R),
// a bucket run continues across it when b1(L) == b0(R), the buckets descend when b0(R) < b1(L))
__device__ __forceinline__ KpPart kp_combine(const KpPart& L, const KpPart& R) {
    KpPart p;
    // the order-free fields
    p.lo = L.lo < R.lo ? L.lo : R.lo;
    p.hi = L.hi > R.hi ? L.hi : R.hi;
    p.bad = L.bad + R.bad;
    p.first_bad = L.first_bad < R.first_bad ? L.first_bad : R.first_bad;
    p.hbm = L.hbm + R.hbm;
    p.len = L.len + R.len;
    const bool le = L.len == 0, re = R.len == 0;
    const bool both = !le && !re;
    p.first = le ? R.first : L.first;
    p.last = re ? L.last : R.last;
    // OR of key ^ first(L) over R's keys = vary(R) | first(R) ^ first(L): first(R) is one of them
    p.vary = L.vary | R.vary | (both ? L.first ^ R.first : 0);
    p.asc = L.asc & R.asc & (u32)(!both || L.last < R.first);
    p.basc = L.basc & R.basc & (u32)(!both || R.b0 >= L.b1);
    p.b0 = le ? R.b0 : L.b0;
    p.b1 = re ? L.b1 : R.b1;
    const bool join = both && L.b1 == R.b0;
    const u64 joined = join ? L.suf + R.pre : 0;
    const bool l_one = L.pre == L.len, r_one = R.pre == R.len;  // (an empty side is "one bucket" of 0)
    p.pre = le ? R.pre : (join && l_one) ? L.len + R.pre : L.pre;
    p.suf = re ? L.suf : (join && r_one) ? L.suf + R.len : R.suf;
    u64 mx = L.mx > R.mx ? L.mx : R.mx;
    p.mx = joined > mx ? joined : mx;
    return p;
}

__device__ __forceinline__ u64 shfl_down64(u64 v, int d) { return (u64)__shfl_down((unsigned long long)v, d, 64); }

__device__ __forceinline__ KpPart kp_shfl_down(const KpPart& a, int d) {
    KpPart p;
    p.first = shfl_down64(a.first, d);
    p.last = shfl_down64(a.last, d);
    p.vary = shfl_down64(a.vary, d);
    p.lo = (i64)shfl_down64((u64)a.lo, d);
    p.hi = (i64)shfl_down64((u64)a.hi, d);
    p.b0 = shfl_down64(a.b0, d);
    p.b1 = shfl_down64(a.b1, d);
    p.pre = shfl_down64(a.pre, d);
    p.suf = shfl_down64(a.suf, d);
    p.mx = shfl_down64(a.mx, d);
    p.len = shfl_down64(a.len, d);
    p.bad = shfl_down64(a.bad, d);
    p.first_bad = shfl_down64(a.first_bad, d);
    p.asc = (u32)__shfl_down((int)a.asc, d, 64);
    p.basc = (u32)__shfl_down((int)a.basc, d, 64);
    p.hbm = shfl_down64(a.hbm, d);
    return p;
}

// lane order = sequence order: after the step of distance d lane l holds lanes [l, l + 2d)
__device__ __forceinline__ KpPart kp_wave_reduce(KpPart p) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const KpPart o = kp_shfl_down(p, d);
        if (lane + d < 64) p = kp_combine(p, o);
    }
    return p;
}

// the 256 lanes' parts in lane order -> the whole (valid in thread 0); sp: KP_NT / 64 parts of LDS
__device__ __forceinline__ KpPart kp_block_reduce(KpPart p, KpPart* sp) {
    p = kp_wave_reduce(p);
    if ((threadIdx.x & 63) == 0) sp[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        p = sp[0];
        for (int w = 1; w < KP_NT / 64; w++) p = kp_combine(p, sp[w]);
    }
    return p;
}

__device__ __forceinline__ void kp_push(KpPart& p, u64 k) {  // one more key behind p (the ordered fields)
    KpPart q = kp_identity();
    q.first = q.last = k;
    q.b0 = q.b1 = k >> 40;
    q.pre = q.suf = q.mx = q.len = 1;
    p = kp_combine(p, q);
}

template <int MODE, typename P>
__device__ __forceinline__ int kp_decode(P s, u64 len, int levels, int hex, u64* key) {
    if (MODE == KD_KEY_INT) return kp::int_entry(s, len, key);
    return kp::hash_entry(s, len, levels, hex, key);
}

template <int MODE, int IPT>
__global__ __launch_bounds__(KP_NT) void k_kp_pack(const u8* __restrict__ paths, const u64* __restrict__ off, u64 n,
                                                    int levels, int hex, u32 budget, u64* __restrict__ keys,
                                                    u8* __restrict__ status, KpPart* __restrict__ part) {
    constexpr int T = KP_NT * IPT;
    __shared__ __attribute__((aligned(16))) u8 s_bytes[KP_LDS + 16];
    __shared__ u64 s_keys[T];
    __shared__ KpPart s_part[KP_NT / 64];
    const int t = threadIdx.x;
    const u64 i0 = (u64)blockIdx.x * T;
    const u64 cnt = n - i0 < (u64)T ? n - i0 : (u64)T;  // (the grid has no empty tile)
    const u64 g_lo = off[0], g_hi = off[n];
    const u64 lo = off[i0], hi = off[i0 + cnt];
    // the tile's span: staged when it is a span of the arena's own range and fits
    const bool staged = lo <= hi && lo >= g_lo && hi <= g_hi && hi - lo <= (u64)budget;
    const uintptr_t a_lo = (uintptr_t)paths + lo;
    const uintptr_t a0 = a_lo & ~(uintptr_t)15;  // the first chunk holds byte lo (when lo < hi)
    if (staged && hi > lo) {
        const u64 chunks = ((uintptr_t)paths + hi - a0 + 15) / 16;  // the last one holds byte hi - 1
        const u32x4* src = (const u32x4*)a0;
        for (u64 c = t; c < chunks; c += KP_NT) ((u32x4*)s_bytes)[c] = src[c];
    }
    __syncthreads();
    const u32 shift = (u32)(a_lo - a0);  // s_bytes[shift + (x - lo)] = arena byte x
    KpPart mine = kp_identity();  // the order-free fields of this lane's entries
#pragma unroll 1
    for (int r = 0; r < IPT; r++) {
        const u64 j = (u64)r * KP_NT + t;
        if (j >= cnt) break;
        const u64 i = i0 + j;
        const u64 a = off[i], b = off[i + 1];
        u64 k = 0;
        int st = 1;
        if (a <= b && a >= g_lo && b <= g_hi) {
            if (staged && a >= lo && b <= hi) st = kp_decode<MODE>((const u8*)s_bytes + shift + (u32)(a - lo), b - a, levels, hex, &k);
            else st = kp_decode<MODE>(paths + a, b - a, levels, hex, &k);  // bounded reads of [a, b)
        }
        keys[i] = k;
        status[i] = (u8)st;
        s_keys[j] = k;
        if (st) {
            mine.bad++;
            mine.first_bad = i < mine.first_bad ? i : mine.first_bad;
        }
        if (MODE == KD_KEY_INT) {
            const i64 pk = wk::int_key_pk(k);
            mine.lo = pk < mine.lo ? pk : mine.lo;
            mine.hi = pk > mine.hi ? pk : mine.hi;
        }
    }
    __syncthreads();
    // the ordered fields: this lane's IPT consecutive keys
    KpPart p = kp_identity();
#pragma unroll
    for (int r = 0; r < IPT; r++) {
        const u64 j = (u64)t * IPT + r;
        if (j < cnt) kp_push(p, s_keys[j]);
    }
    p.lo = mine.lo;
    p.hi = mine.hi;
    p.bad = mine.bad;
    p.first_bad = mine.first_bad;
    p = kp_block_reduce(p, s_part);
    if (t == 0) {
        p.hbm = staged ? 0 : 1;
        part[blockIdx.x] = p;
    }
}

// partials [b * chunk, min(n_in, (b + 1) * chunk)) in order -> out[b]; FINAL (one workgroup, chunk >=
// n_in): the kd_keypack_info and the HBM tile count instead
template <bool FINAL>
__global__ __launch_bounds__(KP_NT) void k_kp_fold(const KpPart* __restrict__ in, u64 n_in, u64 chunk, u32 key_mode,
                                                    KpPart* __restrict__ out, kd_keypack_info* __restrict__ info,
                                                    u64* __restrict__ stat) {
    __shared__ KpPart s_part[KP_NT / 64];
    const u64 a = (u64)blockIdx.x * chunk;
    const u64 b = n_in - a < chunk ? n_in : a + chunk;
    const u64 per = (b - a + KP_NT - 1) / KP_NT;  // each lane a contiguous run
    KpPart p = kp_identity();
    const u64 x0 = a + threadIdx.x * per;
    for (u64 x = x0; x < x0 + per && x < b; x++) p = kp_combine(p, in[x]);
    p = kp_block_reduce(p, s_part);
    if (threadIdx.x) return;
    if (!FINAL) {
        out[blockIdx.x] = p;
        return;
    }
    kd_keypack_info r;
    const bool any = p.len != 0;
    r.info.vary = p.vary;
    r.info.key0 = p.first;
    r.info.pk_min = any && key_mode == KD_KEY_INT ? p.lo : 0;
    r.info.pk_max = any && key_mode == KD_KEY_INT ? p.hi : 0;
    r.info.ascending = (int32_t)p.asc;
    r.info.seg_max = !p.basc ? -1 : (int32_t)(p.mx > 0x7fffffffull ? 0x7fffffff : p.mx);
    r.bad = p.bad;
    r.first_bad = p.first_bad;
    *info = r;
    stat[0] = p.hbm;
}

template <int MODE>
int pack_launch(kd_ctx* ctx, int ipt, u32 ntiles, const u8* paths, const u64* off, u64 n, int levels, int hex, u32 budget,
                u64* keys, u8* status, KpPart* part) {
    return launch(ctx, "k_kp_pack", [&] {
        if (ipt == 4)
            hipLaunchKernelGGL((k_kp_pack<MODE, 4>), dim3(ntiles), dim3(KP_NT), 0, ctx->stream, paths, off, n, levels, hex,
                               budget, keys, status, part);
        else
            hipLaunchKernelGGL((k_kp_pack<MODE, 2>), dim3(ntiles), dim3(KP_NT), 0, ctx->stream, paths, off, n, levels, hex,
                               budget, keys, status, part);
    });
}

}  // namespace

namespace kd {

int keypack_hbm_tiles(kd_ctx* ctx, int64_t* value) {
    auto it = ctx->bufs.find("kp.stat");
    *value = 0;
    if (it == ctx->bufs.end() || !it->second.p) return KD_OK;  // (no call yet)
    KD_HIP(hipSetDevice(ctx->device));
    u64 v = 0;
    KD_HIP(hipMemcpyAsync(&v, it->second.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    *value = (int64_t)v;
    return KD_OK;
}

}  // namespace kd

extern "C" int kd_pack_keys_device(kd_ctx* ctx, const uint8_t* d_paths, const uint64_t* d_path_off, uint64_t n,
                                   uint32_t key_mode, int levels, int hex, uint64_t* d_keys, uint8_t* d_status,
                                   kd_keypack_info* d_info) {
    KD_CHECK(ctx && d_paths && d_path_off && d_keys && d_status && d_info, "kd_pack_keys_device: NULL");
    KD_CHECK(key_mode == KD_KEY_INT || key_mode == KD_KEY_HASH, "kd_pack_keys_device: bad key_mode");
    if (key_mode == KD_KEY_HASH)
        KD_CHECK(levels > 0 && levels <= 16 && kp::hash_bits(levels, hex) < 64,
                 "kd_pack_keys_device: %d %s levels leave no key bits", levels, hex ? "hex" : "base64");
    const int ipt = ctx->opt.kp_tile == 1024 ? 4 : 2;
    KD_CHECK(ctx->opt.kp_tile == 512 || ctx->opt.kp_tile == 1024, "kd_pack_keys_device: kp_tile must be 512 or 1024");
    const u64 T = (u64)KP_NT * ipt;
    const u64 ntiles = (n + T - 1) / T;
    KD_CHECK(ntiles < (1ull << 31), "kd_pack_keys_device: too many entries");
    int lds = ctx->opt.kp_lds_bytes;
    const u32 budget = (u32)(lds < 0 ? 0 : lds > KP_LDS ? KP_LDS : lds);
    KD_HIP(hipSetDevice(ctx->device));
    void *part = nullptr, *part2 = nullptr, *stat = nullptr;
    int rc;
    const u64 n2 = ntiles > KP_FOLD_DIRECT ? (ntiles + KP_FOLD_CHUNK - 1) / KP_FOLD_CHUNK : 0;
    if ((rc = ensure(ctx, "kp.part", (size_t)(ntiles ? ntiles : 1) * sizeof(KpPart), &part))) return rc;
    if ((rc = ensure(ctx, "kp.part2", (size_t)(n2 ? n2 : 1) * sizeof(KpPart), &part2))) return rc;
    if ((rc = ensure(ctx, "kp.stat", 16, &stat))) return rc;
    if (ntiles) {
        rc = key_mode == KD_KEY_INT
                 ? pack_launch<KD_KEY_INT>(ctx, ipt, (u32)ntiles, d_paths, d_path_off, n, levels, hex, budget, d_keys, d_status,
                                           (KpPart*)part)
                 : pack_launch<KD_KEY_HASH>(ctx, ipt, (u32)ntiles, d_paths, d_path_off, n, levels, hex, budget, d_keys,
                                            d_status, (KpPart*)part);
        if (rc) return rc;
    }
    const KpPart* src = (const KpPart*)part;
    u64 n_src = ntiles;
    if (n2) {
        rc = launch(ctx, "k_kp_fold", [&] {
            hipLaunchKernelGGL((k_kp_fold<false>), dim3((u32)n2), dim3(KP_NT), 0, ctx->stream, src, n_src, KP_FOLD_CHUNK,
                               key_mode, (KpPart*)part2, (kd_keypack_info*)nullptr, (u64*)nullptr);
        });
        if (rc) return rc;
        src = (const KpPart*)part2;
        n_src = n2;
    }
    return launch(ctx, "k_kp_info", [&] {
        hipLaunchKernelGGL((k_kp_fold<true>), dim3(1), dim3(KP_NT), 0, ctx->stream, src, n_src, n_src ? n_src : (u64)1, key_mode,
                           (KpPart*)nullptr, d_info, (u64*)stat);
    });
}
