// kd_treehash.hip — kd_tree_hash: the ids (and bodies) of a batch of git tree objects.
//
// <- index.write_tree(repo) (kart/merge.py:122): a git tree's id is SHA-1 over "tree <len>\0" plus
// the concatenation of "<mode> <name>\0<20 oid bytes>" over its entries in git's order, a pure function
// of the (name, oid) runs.  All trees of one level of a feature tree are independent, one call hashes
// one level; tree_oid has the layout of kd_tree_entries.oid, so a resident level feeds the next.
//
// Kernels, in stream order:
//   k_th_check  one lane per entry: its tree (binary search in seg), its name checked (status 3), then
//               either the order check against its predecessor (status 1) or, under KD_TH_RANK_NAMES,
//               its byte offset inside the sorted body from one pass over its run (status 2 on an
//               equal name).  Violations meet in a u32 per tree through atomic max: 3 > 2 > 1.
//   k_th_size   one lane per tree: status out, body length (0 where status != 0), 64-byte SHA-1 blocks
//               of the object (header + body + 0x80 + zeros + 64-bit length).
//   k_th_scan1 / k_th_scan2 / k_th_scan3: exclusive scan of (blocks, body bytes) as two u64 — the
//               project's k_gf_scan is 32-bit and a 100M-leaf level has more than 2^32 body bytes.
//   (one 32-byte readback: the arena's blocks, the body bytes, the long-run flag)
//   k_th_frame  a wave per 64 trees, tree after tree with all lanes on its bytes: header and padding.
//   k_th_format a wave per 64 entries, entry after entry with all lanes on its bytes: the record into
//               the arena (every object starts on a 64-byte boundary) and into body when asked for.
//   k_th_sha1   one lane per tree over its blocks, each read as four aligned 16-byte loads; 80 rounds
//               and the 16-word schedule unrolled with constant indices (no scratch).
//
// Every byte of an object is written by exactly one byte store of k_th_frame or k_th_format, so the
// two need no order between them and the arena needs no clearing.
#include "kd_internal.h"

namespace kd {

constexpr u32 TH_NONE = 0xFFFFFFFFu;
constexpr u64 TH_RANK_MAX = 512;  // the longest run KD_TH_RANK_NAMES orders (k_seg_sort's leaf-tree bound)
constexpr int TH_SC = 2048;       // trees per scan block: 8 rounds of 256

struct ThArgs {
    const u8* name;
    const u64* noff;  // [n + 1]
    const u8* oid;    // [n * 20]
    const u64* seg;   // [nt + 1]
    u64 n, nt;
    u32 kind, rank;
    u32* own;    // [n] tree of each entry (TH_NONE: outside every run)
    u32* roff;   // [n] rank mode: byte offset of the entry's record inside its tree's sorted body
    u32* st;     // [nt] status being collected
    u64x2* sz;   // [nt] (blocks, body bytes)
    u64* aoff;   // [nt + 1] first block of each object in the arena
    u64* boff;   // [nt + 1] body offsets (the caller's body_off where it is device memory)
    u64x2* bs;   // [scan blocks] block sums, scanned in place
    u64* tot;    // [4] arena blocks, body bytes, 1 = a run longer than TH_RANK_MAX under the flag
    u8* arena;
    u8* body;    // optional
    u32* out_oid;
    u8* status;
};

__device__ const u64 TH_P10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                                   100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull,
                                   10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                   100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

__device__ __forceinline__ u32 th_digits(u64 v) {
    u32 d = 1;
    u64 p = 10;
#pragma unroll
    for (int k = 1; k < 20; k++, p *= 10) d = v >= p ? (u32)k + 1 : d;  // (p = 10^19 at the last compare)
    return d;
}

__device__ __forceinline__ u32 th_mlen(u32 kind) { return kind == KD_TE_TREE ? 6u : 7u; }

// entries [lo, hi) of tree t, clamped to the entries there are (a device seg is not checked on the host)
__device__ __forceinline__ void th_run(const ThArgs& a, u64 t, u64* lo, u64* hi) {
    const u64 l = min(a.seg[t], a.n), h = min(a.seg[t + 1], a.n);
    *lo = l;
    *hi = h < l ? l : h;
}

// entry i's name: its first byte and length; false (length 0) unless 1..255 bytes inside the arena
__device__ __forceinline__ bool th_name(const ThArgs& a, u64 i, u64* s, u32* len) {
    const u64 b = a.noff[i], e = a.noff[i + 1], end = a.noff[a.n];
    const bool ok = b < e && e <= end && e - b <= 255;
    *s = ok ? b : 0;
    *len = ok ? (u32)(e - b) : 0u;
    return ok;
}

// git's order: unsigned bytes, a blob's name as if it ended in NUL, a tree's as if it ended in '/'
__device__ __forceinline__ int th_cmp(const u8* __restrict__ p, u32 pl, const u8* __restrict__ q, u32 ql, u32 term) {
    const u32 m = pl < ql ? pl : ql;
    for (u32 k = 0; k < m; k++) {
        const u32 x = p[k], y = q[k];
        if (x != y) return x < y ? -1 : 1;
    }
    if (pl == ql) return 0;
    const u32 x = pl > m ? p[m] : term, y = ql > m ? q[m] : term;
    if (x != y) return x < y ? -1 : 1;
    return pl < ql ? -1 : 1;  // (only a name holding '/': status 3 anyway)
}

__global__ __launch_bounds__(256) void k_th_check(ThArgs a) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    u64 lo = 0, hi = a.nt + 1;  // the first seg index whose value is above i
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a.seg[mid] <= i) lo = mid + 1; else hi = mid;
    }
    u32 t = TH_NONE;
    u64 rl = 0, rh = 0;
    if (lo >= 1 && lo <= a.nt) {
        th_run(a, lo - 1, &rl, &rh);
        if (i >= rl && i < rh) t = (u32)(lo - 1);
    }
    a.own[i] = t;
    if (t == TH_NONE) return;
    u64 s;
    u32 len;
    u32 bad = 0;
    if (!th_name(a, i, &s, &len)) bad = 3;
    const u8* nm = a.name + s;
    for (u32 k = 0; k < len; k++) {
        const u32 c = nm[k];
        if (c == 0 || c == '/') bad = 3;
    }
    const u32 term = a.kind == KD_TE_TREE ? (u32)'/' : 0u;
    if (a.rank) {
        u32 before = 0;
        if (rh - rl > TH_RANK_MAX) {
            a.tot[2] = 1;
        } else {
            for (u64 j = rl; j < rh; j++) {
                if (j == i) continue;
                u64 sj;
                u32 lj;
                th_name(a, j, &sj, &lj);
                const int c = th_cmp(a.name + sj, lj, nm, len, term);
                if (c < 0) before += 28u + lj;
                if (c == 0 && bad < 2) bad = 2;
            }
        }
        a.roff[i] = before;
    } else if (i > rl) {
        u64 sp;
        u32 lp;
        th_name(a, i - 1, &sp, &lp);
        if (th_cmp(a.name + sp, lp, nm, len, term) >= 0 && bad < 1) bad = 1;
    }
    if (bad) atomicMax(a.st + t, bad);
}

__global__ __launch_bounds__(256) void k_th_size(ThArgs a) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nt) return;
    u64 rl, rh;
    th_run(a, t, &rl, &rh);
    const u32 s = a.st[t];
    a.status[t] = (u8)s;
    u64x2 z = {0, 0};
    if (!s) {
        const u64 blen = (rh - rl) * (th_mlen(a.kind) + 21) + (a.noff[rh] - a.noff[rl]);
        z.x = (6 + th_digits(blen) + blen + 9 + 63) / 64;
        z.y = blen;
    }
    a.sz[t] = z;
}

// ---- exclusive scan of sz over the trees: block sums, their scan by one block, the offsets ----
__device__ __forceinline__ u64x2 th_add(u64x2 p, u64x2 q) {
    u64x2 r = {p.x + q.x, p.y + q.y};
    return r;
}

__device__ __forceinline__ u64x2 th_shfl_up(u64x2 v, int o) {
    u64x2 r = {(u64)__shfl_up((unsigned long long)v.x, o, 64), (u64)__shfl_up((unsigned long long)v.y, o, 64)};
    return r;
}

// exclusive scan of one value per thread over a 256-thread block; *all <- the block's sum
__device__ __forceinline__ u64x2 th_block_scan(u64x2 v, u64x2 (*s_w)[4], int round, u64x2* all) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u64x2 s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64x2 y = th_shfl_up(s, o);
        if (lane >= o) s = th_add(s, y);
    }
    if (lane == 63) s_w[round & 1][wid] = s;
    __syncthreads();  // (the buffers alternate: one barrier per round)
    u64x2 wp = {0, 0}, sum = {0, 0};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const u64x2 x = s_w[round & 1][w];
        if (w < wid) wp = th_add(wp, x);
        sum = th_add(sum, x);
    }
    *all = sum;
    u64x2 r = {wp.x + s.x - v.x, wp.y + s.y - v.y};
    return r;
}

__global__ __launch_bounds__(256) void k_th_scan1(ThArgs a) {
    __shared__ u64x2 s_w[2][4];
    const u64 t0 = (u64)blockIdx.x * TH_SC;
    u64x2 acc = {0, 0};
    for (int r = 0; r < TH_SC / 256; r++) {
        const u64 t = t0 + (u64)r * 256 + threadIdx.x;
        if (t < a.nt) acc = th_add(acc, a.sz[t]);
    }
    u64x2 all;
    th_block_scan(acc, s_w, 0, &all);
    if (threadIdx.x == 0) a.bs[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void k_th_scan2(ThArgs a, u64 nb) {
    __shared__ u64x2 s_w[2][4];
    u64x2 carry = {0, 0};
    int round = 0;
    for (u64 b0 = 0; b0 < nb; b0 += 256, round++) {  // (block-uniform)
        const u64 b = b0 + threadIdx.x;
        u64x2 v = {0, 0};
        if (b < nb) v = a.bs[b];
        u64x2 all;
        const u64x2 e = th_block_scan(v, s_w, round, &all);
        if (b < nb) a.bs[b] = th_add(carry, e);
        carry = th_add(carry, all);
    }
    if (threadIdx.x == 0) {
        a.tot[0] = carry.x;
        a.tot[1] = carry.y;
        a.aoff[a.nt] = carry.x;
        a.boff[a.nt] = carry.y;
    }
}

__global__ __launch_bounds__(256) void k_th_scan3(ThArgs a) {
    __shared__ u64x2 s_w[2][4];
    const u64 t0 = (u64)blockIdx.x * TH_SC;
    u64x2 carry = a.bs[blockIdx.x];
    for (int r = 0; r < TH_SC / 256; r++) {  // (block-uniform)
        const u64 t = t0 + (u64)r * 256 + threadIdx.x;
        u64x2 v = {0, 0};
        if (t < a.nt) v = a.sz[t];
        u64x2 all;
        const u64x2 e = th_block_scan(v, s_w, r, &all);
        if (t < a.nt) {
            a.aoff[t] = carry.x + e.x;
            a.boff[t] = carry.y + e.y;
        }
        carry = th_add(carry, all);
    }
}

// ---- bytes ----
__device__ __forceinline__ u32 th_rl(u32 v, int e) { return (u32)__builtin_amdgcn_readlane((int)v, e); }
__device__ __forceinline__ u64 th_rl64(u64 v, int e) { return ((u64)th_rl((u32)(v >> 32), e) << 32) | th_rl((u32)v, e); }

// header "tree <decimal>\0" and the SHA-1 padding of 64 trees per wave
__global__ __launch_bounds__(256) void k_th_frame(ThArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= a.nt) return;  // (wave-uniform)
    const u64 t = c0 + lane;
    u64 base = 0, blen = 0;
    u32 nblk = 0;
    if (t < a.nt) {
        base = a.aoff[t] * 64;
        nblk = (u32)(a.aoff[t + 1] - a.aoff[t]);
        blen = a.boff[t + 1] - a.boff[t];
    }
    for (int e = 0; e < 64; e++) {
        const u32 nb = th_rl(nblk, e);
        if (!nb) continue;
        const u64 d = th_rl64(base, e), bl = th_rl64(blen, e);
        const u32 nd = th_digits(bl);
        const u32 hdr = 6 + nd;
        if ((u32)lane < hdr) {
            u32 v = 0;
            if (lane < 5) {
                v = (u32)((0x2065657274ull >> (8 * lane)) & 0xff);  // "tree "
            } else if ((u32)lane < 5 + nd) {
                const u64 p = TH_P10[nd - 1 - (lane - 5)];
                v = '0' + ((bl >> 32) == 0 ? ((u32)bl / (u32)p) % 10u : (u32)((bl / p) % 10ull));
            }
            a.arena[d + lane] = (u8)v;
        }
        const u64 obj = hdr + bl, total = (u64)nb * 64, bits = obj * 8;
        for (u64 pos = obj + lane; pos < total; pos += 64) {
            u32 v = 0;
            if (pos == obj) v = 0x80;
            else if (pos >= total - 8) v = (u32)(bits >> (8 * (total - 1 - pos))) & 0xff;
            a.arena[d + pos] = (u8)v;
        }
    }
}

// the records "<mode> <name>\0<oid>" of 64 entries per wave
__global__ __launch_bounds__(256) void k_th_format(ThArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= a.n) return;  // (wave-uniform)
    const u32 mlen = th_mlen(a.kind);
    const u64 mode = a.kind == KD_TE_TREE ? 0x203030303034ull : 0x20343436303031ull;  // "40000 " / "100644 "
    const u64 i = c0 + lane;
    u32 rec = 0, len = 0;
    u64 dst = 0, bdst = 0, ns = 0;
    if (i < a.n) {
        const u32 t = a.own[i];
        if (t != TH_NONE && a.st[t] == 0) {
            u64 rl, rh;
            th_run(a, t, &rl, &rh);
            th_name(a, i, &ns, &len);
            const u64 within = a.rank ? (u64)a.roff[i] : (i - rl) * (mlen + 21) + (ns - a.noff[rl]);
            const u64 b0 = a.boff[t];
            dst = a.aoff[t] * 64 + 6 + th_digits(a.boff[t + 1] - b0) + within;
            bdst = b0 + within;
            rec = mlen + len + 21;
        }
    }
    for (int e = 0; e < 64; e++) {
        const u32 r = th_rl(rec, e);
        if (!r) continue;
        const u64 d = th_rl64(dst, e), bd = th_rl64(bdst, e), s = th_rl64(ns, e);
        const u32 L = th_rl(len, e);
        const u8* o = a.oid + 20 * (c0 + (u64)e);
        for (u32 b = lane; b < r; b += 64) {
            u32 v = 0;
            if (b < mlen) v = (u32)(mode >> (8 * b)) & 0xff;
            else if (b < mlen + L) v = a.name[s + (b - mlen)];
            else if (b > mlen + L) v = o[b - mlen - L - 1];
            a.arena[d + b] = (u8)v;
            if (a.body) a.body[bd + b] = (u8)v;
        }
    }
}

// ---- SHA-1 (FIPS 180-4), one lane per tree ----
#define TH_W(i) w[(i) & 15]
#define TH_SCHED(i) (TH_W(i) = __builtin_rotateleft32(TH_W(i + 13) ^ TH_W(i + 8) ^ TH_W(i + 2) ^ TH_W(i), 1))
#define TH_ROUND(f, k, x)                                          \
    {                                                              \
        const u32 tmp = __builtin_rotateleft32(A, 5) + (f) + E + (k) + (x); \
        E = D;                                                     \
        D = C;                                                     \
        C = __builtin_rotateleft32(B, 30);                         \
        B = A;                                                     \
        A = tmp;                                                   \
    }

__global__ __launch_bounds__(256) void k_th_sha1(ThArgs a) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nt) return;
    const u64 b0 = a.aoff[t], nb = a.aoff[t + 1] - b0;
    u32 h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
    if (nb) {
        h0 = 0x67452301u; h1 = 0xEFCDAB89u; h2 = 0x98BADCFEu; h3 = 0x10325476u; h4 = 0xC3D2E1F0u;
        const u32x4* p = (const u32x4*)(a.arena + b0 * 64);
        for (u64 b = 0; b < nb; b++, p += 4) {
            u32 w[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32x4 v = p[j];
                w[4 * j] = __builtin_bswap32(v.x);
                w[4 * j + 1] = __builtin_bswap32(v.y);
                w[4 * j + 2] = __builtin_bswap32(v.z);
                w[4 * j + 3] = __builtin_bswap32(v.w);
            }
            u32 A = h0, B = h1, C = h2, D = h3, E = h4;
#pragma unroll
            for (int i = 0; i < 16; i++) TH_ROUND((B & C) | (~B & D), 0x5A827999u, TH_W(i))
#pragma unroll
            for (int i = 16; i < 20; i++) TH_ROUND((B & C) | (~B & D), 0x5A827999u, TH_SCHED(i))
#pragma unroll
            for (int i = 20; i < 40; i++) TH_ROUND(B ^ C ^ D, 0x6ED9EBA1u, TH_SCHED(i))
#pragma unroll
            for (int i = 40; i < 60; i++) TH_ROUND((B & C) | (B & D) | (C & D), 0x8F1BBCDCu, TH_SCHED(i))
#pragma unroll
            for (int i = 60; i < 80; i++) TH_ROUND(B ^ C ^ D, 0xCA62C1D6u, TH_SCHED(i))
            h0 += A; h1 += B; h2 += C; h3 += D; h4 += E;
        }
        h0 = __builtin_bswap32(h0); h1 = __builtin_bswap32(h1); h2 = __builtin_bswap32(h2);
        h3 = __builtin_bswap32(h3); h4 = __builtin_bswap32(h4);
    }
    u32* o = a.out_oid + 5 * t;
    o[0] = h0; o[1] = h1; o[2] = h2; o[3] = h3; o[4] = h4;
}

}  // namespace kd

using namespace kd;

extern "C" int kd_tree_hash(kd_ctx* ctx, const kd_tree_entries* e, const uint64_t* seg, uint64_t n_trees, uint32_t flags,
                            uint8_t* tree_oid, uint8_t* status, uint8_t* body, uint64_t* body_off, uint64_t body_cap,
                            uint32_t out_mem) {
    KD_CHECK(ctx && e, "kd_tree_hash: NULL argument");
    KD_CHECK(e->kind == KD_TE_BLOB || e->kind == KD_TE_TREE, "kd_tree_hash: kind must be KD_TE_BLOB or KD_TE_TREE");
    KD_CHECK((flags & ~KD_TH_RANK_NAMES) == 0, "kd_tree_hash: unknown flag");
    KD_CHECK(!(flags & KD_TH_RANK_NAMES) || e->kind == KD_TE_BLOB, "kd_tree_hash: KD_TH_RANK_NAMES orders blob entries only");
    KD_CHECK((body == nullptr) == (body_off == nullptr), "kd_tree_hash: body and body_off go together");
    KD_CHECK(e->n < 0xFFFFFFFFull && n_trees < 0xFFFFFFFFull, "kd_tree_hash: too many entries or trees");
    if (n_trees == 0) return KD_OK;
    KD_CHECK(seg && tree_oid && status, "kd_tree_hash: NULL seg or output");
    KD_CHECK(e->name_off && (e->n == 0 || (e->name && e->oid)), "kd_tree_hash: NULL entry array");
    KD_CHECK(((uintptr_t)tree_oid & 3) == 0, "kd_tree_hash: tree_oid must be 4-byte aligned");
    const u64 n = e->n, nt = n_trees;
    const bool host_in = e->mem == KD_MEM_HOST, host_out = out_mem == KD_MEM_HOST;
    u64 name_bytes = 0;
    if (host_in) {  // (device arrays are clamped by the kernels instead)
        for (u64 i = 0; i < n; i++) KD_CHECK(e->name_off[i] <= e->name_off[i + 1], "kd_tree_hash: name_off descends");
        KD_CHECK(seg[nt] <= n, "kd_tree_hash: seg runs past the entries");
        for (u64 t = 0; t < nt; t++) KD_CHECK(seg[t] <= seg[t + 1], "kd_tree_hash: seg descends");
        name_bytes = e->name_off[n];
    }
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    ThArgs a{};
    const void *dn, *dno, *doid, *dseg;
    // (device names pass through whatever their size; host names of no bytes are never read)
    if ((rc = stage_in(ctx, "th.name", host_in && !name_bytes ? nullptr : e->name, name_bytes, e->mem, &dn)) ||
        (rc = stage_in(ctx, "th.noff", e->name_off, 8 * (n + 1), e->mem, &dno)) ||
        (rc = stage_in(ctx, "th.oid", n ? e->oid : nullptr, 20 * n, e->mem, &doid)) ||
        (rc = stage_in(ctx, "th.seg", seg, 8 * (nt + 1), e->mem, &dseg)))
        return rc;
    a.name = (const u8*)dn;
    a.noff = (const u64*)dno;
    a.oid = (const u8*)doid;
    a.seg = (const u64*)dseg;
    a.n = n;
    a.nt = nt;
    a.kind = e->kind;
    a.rank = flags & KD_TH_RANK_NAMES ? 1u : 0u;
    const u64 nsb = (nt + TH_SC - 1) / TH_SC;
    void *w_own, *w_roff, *w_st, *w_sz, *w_aoff, *w_boff, *w_bs, *w_tot;
    if ((rc = ensure(ctx, "th.own", 4 * n, &w_own)) || (rc = ensure(ctx, "th.roff", a.rank ? 4 * n : 0, &w_roff)) ||
        (rc = ensure(ctx, "th.st", 4 * nt, &w_st)) || (rc = ensure(ctx, "th.sz", 16 * nt, &w_sz)) ||
        (rc = ensure(ctx, "th.aoff", 8 * (nt + 1), &w_aoff)) || (rc = ensure(ctx, "th.boff", 8 * (nt + 1), &w_boff)) ||
        (rc = ensure(ctx, "th.bs", 16 * nsb, &w_bs)) || (rc = ensure(ctx, "th.tot", 32, &w_tot)))
        return rc;
    void *o_oid = tree_oid, *o_st = status, *o_body = body;
    if (host_out) {
        if ((rc = ensure(ctx, "th.o_oid", 20 * nt, &o_oid)) || (rc = ensure(ctx, "th.o_st", nt, &o_st))) return rc;
    }
    a.own = (u32*)w_own;
    a.roff = (u32*)w_roff;
    a.st = (u32*)w_st;
    a.sz = (u64x2*)w_sz;
    a.aoff = (u64*)w_aoff;
    a.boff = body_off && !host_out ? body_off : (u64*)w_boff;
    a.bs = (u64x2*)w_bs;
    a.tot = (u64*)w_tot;
    a.out_oid = (u32*)o_oid;
    a.status = (u8*)o_st;
    const dim3 tb(256);
    const dim3 ge((unsigned)((n + 255) / 256)), gt((unsigned)((nt + 255) / 256));
    KD_HIP(hipMemsetAsync(a.st, 0, 4 * nt, ctx->stream));
    KD_HIP(hipMemsetAsync(a.tot, 0, 32, ctx->stream));
    if (n && (rc = launch(ctx, "k_th_check", [&] { hipLaunchKernelGGL(k_th_check, ge, tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_th_size", [&] { hipLaunchKernelGGL(k_th_size, gt, tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_th_scan1", [&] { hipLaunchKernelGGL(k_th_scan1, dim3((unsigned)nsb), tb, 0, ctx->stream, a); })))
        return rc;
    if ((rc = launch(ctx, "k_th_scan2", [&] { hipLaunchKernelGGL(k_th_scan2, dim3(1), tb, 0, ctx->stream, a, nsb); })))
        return rc;
    if ((rc = launch(ctx, "k_th_scan3", [&] { hipLaunchKernelGGL(k_th_scan3, dim3((unsigned)nsb), tb, 0, ctx->stream, a); })))
        return rc;
    u64 tot[4] = {0, 0, 0, 0};
    KD_HIP(hipMemcpyAsync(tot, a.tot, 32, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    if (tot[2]) {
        set_error("kd_tree_hash: KD_TH_RANK_NAMES orders runs of up to %llu entries", (unsigned long long)TH_RANK_MAX);
        return KD_EUNSUPPORTED;
    }
    KD_CHECK(!body || tot[1] <= body_cap, "kd_tree_hash: body_cap %llu below the %llu bytes needed",
             (unsigned long long)body_cap, (unsigned long long)tot[1]);
    void* w_arena;
    if ((rc = ensure(ctx, "th.arena", 64 * tot[0], &w_arena))) return rc;
    a.arena = (u8*)w_arena;
    if (body && host_out && (rc = ensure(ctx, "th.o_body", tot[1], &o_body))) return rc;
    a.body = body ? (u8*)o_body : nullptr;
    const dim3 gfe((unsigned)((n + 255) / 256)), gft((unsigned)((nt + 255) / 256));  // 4 waves of 64 items per block
    if ((rc = launch(ctx, "k_th_frame", [&] { hipLaunchKernelGGL(k_th_frame, gft, tb, 0, ctx->stream, a); }))) return rc;
    if (n && (rc = launch(ctx, "k_th_format", [&] { hipLaunchKernelGGL(k_th_format, gfe, tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_th_sha1", [&] { hipLaunchKernelGGL(k_th_sha1, gt, tb, 0, ctx->stream, a); }))) return rc;
    if (!host_out) return KD_OK;
    if ((rc = stage_d2h(ctx, tree_oid, o_oid, 20 * nt)) || (rc = stage_d2h(ctx, status, o_st, nt))) return rc;
    if (body) {
        if ((rc = stage_d2h(ctx, body_off, a.boff, 8 * (nt + 1)))) return rc;
        if (tot[1] && (rc = stage_d2h(ctx, body, o_body, tot[1]))) return rc;
    }
    return prof_flush(ctx);
}
