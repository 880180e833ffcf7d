// kd_treewalk.hip — kd_tree_join_batch: changed leaf trees parsed, joined and pruned on the GPU.
//
// <- the lowest level of a pruned walk (Walk::join + Walk::pruned, kd_odb_walk.cpp) at a high edit rate:
// every leaf tree of both sides has changed, and each one is parsed and merge-joined entry by entry.
// The trees arrive inflated in one arena (k_inf_streams / k_dl_apply put them there); a task names up
// to three of them, one per root, and a path prefix.
//
// k_tj_count<K> / k_tj_emit<K>: one lane per task, one wave per workgroup, as k_inf_streams.  The
// decoder is kd_treeparse.h (shared with the host).  A lane first validates each of its trees from end
// to end, then runs the K-way merge twice: the count pass adds up what each root keeps (entries and
// path bytes), k_gf_scan turns the counts into positions, the emit pass repeats the merge and writes
// at them.  No atomic decides a position.  Entry boundaries are a sequential chain per tree (SP from
// the entry's start, NUL from the name's start, next entry 21 bytes behind the NUL): the
// searches stop at their first hit and never run over an OID, so an OID's 0x00 / 0x20 bytes
// cannot be taken for a boundary.  Loads and stores are 8 bytes wide at byte addresses (the mode and
// name scans, the name and OID compares, the emit pass's prefix, name and OID copies; tails a byte
// each): a search's chunk begins at the search's start, so its lowest hit is the first hit at or after
// that start, and bytes beyond a tree are masked off — the arena must be readable 8 bytes past its
// last tree.  The accesses are the lane's own: a wave's loads are not coalesced.
// Name compares are unsigned.  Nothing depends on the number of entries of a tree.  The per-root
// state is indexed only inside fully unrolled loops over K (no scratch, no LDS).
//
// The counts of all roots lie in one array, [2 * K] segments of n_task words (root r's entries, then
// its path bytes) and one closing word, scanned in one launch; a segment's positions are relative to
// its first word.
#include "kd_treeparse.h"
#include "kd_internal.h"

namespace kd {

constexpr int TJ_NT = 64;    // lanes per workgroup: one wave, one task per lane
constexpr int TJ_KMAX = 3;   // roots

struct TjRoot {
    u64* path_off;
    u32* mode;
    u8* oid;
    u8* path;
    u64 cap_n, cap_bytes;
};

struct TjArgs {
    const u8* data;
    const u64* off;  // [n_trees + 1]
    u64 n_trees;
    const u32* tree;  // [n_task * K]
    const u8* pfx;
    const u64* pfx_off;  // [n_task + 1]
    u64 n_task;
    int c0, c1;
    u32* scan;    // [2 * K * n_task + 1]
    u32* count;   // [n_task * K]
    u8* status;   // [n_task]
    u64* totals;  // [2 * K]
    TjRoot out[TJ_KMAX];
};

template <int K>
struct TjTask : kd_tj::Trees<K> {
    const u8* pre;
    u32 plen;
};

typedef u64 __attribute__((aligned(1))) tj_u64_b;
typedef u32 __attribute__((aligned(1))) tj_u32_b;

// n bytes from s to w, 8 per load and store while 8 remain, the rest a byte each: no byte outside
// s[0 .. n) is read, none outside w[0 .. n) written
__device__ __forceinline__ void tj_copy(u8* w, const u8* s, u32 n) {
    u32 i = 0;
    for (; i + 8 <= n; i += 8) *(tj_u64_b*)(w + i) = kd_tj::load8(s + i);
    for (; i < n; i++) w[i] = s[i];
}

// device offsets are nobody's checked input: a task's trees and prefix stay inside their arenas
template <int K>
__device__ __forceinline__ u32 tj_setup(const TjArgs& a, u64 t, TjTask<K>& T) {
    u32 st = KD_TJ_OK;
    const u64 po = a.pfx_off[t], pe = a.pfx_off[t + 1], pn = a.pfx_off[a.n_task];
    T.pre = a.pfx;
    T.plen = 0;
    if (po <= pe && pe <= pn) {
        if (pe - po > KD_TJ_MAX_BYTES) st = KD_TJ_EBIG;
        else {
            T.pre = a.pfx + po;
            T.plen = (u32)(pe - po);
        }
    } else {
        st = KD_TJ_ERANGE;
    }
    const u64 dn = a.off[a.n_trees];
#pragma unroll
    for (int r = 0; r < K; r++) {
        T.p[r] = a.data;
        T.len[r] = 0;
        T.has[r] = false;
        const u64 i = a.tree[t * K + r];
        if (i == KD_NONE) continue;
        if (i >= a.n_trees) {
            st = st ? st : KD_TJ_ERANGE;
            continue;
        }
        const u64 o = a.off[i], e = a.off[i + 1];
        if (o <= e && e <= dn) {
            T.p[r] = a.data + o;
            T.len[r] = e - o;
            T.has[r] = true;
        } else {
            st = st ? st : KD_TJ_ERANGE;
        }
    }
    return st;
}

template <int K>
__global__ __launch_bounds__(TJ_NT) void k_tj_count(TjArgs a) {
    const u64 t = (u64)blockIdx.x * TJ_NT + threadIdx.x;
    if (t >= a.n_task) return;
    if (t == 0) a.scan[2 * K * a.n_task] = 0;
    TjTask<K> T;
    u32 st = tj_setup<K>(a, t, T);
    if (st == KD_TJ_OK) st = kd_tj::task_status<K>(T);
    u64 ne[K], nb[K];
#pragma unroll
    for (int r = 0; r < K; r++) ne[r] = nb[r] = 0;
    if (st == KD_TJ_OK) {
        const u64 lead = (u64)T.plen + (T.plen ? 1 : 0);
        kd_tj::join<K>(T, a.c0, a.c1, [&](int r, const kd_tj::Ent& e) {
            ne[r]++;
            nb[r] += lead + e.nlen;
        });
#pragma unroll
        for (int r = 0; r < K; r++)
            if (nb[r] > 0xFFFFFFFFull) st = KD_TJ_EBIG;  // (ne <= nb)
    }
#pragma unroll
    for (int r = 0; r < K; r++) {
        const u32 cn = st == KD_TJ_OK ? (u32)ne[r] : 0u, cb = st == KD_TJ_OK ? (u32)nb[r] : 0u;
        a.scan[(u64)(2 * r) * a.n_task + t] = cn;
        a.scan[(u64)(2 * r + 1) * a.n_task + t] = cb;
        a.count[t * K + r] = cn;
    }
    a.status[t] = (u8)st;
}

template <int K>
__global__ __launch_bounds__(TJ_NT) void k_tj_emit(TjArgs a) {
    const u64 t = (u64)blockIdx.x * TJ_NT + threadIdx.x;
    if (t >= a.n_task) return;
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < K; r++) {
            const u64 n = a.scan[(u64)(2 * r + 1) * a.n_task] - a.scan[(u64)(2 * r) * a.n_task];
            const u64 b = a.scan[(u64)(2 * r + 2) * a.n_task] - a.scan[(u64)(2 * r + 1) * a.n_task];
            if (a.totals) {
                a.totals[2 * r] = n;
                a.totals[2 * r + 1] = b;
            }
            a.out[r].path_off[0] = 0;
        }
    }
    if (a.status[t] != KD_TJ_OK) return;
    TjTask<K> T;
    if (tj_setup<K>(a, t, T) != KD_TJ_OK) return;
    u64 E[K], B[K], En[K], Bn[K];
    bool fits = true;
#pragma unroll
    for (int r = 0; r < K; r++) {
        const u64 se = (u64)(2 * r) * a.n_task, sb = (u64)(2 * r + 1) * a.n_task;
        E[r] = a.scan[se + t] - a.scan[se];
        En[r] = E[r] + (a.scan[se + t + 1] - a.scan[se + t]);
        B[r] = a.scan[sb + t] - a.scan[sb];
        Bn[r] = B[r] + (a.scan[sb + t + 1] - a.scan[sb + t]);
        fits = fits && En[r] <= a.out[r].cap_n && Bn[r] <= a.out[r].cap_bytes;
    }
    if (!fits) {
        a.status[t] = (u8)KD_TJ_ECAP;
#pragma unroll
        for (int r = 0; r < K; r++) a.count[t * K + r] = 0;
        return;
    }
    const u32 plen = T.plen;
    const u8* pre = T.pre;
    kd_tj::join<K>(T, a.c0, a.c1, [&](int r, const kd_tj::Ent& e) {
        const u64 need = (u64)plen + (plen ? 1 : 0) + e.nlen;
        // (the count pass saw these same bytes; the guard keeps every store inside the task's own ranges
        // whatever the arena holds now)
        if (E[r] >= En[r] || need > Bn[r] - B[r]) return;
        const TjRoot& o = a.out[r];
        const u8* src = T.p[r];
        u8* w = o.path + B[r];
        tj_copy(w, pre, plen);
        if (plen) w[plen] = '/';
        tj_copy(w + (need - e.nlen), src + e.name, e.nlen);
        u8* wo = o.oid + 20 * E[r];
        const u8* so = src + e.oid;
        *(tj_u64_b*)wo = kd_tj::load8(so);
        *(tj_u64_b*)(wo + 8) = kd_tj::load8(so + 8);
        *(tj_u32_b*)(wo + 16) = (u32)(kd_tj::load8(so + 12) >> 32);
        o.mode[E[r]] = e.mode;
        B[r] += need;
        E[r]++;
        o.path_off[E[r]] = B[r];
    });
}

template <int K>
static int tj_launch(kd_ctx* ctx, const TjArgs& a, bool emit) {
    const u64 nwg = (a.n_task + TJ_NT - 1) / TJ_NT;
    if (emit) return launch(ctx, "k_tj_emit", [&] { hipLaunchKernelGGL(k_tj_emit<K>, dim3((unsigned)nwg), dim3(TJ_NT), 0, ctx->stream, a); });
    return launch(ctx, "k_tj_count", [&] { hipLaunchKernelGGL(k_tj_count<K>, dim3((unsigned)nwg), dim3(TJ_NT), 0, ctx->stream, a); });
}

static int tj_pass(kd_ctx* ctx, const TjArgs& a, int k, bool emit) {
    return k == 1 ? tj_launch<1>(ctx, a, emit) : k == 2 ? tj_launch<2>(ctx, a, emit) : tj_launch<3>(ctx, a, emit);
}

}  // namespace kd

using namespace kd;

static int tj_check_offsets(const u64* off, u64 n, const char* what) {
    for (u64 i = 0; i < n; i++) KD_CHECK(off[i] <= off[i + 1], "kd_tree_join_batch: %s descends at %llu", what, (unsigned long long)i);
    return KD_OK;
}

extern "C" int kd_tree_join_batch(kd_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n_trees, const uint32_t* tree,
                                  const uint8_t* pfx, const uint64_t* pfx_off, uint64_t n_task, int k, int cmp0, int cmp1,
                                  kd_tj_out* out, uint32_t* count, uint8_t* status, uint64_t* totals, uint32_t mem) {
    KD_CHECK(ctx, "kd_tree_join_batch: NULL context");
    KD_CHECK(mem == KD_MEM_HOST || mem == KD_MEM_DEVICE, "kd_tree_join_batch: mem must be KD_MEM_HOST or KD_MEM_DEVICE");
    KD_CHECK(k >= 1 && k <= TJ_KMAX, "kd_tree_join_batch: k = %d", k);
    KD_CHECK((cmp0 < 0) == (cmp1 < 0) && cmp0 < k && cmp1 < k && (cmp0 < 0 || cmp0 != cmp1),
             "kd_tree_join_batch: compare roots %d/%d of %d", cmp0, cmp1, k);
    KD_CHECK(out && off && pfx_off, "kd_tree_join_batch: NULL argument");
    KD_CHECK(n_task == 0 || (tree && count && status), "kd_tree_join_batch: NULL argument");
    KD_CHECK(n_task < (1ull << 32) / (2 * TJ_KMAX) && n_trees < KD_NONE, "kd_tree_join_batch: too many tasks or trees");
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    TjArgs a{};
    a.n_trees = n_trees;
    a.n_task = n_task;
    a.c0 = cmp0 < 0 ? -1 : cmp0;
    a.c1 = cmp1 < 0 ? -1 : cmp1;
    const u64 nscan = 2 * (u64)k * n_task + 1;
    void *d_scan, *d_tot;
    if ((rc = ensure(ctx, "tj.scan", 4 * nscan + 16, &d_scan)) || (rc = ensure(ctx, "tj.tot", 16 * TJ_KMAX + 16, &d_tot))) return rc;
    a.scan = (u32*)d_scan;
    u64* d_total = (u64*)d_tot + 2 * TJ_KMAX;  // the scan's own total (the closing word says the same)
    if (mem == KD_MEM_DEVICE) {
        if (n_task == 0) return KD_OK;
        KD_CHECK(data && pfx, "kd_tree_join_batch: NULL argument");
        a.data = data;
        a.off = off;
        a.tree = tree;
        a.pfx = pfx;
        a.pfx_off = pfx_off;
        a.count = count;
        a.status = status;
        a.totals = totals;
        for (int r = 0; r < k; r++) {
            KD_CHECK(out[r].path_off && out[r].mode && out[r].oid && out[r].path, "kd_tree_join_batch: NULL output array");
            a.out[r] = TjRoot{out[r].path_off, out[r].mode, out[r].oid, out[r].path, out[r].cap_n, out[r].cap_bytes};
        }
        if ((rc = tj_pass(ctx, a, k, false)) || (rc = gf_scan(ctx, a.scan, (u32)nscan, d_total))) return rc;
        return tj_pass(ctx, a, k, true);
    }
    for (int r = 0; r < k; r++) {
        KD_CHECK(out[r].path_off, "kd_tree_join_batch: NULL output array");
        out[r].n = out[r].bytes = 0;
        out[r].path_off[0] = 0;
    }
    if (n_task == 0) return KD_OK;
    if ((rc = tj_check_offsets(off, n_trees, "off")) || (rc = tj_check_offsets(pfx_off, n_task, "pfx_off"))) return rc;
    const u64 dbytes = off[n_trees] - off[0], pbytes = pfx_off[n_task] - pfx_off[0];
    KD_CHECK((dbytes == 0 || data) && (pbytes == 0 || pfx), "kd_tree_join_batch: NULL argument");
    // the 32-bit scan: an upper bound of everything the call could keep (a tree of L bytes has at most
    // L / 23 entries, whose names are part of the L bytes)
    {
        u64 bound = 0;
        for (u64 t = 0; t < n_task; t++) {
            const u64 lead = pfx_off[t + 1] - pfx_off[t] + 1;
            for (int r = 0; r < k; r++) {
                const u32 i = tree[t * k + r];
                if (i == KD_NONE || i >= n_trees) continue;
                const u64 L = off[i + 1] - off[i];
                if (L > KD_TJ_MAX_BYTES || lead > KD_TJ_MAX_BYTES) continue;  // (KD_TJ_EBIG: keeps nothing)
                bound += L + (L / 23) * (lead + 1);
            }
        }
        KD_CHECK(bound < (1ull << 32), "kd_tree_join_batch: the batch could keep 2^32 entries and path bytes: split it");
    }
    // the staged arenas start at their first item: offsets are uploaded relative to it
    std::vector<u64> rel((n_trees + 1) + (n_task + 1));
    for (u64 i = 0; i <= n_trees; i++) rel[i] = off[i] - off[0];
    for (u64 t = 0; t <= n_task; t++) rel[n_trees + 1 + t] = pfx_off[t] - pfx_off[0];
    void *d_data, *d_off, *d_tree, *d_pfx, *d_cnt, *d_st;
    if ((rc = ensure(ctx, "tj.data", dbytes + 16, &d_data)) || (rc = ensure(ctx, "tj.off", 8 * rel.size(), &d_off)) ||
        (rc = ensure(ctx, "tj.tree", 4 * n_task * k, &d_tree)) || (rc = ensure(ctx, "tj.pfx", std::max<u64>(pbytes, 16), &d_pfx)) ||
        (rc = ensure(ctx, "tj.cnt", 4 * n_task * k, &d_cnt)) || (rc = ensure(ctx, "tj.st", n_task, &d_st)))
        return rc;
    if (dbytes && (rc = stage_h2d(ctx, d_data, data + off[0], dbytes))) return rc;
    if (pbytes && (rc = stage_h2d(ctx, d_pfx, pfx + pfx_off[0], pbytes))) return rc;
    if ((rc = stage_h2d(ctx, d_off, rel.data(), 8 * rel.size()))) return rc;
    if ((rc = stage_h2d(ctx, d_tree, tree, 4 * n_task * k))) return rc;
    KD_HIP(hipStreamSynchronize(ctx->stream));  // (rel is read by a pageable copy)
    a.data = (const u8*)d_data;
    a.off = (const u64*)d_off;
    a.tree = (const u32*)d_tree;
    a.pfx = (const u8*)d_pfx;
    a.pfx_off = (const u64*)d_off + n_trees + 1;
    a.count = (u32*)d_cnt;
    a.status = (u8*)d_st;
    a.totals = nullptr;
    if ((rc = tj_pass(ctx, a, k, false)) || (rc = gf_scan(ctx, a.scan, (u32)nscan, d_total))) return rc;
    // every root's totals: the first word of each segment and the closing word
    u32 seg[2 * TJ_KMAX + 1];
    for (int s = 0; s <= 2 * k; s++)
        if ((rc = stage_d2h(ctx, &seg[s], a.scan + (u64)s * n_task, 4))) return rc;
    if ((rc = stage_d2h(ctx, count, d_cnt, 4 * n_task * k)) || (rc = stage_d2h(ctx, status, d_st, n_task))) return rc;
    u64 tn[TJ_KMAX], tb[TJ_KMAX];
    for (int r = 0; r < k; r++) {
        tn[r] = seg[2 * r + 1] - seg[2 * r];
        tb[r] = seg[2 * r + 2] - seg[2 * r + 1];
        KD_CHECK(tn[r] <= out[r].cap_n && tb[r] <= out[r].cap_bytes,
                 "kd_tree_join_batch: root %d keeps %llu entries / %llu path bytes, above its capacity", r,
                 (unsigned long long)tn[r], (unsigned long long)tb[r]);
        KD_CHECK(tn[r] == 0 || (out[r].mode && out[r].oid), "kd_tree_join_batch: NULL output array");
        KD_CHECK(tb[r] == 0 || out[r].path, "kd_tree_join_batch: NULL output array");
    }
    static const char* const slots[TJ_KMAX][4] = {{"tj.o0.poff", "tj.o0.mode", "tj.o0.oid", "tj.o0.path"},
                                                  {"tj.o1.poff", "tj.o1.mode", "tj.o1.oid", "tj.o1.path"},
                                                  {"tj.o2.poff", "tj.o2.mode", "tj.o2.oid", "tj.o2.path"}};
    for (int r = 0; r < k; r++) {
        void *po, *mo, *oo, *pa;
        if ((rc = ensure(ctx, slots[r][0], 8 * (tn[r] + 1), &po)) || (rc = ensure(ctx, slots[r][1], std::max<u64>(4 * tn[r], 16), &mo)) ||
            (rc = ensure(ctx, slots[r][2], std::max<u64>(20 * tn[r], 16), &oo)) || (rc = ensure(ctx, slots[r][3], std::max<u64>(tb[r], 16), &pa)))
            return rc;
        a.out[r] = TjRoot{(u64*)po, (u32*)mo, (u8*)oo, (u8*)pa, tn[r], tb[r]};
    }
    if ((rc = tj_pass(ctx, a, k, true))) return rc;
    for (int r = 0; r < k; r++) {
        if ((rc = stage_d2h(ctx, out[r].path_off, a.out[r].path_off, 8 * (tn[r] + 1)))) return rc;
        if (tn[r] && ((rc = stage_d2h(ctx, out[r].mode, a.out[r].mode, 4 * tn[r])) || (rc = stage_d2h(ctx, out[r].oid, a.out[r].oid, 20 * tn[r]))))
            return rc;
        if (tb[r] && (rc = stage_d2h(ctx, out[r].path, a.out[r].path, tb[r]))) return rc;
        out[r].n = tn[r];
        out[r].bytes = tb[r];
    }
    return prof_flush(ctx);
}
