// kd_delta.hip — kd_delta_apply_batch: one level of git deltas applied on the GPU.
//
// <- the blob read under the field diff on a repository that was cloned, gc'd or repacked: most feature
// blobs are OFS_DELTA / REF_DELTA entries against an earlier version of the same feature.  The host
// plans a batch into levels of a delta forest (kd_odb_read_batch_device_ex, kd_odb_plan.cpp); k_inf_streams
// inflates the chain bases and the delta payloads, this kernel patches one level per launch.
//
// k_dl_apply: DL_G = 16 lanes per item, four items per wave, 16 per workgroup of 256.  The decoder is
// kd_delta.h (shared with the host).  A group walks its item's op stream together — every lane of the
// group loads the same delta bytes, so the loads are uniform within the group — validates the op, then
// moves its bytes cooperatively: 16 B per lane per step, byte-addressed 16-B loads and stores (gfx950
// runs in unaligned mode, as coop_differs_u in kd_fielddiff.hip relies on).  An op of 16 bytes or more
// ends with one 16-B step at (length - 16), overlapping the step before it with the same bytes; an op
// below 16 bytes is moved a byte per lane.  Neither touches a byte outside the op's ranges.  Sources
// (base, delta) are never written by the launch and an item's ops write disjoint parts of its own dst
// range, so nothing inside an item is ordered but its status.  No LDS, no scratch.
//
// Two forms of one body: the flat one of the C ABI (three arenas with offsets, base_idx), and the
// chained one of the planner (kd::DlItem: each range in the arena or the workspace, parents' statuses).
#include "kd_delta.h"
#include "kd_internal.h"

namespace kd {

constexpr int DL_G = 16;             // lanes per item
constexpr int DL_NT = 256;           // lanes per workgroup
constexpr int DL_IPB = DL_NT / DL_G; // items per workgroup (64 / DL_G = 4 per wave)

typedef u32x4 __attribute__((aligned(1))) dl_u32x4_b;

struct DlArgs {
    u64 n;
    u8* status;
    // flat form
    const u8* base;
    const u64* base_off;  // [nb + 1]
    u64 nb;
    const u32* base_idx;  // [n]
    const u8* delta;
    const u64* delta_off;  // [n + 1]
    u8* dst;
    const u64* dst_off;  // [n + 1]
    // chained form
    const DlItem* items;
    u8* mem[2];
    u64 lim[2];
};

// len bytes from s to o by the group's 16 lanes (j = lane in the group); the ranges do not overlap
__device__ __forceinline__ void dl_move(u8* o, const u8* s, u32 len, u32 j) {
    if (len >= 16) {
        const u32 nch = (len + 15) >> 4;
        for (u32 c = j; c < nch; c += DL_G) {
            const u32 at = min(16 * c, len - 16);
            *(dl_u32x4_b*)(o + at) = *(const dl_u32x4_b*)(s + at);
        }
    } else if (j < len) {
        o[j] = s[j];
    }
}

__device__ __forceinline__ u32 dl_apply(const u8* b, u64 bl, const u8* d, u64 dl, u8* o, u64 ol, u32 j) {
    u64 pos, w = 0;
    u32 st = kd_dl::parse_header(d, dl, bl, ol, &pos);
    while (st == KD_DL_OK) {
        u32 kind, len;
        u64 src;
        st = kd_dl::next_op(d, dl, bl, ol, w, &pos, &kind, &src, &len);
        if (st != KD_DL_OK || kind == kd_dl::OP_END) break;
        dl_move(o + w, (kind == kd_dl::OP_COPY ? b : d) + src, len, j);
        w += len;
    }
    return st;
}

__device__ __forceinline__ bool dl_inside(u64 at, u64 len, u64 lim) { return at <= lim && len <= lim - at; }

template <bool CHAIN>
__global__ __launch_bounds__(DL_NT) void k_dl_apply(DlArgs a) {
    const u32 j = threadIdx.x & (DL_G - 1);
    const u64 i = (u64)blockIdx.x * DL_IPB + threadIdx.x / DL_G;
    if (i >= a.n) return;
    const u8 *b = nullptr, *d = nullptr;
    u8 *o = nullptr, *stp;
    u64 bl = 0, dl = 0, ol = 0;
    u32 st = KD_DL_ERANGE;
    if (CHAIN) {
        const DlItem it = a.items[i];
        const u32 wb = it.where & 1, wd = (it.where >> 1) & 1, wo = (it.where >> 2) & 1;
        stp = a.status + it.out_st;
        if (dl_inside(it.base_at, it.base_len, a.lim[wb]) && dl_inside(it.delta_at, it.delta_len, a.lim[wd]) &&
            dl_inside(it.dst_at, it.dst_len, a.lim[wo])) {
            b = a.mem[wb] + it.base_at;
            d = a.mem[wd] + it.delta_at;
            o = a.mem[wo] + it.dst_at;
            bl = it.base_len;
            dl = it.delta_len;
            ol = it.dst_len;
            st = (a.status[it.base_st] | a.status[it.delta_st]) ? KD_DL_EPARENT : KD_DL_OK;
        }
    } else {
        // device offsets are nobody's checked input: an item stays inside [0, off[last]) of all three arenas
        stp = a.status + i;
        const u64 bi = a.base_idx[i];
        if (bi < a.nb) {
            const u64 bo = a.base_off[bi], be = a.base_off[bi + 1], bn = a.base_off[a.nb];
            const u64 so = a.delta_off[i], se = a.delta_off[i + 1], sn = a.delta_off[a.n];
            const u64 po = a.dst_off[i], pe = a.dst_off[i + 1], pn = a.dst_off[a.n];
            if (bo <= be && be <= bn && so <= se && se <= sn && po <= pe && pe <= pn) {
                b = a.base + bo;
                d = a.delta + so;
                o = a.dst + po;
                bl = be - bo;
                dl = se - so;
                ol = pe - po;
                st = KD_DL_OK;
            }
        }
    }
    if (st == KD_DL_OK) st = dl_apply(b, bl, d, dl, o, ol, j);
    if (j == 0) *stp = (u8)st;
}

// profiling name: "k_dl_apply" for the flat form, "k_dl_apply.<level, two digits>" for a level of the chained
template <bool CHAIN>
static int dl_launch(kd_ctx* ctx, const DlArgs& a, u32 level = 0) {
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v{"k_dl_apply"};
        for (u32 l = 1; l <= KD_DL_MAX_DEPTH; l++) v.push_back("k_dl_apply." + std::string(l < 10 ? "0" : "") + std::to_string(l));
        return v;
    }();
    const u64 nwg = (a.n + DL_IPB - 1) / DL_IPB;
    KD_CHECK(nwg <= 0x7FFFFFFFull, "kd_delta_apply_batch: too many items");
    return launch(ctx, names[level <= KD_DL_MAX_DEPTH ? level : 0].c_str(),
                  [&] { hipLaunchKernelGGL(k_dl_apply<CHAIN>, dim3((unsigned)nwg), dim3(DL_NT), 0, ctx->stream, a); });
}

// kd_odb_read_batch_device_ex's device half (kd_odb_devread.cpp is host-only C++).  Everything but the arena is
// a grow-only "dl.*" slot; every status comes back in one copy.  Returns with the results.
int delta_read_from_host(kd_ctx* ctx, const DlPlan& p) {
    KD_HIP(hipSetDevice(ctx->device));
    const u64 n = p.n, m = p.m, nst = n + m + p.n_items;
    KD_HIP(hipMemcpyAsync(p.d_dst_off, p.off, 8 * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (n == 0) {
        KD_HIP(hipStreamSynchronize(ctx->stream));
        return KD_OK;
    }
    int rc;
    void *d_src, *d_soff, *d_kind, *d_st, *d_ws, *d_woff, *d_items;
    const u64 sbytes = p.soff1[n] + p.soff2[m] + 8;
    if ((rc = ensure(ctx, "dl.src", sbytes, &d_src)) || (rc = ensure(ctx, "dl.soff", 8 * (n + 1 + m + 1), &d_soff)) ||
        (rc = ensure(ctx, "dl.kind", n, &d_kind)) || (rc = ensure(ctx, "dl.st", nst, &d_st)) ||
        (rc = ensure(ctx, "dl.ws", std::max<u64>(p.ws_bytes, 16), &d_ws)) || (rc = ensure(ctx, "dl.woff", 8 * (m + 1), &d_woff)) ||
        (rc = ensure(ctx, "dl.items", std::max<u64>(sizeof(DlItem) * p.n_items, 16), &d_items)))
        return rc;
    u64* d_soff2 = (u64*)d_soff + n + 1;
    KD_HIP(hipMemcpyAsync(d_src, p.h_src, sbytes, hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_soff, p.soff1, 8 * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_soff2, p.soff2, 8 * (m + 1), hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_woff, p.woff, 8 * (m + 1), hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_kind, p.kind1, n, hipMemcpyHostToDevice, ctx->stream));
    if (p.n_items) KD_HIP(hipMemcpyAsync(d_items, p.items, sizeof(DlItem) * p.n_items, hipMemcpyHostToDevice, ctx->stream));
    u8* st = (u8*)d_st;
    InfArgs a1{(const u8*)d_src, (const u64*)d_soff, (const u8*)d_kind, n, p.d_dst, p.d_dst_off, st};
    if ((rc = inflate_launch(ctx, a1))) return rc;
    if (m) {
        InfArgs a2{(const u8*)d_src + p.soff1[n], d_soff2, nullptr, m, (u8*)d_ws, (const u64*)d_woff, st + n};
        if ((rc = inflate_launch(ctx, a2))) return rc;
    }
    for (u32 l = 1; l <= p.depth; l++) {
        const u64 lo = p.level_start[l - 1], hi = p.level_start[l];
        if (hi == lo) continue;
        DlArgs a{};
        a.n = hi - lo;
        a.status = st;
        a.items = (const DlItem*)d_items + lo;
        a.mem[0] = p.d_dst;
        a.mem[1] = (u8*)d_ws;
        a.lim[0] = p.off[n];
        a.lim[1] = p.ws_bytes;
        if ((rc = dl_launch<true>(ctx, a, l))) return rc;
    }
    for (u64 c = 0; c < p.n_copies; c++) {
        const DlCopy& k = p.copies[c];
        if (!k.len) continue;
        KD_HIP(hipMemcpyAsync(p.d_dst + k.dst_at, (k.src_ws ? (const u8*)d_ws : (const u8*)p.d_dst) + k.src_at, k.len,
                              hipMemcpyDeviceToDevice, ctx->stream));
    }
    KD_HIP(hipMemcpyAsync(p.h_status, d_st, nst, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    return prof_flush(ctx);
}

}  // namespace kd

using namespace kd;

static int dl_check_offsets(const u64* off, u64 n, const char* what) {
    for (u64 i = 0; i < n; i++) KD_CHECK(off[i] <= off[i + 1], "kd_delta_apply_batch: %s descends at %llu", what, (unsigned long long)i);
    return KD_OK;
}

extern "C" int kd_delta_apply_batch(kd_ctx* ctx, const uint8_t* base, const uint64_t* base_off, uint64_t nb,
                                    const uint32_t* base_idx, const uint8_t* delta, const uint64_t* delta_off, uint64_t n,
                                    uint8_t* dst, const uint64_t* dst_off, uint8_t* status, uint32_t mem) {
    KD_CHECK(ctx, "kd_delta_apply_batch: NULL context");
    KD_CHECK(mem == KD_MEM_HOST || mem == KD_MEM_DEVICE, "kd_delta_apply_batch: mem must be KD_MEM_HOST or KD_MEM_DEVICE");
    if (n == 0) return KD_OK;
    KD_CHECK(base && base_off && base_idx && delta && delta_off && dst && dst_off && status, "kd_delta_apply_batch: NULL argument");
    KD_CHECK(nb <= 0xFFFFFFFFull, "kd_delta_apply_batch: too many bases");
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    DlArgs a{};
    a.n = n;
    a.nb = nb;
    if (mem == KD_MEM_DEVICE) {
        a.status = status;
        a.base = base;
        a.base_off = base_off;
        a.base_idx = base_idx;
        a.delta = delta;
        a.delta_off = delta_off;
        a.dst = dst;
        a.dst_off = dst_off;
        return dl_launch<false>(ctx, a);
    }
    if ((rc = dl_check_offsets(base_off, nb, "base_off")) || (rc = dl_check_offsets(delta_off, n, "delta_off")) ||
        (rc = dl_check_offsets(dst_off, n, "dst_off")))
        return rc;
    const u64 bbytes = base_off[nb] - base_off[0], sbytes = delta_off[n] - delta_off[0], dbytes = dst_off[n] - dst_off[0];
    // the staged arenas start at their first item: offsets are uploaded relative to it
    std::vector<u64> rel((nb + 1) + 2 * (n + 1));
    for (u64 i = 0; i <= nb; i++) rel[i] = base_off[i] - base_off[0];
    for (u64 i = 0; i <= n; i++) {
        rel[nb + 1 + i] = delta_off[i] - delta_off[0];
        rel[nb + 1 + n + 1 + i] = dst_off[i] - dst_off[0];
    }
    void *d_base, *d_off, *d_idx, *d_delta, *d_dst, *d_st;
    if ((rc = ensure(ctx, "dl.base", std::max<u64>(bbytes, 16), &d_base)) || (rc = ensure(ctx, "dl.off", 8 * rel.size(), &d_off)) ||
        (rc = ensure(ctx, "dl.bidx", 4 * n, &d_idx)) || (rc = ensure(ctx, "dl.delta", std::max<u64>(sbytes, 16), &d_delta)) ||
        (rc = ensure(ctx, "dl.dst", std::max<u64>(dbytes, 16), &d_dst)) || (rc = ensure(ctx, "dl.hst", n, &d_st)))
        return rc;
    if (bbytes && (rc = stage_h2d(ctx, d_base, base + base_off[0], bbytes))) return rc;
    if (sbytes && (rc = stage_h2d(ctx, d_delta, delta + delta_off[0], sbytes))) return rc;
    if ((rc = stage_h2d(ctx, d_off, rel.data(), 8 * rel.size()))) return rc;
    if ((rc = stage_h2d(ctx, d_idx, base_idx, 4 * n))) return rc;
    KD_HIP(hipStreamSynchronize(ctx->stream));  // (rel is read by a pageable copy)
    a.status = (u8*)d_st;
    a.base = (const u8*)d_base;
    a.base_off = (const u64*)d_off;
    a.base_idx = (const u32*)d_idx;
    a.delta = (const u8*)d_delta;
    a.delta_off = (const u64*)d_off + nb + 1;
    a.dst = (u8*)d_dst;
    a.dst_off = (const u64*)d_off + nb + 1 + n + 1;
    if ((rc = dl_launch<false>(ctx, a))) return rc;
    if ((rc = stage_d2h(ctx, status, d_st, n))) return rc;
    if (dbytes && (rc = stage_d2h(ctx, dst + dst_off[0], d_dst, dbytes))) return rc;
    return prof_flush(ctx);
}
