// kd_inflate.hip — kd_inflate_batch: a batch of independent zlib streams inflated on the GPU.
//
// <- the blob read under the field diff: every feature blob of an imported layer is its own deflate
// stream in the pack (git fast-import --depth=0, kart/fast_import.py:204,273), a few hundred bytes
// long.  The host finds the entries and ships the compressed bytes (kd_odb_read_batch_device,
// kd_odb_plan.cpp, kd_odb_devread.cpp); this kernel inflates them into the arena + off[n+1] layout kd_fielddiff reads.
//
// k_inf_streams: one lane per item, one wave per workgroup.  The decoder is kd_inflate.h (shared
// with the host); a lane's Huffman state (KD_INF_WORDS = 204 words: canonical counts, symbols in
// code order, the code lengths a table is built from) lives in LDS at lds[word * 64 + lane], so the
// wave's same-index accesses fall into 64 different banks and no per-lane array is indexed at run
// time (no scratch).  51 KiB of LDS per workgroup: three workgroups per CU (160 KiB).  Compressed
// bytes are read from HBM by 4-byte loads at byte addresses into a 64-bit bit buffer; output bytes
// are stored to HBM and a match reads the lane's own earlier bytes back from there (dst carries no
// __restrict__).  A raw item (kind 1) is copied into its place by the same lane loop.
#include "kd_inflate.h"
#include "kd_internal.h"

namespace kd {

constexpr int INF_LANES = 64;

__global__ __launch_bounds__(INF_LANES) void k_inf_streams(InfArgs a) {
    __shared__ u32 lds[kd_inf::KD_INF_WORDS * INF_LANES];
    const u64 i = (u64)blockIdx.x * INF_LANES + threadIdx.x;
    if (i >= a.n) return;
    // device offsets are nobody's checked input: an item stays inside [0, off[n]) of both arenas
    const u64 so = a.src_off[i], se = a.src_off[i + 1], sn = a.src_off[a.n];
    const u64 po = a.dst_off[i], pe = a.dst_off[i + 1], pn = a.dst_off[a.n];
    u32 st = KD_INF_ERANGE;
    if (so <= se && se <= sn && po <= pe && pe <= pn) {
        const u8* s = a.src + so;
        u8* d = a.dst + po;
        const u64 sl = se - so, dl = pe - po;
        if (a.kind && a.kind[i]) {
            st = sl < dl ? KD_INF_ESRC : sl > dl ? KD_INF_EOVER : KD_INF_OK;
            if (st == KD_INF_OK)
                for (u64 k = 0; k < dl; k++) d[k] = s[k];
        } else {
            st = kd_inf::inflate_stream<INF_LANES>(s, sl, d, dl, lds + threadIdx.x);
        }
    }
    a.status[i] = (u8)st;
}

int inflate_launch(kd_ctx* ctx, const InfArgs& a) {
    const u64 nwg = (a.n + INF_LANES - 1) / INF_LANES;
    KD_CHECK(nwg <= 0x7FFFFFFFull, "kd_inflate_batch: too many items");
    return launch(ctx, "k_inf_streams",
                  [&] { hipLaunchKernelGGL(k_inf_streams, dim3((unsigned)nwg), dim3(INF_LANES), 0, ctx->stream, a); });
}

static int check_offsets(const u64* off, u64 n, const char* what) {
    for (u64 i = 0; i < n; i++) KD_CHECK(off[i] <= off[i + 1], "kd_inflate_batch: %s descends at %llu", what, (unsigned long long)i);
    return KD_OK;
}

// kd_odb_read_batch_device's device half (kd_odb_devread.cpp is host-only C++): h_src (pinned, src_off[n] + 8
// bytes), the offsets and the kinds are uploaded into workspace slots, the items land in d_dst, whose
// offsets d_dst_off receives; h_status <- the n status bytes.  Returns with the results.
int inflate_from_host(kd_ctx* ctx, const uint8_t* h_src, const uint64_t* h_src_off, const uint8_t* h_kind, uint64_t n,
                      uint8_t* d_dst, const uint64_t* h_dst_off, uint64_t* d_dst_off, uint8_t* h_status) {
    KD_HIP(hipSetDevice(ctx->device));
    KD_HIP(hipMemcpyAsync(d_dst_off, h_dst_off, 8 * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (n == 0) {
        KD_HIP(hipStreamSynchronize(ctx->stream));
        return KD_OK;
    }
    int rc;
    void *d_src, *d_soff, *d_kind, *d_st;
    const u64 sbytes = h_src_off[n] + 8;
    if ((rc = ensure(ctx, "inf.src", sbytes, &d_src)) || (rc = ensure(ctx, "inf.soff", 8 * (n + 1), &d_soff)) ||
        (rc = ensure(ctx, "inf.kind", n, &d_kind)) || (rc = ensure(ctx, "inf.st", n, &d_st)))
        return rc;
    KD_HIP(hipMemcpyAsync(d_src, h_src, sbytes, hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_soff, h_src_off, 8 * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    KD_HIP(hipMemcpyAsync(d_kind, h_kind, n, hipMemcpyHostToDevice, ctx->stream));
    InfArgs a{(const u8*)d_src, (const u64*)d_soff, (const u8*)d_kind, n, d_dst, d_dst_off, (u8*)d_st};
    if ((rc = inflate_launch(ctx, a))) return rc;
    KD_HIP(hipMemcpyAsync(h_status, d_st, n, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    return prof_flush(ctx);
}

}  // namespace kd

using namespace kd;

extern "C" int kd_inflate_batch(kd_ctx* ctx, const uint8_t* src, const uint64_t* src_off, const uint8_t* kind, uint64_t n,
                                uint8_t* dst, const uint64_t* dst_off, uint8_t* status, uint32_t mem) {
    KD_CHECK(ctx, "kd_inflate_batch: NULL context");
    KD_CHECK(mem == KD_MEM_HOST || mem == KD_MEM_DEVICE, "kd_inflate_batch: mem must be KD_MEM_HOST or KD_MEM_DEVICE");
    if (n == 0) return KD_OK;
    KD_CHECK(src && src_off && dst && dst_off && status, "kd_inflate_batch: NULL argument");
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    if (mem == KD_MEM_DEVICE) {
        InfArgs a{src, src_off, kind, n, dst, dst_off, status};
        return inflate_launch(ctx, a);
    }
    if ((rc = check_offsets(src_off, n, "src_off")) || (rc = check_offsets(dst_off, n, "dst_off"))) return rc;
    const u64 sbytes = src_off[n] - src_off[0], dbytes = dst_off[n] - dst_off[0];
    // the staged arenas start at the first item: offsets are uploaded relative to it
    std::vector<u64> rel(2 * (n + 1));
    for (u64 i = 0; i <= n; i++) {
        rel[i] = src_off[i] - src_off[0];
        rel[n + 1 + i] = dst_off[i] - dst_off[0];
    }
    void *d_src, *d_off, *d_kind = nullptr, *d_dst, *d_st;
    if ((rc = ensure(ctx, "inf.src", sbytes + 8, &d_src)) || (rc = ensure(ctx, "inf.soff", 16 * (n + 1), &d_off)) ||
        (rc = ensure(ctx, "inf.dst", dbytes, &d_dst)) || (rc = ensure(ctx, "inf.st", n, &d_st)))
        return rc;
    if (kind && (rc = ensure(ctx, "inf.kind", n, &d_kind))) return rc;
    if (sbytes && (rc = stage_h2d(ctx, d_src, src + src_off[0], sbytes))) return rc;
    KD_HIP(hipMemsetAsync((u8*)d_src + sbytes, 0, 8, ctx->stream));  // the padding the bit reader may load
    if ((rc = stage_h2d(ctx, d_off, rel.data(), 16 * (n + 1)))) return rc;
    if (kind && (rc = stage_h2d(ctx, d_kind, kind, n))) return rc;
    KD_HIP(hipStreamSynchronize(ctx->stream));  // (rel is read by a pageable copy)
    InfArgs a{(const u8*)d_src, (const u64*)d_off, (const u8*)d_kind, n, (u8*)d_dst, (const u64*)d_off + n + 1, (u8*)d_st};
    if ((rc = inflate_launch(ctx, a))) return rc;
    if ((rc = stage_d2h(ctx, status, d_st, n))) return rc;
    if (dbytes && (rc = stage_d2h(ctx, dst + dst_off[0], d_dst, dbytes))) return rc;
    return prof_flush(ctx);
}
