// kd_ctx.hip — context, errors, workspaces, profiling and host-side key packing of libkartdiff.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <thread>

#include "kd_internal.h"
#include "kd_keypack.h"
#include "kd_walkkey.h"

namespace kd {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

constexpr size_t SLAB_BYTES = (size_t)64 << 20, SLAB_PIECE_MAX = (size_t)8 << 20;

int ensure(kd_ctx* ctx, const char* slot, size_t bytes, void** out) {
    DevBuf& b = ctx->bufs[slot];
    if (bytes == 0) bytes = 16;
    if (b.bytes < bytes) {
        if (b.p) {
            hipError_t e = hipStreamSynchronize(ctx->stream);
            // (inside kd_diff2_step's side work ctx->stream is the side stream: the stream the step
            // was called on may still run the field diff, so the old buffer waits for it too)
            if (e == hipSuccess && ctx->step_main) e = hipStreamSynchronize(ctx->step_main);
            if (e != hipSuccess) { set_error("sync before realloc: %s", hipGetErrorString(e)); return KD_EHIP; }
            if (!b.slab) KD_HIP(hipFree(b.p));  // (a slab piece is abandoned)
            b.p = nullptr;
            b.bytes = 0;
            b.slab = false;
        }
        const size_t want = (bytes + bytes / 8 + 255) & ~(size_t)255;  // headroom, 256-B aligned
        if (want <= SLAB_PIECE_MAX) {
            if (!ctx->slab) {
                void* s = nullptr;
                if (hipMalloc(&s, SLAB_BYTES) == hipSuccess) ctx->slab = (char*)s;
                ctx->slab_used = 0;
            }
            if (ctx->slab && ctx->slab_used + want <= SLAB_BYTES) {
                b.p = ctx->slab + ctx->slab_used;
                ctx->slab_used += want;
                b.bytes = want;
                b.slab = true;
            }
        }
        if (!b.p) {
            KD_HIP(hipMalloc(&b.p, want));
            b.bytes = want;
        }
    }
    *out = b.p;
    return KD_OK;
}

int device_zeros(kd_ctx* ctx, void** out) {
    kd::DevBuf& b = ctx->bufs["zeros"];
    const bool fresh = b.p == nullptr;
    int rc = ensure(ctx, "zeros", 256, out);
    if (rc) return rc;
    if (fresh) KD_HIP(hipMemsetAsync(*out, 0, 256, ctx->stream));
    return KD_OK;
}

int stage_in(kd_ctx* ctx, const char* slot, const void* p, size_t bytes, u32 mem, const void** dev) {
    if (p == nullptr || bytes == 0 || mem == KD_MEM_DEVICE) {
        *dev = p;
        return KD_OK;
    }
    void* d = nullptr;
    int rc = ensure(ctx, slot, bytes, &d);
    if (rc) return rc;
    if ((rc = stage_h2d(ctx, d, p, bytes))) return rc;
    *dev = d;
    return KD_OK;
}

// Pinned staging for small / middling transfers: a pageable copy pins the caller's pages, which a
// one-shot process pays for every buffer.  From PIN_MAX up the runtime's own pinning of the caller's
// pages (no host copy) is the faster path (10M-entry sides: 48 vs 25 GB/s, r4w).
constexpr size_t PIN_CHUNK = (size_t)4 << 20, PIN_MIN = (size_t)64 << 10, PIN_MAX = (size_t)32 << 20;

int stage_h2d(kd_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes < PIN_MIN || bytes >= PIN_MAX || !ctx->pin[1]) {
        KD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));  // (pageable: staged by the runtime)
        return KD_OK;
    }
    // chunk i's host copy overlaps chunk i-1's DMA; a chunk buffer is refilled once its DMA is done
    for (size_t o = 0; o < bytes; o += PIN_CHUNK) {
        const int j = ctx->pin_next;
        ctx->pin_next ^= 1;
        const size_t c = std::min(PIN_CHUNK, bytes - o);
        KD_HIP(hipEventSynchronize(ctx->pin_ev[j]));
        std::memcpy(ctx->pin[j], (const char*)src + o, c);
        KD_HIP(hipMemcpyAsync((char*)dst + o, ctx->pin[j], c, hipMemcpyHostToDevice, ctx->stream));
        KD_HIP(hipEventRecord(ctx->pin_ev[j], ctx->stream));
    }
    return KD_OK;
}

// device -> pinned host chunk by the library's own kernel (16-B stores over the fabric): the
// runtime's first device-to-host copy of a process waited 8 ms whatever was warmed at init (r4z2)
__global__ __launch_bounds__(256) void k_to_host(const u8* __restrict__ src, u8* __restrict__ dst, u64 bytes) {
    const u64 n16 = bytes / 16;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n16; i += (u64)gridDim.x * 256)
        ((uint4*)dst)[i] = ((const uint4*)src)[i];
    const u64 t = 16 * n16 + (u64)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && t < bytes) dst[t] = src[t];
}

int stage_d2h(kd_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes < PIN_MIN || bytes >= PIN_MAX || !ctx->pin[1]) {
        KD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        KD_HIP(hipStreamSynchronize(ctx->stream));
        return KD_OK;
    }
    // DMA of chunk i+1 is queued before chunk i is copied out of its buffer
    const size_t n = (bytes + PIN_CHUNK - 1) / PIN_CHUNK;
    const bool aligned = ((uintptr_t)src & 15) == 0 && ctx->pin_dev[1];
    auto issue = [&](size_t i) -> hipError_t {
        const size_t o = i * PIN_CHUNK, c = std::min(PIN_CHUNK, bytes - o);
        hipError_t e;
        if (aligned) {
            const unsigned grid = (unsigned)std::min<size_t>((c / 16 + 255) / 256 + 1, 1024);
            hipLaunchKernelGGL(k_to_host, dim3(grid), dim3(256), 0, ctx->stream, (const u8*)src + o,
                               (u8*)ctx->pin_dev[i & 1], (u64)c);
            e = hipGetLastError();
        } else {
            e = hipMemcpyAsync(ctx->pin[i & 1], (const char*)src + o, c, hipMemcpyDeviceToHost, ctx->stream);
        }
        return e == hipSuccess ? hipEventRecord(ctx->pin_ev[i & 1], ctx->stream) : e;
    };
    KD_HIP(issue(0));
    for (size_t i = 0; i < n; i++) {
        if (i + 1 < n) KD_HIP(issue(i + 1));
        KD_HIP(hipEventSynchronize(ctx->pin_ev[i & 1]));
        host_mark(ctx, "d2h chunk wait");
        const size_t o = i * PIN_CHUNK;
        std::memcpy((char*)dst + o, ctx->pin[i & 1], std::min(PIN_CHUNK, bytes - o));
        host_mark(ctx, "d2h chunk copy-out");
    }
    ctx->pin_next = 0;
    return KD_OK;
}

void host_mark(kd_ctx* ctx, const char* name) {
    static thread_local std::chrono::steady_clock::time_point t0;
    if (!ctx->opt.trace_host) return;
    (void)hipStreamSynchronize(ctx->stream);
    const auto t = std::chrono::steady_clock::now();
    if (name) std::fprintf(stderr, "[kd] %-22s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
}

void prof_begin(kd_ctx* ctx, const char* name, hipEvent_t* a) {
    (void)name;
    if (ctx->ev_pool.empty()) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) { *a = nullptr; return; }
        ctx->ev_pool.push_back(e);
    }
    *a = ctx->ev_pool.back();
    ctx->ev_pool.pop_back();
    (void)hipEventRecord(*a, ctx->stream);
}

void prof_end(kd_ctx* ctx, const char* name, hipEvent_t a) {
    if (!a) return;
    hipEvent_t b;
    if (ctx->ev_pool.empty()) {
        if (hipEventCreateWithFlags(&b, hipEventDisableSystemFence) != hipSuccess) return;
    } else {
        b = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
    }
    (void)hipEventRecord(b, ctx->stream);
    ctx->pending.push_back({name, a, b});
}

int prof_flush(kd_ctx* ctx) {
    for (auto& p : ctx->pending) {
        KD_HIP(hipEventSynchronize(p.b));
        float ms = 0;
        KD_HIP(hipEventElapsedTime(&ms, p.a, p.b));
        ProfStat& s = ctx->stats[p.name];
        s.launches++;
        s.ms += ms;
        ctx->ev_pool.push_back(p.a);
        ctx->ev_pool.push_back(p.b);
    }
    ctx->pending.clear();
    return KD_OK;
}

template <typename F>
static void par_for(u64 n, F&& f) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (nt > 32) nt = 32;
    if (n < 65536) nt = 1;
    std::vector<std::thread> th;
    u64 chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        u64 a = t * chunk, b = std::min<u64>(n, a + chunk);
        if (a >= b) break;
        th.emplace_back([&f, a, b] { for (u64 i = a; i < b; i++) f(i); });
    }
    for (auto& t : th) t.join();
}

}  // namespace kd

using namespace kd;

namespace kd {
int occupancy(kd_ctx* ctx, const void* kernel, int block, size_t lds) {
    const auto key = std::make_tuple(kernel, block, lds);
    auto it = ctx->occ.find(key);
    if (it != ctx->occ.end()) return it->second;
    int nb = 0;
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds) != hipSuccess || nb <= 0)
        nb = 1;
    ctx->occ[key] = nb;
    return nb;
}
}  // namespace kd

extern "C" {

int kd_abi_version(void) { return KD_ABI_VERSION; }

const char* kd_last_error(void) { return kd::g_err; }

// one empty launch at context creation: the library's code object is loaded then, not inside the
// first diff a process runs
__global__ void k_load_probe() {}

// the option table: name, KD_* environment variable (read once by kd_init), field
namespace {
struct OptDef {
    const char* name;
    const char* env;
    int64_t kd_opts::*i64;
    int kd_opts::*i32;
    uint64_t kd_opts::*u64;
};
const OptDef OPTS[] = {
    {"merge3_join", "KD_MERGE3_JOIN", nullptr, &kd_opts::merge3_join, nullptr},
    {"j2_oidlds_min", "KD_J2_OIDLDS_MIN", nullptr, nullptr, &kd_opts::j2_oidlds_min},
    {"j2_walk", "KD_J2_WALK", nullptr, &kd_opts::j2_walk, nullptr},
    {"fd_stream", "KD_FD_STREAM", nullptr, &kd_opts::fd_stream, nullptr},
    {"fd_walk", "KD_FD_WALK", nullptr, &kd_opts::fd_walk, nullptr},
    {"pkm_max_blocks", "KD_PKM_MAX_BLOCKS", nullptr, nullptr, &kd_opts::pkm_max_blocks},
    {"trace_host", "KD_TRACE_HOST", nullptr, &kd_opts::trace_host, nullptr},
    {"step_overlap", "KD_STEP_OVERLAP", nullptr, &kd_opts::step_overlap, nullptr},
    {"step_overlap_min", "KD_STEP_OVERLAP_MIN", nullptr, nullptr, &kd_opts::step_overlap_min},
    {"pkm_wave", "KD_PKM_WAVE", nullptr, &kd_opts::pkm_wave, nullptr},
    {"step_count", "KD_STEP_COUNT", nullptr, &kd_opts::step_count, nullptr},
    {"kp_tile", "KD_KP_TILE", nullptr, &kd_opts::kp_tile, nullptr},
    {"kp_lds_bytes", "KD_KP_LDS_BYTES", nullptr, &kd_opts::kp_lds_bytes, nullptr},
};
void opt_set(kd_opts& o, const OptDef& d, int64_t v) {
    if (d.i32) o.*(d.i32) = (int)v;
    else if (d.u64) o.*(d.u64) = (uint64_t)v;
}
}  // namespace

int kd_set_option(kd_ctx* ctx, const char* name, int64_t value) {
    KD_CHECK(ctx && name, "kd_set_option: NULL");
    for (const OptDef& d : OPTS)
        if (!strcmp(d.name, name)) {
            opt_set(ctx->opt, d, value);
            return KD_OK;
        }
    KD_CHECK(false, "kd_set_option: unknown option '%s'", name);
}

int kd_get_option(kd_ctx* ctx, const char* name, int64_t* value) {
    KD_CHECK(ctx && name && value, "kd_get_option: NULL");
    if (!strcmp(name, "kp_hbm_tiles")) return kd::keypack_hbm_tiles(ctx, value);  // read-only (kd_keypack.hip)
    for (const OptDef& d : OPTS)
        if (!strcmp(d.name, name)) {
            *value = d.i32 ? (int64_t)(ctx->opt.*(d.i32)) : (int64_t)(ctx->opt.*(d.u64));
            return KD_OK;
        }
    KD_CHECK(false, "kd_get_option: unknown option '%s'", name);
}

int kd_init(int device_ordinal, kd_ctx** out) {
    KD_CHECK(out != nullptr, "kd_init: out is NULL");
    int n = 0;
    KD_HIP(hipGetDeviceCount(&n));
    KD_CHECK(device_ordinal >= 0 && device_ordinal < n, "kd_init: device %d of %d", device_ordinal, n);
    KD_HIP(hipSetDevice(device_ordinal));
    kd_ctx* c = new kd_ctx();
    c->device = device_ordinal;
    for (const OptDef& d : OPTS)  // init-time settings: the KD_* environment, read once here
        if (const char* v = std::getenv(d.env)) opt_set(c->opt, d, strtoll(v, nullptr, 10));
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        set_error("hipStreamCreate: %s", hipGetErrorString(e));
        return KD_EHIP;
    }
    c->stream = c->own_stream;
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cu > 0)
        c->n_cu = cu;
    {   // the workspace slab too (ensure() carves it; a failure here is retried there)
        void* s = nullptr;
        if (hipMalloc(&s, SLAB_BYTES) == hipSuccess) c->slab = (char*)s;
        c->slab_used = 0;
    }
    for (int j = 0; j < 2; j++) {  // the pinned staging chunks (without them: pageable copies)
        void* h = nullptr;
        if (hipHostMalloc(&h, PIN_CHUNK, hipHostMallocMapped) != hipSuccess) break;
        if (hipEventCreateWithFlags(&c->pin_ev[j], hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(h);
            break;
        }
        c->pin[j] = (char*)h;
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, h, 0) == hipSuccess) c->pin_dev[j] = dp;
    }
    hipLaunchKernelGGL(k_load_probe, dim3(1), dim3(64), 0, c->stream);
    if (c->slab) {
        // What a process's first diff would otherwise pay (r4x: 16 ms of a 17-ms first kd_diff2 on
        // 60k-entry sides): the runtime's fill / copy kernels and DMA queues come up on first use,
        // and the pinned chunks' pages on first touch — a memset, a device copy and a full-chunk
        // pinned round trip each way here; then one 1 + 1-entry classify2, the first launch of each
        // of its kernels.  The slab's first pieces are the scratch (re-carved by later ensure()s).
        (void)hipMemsetAsync(c->slab, 0, 1024, c->stream);
        (void)hipMemcpyAsync(c->slab + 512, c->slab, 256, hipMemcpyDeviceToDevice, c->stream);
        for (int j = 0; j < 2; j++)
            if (c->pin[j]) {
                std::memset(c->pin[j], 0, PIN_CHUNK);
                (void)hipMemcpyAsync(c->slab + 4096, c->pin[j], PIN_CHUNK, hipMemcpyHostToDevice, c->stream);
                if (c->pin_dev[j])
                    hipLaunchKernelGGL(k_to_host, dim3(64), dim3(256), 0, c->stream, (const u8*)(c->slab + 4096),
                                       (u8*)c->pin_dev[j], (u64)PIN_CHUNK);
                (void)hipEventRecord(c->pin_ev[j], c->stream);  // (and a blocking wait on each event)
                (void)hipEventSynchronize(c->pin_ev[j]);
            }
        kd_side A{};
        A.n = 1;
        A.key = (const u64*)c->slab;  // zero key, zero OID on both sides: one unchanged pair
        A.oid = (const u8*)c->slab;
        A.mem = KD_MEM_DEVICE;
        A.key_mode = KD_KEY_INT;
        u32* out = (u32*)(c->slab + 512);
        c->slab_used = (size_t)8 << 20;  // the join's own workspaces past the scratch above
        (void)diff2_device(c, &A, &A, 0, out, out + 8, (u64*)(c->slab + 768), (u32*)(c->slab + 800));
        c->slab_used = 0;  // (every ensure() piece above is released with the warm-up)
        for (auto& kv : c->bufs)  // a piece that did not fit the slab came from hipMalloc (hipFree waits for the join)
            if (!kv.second.slab && kv.second.p) (void)hipFree(kv.second.p);
        c->bufs.clear();
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        if (c->slab) (void)hipFree(c->slab);
        for (int j = 0; j < 2; j++) {
            if (c->pin[j]) (void)hipHostFree(c->pin[j]);
            if (c->pin_ev[j]) (void)hipEventDestroy(c->pin_ev[j]);
        }
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        set_error("kd_init: %s", hipGetErrorString(e));
        return KD_EHIP;
    }
    *out = c;
    return KD_OK;
}

int kd_fini(kd_ctx* ctx) {
    if (!ctx) return KD_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    prof_flush(ctx);
    comm_release(ctx);
    gather_release(ctx);
    // kd_diff2_step's side stream: every step joined it back into the stream it was called on (a
    // caller's stream, if kd_set_stream has changed since, is not the one synchronised above)
    if (ctx->side_stream) {
        (void)hipStreamSynchronize(ctx->side_stream);
        (void)hipStreamDestroy(ctx->side_stream);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    for (auto& kv : ctx->bufs)
        if (kv.second.p && !kv.second.slab) (void)hipFree(kv.second.p);
    if (ctx->slab) (void)hipFree(ctx->slab);
    for (int j = 0; j < 2; j++) {
        if (ctx->pin[j]) (void)hipHostFree(ctx->pin[j]);
        if (ctx->pin_ev[j]) (void)hipEventDestroy(ctx->pin_ev[j]);
    }
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return KD_OK;
}

int kd_set_stream(kd_ctx* ctx, void* hip_stream) {
    KD_CHECK(ctx, "kd_set_stream: ctx is NULL");
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return KD_OK;
}

int kd_sync(kd_ctx* ctx) {
    KD_CHECK(ctx, "kd_sync: ctx is NULL");
    KD_HIP(hipSetDevice(ctx->device));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    return prof_flush(ctx);
}

void kd_free(void* p) {
    if (!p) return;
    // both result structs begin with counters and hold malloc'd arrays; they are allocated as a
    // single block (struct + arrays), see kd_classify.hip
    std::free(p);
}

int kd_prof_enable(kd_ctx* ctx, int on) {
    KD_CHECK(ctx, "kd_prof_enable: ctx is NULL");
    ctx->prof = on != 0;
    return KD_OK;
}

int kd_prof_select(kd_ctx* ctx, const char* names) {
    KD_CHECK(ctx, "kd_prof_select: ctx is NULL");
    ctx->prof_only = names && *names ? "," + std::string(names) + "," : std::string();
    return KD_OK;
}

int kd_prof_get(kd_ctx* ctx, const char* name, uint64_t* launches, double* total_ms) {
    KD_CHECK(ctx && name, "kd_prof_get: bad args");
    int rc = prof_flush(ctx);
    if (rc) return rc;
    auto it = ctx->stats.find(name);
    if (launches) *launches = it == ctx->stats.end() ? 0 : it->second.launches;
    if (total_ms) *total_ms = it == ctx->stats.end() ? 0 : it->second.ms;
    return KD_OK;
}

int kd_prof_reset(kd_ctx* ctx) {
    KD_CHECK(ctx, "kd_prof_reset: ctx is NULL");
    int rc = prof_flush(ctx);
    ctx->stats.clear();
    return rc;
}

// ------------------------------------------------------------------------------------------
// host-side key packing (Dataset3.decode_path_to_1pk / PathEncoder, see kartdiff.h)
// ------------------------------------------------------------------------------------------

int64_t kd_pack_int_keys(const uint8_t* names, const uint64_t* name_off, uint64_t n, uint64_t* keys,
                         uint8_t* status) {
    if (!names || !name_off || !keys || !status) { set_error("kd_pack_int_keys: NULL"); return KD_EINVAL; }
    std::mutex m;
    u64 bad = 0;
    par_for(n, [&](u64 i) {  // (kd_keypack.h: the filename of a relative path "c/c/c/c/<filename>")
        u64 k = 0;
        const int st = kp::int_entry(names + name_off[i], name_off[i + 1] - name_off[i], &k);
        keys[i] = k;
        status[i] = (u8)st;
        if (st) { std::lock_guard<std::mutex> g(m); bad++; }
    });
    return (int64_t)bad;
}

int64_t kd_pack_hash_keys(const uint8_t* paths, const uint64_t* path_off, uint64_t n, int levels, int hex,
                          uint64_t* keys, uint8_t* status) {
    if (!paths || !path_off || !keys || !status || levels <= 0) { set_error("kd_pack_hash_keys: bad args"); return KD_EINVAL; }
    std::mutex m;
    u64 bad = 0;
    par_for(n, [&](u64 i) {
        u64 k = 0;
        const int st = kp::hash_entry(paths + path_off[i], path_off[i + 1] - path_off[i], levels, hex, &k);
        keys[i] = k;
        status[i] = (u8)st;
        if (st) { std::lock_guard<std::mutex> g(m); bad++; }
    });
    return (int64_t)bad;
}

int kd_keys_scan(const uint64_t* keys, uint64_t n, uint32_t key_mode, kd_keys_info* out) {
    KD_CHECK(out && (n == 0 || keys), "kd_keys_scan: NULL");
    KD_CHECK(key_mode == KD_KEY_INT || key_mode == KD_KEY_HASH, "kd_keys_scan: bad key_mode");
    *out = kd_keys_info{};
    out->ascending = 1;
    if (n == 0) return KD_OK;
    const u64 k0 = keys[0];
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : nt > 32 ? 32 : nt;
    if (n < 65536) nt = 1;
    // per part: the runs of equal top-24-bit buckets (first and last run, longest inside) and
    // whether the buckets are non-decreasing
    struct Part {
        u64 vary = 0;
        i64 lo = INT64_MAX, hi = INT64_MIN;
        bool asc = true, basc = true;
        u64 b0 = 0, b1 = 0, pre = 0, suf = 0, mx = 0, len = 0;
    };
    std::vector<Part> part(nt);
    std::vector<std::thread> th;
    const u64 chunk = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const u64 a = t * chunk, b = std::min<u64>(n, a + chunk);
        if (a >= b) break;
        th.emplace_back([&, t, a, b] {
            Part p;
            p.len = b - a;
            p.b0 = keys[a] >> 40;
            u64 run = 0, prev = p.b0;
            bool first = true;
            for (u64 i = a; i < b; i++) {
                const u64 k = keys[i];
                p.vary |= k ^ k0;
                if (i > 0) p.asc &= keys[i - 1] < k;
                const u64 bk = k >> 40;
                if (bk != prev) {
                    p.basc &= bk > prev;
                    if (first) p.pre = run;
                    first = false;
                    p.mx = run > p.mx ? run : p.mx;
                    run = 0;
                    prev = bk;
                }
                run++;
                if (key_mode == KD_KEY_INT) {
                    const i64 pk = wk::int_key_pk(k);
                    p.lo = pk < p.lo ? pk : p.lo;
                    p.hi = pk > p.hi ? pk : p.hi;
                }
            }
            if (first) p.pre = run;
            p.suf = run;
            p.b1 = prev;
            p.mx = run > p.mx ? run : p.mx;
            part[t] = p;
        });
    }
    for (auto& t : th) t.join();
    i64 lo = INT64_MAX, hi = INT64_MIN;
    bool basc = true, have = false;
    u64 cur_b = 0, cur_run = 0, seg = 0;  // the run still open at the end of the parts combined so far
    for (auto& p : part) {
        if (!p.len) continue;
        out->vary |= p.vary;
        out->ascending &= p.asc ? 1 : 0;
        lo = p.lo < lo ? p.lo : lo;
        hi = p.hi > hi ? p.hi : hi;
        basc &= p.basc;
        const bool one = p.pre == p.len;  // the whole part is one bucket
        if (have && p.b0 == cur_b) {
            cur_run += p.pre;
        } else {
            if (have) { basc &= p.b0 > cur_b; seg = cur_run > seg ? cur_run : seg; }
            cur_run = p.pre;
        }
        if (!one) {
            seg = cur_run > seg ? cur_run : seg;
            seg = p.mx > seg ? p.mx : seg;
            cur_run = p.suf;
        }
        cur_b = p.b1;
        have = true;
    }
    seg = cur_run > seg ? cur_run : seg;
    out->seg_max = !basc ? -1 : (int32_t)(seg > 0x7fffffffull ? 0x7fffffff : seg);
    out->key0 = k0;
    out->pk_min = key_mode == KD_KEY_INT ? lo : 0;
    out->pk_max = key_mode == KD_KEY_INT ? hi : 0;
    return KD_OK;
}

int kd_int_keys_to_pks(const uint64_t* keys, uint64_t n, int64_t* pks) {
    KD_CHECK(keys && pks, "kd_int_keys_to_pks: NULL");
    par_for(n, [&](u64 i) { pks[i] = wk::int_key_pk(keys[i]); });
    return KD_OK;
}

}  // extern "C"
