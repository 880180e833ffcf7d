// kd_internal.h — shared internals of libkartdiff (gfx950 / MI355X).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "kartdiff.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;
typedef int16_t i16;
typedef int8_t i8;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // native 16-B vector (SROA-friendly)
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

namespace kd {

void set_error(const char* fmt, ...);

#define KD_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            ::kd::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return KD_EHIP;                                                                 \
        }                                                                                   \
    } while (0)

#define KD_CHECK(cond, ...)            \
    do {                               \
        if (!(cond)) {                 \
            ::kd::set_error(__VA_ARGS__); \
            return KD_EINVAL;          \
        }                              \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool slab = false;  // carved from the context's slab (never freed on its own)
};

struct ProfStat {
    u64 launches = 0;
    double ms = 0;
};

struct PendingEv {
    std::string name;
    hipEvent_t a, b;
};

// kd_fielddiff's body; n_part > 0: the update count is the sum of n_part (<= 64) counters 16 words
// (C2_UCNT_STRIDE) apart at d_n_upd (the join's partial counters) instead of *d_n_upd
int fielddiff_device(kd_ctx* ctx, const kd_blobs* ob, const kd_blobs* nb, const uint32_t* pu, uint64_t n_upd,
                     const uint64_t* d_n_upd, int n_part, uint32_t pairs_mem, const kd_legend_maps* mp, uint64_t* masks,
                     uint8_t* status, uint32_t out_mem);

}  // namespace kd

// Tuning options of a context (kd_set_option; kd_init seeds them once from the KD_* environment
// variables of the same names, documented in kartdiff.h).  Defaults are the measured optima.
struct kd_opts {
    int merge3_join = 1;             // KD_MERGE3_JOIN: 0 = round 3's two-step merge (classify2 + k_resolve3)
    uint64_t j2_oidlds_min = 1ull << 26;  // KD_J2_OIDLDS_MIN: k_join2 stages OIDs in LDS from this many entries
    int j2_walk = 1;                 // KD_J2_WALK: 1 = the tile's guided split search and straight-line walk / checks, 0 = the blind search
    int fd_stream = -1;              // KD_FD_STREAM: -1 auto, 0 windowed k_fielddiff, 1 streamed k_fielddiff_s
    int fd_walk = -1;                // KD_FD_WALK: -1 / 0 off, 1 the walked k_fdwalk (A/B)
    uint64_t pkm_max_blocks = 1ull << 26;  // KD_PKM_MAX_BLOCKS: largest pk range (64-pk blocks) of the bitmap pk order
    int trace_host = 0;              // KD_TRACE_HOST: 1 = stream-synced wall-clock marks to stderr
    // KD_STEP_OVERLAP: kd_diff2_step's schedule — 0 everything on the context's stream; 1 / 2 the
    // placement and the pk order on the side stream beside the field diff, which is queued first (1)
    // or after them (2)
    int step_overlap = 1;
    // KD_STEP_OVERLAP_MIN: the side stream is used from this many entries of both sides together.
    // Measured (profiles/step_overlap/bench_ab.json): C3's 200M-entry step gains 0.11 ms of 2.92; C2's
    // 20M-entry step, whose field diff runs 40 us, loses 0.004 ms of 0.243 to the two cross-stream
    // waits.  2^26 lies between the two.
    uint64_t step_overlap_min = 1ull << 26;
    // KD_STEP_COUNT: 1 = kd_diff2_step's field diff of update-order arenas takes the update count
    // from the join's partial counters and is queued directly behind k_join2, k_gscan2 goes to the
    // side stream in front of k_place2 (where the side stream is used at all); 0 = k_gscan2 first
    int step_count = 1;
    // KD_PKM_WAVE: the bitmap pk order's scans in their LDS-free one-wave-per-chunk form: -1 on
    // kd_diff2_step's side stream only, 0 never, 1 always
    int pkm_wave = -1;
    // KD_KP_TILE: entries per workgroup of kd_pack_keys_device's k_kp_pack, 512 or 1024 (kd_keypack.hip)
    int kp_tile = 512;
    // KD_KP_LDS_BYTES: the largest tile span k_kp_pack stages in LDS (at most 30720); a tile whose
    // paths are longer decodes from HBM.  (Lowering it is how the tests reach that branch cheaply.)
    int kp_lds_bytes = 30720;
};

struct kd_ctx {
    int device = 0;
    kd_opts opt;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::map<std::string, kd::DevBuf> bufs;
    // kd_diff2_step's side stream (created on first use, released by kd_fini) and its fork / join
    // events.  While the step queues the side work, `stream` IS the side stream (kd::StreamScope:
    // every launch, copy and profiling event of the library goes to ctx->stream) and step_main is the
    // stream the step was called on; nullptr outside that window.
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t step_main = nullptr;
    // profiling
    bool prof = false;
    std::string prof_only;  // ",name,name," selection (empty = every kernel)
    std::vector<hipEvent_t> ev_pool;
    std::vector<kd::PendingEv> pending;
    std::map<std::string, kd::ProfStat> stats;
    // last uploaded kd_fielddiff table (host copy kept alive for the async upload, and reused
    // when the next call's tables are identical)
    std::vector<uint8_t> fd_tab;
    int n_cu = 256;  // compute units (grid sizing of grid-stride kernels)
    // multi-GPU (kd_comm.hip): this rank's communicator, and kd_diff2_sharded's per-device set
    void* comm = nullptr;
    int nranks = 1, rank = 0;
    std::vector<int> group_devs;
    std::vector<void*> group_comms;
    // kd_diff2_gather_begin / _end: the counts' pinned landing area, the event after it, and the
    // stream the record all-gather runs on (overlapping whatever the caller queued in between)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_counts = nullptr, ev_gathered = nullptr;
    uint64_t* h_counts_pin = nullptr;
    int h_counts_ranks = 0;
    uint64_t gather_send_cap = 0;  // records the last _begin's d_delta holds (base.n + target.n + 1)
    int occ_resolve3 = 0;  // resident k_resolve3 workgroups per CU
    // resident workgroups per CU by (kernel, block size, dynamic LDS): asked once per context (kd::occupancy)
    std::map<std::tuple<const void*, int, size_t>, int> occ;
    uint32_t rs_epoch = 0;  // kd_sort: epoch of the last pass's look-back words (kd_sort.hip)
    // kd_delta_pk_order's two mask buffers: a call marks one and its scan zeroes the other for the
    // next call; zeroed = (buffer address, blocks known zero) — a reallocated buffer is zeroed again
    int pkm_cur = 0;
    void* pkm_zero_ptr[2] = {nullptr, nullptr};
    uint64_t pkm_zero_nb[2] = {0, 0};
    // small workspaces come from one slab (one hipMalloc instead of one per slot on a process's
    // first calls); grown slots take a fresh piece, the slab is freed with the context
    char* slab = nullptr;
    size_t slab_used = 0;
    // host inputs / results cross PCIe through two pinned chunks (stage_h2d / stage_d2h): a
    // pageable hipMemcpy pins the caller's pages on first use, which a one-shot process pays for
    // every buffer it hands over
    char* pin[2] = {nullptr, nullptr};
    void* pin_dev[2] = {nullptr, nullptr};  // the chunks' device-side addresses (k_to_host writes them)
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    int pin_next = 0;
    // kd_geom_refine: the filter polygon whose device copy sits in slot "gr.filter" — the host
    // pointer, vertex and ring counts and a hash of its bytes (0 vertices: none yet)
    const void* gr_ptr = nullptr;
    void* gr_dev = nullptr;  // where that copy was written (a regrown slot is filled again)
    uint64_t gr_nv = 0, gr_nr = 0, gr_hash = 0;
};

namespace kd {

// device scratch slot, grown as needed (never shrinks).  Not called inside timed regions once
// kd_reserve() has sized it.
void gather_release(kd_ctx* ctx);  // kd_comm.hip: kd_diff2_gather_begin/_end resources
int ensure(kd_ctx* ctx, const char* slot, size_t bytes, void** out);
// host -> device on ctx->stream through the pinned chunks (returns when src may be reused);
// device -> host, blocking (the stream is synchronised)
int stage_h2d(kd_ctx* ctx, void* dst, const void* src, size_t bytes);
// KD_TRACE_HOST=1: stream sync + wall time since the previous mark to stderr (diagnosis only;
// name nullptr starts a sequence)
void host_mark(kd_ctx* ctx, const char* name);
int stage_d2h(kd_ctx* ctx, void* dst, const void* src, size_t bytes);

// 256 zero bytes of device memory: what empty inputs point at, and the target of loads issued by
// masked-off lanes in branch-free load batches (never a host address)
int device_zeros(kd_ctx* ctx, void** out);

// resident workgroups per CU of `kernel` at `block` threads and `lds` dynamic LDS bytes on the
// context's device (>= 1), from the occupancy calculator once per context
int occupancy(kd_ctx* ctx, const void* kernel, int block, size_t lds);

// ctx->stream pointed at another stream for a scope (kd_diff2_step's side work): launch(),
// prof_begin / prof_end, ensure() and every entry point's body follow ctx->stream, so the events of
// a kernel are recorded on the stream it was launched on
struct StreamScope {
    kd_ctx* ctx;
    hipStream_t saved;
    StreamScope(kd_ctx* c, hipStream_t s) : ctx(c), saved(c->stream) {
        c->step_main = saved;
        c->stream = s;
    }
    ~StreamScope() {
        ctx->stream = saved;
        ctx->step_main = nullptr;
    }
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
};

// profiling wrappers around a launch on ctx->stream
void prof_begin(kd_ctx* ctx, const char* name, hipEvent_t* a);
void prof_end(kd_ctx* ctx, const char* name, hipEvent_t a);
int prof_flush(kd_ctx* ctx);

inline bool prof_on(const kd_ctx* ctx, const char* name) {
    return ctx->prof && (ctx->prof_only.empty() || ctx->prof_only.find("," + std::string(name) + ",") != std::string::npos);
}

template <typename F>
inline int launch(kd_ctx* ctx, const char* name, F&& f) {
    hipEvent_t a = nullptr;
    const bool prof = prof_on(ctx, name);
    if (prof) prof_begin(ctx, name, &a);
    f();
    hipError_t e = hipGetLastError();
    if (prof) prof_end(ctx, name, a);
    if (e != hipSuccess) {
        set_error("launch %s: %s", name, hipGetErrorString(e));
        return KD_EHIP;
    }
    return KD_OK;
}

// copy a host/device side array to device (returns device pointer; device input is passed through)
int stage_in(kd_ctx* ctx, const char* slot, const void* p, size_t bytes, u32 mem, const void** dev);
// a side's arrays staged to device scratch slots "<tag>.*" (device sides pass through); checks
int stage_side(kd_ctx* ctx, const kd_side* s, const char* tag, kd_side* dev);
int check_side(const kd_side* s, const char* which);
// kd_geomfilter.hip: the kept list rebuilt from finished codes (device memory; kd_geom_refine)
int gf_rekeep(kd_ctx* ctx, const u8* match, u64 n, const u64* d_n, u32* keep, u64* nk_dst);
int gf_scan(kd_ctx* ctx, u32* cnt, u32 n, u64* total);
// destroy the context's communicators (kd_fini)
void comm_release(kd_ctx* ctx);

// kd_inflate.hip: one launch of k_inf_streams on ctx->stream, every array device memory (kd_delta.hip
// inflates chain bases and delta payloads into its workspace with it)
struct InfArgs {
    const u8* src;
    const u64* src_off;  // [n + 1]
    const u8* kind;      // [n] or nullptr
    u64 n;
    u8* dst;
    const u64* dst_off;  // [n + 1]
    u8* status;
};
int inflate_launch(kd_ctx* ctx, const InfArgs& a);

// kd_keypack.hip: the tiles of the last kd_pack_keys_device call that decoded from HBM because their
// paths did not fit the LDS budget (kd_get_option "kp_hbm_tiles"; waits for the stream)
int keypack_hbm_tiles(kd_ctx* ctx, int64_t* value);

// ---- classify2 (device form), kd_classify.hip ----
// ordA / ordB (both or neither): the sides' OIDs and filename offsets are in another order, row
// ord[i] belongs to sorted entry i (kd_diff2_device_perm)
// d_dkey / d_ukey (optional): the join key of every delta / update record, beside the lists
// three-way merge in one pass (k_join3b): conflicts (a, o, t) and merge deltas (o, t) in path order,
// counts = clean, conflicts, merge deltas, 0; ord*: late materialisation (walk rows of sorted entries)
int merge3_join_device(kd_ctx* ctx, const kd_side& K, const kd_side& O, const kd_side& T, u32* d_conf, uint2* d_md,
                       u64* d_counts, u32* d_err, const u32* ordK = nullptr, const u32* ordO = nullptr,
                       const u32* ordT = nullptr);
int diff2_device(kd_ctx* ctx, const kd_side* A, const kd_side* B, u32 flags, u32* d_delta,
                 u32* d_upd, u64* d_counts, u32* d_err, const u32* ordA = nullptr, const u32* ordB = nullptr,
                 u64* d_dkey = nullptr, u64* d_ukey = nullptr);
// diff2_device in three parts (kd_diff2_step queues them on different streams): the front runs
// k_partition2 and k_join2 and fills `pl` with what the other two need; diff2_scan launches k_gscan2
// on ctx->stream (lds_free: its one-wave form, which becomes resident beside a field diff that fills
// every CU's LDS) — the counts are final after it — and diff2_place k_place2, which reads the scan's
// prefixes (nothing to do when !pl.needed: KD_DIFF_UNORDERED, whose join writes the counts itself,
// or two empty sides).  count_upd: the ordered join also adds every tile's update count into the
// partial counters pl.ucnt (C2_UCNT of them, C2_UCNT_STRIDE words apart, zeroed by k_partition2),
// whose sum is the update count as soon as the join has finished.
constexpr u64 C2_UCNT = 64, C2_UCNT_STRIDE = 16;
struct Diff2Place {
    bool needed = false;
    u64 ntiles = 0;
    const void *sdel = nullptr, *tcnt = nullptr, *gsum = nullptr, *gpre = nullptr, *skd = nullptr;
    const u64* ucnt = nullptr;
    u64* d_counts = nullptr;
    u32 *d_delta = nullptr, *d_upd = nullptr;
    u64 *d_dkey = nullptr, *d_ukey = nullptr;
};
int diff2_front(kd_ctx* ctx, const kd_side* A, const kd_side* B, u32 flags, u32* d_delta, u32* d_upd, u64* d_counts,
                u32* d_err, const u32* ordA, const u32* ordB, u64* d_dkey, u64* d_ukey, Diff2Place* pl, bool count_upd);
int diff2_scan(kd_ctx* ctx, const Diff2Place& pl, bool lds_free);
int diff2_place(kd_ctx* ctx, const Diff2Place& pl);
// kd_delta_pk_order's body; lds_free: the scans in their one-wave-per-chunk form (no LDS, so they
// become resident beside a field diff that fills every CU's LDS)
int delta_pk_order(kd_ctx* ctx, const kd_side* base, const kd_side* target, const u32* d_delta, const u64* d_keys,
                   u64 cap, const u64* d_n, i64 pk_lo, i64 pk_hi, i64* d_pk, u32* d_perm, bool lds_free);
#ifndef KD_C2_NT
#define KD_C2_NT 256
#endif
constexpr int C2_NT = KD_C2_NT;
#ifndef KD_C2_IPT
#define KD_C2_IPT 4
#endif
constexpr int C2_IPT = KD_C2_IPT;
constexpr int C2_TILE = C2_NT * C2_IPT;

}  // namespace kd
