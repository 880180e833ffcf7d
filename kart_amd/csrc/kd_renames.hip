// kd_renames.hip — kd_find_renames: the deletes and inserts of a two-way diff paired by blob OID.
//
// <- WorkingCopy.find_renames (kart/working_copy/base.py:829-854) for a commit<>commit diff, the TODO
// at kart/rich_base_dataset.py:233.  A V3 feature blob is msg_pack([legend hash, non-pk values])
// (kart/dataset3.py:261-272), the pk lives in the path only, so Schema.hash_feature(f, without_pk=True)
// of a feature stored under the current legend is its blob's OID: the pass is one join of two unsorted
// 20-byte key lists that are resident beside the delta list.
//
// Semantics (the reference's two dicts, filled in iteration order, later entries overwriting earlier
// ones): for every OID on at least one delete and at least one insert, the delete with the largest
// delta index pairs with the insert with the largest delta index; every other delta stays.
//
// Kernels: k_rn_list compacts the delete and the insert delta indices (and the OID row of each) into
// per-block slots; k_gf_scan scans the block counts; k_rn_zero clears the table; k_rn_build claims one
// table slot per distinct delete OID and keeps the largest delete index there; k_rn_probe finds each
// insert's slot and keeps the largest insert index; k_rn_count / k_gf_scan / k_rn_place emit the
// winning pairs in ascending delete order.
//
// The table (open addressing, linear probing, wraps): cap = max(1024, 2^ceil(log2(2 * deletes))) slots of
// 16 bytes: u64 claim word, u32 del_max, u32 ins_max.  claim = (OID bytes 0..3 << 32) | (position of the
// claiming delete in the build list + 1), never zero; the home slot is the little-endian u64 of OID
// bytes 8..15 masked with cap - 1.  A tag match is never trusted: the claimer's OID (immutable input,
// found through its position) is compared over all 20 bytes.
//
// Coherence: in k_rn_build and k_rn_probe, which write the table, every access to a table word is an
// agent-scope atomic (the CAS's returned value, an atomic max, or a relaxed agent-scope load): the
// XCDs' L2s are not coherent with each other inside a kernel.  Everything else those kernels read was
// written by an earlier kernel.  k_rn_count and k_rn_place read the finished table plainly.
#include "kd_internal.h"

namespace kd {

constexpr int RN_LB = 4096;          // deltas per k_rn_list block (k_gr_list's grouping): its slots are its own
constexpr int RN_RPW = RN_LB / 256;  // rounds of one wave over its quarter of the block
constexpr u64 RN_CAP_MIN = 1024;
// threads per block of k_rn_build / k_rn_probe: a lane's probe is a chain of dependent memory round trips
// (list, row, OID, claim word, the claimer's row and OID, max), so more chains in flight help: 1,024
// lanes against 256 (-DKD_RN_PT=256), alternated in one session at C3 20M, took the probe from 0.107 to
// 0.092 ms and the build from 0.112 to 0.110 ms (profiles/find_renames/block_size_ab.json)
#ifndef KD_RN_PT
#define KD_RN_PT 1024
#endif
constexpr int RN_PT = KD_RN_PT;

struct RnSlot {
    unsigned long long claim;
    u32 del_max, ins_max;
};

struct RnArgs {
    const uint2* delta;  // [cap] (base | NONE, target | NONE)
    u64 cap;
    const u64* d_n;      // device count (nullptr: cap)
    const u32* oid[2];   // the sides' OIDs as words (5 per entry)
    const u32* ord[2];   // row of sorted entry i (nullptr: i)
    u64 n_side[2];
    u32* list[2];        // [nblk * RN_LB] delta indices of the deletes / inserts, block b's from b * RN_LB
    u32* row[2];         // [nblk * RN_LB] OID row of each listed delta
    u32* bcnt;           // [2 * nblk] deletes per block, then inserts per block (scanned in place)
    const u64* tot;      // the scan's total (deletes + inserts)
    u32 nblk;
    RnSlot* table;
    u64 table_slots;     // allocated slots (a power of two >= any cap the device count can ask for)
    u32* dslot;          // [nblk * RN_LB] table slot of each listed delete
    u32* wcnt;           // [nblk] winners per block (scanned in place)
    uint2* ren;
};

// the table's size for n_del deletes (every kernel derives it from the scanned delete count)
__device__ __forceinline__ u64 rn_cap(u64 n_del, u64 table_slots) {
    u64 c = RN_CAP_MIN;
    while (c < 2 * n_del) c <<= 1;
    return c < table_slots ? c : table_slots;
}

__device__ __forceinline__ u32 rn_lane_rank(u64 bal) {
    return __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0));
}

// one lane per delta, RN_LB per block, each wave a contiguous quarter (so a wave's ballots alone
// order its slots and one barrier orders the waves): deletes and inserts classified from the records
// alone, a record whose index lies outside its side is neither
__global__ __launch_bounds__(256) void k_rn_list(RnArgs a) {
    __shared__ u32 s_w[2][4];
    const u64 n = a.d_n ? min(*a.d_n, a.cap) : a.cap;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const u64 t0 = (u64)blockIdx.x * RN_LB;
    const u64 w0 = t0 + (u64)wid * (RN_LB / 4);
    u32 rw[RN_RPW];  // OID row of this lane's delta of round r
    u32 kind = 0;    // 2 bits per round: 1 delete, 2 insert
    u32 cnt[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < RN_RPW; r++) {
        const u64 d = w0 + (u64)r * 64 + lane;
        u32 k = 0, x = 0;
        if (d < n) {
            const uint2 rec = a.delta[d];
            if (rec.x != KD_NONE && rec.y == KD_NONE && rec.x < a.n_side[0]) {
                x = a.ord[0] ? a.ord[0][rec.x] : rec.x;
                k = x < a.n_side[0] ? 1u : 0u;
            } else if (rec.x == KD_NONE && rec.y != KD_NONE && rec.y < a.n_side[1]) {
                x = a.ord[1] ? a.ord[1][rec.y] : rec.y;
                k = x < a.n_side[1] ? 2u : 0u;
            }
        }
        rw[r] = x;
        kind |= k << (2 * r);
        cnt[0] += (u32)__popcll(__ballot(k == 1));
        cnt[1] += (u32)__popcll(__ballot(k == 2));
    }
    if (lane == 0) {
        s_w[0][wid] = cnt[0];
        s_w[1][wid] = cnt[1];
    }
    __syncthreads();
    u32 run[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wid) {
            run[0] += s_w[0][w];
            run[1] += s_w[1][w];
        }
    }
#pragma unroll
    for (int r = 0; r < RN_RPW; r++) {
        const u32 k = (kind >> (2 * r)) & 3u;
        const u64 bd = __ballot(k == 1), bi = __ballot(k == 2);
        if (k) {
            const int s = (int)k - 1;
            const u64 p = t0 + run[s] + rn_lane_rank(s ? bi : bd);
            a.list[s][p] = (u32)(w0 + (u64)r * 64 + lane);
            a.row[s][p] = rw[r];
        }
        run[0] += (u32)__popcll(bd);
        run[1] += (u32)__popcll(bi);
    }
    if (tid == 0) {
        a.bcnt[blockIdx.x] = s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3];
        a.bcnt[a.nblk + blockIdx.x] = s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3];
    }
}

// the table's cap slots zeroed (grid-stride, one 16-B store per slot)
__global__ __launch_bounds__(256) void k_rn_zero(RnArgs a) {
    const u64 cap = rn_cap(a.bcnt[a.nblk], a.table_slots);  // (bcnt[nblk]: the inserts' first prefix = every delete)
    u32x4* t = (u32x4*)a.table;
    const u32x4 z = {0, 0, 0, 0};
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cap; i += (u64)gridDim.x * 256) t[i] = z;
}

__device__ __forceinline__ bool rn_oid_eq(const u32* __restrict__ p, u32 o0, u32 o1, u32 o2, u32 o3, u32 o4) {
    return ((p[0] ^ o0) | (p[1] ^ o1) | (p[2] ^ o2) | (p[3] ^ o3) | (p[4] ^ o4)) == 0;
}

// block b's listed deltas of one kind: [lo, lo + cnt) of the list, from the scanned counts
__device__ __forceinline__ u32 rn_block_count(const RnArgs& a, int s, u32 b) {
    const u32* c = a.bcnt + (s ? a.nblk : 0);
    const u32 end = b + 1 < a.nblk ? c[b + 1] : (s ? (u32)*a.tot : a.bcnt[a.nblk]);
    const u32 cnt = end - c[b];
    return cnt <= (u32)RN_LB ? cnt : 0u;  // (what k_rn_list can have written)
}

// one lane per delete: its OID's slot claimed or found, the largest delete index kept there
__global__ __launch_bounds__(RN_PT) void k_rn_build(RnArgs a) {
    const u32 b = blockIdx.x;
    const u32 cnt = rn_block_count(a, 0, b);
    if (!cnt) return;
    const u64 mask = rn_cap(a.bcnt[a.nblk], a.table_slots) - 1;
    const u64 t0 = (u64)b * RN_LB;
    for (u32 i = threadIdx.x; i < cnt; i += RN_PT) {
        const u64 pos = t0 + i;
        const u32 di = a.list[0][pos];
        const u32* o = a.oid[0] + 5ull * a.row[0][pos];
        const u32 o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3], o4 = o[4];
        const unsigned long long mine = ((unsigned long long)o0 << 32) | (unsigned long long)(pos + 1);
        u64 s = (((u64)o3 << 32) | o2) & mask;
        for (u64 step = 0; step <= mask; step++) {  // (an empty slot exists: cap >= 2 * deletes)
            unsigned long long cur = 0;
            if (__hip_atomic_compare_exchange_strong(&a.table[s].claim, &cur, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                break;  // claimed
            if ((u32)(cur >> 32) == o0) {
                const u64 cp = (u64)(u32)cur - 1;  // the claimer: its OID through the build list (earlier kernels' data)
                if (cp < (u64)a.nblk * RN_LB && rn_oid_eq(a.oid[0] + 5ull * a.row[0][cp], o0, o1, o2, o3, o4)) break;
            }
            s = (s + 1) & mask;
        }
        __hip_atomic_fetch_max(&a.table[s].del_max, di + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.dslot[pos] = (u32)s;
    }
}

// one lane per insert: the same probe without claiming; on its OID's slot the largest insert index
// is kept, an empty slot means no delete has this OID
__global__ __launch_bounds__(RN_PT) void k_rn_probe(RnArgs a) {
    const u32 b = blockIdx.x;
    const u32 cnt = rn_block_count(a, 1, b);
    if (!cnt) return;
    const u64 mask = rn_cap(a.bcnt[a.nblk], a.table_slots) - 1;
    const u64 t0 = (u64)b * RN_LB;
    for (u32 i = threadIdx.x; i < cnt; i += RN_PT) {
        const u64 pos = t0 + i;
        const u32 ii = a.list[1][pos];
        const u32* o = a.oid[1] + 5ull * a.row[1][pos];
        const u32 o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3], o4 = o[4];
        u64 s = (((u64)o3 << 32) | o2) & mask;
        for (u64 step = 0; step <= mask; step++) {
            const unsigned long long cur = __hip_atomic_load(&a.table[s].claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) break;  // no partner
            if ((u32)(cur >> 32) == o0) {
                const u64 cp = (u64)(u32)cur - 1;
                if (cp < (u64)a.nblk * RN_LB && rn_oid_eq(a.oid[0] + 5ull * a.row[0][cp], o0, o1, o2, o3, o4)) {
                    __hip_atomic_fetch_max(&a.table[s].ins_max, ii + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
            s = (s + 1) & mask;
        }
    }
}

// a delete wins iff it is its slot's largest delete and the slot has an insert (the table is final:
// plain loads); *ins <- the insert's delta index
__device__ __forceinline__ bool rn_wins(const RnArgs& a, u64 pos, u32* di, u32* ins) {
    *di = a.list[0][pos];
    const RnSlot* t = a.table + a.dslot[pos];
    const u32 dm = t->del_max, im = t->ins_max;
    *ins = im - 1;
    return dm == *di + 1 && im != 0;
}

__global__ __launch_bounds__(256) void k_rn_count(RnArgs a) {
    __shared__ u32 s_w[4];
    const u32 b = blockIdx.x;
    const u32 cnt = rn_block_count(a, 0, b);
    const u64 t0 = (u64)b * RN_LB;
    u32 won = 0;
    for (u32 i0 = 0; i0 < cnt; i0 += 256) {  // (block-uniform)
        const u32 i = i0 + threadIdx.x;
        u32 di, ins;
        const bool w = i < cnt && rn_wins(a, t0 + i, &di, &ins);
        won += (u32)__popcll(__ballot(w));
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = won;
    __syncthreads();
    if (threadIdx.x == 0) a.wcnt[b] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the pairs in ascending delete order: block base (scanned) + rank inside the block (the block's
// deletes are listed in ascending delta order, the blocks are in order)
__global__ __launch_bounds__(256) void k_rn_place(RnArgs a) {
    __shared__ u32 s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const u32 b = blockIdx.x;
    const u32 cnt = rn_block_count(a, 0, b);
    const u64 t0 = (u64)b * RN_LB;
    u32 run = a.wcnt[b];
    for (u32 i0 = 0; i0 < cnt; i0 += 256) {  // (block-uniform)
        const u32 i = i0 + tid;
        u32 di = 0, ins = 0;
        const bool w = i < cnt && rn_wins(a, t0 + i, &di, &ins);
        const u64 bal = __ballot(w);
        if (lane == 0) s_w[wid] = (u32)__popcll(bal);
        __syncthreads();
        u32 wp = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < wid) wp += s_w[k];
            all += s_w[k];
        }
        if (w) a.ren[run + wp + rn_lane_rank(bal)] = make_uint2(di, ins);
        run += all;
        __syncthreads();
    }
}

}  // namespace kd

using namespace kd;

extern "C" int kd_find_renames(kd_ctx* ctx, const kd_side* base, const kd_side* target, const uint32_t* base_order,
                               const uint32_t* target_order, const uint32_t* delta, uint64_t n_delta,
                               const uint64_t* d_n_delta, uint32_t list_mem, uint32_t* ren, uint64_t* n_ren,
                               uint32_t out_mem) {
    KD_CHECK(ctx && base && target && n_ren, "kd_find_renames: NULL argument");
    KD_CHECK((base_order == nullptr) == (target_order == nullptr), "kd_find_renames: one order without the other");
    KD_CHECK(n_delta <= 0xFFFFFFFEull, "kd_find_renames: too many deltas");
    KD_CHECK(n_delta == 0 || delta, "kd_find_renames: delta NULL");
    KD_CHECK(n_delta < 2 || ren, "kd_find_renames: ren NULL");
    KD_CHECK((base->n == 0 || base->oid) && (target->n == 0 || target->oid), "kd_find_renames: a side's oid NULL");
    KD_CHECK(d_n_delta == nullptr || (list_mem == KD_MEM_DEVICE && out_mem == KD_MEM_DEVICE),
             "kd_find_renames: a device count needs a device list and device outputs");
    KD_HIP(hipSetDevice(ctx->device));
    int rc;
    const bool host_out = out_mem == KD_MEM_HOST;
    void* t_n;
    if ((rc = ensure(ctx, "rn.n", 16, &t_n))) return rc;  // the pair count (host outputs), the list scan's total at 8
    u64* const n_dst = host_out ? (u64*)t_n : n_ren;
    if (n_delta < 2) {  // (one delta pairs with nothing)
        KD_HIP(hipMemsetAsync(n_dst, 0, 8, ctx->stream));
        if (host_out) {
            KD_HIP(hipStreamSynchronize(ctx->stream));
            *n_ren = 0;
        }
        return KD_OK;
    }
    RnArgs a{};
    const kd_side* sd[2] = {base, target};
    const u32* od[2] = {base_order, target_order};
    const char* otag[2] = {"rn.oa", "rn.ob"};
    const char* rtag[2] = {"rn.ra", "rn.rb"};
    for (int s = 0; s < 2; s++) {
        const void *o, *r;
        if ((rc = stage_in(ctx, otag[s], sd[s]->n ? sd[s]->oid : nullptr, sd[s]->n * 20, sd[s]->mem, &o))) return rc;
        if ((rc = stage_in(ctx, rtag[s], sd[s]->n ? od[s] : nullptr, sd[s]->n * 4, sd[s]->mem, &r))) return rc;
        KD_CHECK(((u64)o & 3) == 0, "kd_find_renames: oid must be 4-byte aligned");
        a.oid[s] = (const u32*)o;
        a.ord[s] = (const u32*)r;
        a.n_side[s] = sd[s]->n;
    }
    const void* dd;
    if ((rc = stage_in(ctx, "rn.delta", delta, n_delta * 8, list_mem, &dd))) return rc;
    a.delta = (const uint2*)dd;
    a.cap = n_delta;
    a.d_n = d_n_delta;
    const u64 nblk = (n_delta + RN_LB - 1) / RN_LB;
    // a table for as many distinct delete OIDs as there can be: a slot is claimed per distinct OID, a
    // listed delete names a base entry, so min(n_delta, base->n) bounds them (a hand-written list that
    // names one entry twice adds deletes, not OIDs).  The device sizes its cap from the scanned delete
    // count and never beyond these slots; at most 2^32 of them, so a slot index fits 32 bits (more
    // than 2^31 distinct OIDs then probe a table more than half full, still with empty slots)
    u64 slots = RN_CAP_MIN;
    while (slots < 2 * std::min<u64>(n_delta, base->n) && slots < (1ull << 32)) slots <<= 1;
    void *dl, *dr, *db, *dt, *ds, *dw;
    if ((rc = ensure(ctx, "rn.list", 8 * RN_LB * nblk, &dl)) || (rc = ensure(ctx, "rn.row", 8 * RN_LB * nblk, &dr)) ||
        (rc = ensure(ctx, "rn.bcnt", 8 * nblk + 16, &db)) || (rc = ensure(ctx, "rn.table", sizeof(RnSlot) * slots, &dt)) ||
        (rc = ensure(ctx, "rn.dslot", 4 * RN_LB * nblk, &ds)) || (rc = ensure(ctx, "rn.wcnt", 4 * nblk + 16, &dw)))
        return rc;
    u32* dren = ren;
    if (host_out) {
        void* x;
        if ((rc = ensure(ctx, "rn.ren", 8 * (n_delta / 2) + 8, &x))) return rc;
        dren = (u32*)x;
    }
    a.list[0] = (u32*)dl;
    a.list[1] = (u32*)dl + RN_LB * nblk;
    a.row[0] = (u32*)dr;
    a.row[1] = (u32*)dr + RN_LB * nblk;
    a.bcnt = (u32*)db;
    a.tot = (const u64*)((char*)t_n + 8);
    a.nblk = (u32)nblk;
    a.table = (RnSlot*)dt;
    a.table_slots = slots;
    a.dslot = (u32*)ds;
    a.wcnt = (u32*)dw;
    a.ren = (uint2*)dren;
    const dim3 gb((unsigned)nblk), tb(256);
    const unsigned gz = (unsigned)std::max<u64>(1, std::min<u64>((std::min<u64>(slots, 4 * n_delta) + 255) / 256, (u64)ctx->n_cu * 8));
    if ((rc = launch(ctx, "k_rn_list", [&] { hipLaunchKernelGGL(k_rn_list, gb, tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = gf_scan(ctx, a.bcnt, (u32)(2 * nblk), (u64*)((char*)t_n + 8)))) return rc;
    if ((rc = launch(ctx, "k_rn_zero", [&] { hipLaunchKernelGGL(k_rn_zero, dim3(gz), tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_rn_build", [&] { hipLaunchKernelGGL(k_rn_build, gb, dim3(RN_PT), 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_rn_probe", [&] { hipLaunchKernelGGL(k_rn_probe, gb, dim3(RN_PT), 0, ctx->stream, a); }))) return rc;
    if ((rc = launch(ctx, "k_rn_count", [&] { hipLaunchKernelGGL(k_rn_count, gb, tb, 0, ctx->stream, a); }))) return rc;
    if ((rc = gf_scan(ctx, a.wcnt, (u32)nblk, n_dst))) return rc;
    if ((rc = launch(ctx, "k_rn_place", [&] { hipLaunchKernelGGL(k_rn_place, gb, tb, 0, ctx->stream, a); }))) return rc;
    if (!host_out) return KD_OK;
    u64 nr = 0;
    KD_HIP(hipMemcpyAsync(&nr, t_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    KD_CHECK(nr <= n_delta / 2, "kd_find_renames: pair count out of range");
    if (nr) KD_HIP(hipMemcpyAsync(ren, dren, 8 * nr, hipMemcpyDeviceToHost, ctx->stream));
    KD_HIP(hipStreamSynchronize(ctx->stream));
    *n_ren = nr;
    return prof_flush(ctx);
}
