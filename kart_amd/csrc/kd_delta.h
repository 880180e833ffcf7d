// kd_delta.h — git's delta format decoded op by op: the header's two sizes, then copy / insert ops.
//
// Shared by the device kernel (kd_delta.hip: a group of lanes per item walks the ops together and moves
// each op's bytes cooperatively) and the host (tests/delta_host_check.cpp runs this same text under the
// sanitizers with memcpy as the mover), as kd_inflate.h and kd_exact.h are shared.  Written from git's
// pack format documentation (Documentation/technical/pack-format.txt, "Deltified representation"):
//   header   two little-endian base-128 varints: the base's size, the result's size (at most 10 bytes
//            each; longer or truncated: KD_DL_EHEADER)
//   copy     0x80 | mask: mask bits 0..3 say which offset bytes follow, bits 4..6 which size bytes, each
//            little-endian, an absent byte is 0, size 0 means 0x10000
//   insert   1..127: that many literal bytes follow
//   0        reserved (KD_DL_EOP)
// This header is only about ops and bounds; how an op's bytes are moved is the caller's business.
// next_op yields (kind, source offset, length) of one op after the whole op was validated.
//
// Access rules (each holds by construction):
//   * no byte of the delta is read at or beyond delta_len: every load of d[pos] follows pos < delta_len;
//   * a copy is yielded only after offset + length <= base_len, an insert only after its literals lie
//     inside the delta, and either only after written + length <= dst_len: a mover that copies exactly
//     (source offset, length) to dst + written reads no byte outside the item's base and delta ranges
//     and writes none outside its dst range;
//   * a byte is stored (by the caller) only after the whole op passed those checks;
//   * next_op consumes at least one delta byte per call that yields an op, so a loop over it ends
//     after at most delta_len calls whatever the input;
//   * the first error ends the item: nothing more is read or written.
#pragma once
#include <stdint.h>

#include "kartdiff.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KD_DL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KD_DL_HD inline
#endif

namespace kd_dl {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum { OP_END = 0, OP_COPY = 1, OP_INSERT = 2 };

// one size varint at d[*pos ..): false when it is truncated or longer than 10 bytes
KD_DL_HD bool size_varint(const u8* d, u64 dlen, u64* pos, u64* out) {
    u64 v = 0;
    for (int k = 0; k < 10; k++) {
        if (*pos >= dlen) return false;
        const u8 c = d[(*pos)++];
        if (7 * k < 64) v |= (u64)(c & 0x7F) << (7 * k);
        if (!(c & 0x80)) {
            *out = v;
            return true;
        }
    }
    return false;
}

// the header of the delta d[0 .. dlen) checked against the ranges it is applied to; *pos <- the first op
KD_DL_HD u32 parse_header(const u8* d, u64 dlen, u64 base_len, u64 dst_len, u64* pos) {
    u64 bs, rs;
    *pos = 0;
    if (!size_varint(d, dlen, pos, &bs) || !size_varint(d, dlen, pos, &rs)) return KD_DL_EHEADER;
    if (bs != base_len) return KD_DL_EBASE;
    if (rs != dst_len) return KD_DL_ESIZE;
    return KD_DL_OK;
}

// the op at d[*pos]; `written` result bytes exist so far.  KD_DL_OK with
//   *kind = OP_COPY:   base[*src .. *src + *len) is the next *len result bytes
//   *kind = OP_INSERT: d[*src .. *src + *len) is
//   *kind = OP_END:    the delta is used up and the result is complete
// and *pos behind the op; anything else is the item's status.
KD_DL_HD u32 next_op(const u8* d, u64 dlen, u64 base_len, u64 dst_len, u64 written, u64* pos, u32* kind, u64* src, u32* len) {
    u64 p = *pos;
    if (p >= dlen) {
        *kind = OP_END;
        return written == dst_len ? KD_DL_OK : KD_DL_ESHORT;
    }
    const u32 op = d[p++];
    if (op == 0) return KD_DL_EOP;
    if (op & 0x80) {
        u64 off = 0;
        u32 sz = 0;
        for (int b = 0; b < 4; b++)
            if (op & (1u << b)) {
                if (p >= dlen) return KD_DL_ETRUNC;
                off |= (u64)d[p++] << (8 * b);
            }
        for (int b = 0; b < 3; b++)
            if (op & (0x10u << b)) {
                if (p >= dlen) return KD_DL_ETRUNC;
                sz |= (u32)d[p++] << (8 * b);
            }
        if (sz == 0) sz = 0x10000;
        if (off > base_len || sz > base_len - off) return KD_DL_ECOPY;
        if (sz > dst_len - written) return KD_DL_EOVER;
        *kind = OP_COPY;
        *src = off;
        *len = sz;
    } else {
        if (op > dlen - p) return KD_DL_ETRUNC;
        if (op > dst_len - written) return KD_DL_EOVER;
        *kind = OP_INSERT;
        *src = p;
        *len = op;
        p += op;
    }
    *pos = p;
    return KD_DL_OK;
}

}  // namespace kd_dl

// ---------------------------------------------------------------------------------------------
// the chained form (library internal): what the planner (kd_odb_plan.cpp) hands to kd_delta.hip
// ---------------------------------------------------------------------------------------------
namespace kd {

// one delta node of a level.  Each of its three ranges lies in one of two allocations: 0 the returned
// arena, 1 the workspace (bits 0 / 1 / 2 of `where`: base / delta / dst).  *_st index one status array
// shared by the two inflate launches and every level: an item whose base or payload status is not 0
// is KD_DL_EPARENT.
struct DlItem {
    uint64_t base_at, delta_at, dst_at;
    uint32_t base_len, delta_len, dst_len, where;
    uint32_t base_st, delta_st, out_st, pad;
};

// a further request of a node already rebuilt: copied device to device after the last level
struct DlCopy {
    uint64_t src_at, dst_at, len;
    uint32_t src_ws, pad;
};

struct DlPlan {
    const uint8_t* h_src;     // pinned: launch 1's sources, launch 2's behind them, 8 bytes of padding
    // launch 1 (k_inf_streams into the arena): the n requests, as kd::inflate_from_host takes them
    uint64_t n;
    const uint64_t* soff1;    // [n + 1]
    const uint8_t* kind1;     // [n]
    const uint64_t* off;      // [n + 1] the arena's offsets
    // launch 2 (k_inf_streams into the workspace): unrequested chain bases, then every delta payload
    uint64_t m;
    const uint64_t* soff2;    // [m + 1], relative to h_src + soff1[n]
    const uint64_t* woff;     // [m + 1] workspace offsets
    uint64_t ws_bytes;        // the workspace: launch 2's results, then unrequested delta results
    // the levels: items[level_start[l - 1] .. level_start[l]) is level l = 1 .. depth
    const DlItem* items;
    uint64_t n_items;
    const uint64_t* level_start;  // [depth + 1]
    uint32_t depth;
    const DlCopy* copies;
    uint64_t n_copies;
    uint8_t* h_status;        // [n + m + n_items]
    uint8_t* d_dst;           // the arena (off[n] bytes) and its offsets
    uint64_t* d_dst_off;
};

// upload, two inflate launches, one k_dl_apply launch per level, the copies, every status back
int delta_read_from_host(kd_ctx* ctx, const DlPlan& p);

}  // namespace kd
