// kd_treeparse.h — git's tree object decoded entry by entry, for leaf trees.
//
// Shared by the device kernels (kd_treewalk.hip: the k-way join of changed leaf trees, whose merge loop
// is at the end of this file) and the host (tests/treeparse_host_check.cpp runs this same text under
// the sanitizers), as kd_inflate.h and kd_delta.h are shared.  Written from git's tree format:
//   entry    <octal mode> SP <name> NUL <20 raw OID bytes>, repeated to the end of the object
//   order    between non-tree entries: names ascending by unsigned bytewise compare, then length
// The decoder defines the *device class* of a tree: the trees for which the device join is provably
// kd_walk's.  It is stricter than kd_odb_walk.cpp's parse_tree and never laxer — whatever it refuses goes
// to the host walk, which then behaves as it always did:
//   KD_TJ_EMODE   a mode byte that is no octal digit, no digits at all, more than 11 digits or a
//                 value above 2^32 - 1 (parse_tree wraps), or the object ends inside the mode
//   KD_TJ_ENAME   an empty name, or no NUL before the end
//   KD_TJ_EOID    fewer than 20 bytes behind the NUL
//   KD_TJ_ETREE   mode 040000: a subtree at leaf depth is the host's (every other mode is a leaf, as
//                 in kd_walk; so git's '/' rule for tree names never applies inside the class)
//   KD_TJ_EORDER  a name not strictly above the one before it
//   KD_TJ_EBIG    a tree of more than KD_TJ_MAX_BYTES bytes (name lengths and per-task counts are
//                 32-bit)
// The zero-length tree is valid and has no entries.
//
// Access rules (each holds by construction):
//   * no byte at or beyond len is looked at: a chunk's bytes beyond len are masked off (the host form
//     does not even read them; the device form reads up to 7 of them, the arena's documented pad), and
//     an entry's OID is yielded only after oid + 20 <= len;
//   * entry boundaries are a sequential chain: the SP is searched from the entry's first byte, the NUL
//     from the name's first byte, and the next entry starts 21 bytes behind that NUL.  An OID byte may
//     be 0x00 or 0x20; it is never looked at by either search, because both start behind the previous
//     entry's OID and stop at their first hit — the searches read 8 bytes at a time, in chunks that begin
//     at the search's start, so the first hit of a chunk is the first hit at or after that start;
//   * next_entry consumes at least 23 bytes per entry it yields, so a loop over it ends after at most
//     len / 23 + 1 calls whatever the input;
//   * nothing is allocated and nothing is written but the cursor and the entry.
#pragma once
#include <stdint.h>
#include <string.h>

#include "kartdiff.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KD_TJ_HD __host__ __device__ inline __attribute__((always_inline))
#define KD_TJ_UNROLL _Pragma("unroll")
#else
#define KD_TJ_HD inline
#define KD_TJ_UNROLL
#endif

namespace kd_tj {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 MODE_TREE = 040000;
constexpr int MODE_DIGITS = 11;  // what a u32 mode needs in octal

// one entry: name and oid are offsets into the tree
struct Ent {
    u64 name;
    u64 oid;
    u32 nlen;
    u32 mode;
};

// where the decoder stands: the next entry's offset and the name it must lie above
struct Cur {
    u64 pos = 0;
    u64 pname = 0;
    u32 pnlen = 0;  // 0: no entry yet (a name is never empty)
};

// ---- loads: 8 bytes per access at any byte address (gfx950 runs in unaligned mode, as kd_delta.hip's
// 16-byte moves rely on).  The host form never reads a byte it does not return, so the sanitizers see
// exactly the decoder's own range; the device form of load_upto8 reads all 8 and masks, which is why
// a device arena must be readable 8 bytes past its last tree (kartdiff.h) ----
KD_TJ_HD u64 load8(const u8* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef u64 __attribute__((aligned(1))) u64_b;
    return *(const u64_b*)p;
#else
    u64 v;
    memcpy(&v, p, 8);
    return v;
#endif
}

// the first `have` (1..8) bytes at p, little-endian, the others zero
KD_TJ_HD u64 load_upto8(const u8* p, u32 have) {
#if defined(__HIP_DEVICE_COMPILE__)
    const u64 v = load8(p);
    return have < 8 ? v & ~(~0ull << (8 * have)) : v;
#else
    u64 v = 0;
    memcpy(&v, p, have < 8 ? have : 8);
    return v;
#endif
}

// x != y: the order of the first byte (the lowest, little-endian) in which they differ, unsigned
KD_TJ_HD int first_diff(u64 x, u64 y) {
    const int k = __builtin_ctzll(x ^ y) & ~7;
    return (u32)((x >> k) & 0xFF) < (u32)((y >> k) & 0xFF) ? -1 : 1;
}

// git's order between non-tree names: unsigned bytes, then length.  Both are names of decoded entries:
// 21 bytes of their own tree follow each (the NUL and the OID), so an 8-byte load that starts inside a
// name stays inside the tree.
KD_TJ_HD int name_cmp(const u8* a, u32 al, const u8* b, u32 bl) {
    const u32 n = al < bl ? al : bl;
    u32 i = 0;
    for (; i + 8 <= n; i += 8) {
        const u64 x = load8(a + i), y = load8(b + i);
        if (x != y) return first_diff(x, y);
    }
    if (i < n) {
        const u64 m = ~(~0ull << (8 * (n - i)));
        const u64 x = load8(a + i) & m, y = load8(b + i) & m;
        if (x != y) return first_diff(x, y);
    }
    return al < bl ? -1 : al > bl ? 1 : 0;
}

KD_TJ_HD bool oid_eq(const u8* a, const u8* b) {  // (bytes 0..7, 8..15 and 12..19)
    return ((load8(a) ^ load8(b)) | (load8(a + 8) ^ load8(b + 8)) | (load8(a + 12) ^ load8(b + 12))) == 0;
}

// the entry at p[c->pos ..) of the tree p[0 .. len).  KD_TJ_OK with *more = true: *e is it and the
// cursor is behind it; KD_TJ_OK with *more = false: the tree is used up; anything else is the tree's
// status (the cursor and *e are then unspecified and the tree is not decoded further).  len <=
// KD_TJ_MAX_BYTES is the caller's check (tree_status).
// The mode and the name are read in chunks of up to 8 bytes that START at the entry's first byte and at
// the name's first byte: a chunk never holds a byte in front of the position its search starts from, so
// "the first SP / NUL at or after the start" is the lowest hit of the chunk; bytes at or beyond len are
// masked off before they are looked at.
KD_TJ_HD u32 next_entry(const u8* p, u64 len, Cur* c, Ent* e, bool* more) {
    u64 q = c->pos;
    *more = false;
    if (q >= len) return KD_TJ_OK;
    u64 mode = 0;
    int nd = 0;
    for (bool sp = false; !sp;) {
        if (q >= len) return KD_TJ_EMODE;
        const u32 have = len - q < 8 ? (u32)(len - q) : 8u;
        const u64 w = load_upto8(p + q, have);
        u32 i = 0;
        for (; i < have; i++) {
            const u32 b = (u32)(w >> (8 * i)) & 0xFF;
            if (b == ' ') {
                sp = true;
                break;
            }
            if (b < '0' || b > '7' || nd == MODE_DIGITS) return KD_TJ_EMODE;
            mode = mode * 8 + (b - '0');
            nd++;
        }
        q += i;
    }
    if (nd == 0 || mode > 0xFFFFFFFFull) return KD_TJ_EMODE;
    const u64 name = ++q;
    for (u64 s = name;;) {
        if (s >= len) return KD_TJ_ENAME;
        const u32 have = len - s < 8 ? (u32)(len - s) : 8u;
        u64 v = load_upto8(p + s, have);
        if (have < 8) v |= ~0ull << (8 * have);  // (no NUL beyond the tree)
        const u64 z = (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;  // lowest flag: the first NUL
        if (z) {
            q = s + ((u32)__builtin_ctzll(z) >> 3);
            break;
        }
        s += have;
    }
    if (q == name) return KD_TJ_ENAME;
    if (len - q < 21) return KD_TJ_EOID;
    if ((u32)mode == MODE_TREE) return KD_TJ_ETREE;
    const u32 nlen = (u32)(q - name);
    // DO NOT MOVE these assignments behind the order check.  With the fields assigned after it, a gfx950
    // build gave every later entry of a tree the first entry's mode (profiles/device_walk/
    // stale_mode_asm.txt; unexplained, host builds were right).  Written before the check,
    // unconditionally, no value is merged across the compare loop; a refused tree's cursor and entry are
    // nobody's to read.  The only tripwire is tests/test_gpu_tree_join.py::test_every_task_shape_and_compare,
    // which compares every mode on the device: run it after any change here or of the compiler.
    const u64 pname = c->pname;
    const u32 pnlen = c->pnlen;
    e->name = name;
    e->nlen = nlen;
    e->mode = (u32)mode;
    e->oid = q + 1;
    c->pos = q + 21;
    c->pname = name;
    c->pnlen = nlen;
    if (pnlen && name_cmp(p + pname, pnlen, p + name, nlen) >= 0) return KD_TJ_EORDER;
    *more = true;
    return KD_TJ_OK;
}

// a whole tree's status and entry count (what the host check and a planner ask)
KD_TJ_HD u32 tree_status(const u8* p, u64 len, u64* n_entries) {
    *n_entries = 0;
    if (len > KD_TJ_MAX_BYTES) return KD_TJ_EBIG;
    Cur c;
    Ent e;
    for (;;) {
        bool more;
        const u32 st = next_entry(p, len, &c, &e, &more);
        if (st != KD_TJ_OK) return st;
        if (!more) return KD_TJ_OK;
        (*n_entries)++;
    }
}

// ---------------------------------------------------------------------------------------------
// the K-way join of one task's trees (what a lane of k_tj_count / k_tj_emit runs, and the host check)
// ---------------------------------------------------------------------------------------------
template <int K>
struct Trees {
    const u8* p[K];  // (a valid pointer also where has[r] is false)
    u64 len[K];
    bool has[K];
};

// the task's status: that of the first root's tree that is refused
template <int K>
KD_TJ_HD u32 task_status(const Trees<K>& T) {
    u32 st = KD_TJ_OK;
    KD_TJ_UNROLL
    for (int r = 0; r < K; r++) {
        u64 ne;
        if (st == KD_TJ_OK && T.has[r]) st = tree_status(T.p[r], T.len[r], &ne);
    }
    return st;
}

// Walk::join + Walk::pruned of kd_odb_walk.cpp restricted to non-tree entries: the K entry lists merged by
// name; a name is dropped in every root when roots c0 and c1 agree on it (both lack it, or both have it
// with equal mode and OID; c0 < 0: nothing is dropped); fn(r, entry) for every other entry of each root
// that has it, in name order and within a name in root order.  The trees passed task_status; a tree
// that fails all the same just ends there.  The per-root state is indexed only inside loops over K that
// are fully unrolled on the device (no runtime-indexed array, no scratch).
template <int K, class F>
KD_TJ_HD void join(const Trees<K>& T, int c0, int c1, F&& fn) {
    Cur c[K];
    Ent e[K];
    bool v[K];
    KD_TJ_UNROLL
    for (int r = 0; r < K; r++) {
        e[r] = Ent{0, 0, 0, 0};
        v[r] = false;
        if (T.has[r] && next_entry(T.p[r], T.len[r], &c[r], &e[r], &v[r]) != KD_TJ_OK) v[r] = false;
    }
    for (;;) {
        bool any = false;
        const u8* mn = T.p[0];
        u32 ml = 0;
        KD_TJ_UNROLL
        for (int r = 0; r < K; r++) {
            if (!v[r]) continue;
            const u8* nm = T.p[r] + e[r].name;
            if (!any || name_cmp(nm, e[r].nlen, mn, ml) < 0) {
                mn = nm;
                ml = e[r].nlen;
                any = true;
            }
        }
        if (!any) break;
        bool in[K];
        KD_TJ_UNROLL
        for (int r = 0; r < K; r++) in[r] = v[r] && name_cmp(T.p[r] + e[r].name, e[r].nlen, mn, ml) == 0;
        bool drop = false;
        if (c0 >= 0) {
            bool x = false, y = false;
            u32 xm = 0, ym = 0;
            const u8 *xo = mn, *yo = mn;
            KD_TJ_UNROLL
            for (int r = 0; r < K; r++) {
                if (r == c0) {
                    x = in[r];
                    xm = e[r].mode;
                    xo = T.p[r] + e[r].oid;
                }
                if (r == c1) {
                    y = in[r];
                    ym = e[r].mode;
                    yo = T.p[r] + e[r].oid;
                }
            }
            if (x != y) drop = false;
            else if (!x) drop = true;
            else drop = xm == ym && oid_eq(xo, yo);
        }
        KD_TJ_UNROLL
        for (int r = 0; r < K; r++) {
            if (!in[r]) continue;
            if (!drop) fn(r, e[r]);
            if (next_entry(T.p[r], T.len[r], &c[r], &e[r], &v[r]) != KD_TJ_OK) v[r] = false;
        }
    }
}

}  // namespace kd_tj
