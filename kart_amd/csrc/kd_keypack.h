// kd_keypack.h — a leaf path's join key, decoded the same way on the host and on the device
// (Dataset3.decode_path_to_1pk and the path encoders, see kartdiff.h): what kd_pack_int_keys /
// kd_pack_hash_keys (kd_ctx.hip) and k_kp_pack (kd_keypack.hip) both call.  Every function reads the
// bytes s[0 .. len) of its entry and nothing else; P is a byte pointer of any address space.
//
// The rules are the host packer's as they stand, the lax ones included (parity-unpinned):
//   KD_KEY_INT   the name is what follows the entry's last '/' (no '/': the whole entry); more than 24
//                bytes: status 1.  Base-64 decoding stops at the first '=' (what follows it is not
//                looked at, left-over bits are ignored); a byte outside the alphabet before it: 1; more
//                than 16 decoded bytes: 1; fewer than 2, or a first byte other than 0x91: 1.  Type
//                bytes fixint, negative fixint, 0xcc..0xcf and 0xd0..0xd3, any width for any value;
//                the decoded length must be 2 + w exactly.  An unsigned value of 2^63 or more: 2.
//   KD_KEY_HASH  `levels` segments of one base-64 character (rank-mapped) or two lowercase hex
//                characters, each followed by '/'; any shortfall: 1.  key = bucket << low |
//                fnv1a64(filename) >> (64 - low); an empty filename is valid.
// The key is 0 whenever the status is not.
#pragma once
#include <cstdint>

#include "kd_walkkey.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KD_KP_HD __host__ __device__
#else
#define KD_KP_HD
#endif

namespace kd {
namespace kp {

typedef uint64_t ku64;
typedef int64_t ki64;
typedef uint8_t ku8;

constexpr int INT_NAME_MAX = 24;  // the longest KD_KEY_INT filename looked at

KD_KP_HD inline int b64v(ku8 c) {
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26;
    if (c >= '0' && c <= '9') return c - '0' + 52;
    if (c == '-') return 62;
    if (c == '_') return 63;
    return -1;
}

// b64(msgpack([pk])) of n <= 24 bytes -> the KD_KEY_INT walk key; 0 ok, 1 not an int pk, 2 outside
// [-2^63, 2^63).  Of the up to 16 decoded bytes only the first ten can belong to an accepted name
// (0x91, the type byte, at most eight payload bytes): they are kept in registers, the rest counted.
template <typename P>
KD_KP_HD inline int decode_int_name(P s, int n, ku64* key) {
    unsigned acc = 0, b0 = 0, b1 = 0;
    int o = 0, bits = 0;
    ku64 pay = 0;
    for (int i = 0; i < n; i++) {
        const ku8 c = s[i];
        if (c == '=') break;
        const int v = b64v(c);
        if (v < 0) return 1;
        acc = ((acc << 6) | (unsigned)v) & 0x3fffu;  // (the bits still to come out are the low 13)
        bits += 6;
        if (bits >= 8) {
            bits -= 8;
            if (o >= 16) return 1;
            const unsigned b = (acc >> bits) & 0xFFu;
            if (o == 0) b0 = b;
            else if (o == 1) b1 = b;
            else if (o < 10) pay = (pay << 8) | b;
            o++;
        }
    }
    if (o < 2 || b0 != 0x91) return 1;
    const unsigned t = b1;
    int w = 0;
    bool sgn = false;
    ku64 u = 0;
    if (t <= 0x7f) { u = t; }
    else if (t >= 0xe0) { sgn = true; u = (ku64)(ki64)(int8_t)t; }
    else if (t >= 0xcc && t <= 0xcf) { w = 1 << (t - 0xcc); }
    else if (t >= 0xd0 && t <= 0xd3) { w = 1 << (t - 0xd0); sgn = true; }
    else return 1;
    if (o != 2 + w) return 1;
    if (w) {
        u = pay;  // exactly w bytes, big-endian
        if (sgn) { const int sh = 64 - 8 * w; u = (ku64)(((ki64)(u << sh)) >> sh); }
    }
    if (!sgn && u >= (1ull << 63)) return 2;  // (a signed value is an int64 as it stands)
    *key = wk::int_key((ki64)u);
    return 0;
}

// one KD_KEY_INT entry (a filename or a relative path "c/c/c/c/<filename>") of len bytes.  At most the
// entry's last 25 bytes are read: a name is refused as soon as it is known to be longer than 24.
template <typename P>
KD_KP_HD inline int int_entry(P s, ku64 len, ku64* key) {
    *key = 0;
    int nm = -1;  // the name's length
    for (int k = 0; k <= INT_NAME_MAX; k++) {
        if ((ku64)k == len || s[len - 1 - (ku64)k] == '/') { nm = k; break; }
    }
    if (nm < 0) return 1;
    ku64 k = 0;
    const int st = decode_int_name(s + (len - (ku64)nm), nm, &k);
    if (!st) *key = k;
    return st;
}

template <typename P>
KD_KP_HD inline ku64 fnv1a64(P p, ku64 n) {
    ku64 h = 1469598103934665603ull;
    for (ku64 i = 0; i < n; i++) { h ^= (ku64)(ku8)p[i]; h *= 1099511628211ull; }
    return h;
}

// one KD_KEY_HASH entry "c1/../cL/<filename>" of len bytes; the bucket bits (6 or 8 per level) must be
// fewer than 64 (the callers check)
template <typename P>
KD_KP_HD inline int hash_entry(P s, ku64 len, int levels, int hex, ku64* key) {
    *key = 0;
    ku64 bucket = 0, pos = 0;
    int bits = 0;
    const int seg = hex ? 2 : 1;
    for (int l = 0; l < levels; l++) {
        for (int c = 0; c < seg; c++) {
            if (pos >= len) return 1;
            const ku8 ch = s[pos++];
            if (hex) {
                const int v = (ch >= '0' && ch <= '9') ? ch - '0' : (ch >= 'a' && ch <= 'f') ? ch - 'a' + 10 : -1;
                if (v < 0) return 1;
                bucket = (bucket << 4) | (ku64)v;
                bits += 4;
            } else {
                const int v = b64v(ch);
                if (v < 0) return 1;
                // the digit's ASCII rank: bucket order = git's tree order (kd_walkkey.h)
                bucket = (bucket << 6) | (ku64)wk::T.rank[v];
                bits += 6;
            }
        }
        if (pos >= len || s[pos] != '/') return 1;
        pos++;
    }
    const int low = 64 - bits;
    const ku64 h = fnv1a64(s + pos, len - pos);
    *key = (bucket << low) | (h >> (64 - low));
    return 0;
}

// bucket bits of a hash path structure (64 or more: no key)
KD_KP_HD inline int hash_bits(int levels, int hex) { return levels * (hex ? 8 : 6); }

}  // namespace kp
}  // namespace kd
