// kd_inflate.h — one zlib stream (RFC 1950 around RFC 1951) decoded into a buffer of known size.
//
// Shared by the device kernel (kd_inflate.hip: one lane per stream, the tables in LDS) and the host
// (tests/inflate_host_check.cpp runs this same text under the sanitizers), as kd_exact.h is shared.
// Written from the two RFCs; zlib is what the results are compared with, and its choices are followed
// where the RFCs leave one (which incomplete code sets are accepted, HLIT above 286, HDIST above 30).
//
// Huffman state is canonical (RFC 1951 §3.2.2): per code length the number of codes, and the symbols
// in code order.  A code is found by walking the lengths 1..15 over the next 15 bits, reversed into
// the order the codes are packed in.  The state of one stream is KD_INF_WORDS 32-bit words; word w is
// at st[w * S], so S = 1 on the host and S = 64 with st = lds + lane on the device (lane-interleaved:
// the 64 lanes' same-index words lie in 64 different banks).
//
// Access rules (each holds by construction):
//   * dst[k] is stored only after k < dst_len was checked; a match is copied only after its distance
//     was checked against the bytes already written and its length against dst_len;
//   * the bit reader loads 4 bytes at a time and only at positions <= src_len + 4, so no byte at or
//     beyond src + src_len + 8 is touched (callers pad the source by 8 bytes); bits past src_len are
//     never used: every consumption is followed by a check of the bit position (KD_INF_ESRC);
//   * symbol table indices are below the number of codes of a set that was checked not to be
//     over-subscribed, code-length indices below HLIT + HDIST <= 316;
//   * the first error ends the stream: nothing more is read or written.
#pragma once
#include <stdint.h>

#include "kartdiff.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KD_INF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KD_INF_HD inline
#endif

namespace kd_inf {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

// words of one stream's state.  The literal/length table holds 16-bit counts and symbols, the small
// table (distance codes, and the code-length code while a dynamic header is read) 8-bit ones:
// 204 words = 816 bytes per stream.
constexpr int W_LCNT = 0;    // 16 x u16: literal/length codes per length
constexpr int W_DCNT = 8;    // 16 x u8: small-table codes per length
constexpr int W_LSYM = 12;   // 288 x u16: literal/length symbols in code order
constexpr int W_DSYM = 156;  // 32 x u8: small-table symbols in code order
constexpr int W_LENS = 164;  // 320 x 4 bits: the code lengths a table is built from
constexpr int KD_INF_WORDS = 204;

// element i of the B-byte-wide array that starts at word w0
template <int S, int B>
KD_INF_HD u32 ldv(const u32* st, int w0, u32 i) {
    if (B == 2) return ((const u16*)(st + (w0 + (int)(i >> 1)) * S))[i & 1];
    return ((const u8*)(st + (w0 + (int)(i >> 2)) * S))[i & 3];
}
template <int S, int B>
KD_INF_HD void stv(u32* st, int w0, u32 i, u32 v) {
    if (B == 2) ((u16*)(st + (w0 + (int)(i >> 1)) * S))[i & 1] = (u16)v;
    else ((u8*)(st + (w0 + (int)(i >> 2)) * S))[i & 3] = (u8)v;
}
template <int S>
KD_INF_HD u32 ld4(const u32* st, u32 i) {
    return (st[(W_LENS + (int)(i >> 3)) * S] >> (4 * (i & 7))) & 15u;
}
template <int S>
KD_INF_HD void st4(u32* st, u32 i, u32 v) {
    u32* p = st + (W_LENS + (int)(i >> 3)) * S;
    const u32 sh = 4 * (i & 7);
    *p = (*p & ~(15u << sh)) | (v << sh);
}

// ---- bit reader: LSB-first, 64-bit buffer, refilled by 4-byte loads ----
struct Bits {
    const u8* src;
    u64 len;  // src_len
    u64 pos;  // next byte to load (may run past len: zeros are fed, and using them is KD_INF_ESRC)
    u64 bb;
    u32 nb;
};

KD_INF_HD void refill(Bits& b) {
    u32 w = 0;
    if (b.pos <= b.len + 4) __builtin_memcpy(&w, b.src + b.pos, 4);  // bytes pos .. pos+3 < len + 8
    b.bb |= (u64)w << b.nb;
    b.nb += 32;
    b.pos += 4;
}
// at least n <= 32 bits in the buffer
KD_INF_HD void need(Bits& b, u32 n) {
    if (b.nb < n) refill(b);
}
// true when a consumed bit lies at or beyond src_len
KD_INF_HD bool spent(const Bits& b) { return b.pos * 8 - b.nb > b.len * 8; }
KD_INF_HD u32 take(Bits& b, u32 n) {  // n <= 32, after need(b, n)
    const u32 v = (u32)(b.bb & ((1ull << n) - 1));
    b.bb >>= n;
    b.nb -= n;
    return v;
}

KD_INF_HD u32 rev16(u32 v) {
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
    return ((v >> 8) & 0x00FFu) | ((v & 0x00FFu) << 8);
}

// Build the canonical table of the n code lengths at LENS[first ..) into (count words cw, symbol
// words sw, B bytes per element).  Returns -1 for an over-subscribed set, else the unused code space
// in units of 2^-15 (0: complete); *ncodes <- the symbols with a nonzero length.
// No array is indexed in registers: the counts themselves serve as the running slot of each length
// while the symbols are placed (count -> first slot -> one past the last slot -> count again).
template <int S, int B>
KD_INF_HD int build(u32* st, int cw, int sw, u32 first, u32 n, u32* ncodes) {
    for (u32 l = 0; l < 16; l++) stv<S, B>(st, cw, l, 0);
    u32 zeros = 0;
    for (u32 i = 0; i < n; i++) {
        const u32 l = ld4<S>(st, first + i);
        if (l) stv<S, B>(st, cw, l, ldv<S, B>(st, cw, l) + 1);  // (<= n: fits B bytes)
        else zeros++;
    }
    *ncodes = n - zeros;
    int left = 1;
    u32 o = 0;
    for (u32 l = 1; l < 16; l++) {
        const u32 c = ldv<S, B>(st, cw, l);
        left = (left << 1) - (int)c;
        if (left < 0) return -1;
        stv<S, B>(st, cw, l, o);
        o += c;
    }
    for (u32 i = 0; i < n; i++) {
        const u32 l = ld4<S>(st, first + i);
        if (l) {
            const u32 at = ldv<S, B>(st, cw, l);  // < ncodes <= n: the set is not over-subscribed
            stv<S, B>(st, sw, at, i);
            stv<S, B>(st, cw, l, at + 1);
        }
    }
    o = 0;
    for (u32 l = 1; l < 16; l++) {
        const u32 e = ldv<S, B>(st, cw, l);
        stv<S, B>(st, cw, l, e - o);
        o = e;
    }
    return left;
}

// The next symbol of the table (cw, sw): >= 0, or -1 for a code the set does not assign.
// *err <- KD_INF_ESRC when the code's bits run past src_len.
template <int S, int B>
KD_INF_HD int decode(const u32* st, int cw, int sw, Bits& b, u32* err) {
    need(b, 15);
    const u32 r = rev16((u32)b.bb & 0x7FFFu) >> 1;  // the next 15 bits, first bit on top
    u32 first = 0, index = 0;
    for (u32 l = 1; l < 16; l++) {
        const u32 c = ldv<S, B>(st, cw, l);
        const u32 code = r >> (15 - l);
        if (code - first < c) {  // (code >= first: the codes below belong to shorter lengths)
            take(b, l);
            if (spent(b)) *err = KD_INF_ESRC;
            return (int)ldv<S, B>(st, sw, index + (code - first));
        }
        index += c;
        first = (first + c) << 1;
    }
    return -1;
}

// RFC 1951 §3.2.6: the fixed code's lengths, then both tables
template <int S>
KD_INF_HD void build_fixed(u32* st) {
    for (u32 i = 0; i < 288; i++) st4<S>(st, i, i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : 8u);
    for (u32 i = 288; i < 318; i++) st4<S>(st, i, 5u);
    u32 nc;
    build<S, 2>(st, W_LCNT, W_LSYM, 0, 288, &nc);
    build<S, 1>(st, W_DCNT, W_DSYM, 288, 30, &nc);
}

// RFC 1951 §3.2.7: HLIT, HDIST, HCLEN, the code-length code, the two sets of lengths
template <int S>
KD_INF_HD u32 build_dynamic(u32* st, Bits& b) {
    need(b, 14);
    const u32 nlen = take(b, 5) + 257, ndist = take(b, 5) + 1, ncl = take(b, 4) + 4;
    if (spent(b)) return KD_INF_ESRC;
    if (nlen > 286 || ndist > 30) return KD_INF_ELENS;  // (as zlib: symbols that can never be used)
    // the order the code-length code's lengths come in, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const u64 ord_a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                      10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const u64 ord_b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (u32 i = 0; i < 19; i++) st4<S>(st, i, 0);
    for (u32 i = 0; i < ncl; i++) {
        need(b, 3);
        const u32 l = take(b, 3);
        if (spent(b)) return KD_INF_ESRC;
        st4<S>(st, (u32)((i < 12 ? ord_a >> (5 * i) : ord_b >> (5 * (i - 12))) & 31), l);
    }
    u32 nc;
    if (build<S, 1>(st, W_DCNT, W_DSYM, 0, 19, &nc) != 0) return KD_INF_ELENS;  // must be complete
    const u32 total = nlen + ndist;
    u32 have = 0, prev = 0;
    while (have < total) {
        u32 err = 0;
        const int sym = decode<S, 1>(st, W_DCNT, W_DSYM, b, &err);
        if (err) return err;
        if (sym < 0) return KD_INF_ELENS;  // (a complete set assigns every code: not reached)
        if (sym < 16) {
            st4<S>(st, have++, prev = (u32)sym);
            continue;
        }
        u32 rep, val = 0;
        if (sym == 16) {
            if (have == 0) return KD_INF_ELENS;  // nothing to repeat
            val = prev;
            need(b, 2);
            rep = 3 + take(b, 2);
        } else if (sym == 17) {
            need(b, 3);
            rep = 3 + take(b, 3);
        } else {
            need(b, 7);
            rep = 11 + take(b, 7);
        }
        if (spent(b)) return KD_INF_ESRC;
        if (have + rep > total) return KD_INF_ELENS;  // a repeat running past HLIT + HDIST
        prev = val;
        for (u32 k = 0; k < rep; k++) st4<S>(st, have++, val);
    }
    if (ld4<S>(st, 256) == 0) return KD_INF_ELENS;  // no end-of-block code
    // an incomplete set is accepted only as one code of one bit (what zlib accepts); a distance set
    // may also be empty (a block of literals)
    int left = build<S, 2>(st, W_LCNT, W_LSYM, 0, nlen, &nc);
    if (left < 0 || (left > 0 && !(nc == 1 && ldv<S, 2>(st, W_LCNT, 1) == 1))) return KD_INF_ELENS;
    left = build<S, 1>(st, W_DCNT, W_DSYM, nlen, ndist, &nc);
    if (left < 0 || (left > 0 && nc != 0 && !(nc == 1 && ldv<S, 1>(st, W_DCNT, 1) == 1))) return KD_INF_ELENS;
    return KD_INF_OK;
}

// One zlib stream from src[0 .. src_len) into exactly dst_len bytes; a KD_INF_* status.
// src_len bounds the stream (bytes after its end are ignored).  dst is read back by matches: no
// __restrict__, no non-temporal stores.  st: KD_INF_WORDS words of state, S words apart.
template <int S>
KD_INF_HD u32 inflate_stream(const u8* src, u64 src_len, u8* dst, u64 dst_len, u32* st) {
    Bits b;
    b.src = src;
    b.len = src_len;
    b.pos = 0;
    b.bb = 0;
    b.nb = 0;
    need(b, 16);
    const u32 cmf = take(b, 8), flg = take(b, 8);
    if (spent(b)) return KD_INF_ESRC;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return KD_INF_EHEADER;
    u64 out = 0;
    u32 s1 = 1, s2 = 0, until = 5552;  // Adler-32: 5552 bytes keep s2 below 2^32 between two modulos
#define KD_INF_EMIT(byte_)                  \
    {                                       \
        const u32 v_ = (byte_);             \
        dst[out++] = (u8)v_;                \
        s1 += v_;                           \
        s2 += s1;                           \
        if (--until == 0) {                 \
            s1 %= 65521u;                   \
            s2 %= 65521u;                   \
            until = 5552;                   \
        }                                   \
    }
    for (;;) {
        need(b, 3);
        const u32 last = take(b, 1), type = take(b, 2);
        if (spent(b)) return KD_INF_ESRC;
        if (type == 3) return KD_INF_EBTYPE;
        if (type == 0) {
            take(b, b.nb & 7);  // to the byte boundary (pos * 8 is one)
            need(b, 32);
            const u32 len = take(b, 16), nlen = take(b, 16);
            if (spent(b)) return KD_INF_ESRC;
            if ((len ^ nlen) != 0xFFFFu) return KD_INF_ESTORED;
            if (len > dst_len - out) return KD_INF_EOVER;
            for (u32 k = 0; k < len; k++) {
                need(b, 8);
                const u32 v = take(b, 8);
                if (spent(b)) return KD_INF_ESRC;
                KD_INF_EMIT(v)  // out < dst_len: len <= dst_len - out was checked
            }
        } else {
            if (type == 1) {
                build_fixed<S>(st);
            } else {
                const u32 e = build_dynamic<S>(st, b);
                if (e) return e;
            }
            for (;;) {
                u32 err = 0;
                int sym = decode<S, 2>(st, W_LCNT, W_LSYM, b, &err);
                if (err) return err;
                if (sym < 0 || sym > 285) return KD_INF_ESYMBOL;
                if (sym < 256) {
                    if (out >= dst_len) return KD_INF_EOVER;
                    KD_INF_EMIT((u32)sym)
                    continue;
                }
                if (sym == 256) break;
                // length 3..258: symbols 257..264 one each, then four symbols per extra-bit count
                u32 len;
                if (sym < 265) {
                    len = (u32)sym - 254;
                } else if (sym == 285) {
                    len = 258;
                } else {
                    const u32 e = ((u32)sym - 261) >> 2;
                    need(b, e);
                    len = 3 + ((4 + (((u32)sym - 261) & 3)) << e) + take(b, e);
                    if (spent(b)) return KD_INF_ESRC;
                }
                sym = decode<S, 1>(st, W_DCNT, W_DSYM, b, &err);
                if (err) return err;
                if (sym < 0 || sym > 29) return KD_INF_ESYMBOL;
                // distance 1..32768: symbols 0..3 one each, then two symbols per extra-bit count
                u64 dist;
                if (sym < 4) {
                    dist = (u32)sym + 1;
                } else {
                    const u32 e = ((u32)sym >> 1) - 1;
                    need(b, e);
                    dist = 1 + ((2 + ((u32)sym & 1)) << e) + take(b, e);
                    if (spent(b)) return KD_INF_ESRC;
                }
                if (dist > out) return KD_INF_EDIST;
                if (len > dst_len - out) return KD_INF_EOVER;
                for (u32 k = 0; k < len; k++) KD_INF_EMIT(dst[out - dist])  // byte by byte: dist < len repeats
            }
        }
        if (last) break;
    }
#undef KD_INF_EMIT
    if (out != dst_len) return KD_INF_ESHORT;
    s1 %= 65521u;
    s2 %= 65521u;
    take(b, b.nb & 7);
    need(b, 32);
    const u32 t = take(b, 32);
    if (spent(b)) return KD_INF_ESRC;
    const u32 adler = (t >> 24) | ((t >> 8) & 0xFF00u) | ((t << 8) & 0xFF0000u) | (t << 24);  // big-endian
    return adler == ((s2 << 16) | s1) ? KD_INF_OK : KD_INF_EADLER;
}

}  // namespace kd_inf
