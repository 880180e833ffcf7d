// delta_host_check — kd_delta.h on the CPU, for a sanitizer build (tests/test_delta_host.py):
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I kart_amd/csrc
//
// usage: delta_host_check <corpus> <out>
// corpus: u32 n, then per item u32 base_len, u32 delta_len, u32 dst_len, base bytes, delta bytes
//         (little-endian).
// out:    per item one status byte, then its dst_len bytes when the status is 0.
// Base, delta and dst each sit in a heap block of exactly their length, so a load or store outside
// what kd_delta.h yields is an AddressSanitizer report.  The mover is memcpy.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kd_delta.h"

static bool rd32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

static uint32_t apply(const uint8_t* base, uint64_t bl, const uint8_t* d, uint64_t dl, uint8_t* dst, uint64_t ol) {
    uint64_t pos, w = 0, iterations = 0;
    uint32_t st = kd_dl::parse_header(d, dl, bl, ol, &pos);
    while (st == KD_DL_OK) {
        uint32_t kind, len;
        uint64_t src;
        if (++iterations > dl + 1) abort();  // the loop's bound, as the header states it
        st = kd_dl::next_op(d, dl, bl, ol, w, &pos, &kind, &src, &len);
        if (st != KD_DL_OK || kind == kd_dl::OP_END) break;
        memcpy(dst + w, (kind == kd_dl::OP_COPY ? base : d) + src, len);
        w += len;
    }
    return st;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <corpus> <out>\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        perror("open");
        return 2;
    }
    uint32_t n;
    if (!rd32(in, &n)) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t bl, dl, ol;
        if (!rd32(in, &bl) || !rd32(in, &dl) || !rd32(in, &ol)) return 2;
        uint8_t* base = (uint8_t*)malloc(bl);  // (length 0: a block no byte of which may be touched)
        uint8_t* delta = (uint8_t*)malloc(dl);
        uint8_t* dst = (uint8_t*)malloc(ol);
        if (!base || !delta || !dst) return 2;
        if (bl && fread(base, 1, bl, in) != bl) return 2;
        if (dl && fread(delta, 1, dl, in) != dl) return 2;
        if (ol) memset(dst, 0xEE, ol);
        const uint8_t status = (uint8_t)apply(base, bl, delta, dl, dst, ol);
        fwrite(&status, 1, 1, out);
        if (status == 0 && ol) fwrite(dst, 1, ol, out);
        free(dst);
        free(delta);
        free(base);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
