// inflate_host_check — kd_inflate.h on the CPU, for a sanitizer build (tests/test_inflate_host.py):
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I kart_amd/csrc
//
// usage: inflate_host_check <corpus> <out>
// corpus: u32 n, then per stream u32 src_len, u32 dst_len, src bytes (little-endian).
// out:    per stream one status byte, then its dst_len bytes when the status is 0.
// Every stream gets heap blocks of exactly src_len + 8 and dst_len bytes, so a load or store outside
// what kd_inflate.h promises to touch is an AddressSanitizer report.  The 8 bytes of padding are 0xA5:
// a decoder that used them would not see the zeros a short read feeds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kd_inflate.h"

static bool rd32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

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
        uint32_t sl, dl;
        if (!rd32(in, &sl) || !rd32(in, &dl)) return 2;
        uint8_t* src = (uint8_t*)malloc((size_t)sl + 8);
        uint8_t* dst = (uint8_t*)malloc(dl);  // (dl = 0: a block no byte of which may be touched)
        uint32_t* st = (uint32_t*)calloc(kd_inf::KD_INF_WORDS, 4);
        if (!src || !dst || !st) return 2;
        if (sl && fread(src, 1, sl, in) != sl) return 2;
        memset(src + sl, 0xA5, 8);
        if (dl) memset(dst, 0xEE, dl);
        const uint8_t status = (uint8_t)kd_inf::inflate_stream<1>(src, sl, dst, dl, st);
        fwrite(&status, 1, 1, out);
        if (status == 0 && dl) fwrite(dst, 1, dl, out);
        free(st);
        free(dst);
        free(src);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
