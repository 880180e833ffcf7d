// keypack_host_check — kd_keypack.h on the CPU for tests/test_keypack_host.py (built with
// -fsanitize=address,undefined).  Reads a corpus
//   u32 count, then per item: u32 key_mode, i32 levels, i32 hex, u32 len, len bytes
// decodes every entry from a heap block of exactly its length (a read outside the entry ends the program
// under the sanitizer) and writes per item: u64 key, u8 status.
#define __host__
#define __device__
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kartdiff.h"
#include "kd_keypack.h"

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t mode = 0, len = 0;
        int32_t levels = 0, hex = 0;
        if (!rd(f, &mode, 4) || !rd(f, &levels, 4) || !rd(f, &hex, 4) || !rd(f, &len, 4)) return 2;
        uint8_t* s = (uint8_t*)malloc(len);  // exactly the entry (len 0: a block nothing may read)
        if (len && (!s || !rd(f, s, len))) return 2;
        uint64_t key = 0xdeadbeefdeadbeefull;
        int st;
        if (mode == KD_KEY_INT) st = kd::kp::int_entry((const uint8_t*)s, (uint64_t)len, &key);
        else st = kd::kp::hash_entry((const uint8_t*)s, (uint64_t)len, levels, hex, &key);
        free(s);
        const uint8_t b = (uint8_t)st;
        fwrite(&key, 8, 1, o);
        fwrite(&b, 1, 1, o);
    }
    fclose(f);
    return fclose(o) ? 2 : 0;
}
