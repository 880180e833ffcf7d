// treeparse_host_check — kd_treeparse.h run on the CPU under AddressSanitizer and UBSan.
//
// usage: treeparse_host_check corpus.bin out.bin
//   corpus: u32 n, then per tree u32 len and the bytes
//   out:    per tree u8 status (tree_status), u32 entries, then per entry u32 mode, name offset, name
//           length, oid offset (none unless the status is 0); one closing byte: the status of a tree one
//           byte above KD_TJ_MAX_BYTES
// usage: treeparse_host_check join corpus.bin out.bin   (the K-way join of kd_treeparse.h)
//   corpus: u32 tasks, then per task u32 k, i32 cmp0, i32 cmp1 and per root u32 present, u32 len, bytes
//   out:    per task u8 status (task_status); if 0, per root u32 kept entries and per entry u32 mode,
//           u32 name length, the name, the 20 OID bytes
// Each tree is copied into a heap block of exactly its length, so any access outside [p, p + len) ends
// the program.  The oversized tree is a one-byte block with a claimed length of KD_TJ_MAX_BYTES + 1:
// the decoder must refuse it before it reads anything.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kd_treeparse.h"

static bool read_all(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + r);
    fclose(f);
    return true;
}

static void put32(std::vector<uint8_t>& o, uint32_t v) {
    for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i)));
}

template <int K>
static void join_task(uint8_t* const* blk, const uint32_t* len, const uint32_t* present, int c0, int c1, std::vector<uint8_t>& out) {
    kd_tj::Trees<K> T;
    for (int r = 0; r < K; r++) {
        T.p[r] = len[r] ? blk[r] : blk[r] + 1;
        T.len[r] = len[r];
        T.has[r] = present[r] != 0;
    }
    const uint32_t st = kd_tj::task_status<K>(T);
    out.push_back((uint8_t)st);
    if (st != KD_TJ_OK) return;
    std::vector<uint8_t> kept[K];
    uint32_t n[K] = {};
    kd_tj::join<K>(T, c0, c1, [&](int r, const kd_tj::Ent& e) {
        n[r]++;
        put32(kept[r], e.mode);
        put32(kept[r], e.nlen);
        kept[r].insert(kept[r].end(), T.p[r] + e.name, T.p[r] + e.name + e.nlen);
        kept[r].insert(kept[r].end(), T.p[r] + e.oid, T.p[r] + e.oid + 20);
    });
    for (int r = 0; r < K; r++) {
        put32(out, n[r]);
        out.insert(out.end(), kept[r].begin(), kept[r].end());
    }
}

static int join_main(const char* corpus, const char* dst) {
    std::vector<uint8_t> in, out;
    if (!read_all(corpus, in)) return 2;
    size_t at = 0;
    auto get32 = [&](uint32_t* v) {
        if (at + 4 > in.size()) return false;
        memcpy(v, in.data() + at, 4);
        at += 4;
        return true;
    };
    uint32_t nt;
    if (!get32(&nt)) return 2;
    for (uint32_t t = 0; t < nt; t++) {
        uint32_t k, c0, c1, present[3] = {}, len[3] = {};
        uint8_t* blk[3] = {};
        if (!get32(&k) || !get32(&c0) || !get32(&c1) || k < 1 || k > 3) return 2;
        for (uint32_t r = 0; r < k; r++) {
            if (!get32(&present[r]) || !get32(&len[r]) || at + len[r] > in.size()) return 2;
            blk[r] = (uint8_t*)malloc(len[r] ? len[r] : 1);
            if (!blk[r]) return 2;
            if (len[r]) memcpy(blk[r], in.data() + at, len[r]);
            at += len[r];
        }
        if (k == 1) join_task<1>(blk, len, present, (int)c0, (int)c1, out);
        else if (k == 2) join_task<2>(blk, len, present, (int)c0, (int)c1, out);
        else join_task<3>(blk, len, present, (int)c0, (int)c1, out);
        for (uint32_t r = 0; r < k; r++) free(blk[r]);
    }
    FILE* f = fopen(dst, "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "join")) return join_main(argv[2], argv[3]);
    if (argc != 3) return 2;
    std::vector<uint8_t> in, out;
    if (!read_all(argv[1], in) || in.size() < 4) return 2;
    size_t at = 0;
    auto get32 = [&](uint32_t* v) {
        if (at + 4 > in.size()) return false;
        memcpy(v, in.data() + at, 4);
        at += 4;
        return true;
    };
    uint32_t n;
    if (!get32(&n)) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len;
        if (!get32(&len) || at + len > in.size()) return 2;
        uint8_t* p = (uint8_t*)malloc(len ? len : 1);
        if (!p) return 2;
        if (len) memcpy(p, in.data() + at, len);
        at += len;
        const uint8_t* tree = len ? p : p + 1;  // (an empty tree: one past a block nobody may read)
        uint64_t cnt = 0;
        const uint32_t st = kd_tj::tree_status(tree, len, &cnt);
        out.push_back((uint8_t)st);
        put32(out, st ? 0 : (uint32_t)cnt);
        if (st == KD_TJ_OK) {
            // the entries again, one by one, as the kernels walk them
            kd_tj::Cur c;
            kd_tj::Ent e;
            uint64_t seen = 0;
            for (;;) {
                bool more;
                if (kd_tj::next_entry(tree, len, &c, &e, &more) != KD_TJ_OK) return 3;
                if (!more) break;
                if (e.oid + 20 > len || e.name + e.nlen + 1 != e.oid) return 3;
                put32(out, e.mode);
                put32(out, (uint32_t)e.name);
                put32(out, e.nlen);
                put32(out, (uint32_t)e.oid);
                seen++;
            }
            if (seen != cnt) return 3;
        }
        free(p);
    }
    uint8_t* one = (uint8_t*)malloc(1);
    uint64_t cnt = 0;
    out.push_back((uint8_t)kd_tj::tree_status(one, (uint64_t)KD_TJ_MAX_BYTES + 1, &cnt));
    free(one);
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
