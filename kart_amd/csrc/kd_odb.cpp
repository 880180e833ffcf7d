// kd_odb.cpp — the git object database read natively (loose objects, pack v2 with idx v1/v2,
// zlib, OFS/REF delta chains) and Dataset3's leaf walk over it, with tree-OID pruning.
//
// Replaces what Kart gets from libgit2 (koordinates fork @ bb69c8fa, vendor/libgit2/Makefile:1-3)
// on the diff path: the feature-tree iteration of Dataset3 (kart/dataset3.py:26-35,225-231), the
// blob reads of BaseDataset.get_blob_at (kart/base_dataset.py:230-265), and the subtree pruning
// of tree-to-tree diff (pygit2 Tree.diff_to_tree, called at kart/rich_base_dataset.py:212-232):
// a subtree whose OID is the same in both trees is never opened.
//
// Host code (no GPU).  The walk feeds the packer (kd_pack_*_keys, kd_sort_side): its output is
// the flat (path arena, offsets, OIDs) layout those take.  Formats follow git's documented ones
// (Documentation/technical/pack-format.txt): idx v2 = magic, fanout[256], sha[n], crc[n],
// off32[n] (MSB -> index into off64[]); pack entries = type/size varint header, zlib stream;
// OFS_DELTA base = this offset - (offset varint); delta = src/dst size varints + copy/insert ops.
#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "kartdiff.h"
#include "kd_delta.h"

namespace kd {
void set_error(const char* fmt, ...);
}

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

enum { OBJ_COMMIT = 1, OBJ_TREE = 2, OBJ_BLOB = 3, OBJ_TAG = 4, OBJ_OFS_DELTA = 6, OBJ_REF_DELTA = 7 };
enum { RD_OK = 0, RD_MISSING = 1, RD_CORRUPT = 2 };

constexpr int MAX_CHAIN = 10000;       // delta chain guard (git's default depth is 50)
constexpr u64 CACHE_MAX_OBJ = 1 << 16; // resolved objects at most this big enter the base cache
constexpr int CACHE_SLOTS = 1024;      // per reader, direct-mapped by pack offset

inline u32 be32(const u8* p) { return (u32)p[0] << 24 | (u32)p[1] << 16 | (u32)p[2] << 8 | p[3]; }
inline u64 be64(const u8* p) { return (u64)be32(p) << 32 | be32(p + 4); }

struct MappedFile {
    const u8* p = nullptr;
    size_t n = 0;
    bool open(const std::string& path) {
        int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) { ::close(fd); return false; }
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return false;
        p = (const u8*)m;
        n = (size_t)st.st_size;
        return true;
    }
    ~MappedFile() {
        if (p) munmap((void*)p, n);
    }
};

struct Pack {
    MappedFile idx, pack;
    int ver = 0;  // idx version 1 or 2
    u32 n = 0;
    const u8 *fan = nullptr, *sha = nullptr, *off32 = nullptr, *off64 = nullptr;
    size_t n64 = 0;

    bool open(const std::string& idx_path, const std::string& pack_path) {
        if (!idx.open(idx_path) || !pack.open(pack_path)) return false;
        if (pack.n < 32 || memcmp(pack.p, "PACK", 4) != 0) return false;
        const u32 pv = be32(pack.p + 4);
        if (pv != 2 && pv != 3) return false;
        const u8* p = idx.p;
        if (idx.n >= 8 && memcmp(p, "\377tOc", 4) == 0) {
            if (be32(p + 4) != 2) return false;
            ver = 2;
            fan = p + 8;
            if (idx.n < 8 + 1024) return false;
            n = be32(fan + 4 * 255);
            const size_t need = 8 + 1024 + (size_t)n * 28 + 40;
            if (idx.n < need) return false;
            sha = fan + 1024;
            off32 = sha + (size_t)n * 24;  // after sha[n] and crc[n]
            off64 = off32 + (size_t)n * 4;
            n64 = (idx.n - need) / 8;
        } else {
            ver = 1;
            fan = p;
            if (idx.n < 1024) return false;
            n = be32(fan + 4 * 255);
            if (idx.n < 1024 + (size_t)n * 24 + 40) return false;
        }
        return true;
    }

    // offset of `oid` in the pack, or false
    bool find(const u8* oid, u64* off) const {
        u32 lo = oid[0] ? be32(fan + 4 * (oid[0] - 1)) : 0, hi = be32(fan + 4 * oid[0]);
        if (hi > n || lo > hi) return false;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2;
            const u8* s = ver == 2 ? sha + 20 * (size_t)mid : fan + 1024 + 24 * (size_t)mid + 4;
            const int c = memcmp(s, oid, 20);
            if (c == 0) {
                if (ver == 1) { *off = be32(fan + 1024 + 24 * (size_t)mid); return true; }
                const u32 o = be32(off32 + 4 * (size_t)mid);
                if (!(o & 0x80000000u)) { *off = o; return true; }
                const size_t j = o & 0x7FFFFFFFu;
                if (j >= n64) return false;
                *off = be64(off64 + 8 * j);
                return true;
            }
            if (c < 0) lo = mid + 1;
            else hi = mid;
        }
        return false;
    }
};

}  // namespace

namespace {
struct Reader;
}

struct kd_odb {
    std::vector<std::string> objdirs;  // objects/ and its alternates
    std::vector<std::unique_ptr<Pack>> packs;
    // idle readers (zlib stream + base cache) reused by single-object reads: building one costs
    // more than reading a small object (ctypes drops the GIL, so calls may be concurrent)
    std::mutex pool_mu;
    std::vector<Reader*> pool;
    // options (kd_odb_set_option; kd_odb_open seeds them from the environment)
    int zlib_only = 0;  // "zlib" [KD_ODB_ZLIB]: 1 = inflate with zlib even when libdeflate is present (A/B)
    // "walk_batch_bytes" [KD_WALK_BATCH_BYTES]: kd_walk_device reads its leaf trees in batches of about this
    // many compressed and host-read bytes (what bounds the pinned staging and the device arena of a walk)
    u64 walk_batch_bytes = 64ull << 20;
    // kd_odb_read_batch_device: the pinned staging its sources are gathered into (grow-only), one call at a time
    std::mutex dev_mu;
    u8* pin = nullptr;
    u64 pin_cap = 0;
    // the last kd_odb_read_batch_device_ex call's host phases in microseconds (kd_odb_get_option "rbd_*_us")
    int64_t rbd_us[4] = {0, 0, 0, 0};  // plan (all of it), peek (the header peeks in it), host reads + gather, device
};

namespace {

void add_objdir(kd_odb* db, const std::string& dir, int depth) {
    for (auto& d : db->objdirs)
        if (d == dir) return;
    db->objdirs.push_back(dir);
    if (DIR* dp = opendir((dir + "/pack").c_str())) {
        std::vector<std::string> names;
        while (struct dirent* e = readdir(dp)) {
            std::string nm = e->d_name;
            if (nm.size() > 4 && nm.compare(nm.size() - 4, 4, ".idx") == 0) names.push_back(nm);
        }
        closedir(dp);
        std::sort(names.begin(), names.end());
        for (auto& nm : names) {
            auto pk = std::make_unique<Pack>();
            const std::string base = dir + "/pack/" + nm.substr(0, nm.size() - 4);
            if (pk->open(base + ".idx", base + ".pack")) db->packs.push_back(std::move(pk));
        }
    }
    if (depth >= 5) return;
    FILE* f = fopen((dir + "/info/alternates").c_str(), "r");
    if (!f) return;
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        std::string s = line;
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
        if (s.empty() || s[0] == '#') continue;
        add_objdir(db, s[0] == '/' ? s : dir + "/" + s, depth + 1);
    }
    fclose(f);
}

int read_varint_le(const u8* d, size_t n, size_t* i, u64* out) {
    u64 v = 0;
    int shift = 0;
    for (;;) {
        if (*i >= n || shift > 63) return -1;
        const u8 c = d[(*i)++];
        v |= (u64)(c & 0x7F) << shift;
        shift += 7;
        if (!(c & 0x80)) break;
    }
    *out = v;
    return 0;
}

// git's delta: src size, dst size, then ops (copy from base: 0x80 | offset/size byte masks;
// insert: 1..127 literal bytes)
int apply_delta(const u8* base, size_t blen, const u8* d, size_t dlen, std::vector<u8>& out) {
    size_t i = 0;
    u64 src, dst;
    if (read_varint_le(d, dlen, &i, &src) || read_varint_le(d, dlen, &i, &dst)) return -1;
    if (src != blen) return -1;
    out.resize(dst);
    u8* o = out.data();
    u64 w = 0;
    while (i < dlen) {
        const u8 op = d[i++];
        if (op & 0x80) {
            u64 off = 0, sz = 0;
            for (int b = 0; b < 4; b++)
                if (op & (1 << b)) {
                    if (i >= dlen) return -1;
                    off |= (u64)d[i++] << (8 * b);
                }
            for (int b = 0; b < 3; b++)
                if (op & (0x10 << b)) {
                    if (i >= dlen) return -1;
                    sz |= (u64)d[i++] << (8 * b);
                }
            if (sz == 0) sz = 0x10000;
            if (off + sz > blen || w + sz > dst) return -1;
            memcpy(o + w, base + off, sz);
            w += sz;
        } else if (op) {
            if (i + op > dlen || w + op > dst) return -1;
            memcpy(o + w, d + i, op);
            i += op;
            w += op;
        } else {
            return -1;
        }
    }
    return w == dst ? 0 : -1;
}

// libdeflate (the image's libdeflate.so.0, when present) inflates a whole zlib stream of known
// size in one call, without zlib's per-stream state machine: a pack read is mostly tiny delta
// streams, so this is most of its CPU time.  Its documented C API, declared here (no header in the
// image); zlib when the library is absent.
struct Deflate {
    typedef void* (*alloc_fn)();
    typedef void (*free_fn)(void*);
    typedef int (*zlib_ex_fn)(void*, const void*, size_t, void*, size_t, size_t*, size_t*);
    alloc_fn alloc = nullptr;
    free_fn release = nullptr;
    zlib_ex_fn zlib_ex = nullptr;
    Deflate() {
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = (alloc_fn)dlsym(h, "libdeflate_alloc_decompressor");
        release = (free_fn)dlsym(h, "libdeflate_free_decompressor");
        zlib_ex = (zlib_ex_fn)dlsym(h, "libdeflate_zlib_decompress_ex");
        if (!alloc || !release || !zlib_ex) alloc = nullptr;
    }
    bool ok() const { return alloc != nullptr; }
};
const Deflate& deflate_lib() {
    static const Deflate d;
    return d;
}

// One thread's reader: a zlib stream, a delta-base cache, scratch buffers.
struct Reader {
    const kd_odb* db;
    z_stream z;
    bool zok = false;
    struct Slot {
        const Pack* pk = nullptr;
        u64 off = ~0ull;
        int type = 0;
        std::vector<u8> data;
    };
    std::vector<Slot> cache;
    std::vector<u8> dbuf, tmp;

    void* dec = nullptr;  // libdeflate decompressor

    explicit Reader(const kd_odb* d) : db(d), cache(CACHE_SLOTS) {
        memset(&z, 0, sizeof z);
        zok = inflateInit(&z) == Z_OK;
        if (!d->zlib_only && deflate_lib().ok()) dec = deflate_lib().alloc();
    }
    ~Reader() {
        if (zok) inflateEnd(&z);
        if (dec) deflate_lib().release(dec);
    }
    Reader(const Reader&) = delete;

    // inflate one zlib stream starting at src into exactly `size` bytes
    int inflate_exact(const u8* src, size_t avail, u8* dst, size_t size) {
        if (dec) {
            u8 dummy;
            size_t in_used = 0, out_used = 0;
            const int r = deflate_lib().zlib_ex(dec, src, avail, size ? dst : &dummy, size, &in_used, &out_used);
            return r == 0 && out_used == size ? RD_OK : RD_CORRUPT;  // 0: LIBDEFLATE_SUCCESS
        }
        if (!zok || inflateReset(&z) != Z_OK) return RD_CORRUPT;
        z.next_in = (Bytef*)src;
        z.avail_in = (uInt)std::min<size_t>(avail, 0xFFFFFFFFu);
        u8 dummy;
        z.next_out = size ? dst : &dummy;
        z.avail_out = (uInt)size;
        const int r = inflate(&z, Z_FINISH);
        if (r != Z_STREAM_END || z.total_out != size) return RD_CORRUPT;
        return RD_OK;
    }

    Slot& slot(const Pack* pk, u64 off) { return cache[(off * 0x9E3779B97F4A7C15ull) >> 54 & (CACHE_SLOTS - 1)]; }

    // entry header at `off`: type, inflated size, start of the zlib data (after the delta base)
    int entry_header(const Pack& pk, u64 off, int* type, u64* size, u64* data, u64* base_off, const u8** base_oid) {
        const u8* p = pk.pack.p;
        const u64 n = pk.pack.n - 20;  // trailing checksum
        if (off < 12 || off >= n) return RD_CORRUPT;
        u64 i = off;
        u8 c = p[i++];
        *type = (c >> 4) & 7;
        u64 sz = c & 15;
        int shift = 4;
        while (c & 0x80) {
            if (i >= n || shift > 60) return RD_CORRUPT;
            c = p[i++];
            sz |= (u64)(c & 0x7F) << shift;
            shift += 7;
        }
        *size = sz;
        if (*type == OBJ_OFS_DELTA) {
            if (i >= n) return RD_CORRUPT;
            c = p[i++];
            u64 rel = c & 0x7F;
            while (c & 0x80) {
                if (i >= n || rel >= (1ull << 56)) return RD_CORRUPT;
                c = p[i++];
                rel = ((rel + 1) << 7) | (c & 0x7F);
            }
            if (rel == 0 || rel > off) return RD_CORRUPT;
            *base_off = off - rel;
        } else if (*type == OBJ_REF_DELTA) {
            if (i + 20 > n) return RD_CORRUPT;
            *base_oid = p + i;
            i += 20;
        } else if (*type < OBJ_COMMIT || *type > OBJ_TAG) {
            return RD_CORRUPT;
        }
        *data = i;
        return RD_OK;
    }

    // object at `off` of `pk` (delta chains resolved) into out
    int read_packed(const Pack& pk, u64 off, int* type, std::vector<u8>& out, int depth = 0) {
        struct Link { u64 off, data, size; };
        std::vector<Link> chain;
        u64 cur = off;
        int btype = 0;
        for (;;) {
            Slot& s = slot(&pk, cur);
            if (s.pk == &pk && s.off == cur) {  // resolved before
                out = s.data;
                btype = s.type;
                break;
            }
            int t;
            u64 sz, data, boff = 0;
            const u8* boid = nullptr;
            int rc = entry_header(pk, cur, &t, &sz, &data, &boff, &boid);
            if (rc) return rc;
            if (t == OBJ_OFS_DELTA || t == OBJ_REF_DELTA) {
                if ((int)chain.size() >= MAX_CHAIN) return RD_CORRUPT;
                chain.push_back({cur, data, sz});
                if (t == OBJ_OFS_DELTA) {
                    cur = boff;
                    continue;
                }
                u64 o;
                if (pk.find(boid, &o)) {
                    cur = o;
                    continue;
                }
                if (depth > 8) return RD_CORRUPT;
                rc = read(boid, &btype, out, depth + 1);  // base in another pack / loose (thin pack fixed up)
                if (rc) return rc == RD_MISSING ? RD_CORRUPT : rc;
                break;
            }
            out.resize(sz);
            rc = inflate_exact(pk.pack.p + data, pk.pack.n - data, out.data(), sz);
            if (rc) return rc;
            btype = t;
            // a chain's base, and every whole tree: a compare walk reads the old side's tree just
            // before the new side's, which git stores as a delta against it
            if (!chain.empty() || t == OBJ_TREE) remember(&pk, cur, t, out);
            break;
        }
        for (size_t j = chain.size(); j-- > 0;) {
            const Link& L = chain[j];
            dbuf.resize(L.size);
            int rc = inflate_exact(pk.pack.p + L.data, pk.pack.n - L.data, dbuf.data(), L.size);
            if (rc) return rc;
            if (apply_delta(out.data(), out.size(), dbuf.data(), dbuf.size(), tmp)) return RD_CORRUPT;
            out.swap(tmp);
            // every resolved link, the object itself included: in a batch read in pack order the
            // next object is usually a delta against this one (fast-import and repack chains)
            remember(&pk, L.off, btype, out);
        }
        *type = btype;
        return RD_OK;
    }

    void remember(const Pack* pk, u64 off, int type, const std::vector<u8>& data) {
        if (data.size() > CACHE_MAX_OBJ) return;
        Slot& s = slot(pk, off);
        s.pk = pk;
        s.off = off;
        s.type = type;
        s.data = data;
    }

    // one loose object file: zlib("<type> <size>\0" + content)
    int parse_loose(const std::vector<u8>& raw, int* type, std::vector<u8>& out) {
        if (!zok || inflateReset(&z) != Z_OK) return RD_CORRUPT;
        u8 hdr[64];
        z.next_in = const_cast<u8*>(raw.data());
        z.avail_in = (uInt)raw.size();
        z.next_out = hdr;
        z.avail_out = sizeof hdr;
        int zr = inflate(&z, Z_NO_FLUSH);
        if (zr != Z_OK && zr != Z_STREAM_END) return RD_CORRUPT;
        const size_t got = sizeof hdr - z.avail_out;
        const u8* nul = (const u8*)memchr(hdr, 0, got);
        if (!nul) return RD_CORRUPT;
        const u8* sp = (const u8*)memchr(hdr, ' ', nul - hdr);
        if (!sp) return RD_CORRUPT;
        const size_t tl = sp - hdr;
        int t = tl == 4 && !memcmp(hdr, "blob", 4) ? OBJ_BLOB
                : tl == 4 && !memcmp(hdr, "tree", 4) ? OBJ_TREE
                : tl == 6 && !memcmp(hdr, "commit", 6) ? OBJ_COMMIT
                : tl == 3 && !memcmp(hdr, "tag", 3) ? OBJ_TAG : 0;
        if (!t) return RD_CORRUPT;
        u64 size = 0;
        for (const u8* q = sp + 1; q < nul; q++) {
            if (*q < '0' || *q > '9' || size > (1ull << 50)) return RD_CORRUPT;
            size = size * 10 + (*q - '0');
        }
        const size_t have = got - (nul + 1 - hdr);
        if (have > size) return RD_CORRUPT;
        out.resize(size);
        memcpy(out.data(), nul + 1, have);
        if (zr != Z_STREAM_END) {
            z.next_out = out.data() + have;
            z.avail_out = (uInt)(size - have);
            zr = inflate(&z, Z_FINISH);
            if (zr != Z_STREAM_END) return RD_CORRUPT;
        }
        if (z.total_out != size + (nul + 1 - hdr)) return RD_CORRUPT;
        *type = t;
        return RD_OK;
    }

    // the object's loose file in the first object directory (own, then alternates) that holds a
    // readable copy: a corrupt copy in one directory does not hide a good one in the next
    int read_loose(const u8* oid, int* type, std::vector<u8>& out) {
        static const char hx[] = "0123456789abcdef";
        char name[42];
        for (int i = 0; i < 20; i++) {
            name[2 * i] = hx[oid[i] >> 4];
            name[2 * i + 1] = hx[oid[i] & 15];
        }
        int result = RD_MISSING;
        for (const std::string& dir : db->objdirs) {
            std::string path = dir + "/" + std::string(name, 2) + "/" + std::string(name + 2, 38);
            int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
            if (fd < 0) continue;
            std::vector<u8> raw;
            u8 buf[65536];
            ssize_t r;
            while ((r = ::read(fd, buf, sizeof buf)) > 0) raw.insert(raw.end(), buf, buf + r);
            ::close(fd);
            const int rc = r < 0 ? RD_CORRUPT : parse_loose(raw, type, out);
            if (rc == RD_OK) return RD_OK;
            result = rc;
        }
        return result;
    }

    // the pack holding oid, or -1.  The packs that held the last few objects are searched first,
    // most recent first: a batch's objects tend to share packs, a compare walk alternates between
    // its roots' packs (one per side and subtree in a repository written by parallel imports), and
    // every miss is a binary search of another index
    static constexpr int MRU = 4;
    size_t mru[MRU] = {~size_t(0), ~size_t(0), ~size_t(0), ~size_t(0)};
    long locate(const u8* oid, u64* off) {
        const size_t np = db->packs.size();
        for (int j = 0; j < MRU; j++) {
            const size_t p = mru[j];
            if (p >= np) break;
            if (db->packs[p]->find(oid, off)) {
                for (int q = j; q > 0; q--) mru[q] = mru[q - 1];
                mru[0] = p;
                return (long)p;
            }
        }
        for (size_t p = 0; p < np; p++) {
            bool tried = false;
            for (int j = 0; j < MRU; j++) tried |= mru[j] == p;
            if (tried || !db->packs[p]->find(oid, off)) continue;
            for (int q = MRU - 1; q > 0; q--) mru[q] = mru[q - 1];
            mru[0] = p;
            return (long)p;
        }
        return -1;
    }

    int read(const u8* oid, int* type, std::vector<u8>& out, int depth = 0) {
        u64 off;
        const long p = locate(oid, &off);
        if (p >= 0) return read_packed(*db->packs[p], off, type, out, depth);
        return read_loose(oid, type, out);
    }
};

void hex40(const u8* oid, char* out) {
    static const char hx[] = "0123456789abcdef";
    for (int i = 0; i < 20; i++) {
        out[2 * i] = hx[oid[i] >> 4];
        out[2 * i + 1] = hx[oid[i] & 15];
    }
    out[40] = 0;
}

bool unhex40(const u8* s, u8* oid) {
    for (int i = 0; i < 20; i++) {
        int v = 0;
        for (int j = 0; j < 2; j++) {
            const u8 c = s[2 * i + j];
            const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
            if (d < 0) return false;
            v = v * 16 + d;
        }
        oid[i] = (u8)v;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// trees
// ---------------------------------------------------------------------------------------------
struct TEnt {
    const u8* name;
    u32 nlen;
    u32 mode;
    const u8* oid;
    bool tree() const { return mode == 040000; }
};

bool parse_tree(const std::vector<u8>& t, std::vector<TEnt>& out) {
    out.clear();
    const u8 *p = t.data(), *end = p + t.size();
    while (p < end) {
        u32 mode = 0;
        while (p < end && *p != ' ') {
            if (*p < '0' || *p > '7') return false;
            mode = mode * 8 + (*p++ - '0');
        }
        if (p >= end) return false;
        const u8* name = ++p;
        const u8* nul = (const u8*)memchr(p, 0, end - p);
        if (!nul || nul == name || nul + 21 > end) return false;
        out.push_back({name, (u32)(nul - name), mode, nul + 1});
        p = nul + 21;
    }
    return true;
}

// git's tree order: names compared bytewise, a tree's name continuing with '/'
int git_cmp(const TEnt& a, const TEnt& b) {
    const u32 n = std::min(a.nlen, b.nlen);
    const int c = memcmp(a.name, b.name, n);
    if (c) return c;
    const int ca = n < a.nlen ? a.name[n] : (a.tree() ? '/' : 0);
    const int cb = n < b.nlen ? b.name[n] : (b.tree() ? '/' : 0);
    return ca - cb;
}

constexpr int KMAX = 3;

struct WalkOut {
    std::string path;
    std::vector<u64> end;  // end offset of each path in `path`
    std::vector<u8> oid;
    std::vector<u32> mode;
    void add(const std::string& p, const u8* o, u32 m) {
        path += p;
        end.push_back(path.size());
        oid.insert(oid.end(), o, o + 20);
        mode.push_back(m);
    }
};

// a walk item: one path with its entry in each root (a leaf group or a subtree group)
struct Item {
    std::string path;  // relative to the walked tree
    bool tree = false;
    u8 has[KMAX] = {0, 0, 0};
    u8 oid[KMAX][20];
    u32 mode[KMAX] = {0, 0, 0};
};

struct Walk {
    int k, c0, c1;
    std::atomic<int> err{0};
    std::mutex emu;
    std::string emsg;
    void fail(int code, const std::string& m) {
        int z = 0;
        if (err.compare_exchange_strong(z, code)) {
            std::lock_guard<std::mutex> g(emu);
            emsg = m;
        }
    }

    // pruned?  (entries identical in the two compared roots; absent in both counts as identical)
    bool pruned(const Item& it) const {
        if (c0 < 0) return false;
        if (it.has[c0] != it.has[c1]) return false;
        if (!it.has[c0]) return true;
        return it.mode[c0] == it.mode[c1] && !memcmp(it.oid[c0], it.oid[c1], 20);
    }
    bool pruned(const TEnt* const* e) const {
        if (c0 < 0) return false;
        const TEnt *x = e[c0], *y = e[c1];
        if (!x || !y) return x == y;
        return x->mode == y->mode && !memcmp(x->oid, y->oid, 20);
    }

    // one level's trees of every root, parsed (a frame of the depth-first walk)
    struct Frame {
        std::vector<u8> buf[KMAX];
        std::vector<TEnt> ents[KMAX];
    };

    bool load(Reader& rd, const Item& it, Frame& f) {
        for (int r = 0; r < k && r < KMAX; r++) {
            f.ents[r].clear();
            if (!it.has[r]) continue;
            int type = 0;
            const int rc = rd.read(it.oid[r], &type, f.buf[r]);
            if (rc || type != OBJ_TREE || !parse_tree(f.buf[r], f.ents[r])) {
                char hx[41];
                hex40(it.oid[r], hx);
                if (rc) fail(rc == RD_MISSING ? KD_ENOTFOUND : KD_EINVAL,
                             std::string(rc == RD_MISSING ? "tree missing: " : "corrupt object: ") + hx);
                else fail(KD_EINVAL, std::string("not a valid tree: ") + hx);
                return false;
            }
        }
        return true;
    }

    // merge-join a frame's entries in git order: fn(e[KMAX]) per name (nullptr = absent in that
    // root), entries identical in the compared roots skipped
    template <class F>
    void join(Frame& f, F&& fn) {
        size_t pos[KMAX] = {0, 0, 0};
        for (;;) {
            int lo = -1;
            for (int r = 0; r < k && r < KMAX; r++)
                if (pos[r] < f.ents[r].size() && (lo < 0 || git_cmp(f.ents[r][pos[r]], f.ents[lo][pos[lo]]) < 0)) lo = r;
            if (lo < 0) break;
            const TEnt& e0 = f.ents[lo][pos[lo]];
            const TEnt* e[KMAX] = {nullptr, nullptr, nullptr};
            for (int r = 0; r < k && r < KMAX; r++)
                if (r == lo || (pos[r] < f.ents[r].size() && git_cmp(f.ents[r][pos[r]], e0) == 0)) e[r] = &f.ents[r][pos[r]];
            for (int r = 0; r < k && r < KMAX; r++)
                if (e[r]) pos[r]++;
            if (!pruned(e)) fn(e);
        }
    }

    Item child(const std::string& parent, const TEnt* const* e) const {
        Item c;
        const TEnt* e0 = nullptr;
        for (int r = 0; r < k && r < KMAX; r++)
            if (e[r]) {
                e0 = e0 ? e0 : e[r];
                c.has[r] = 1;
                c.mode[r] = e[r]->mode;
                memcpy(c.oid[r], e[r]->oid, 20);
            }
        c.tree = e0->tree();
        c.path = parent;
        if (!c.path.empty()) c.path += '/';
        c.path.append((const char*)e0->name, e0->nlen);
        return c;
    }

    // the children of a subtree item (breadth-first expansion of the top levels)
    template <class F>
    bool expand(Reader& rd, const Item& it, F&& fn) {
        Frame f;
        if (!load(rd, it, f)) return false;
        join(f, [&](const TEnt* const* e) { fn(child(it.path, e)); });
        return true;
    }

    // every leaf under a subtree item, depth first in git order; `path` = the item's path, grown
    // and shrunk in place, frames reused per depth (no allocation per entry)
    void descend(Reader& rd, const Item& it, std::string& path, std::vector<std::unique_ptr<Frame>>& frames,
                 WalkOut* out, int depth) {
        if (err.load(std::memory_order_relaxed)) return;
        if (depth > 64) {
            fail(KD_EINVAL, "tree nesting deeper than 64 at '" + path + "'");
            return;
        }
        if ((int)frames.size() <= depth) frames.push_back(std::make_unique<Frame>());
        Frame& f = *frames[depth];
        if (!load(rd, it, f)) return;
        const size_t plen = path.size();
        join(f, [&](const TEnt* const* e) {
            const TEnt* e0 = nullptr;
            for (int r = 0; r < k && r < KMAX && !e0; r++) e0 = e[r];
            if (e0->tree()) {
                Item c;
                for (int r = 0; r < k && r < KMAX; r++)
                    if (e[r]) {
                        c.has[r] = 1;
                        c.mode[r] = e[r]->mode;
                        memcpy(c.oid[r], e[r]->oid, 20);
                    }
                c.tree = true;
                if (plen) path += '/';
                path.append((const char*)e0->name, e0->nlen);
                descend(rd, c, path, frames, out, depth + 1);
                path.resize(plen);
                return;
            }
            for (int r = 0; r < k && r < KMAX; r++) {
                if (!e[r]) continue;
                WalkOut& o = out[r];
                o.path += path;
                if (plen) o.path += '/';
                o.path.append((const char*)e0->name, e0->nlen);
                o.end.push_back(o.path.size());
                o.oid.insert(o.oid.end(), e[r]->oid, e[r]->oid + 20);
                o.mode.push_back(e[r]->mode);
            }
        });
    }

    void walk_item(Reader& rd, const Item& it, WalkOut* out) {
        std::vector<std::unique_ptr<Frame>> frames;
        std::string path = it.path;
        descend(rd, it, path, frames, out, 0);
    }

    void emit(const Item& c, WalkOut* out) {
        for (int r = 0; r < k && r < KMAX; r++)
            if (c.has[r]) out[r].add(c.path, c.oid[r], c.mode[r]);
    }
};

template <class F>
void par_items(size_t n, int threads, F&& fn) {
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)threads, n));
    std::atomic<size_t> next{0};
    auto work = [&](int tid) {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            fn(i, tid);
        }
    };
    if (nt == 1) { work(0); return; }
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
}

int default_threads(int threads) {
    if (threads > 0) return std::min(threads, 256);
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hc ? hc : 1u, 16u));
}

// commit -> its tree; tree -> itself (the walk's roots may be either)
int peel_to_tree(Reader& rd, const u8* oid, u8* tree, std::string& msg) {
    std::vector<u8> buf;
    u8 cur[20];
    memcpy(cur, oid, 20);
    for (int hop = 0; hop < 8; hop++) {
        int type = 0;
        const int rc = rd.read(cur, &type, buf);
        char hx[41];
        hex40(cur, hx);
        if (rc) {
            msg = std::string(rc == RD_MISSING ? "object missing: " : "corrupt object: ") + hx;
            return rc == RD_MISSING ? KD_ENOTFOUND : KD_EINVAL;
        }
        if (type == OBJ_TREE) { memcpy(tree, cur, 20); return KD_OK; }
        const char* tag = type == OBJ_COMMIT ? "tree " : type == OBJ_TAG ? "object " : nullptr;
        const size_t tl = tag ? strlen(tag) : 0;
        if (!tag || buf.size() < tl + 40 || memcmp(buf.data(), tag, tl) != 0 || !unhex40(buf.data() + tl, cur)) {
            msg = std::string("not a tree-ish: ") + hx;
            return KD_EINVAL;
        }
    }
    msg = "tag chain too long";
    return KD_EINVAL;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int kd_odb_open(const char* gitdir, kd_odb** out) {
    if (!gitdir || !out) { kd::set_error("kd_odb_open: NULL"); return KD_EINVAL; }
    *out = nullptr;
    std::string dir = gitdir;
    while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
    struct stat st;
    if (stat((dir + "/objects").c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) {
        kd::set_error("kd_odb_open: %s has no objects/ directory", gitdir);
        return KD_EINVAL;
    }
    kd_odb* db = new kd_odb();
    if (const char* v = std::getenv("KD_ODB_ZLIB")) db->zlib_only = (int)strtol(v, nullptr, 10) != 0;
    if (const char* v = std::getenv("KD_WALK_BATCH_BYTES")) {
        const long long b = strtoll(v, nullptr, 10);
        if (b > 0) db->walk_batch_bytes = (u64)b;
    }
    add_objdir(db, dir + "/objects", 0);
    *out = db;
    return KD_OK;
}

extern "C" int kd_odb_set_option(kd_odb* odb, const char* name, int64_t value) {
    if (!odb || !name) { kd::set_error("kd_odb_set_option: NULL"); return KD_EINVAL; }
    if (strcmp(name, "walk_batch_bytes") == 0) {
        if (value <= 0) { kd::set_error("kd_odb_set_option: walk_batch_bytes must be positive"); return KD_EINVAL; }
        std::lock_guard<std::mutex> lk(odb->dev_mu);
        odb->walk_batch_bytes = (u64)value;
        return KD_OK;
    }
    if (strcmp(name, "zlib") != 0) { kd::set_error("kd_odb_set_option: unknown option '%s'", name); return KD_EINVAL; }
    std::lock_guard<std::mutex> lk(odb->pool_mu);
    odb->zlib_only = value != 0;
    for (Reader* r : odb->pool) delete r;  // pooled readers were built for the old setting
    odb->pool.clear();
    return KD_OK;
}

extern "C" int kd_odb_get_option(kd_odb* odb, const char* name, int64_t* value) {
    if (!odb || !name || !value) { kd::set_error("kd_odb_get_option: NULL"); return KD_EINVAL; }
    static const char* const rbd_names[4] = {"rbd_plan_us", "rbd_peek_us", "rbd_host_us", "rbd_device_us"};
    for (int k = 0; k < 4; k++)
        if (strcmp(name, rbd_names[k]) == 0) {
            std::lock_guard<std::mutex> lk(odb->dev_mu);
            *value = odb->rbd_us[k];
            return KD_OK;
        }
    if (strcmp(name, "walk_batch_bytes") == 0) {
        std::lock_guard<std::mutex> lk(odb->dev_mu);
        *value = (int64_t)odb->walk_batch_bytes;
        return KD_OK;
    }
    if (strcmp(name, "zlib") != 0) { kd::set_error("kd_odb_get_option: unknown option '%s'", name); return KD_EINVAL; }
    *value = odb->zlib_only;
    return KD_OK;
}

extern "C" int kd_odb_close(kd_odb* odb) {
    if (odb) {
        for (Reader* r : odb->pool) delete r;
        if (odb->pin) kd_host_free(odb->pin);
    }
    delete odb;
    return KD_OK;
}

namespace {
// a pooled reader for the duration of one call
struct PooledReader {
    kd_odb* db;
    Reader* r;
    explicit PooledReader(kd_odb* d) : db(d), r(nullptr) {
        {
            std::lock_guard<std::mutex> g(db->pool_mu);
            if (!db->pool.empty()) {
                r = db->pool.back();
                db->pool.pop_back();
            }
        }
        if (!r) r = new Reader(db);
    }
    ~PooledReader() {
        std::lock_guard<std::mutex> g(db->pool_mu);
        if (db->pool.size() < 64) db->pool.push_back(r);
        else delete r;
    }
};
}  // namespace

extern "C" int kd_odb_read(kd_odb* odb, const uint8_t* oid, int* type, uint8_t** data, uint64_t* len) {
    if (!odb || !oid || !type || !data || !len) { kd::set_error("kd_odb_read: NULL"); return KD_EINVAL; }
    *data = nullptr;
    *len = 0;
    PooledReader pr(odb);
    std::vector<u8> buf;
    const int rc = pr.r->read(oid, type, buf);
    char hx[41];
    hex40(oid, hx);
    if (rc == RD_MISSING) { kd::set_error("object %s missing", hx); return KD_ENOTFOUND; }
    if (rc) { kd::set_error("object %s corrupt", hx); return KD_EINVAL; }
    u8* p = (u8*)std::malloc(std::max<size_t>(buf.size(), 1));
    if (!p) { kd::set_error("kd_odb_read: out of memory"); return KD_EINVAL; }
    memcpy(p, buf.data(), buf.size());
    *data = p;
    *len = buf.size();
    return KD_OK;
}

extern "C" int kd_odb_read_batch(kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint8_t** data,
                                 uint64_t* off, uint8_t* status) {
    if (!odb || !off || (n && (!oids || !status)) || !data) { kd::set_error("kd_odb_read_batch: NULL"); return KD_EINVAL; }
    *data = nullptr;
    const int nt = default_threads(threads);
    constexpr u64 CH = 256;
    const u64 nch = (n + CH - 1) / CH;
    // the objects are read in pack order (pack, then offset; loose objects last), as git's
    // unordered batch reads do: a delta chain's objects lie together (fast-import deltas each blob
    // against the one before), so the next object's base is usually in the reader's cache and a
    // chain of d deltas costs one inflate per object instead of up to d
    std::vector<std::pair<u64, u64>> ord(n);  // (pack << 48 | offset, or ~0: read by id; input index)
    std::vector<std::unique_ptr<Reader>> rds(nt);
    par_items(nch, nt, [&](size_t c, int tid) {
        if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
        Reader& rd = *rds[tid];
        for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
            u64 o;
            const long p = rd.locate(oids + 20 * i, &o);
            ord[i] = {p >= 0 && p < 0xFFFF && o < (1ull << 48) ? (u64)p << 48 | o : ~0ull, i};
        }
    });
    std::sort(ord.begin(), ord.end());
    // chunks of 256 objects in that order per task, each into its own buffer; stitched in input
    // order after
    std::vector<std::vector<u8>> part(nch);
    std::vector<u64> at(n);  // object i's bytes: part[chunk of its sorted position] at at[i]
    std::vector<u32> chunk_of(n);
    off[0] = 0;
    par_items(nch, nt, [&](size_t c, int tid) {
        if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
        Reader& rd = *rds[tid];
        std::vector<u8> buf;
        for (u64 s = c * CH; s < std::min(n, (c + 1) * CH); s++) {
            const u64 key = ord[s].first, i = ord[s].second;
            int type = 0;
            const int rc = key != ~0ull ? rd.read_packed(*odb->packs[key >> 48], key & ((1ull << 48) - 1), &type, buf)
                                        : rd.read(oids + 20 * i, &type, buf);
            status[i] = rc == RD_OK && type != OBJ_BLOB ? 2 : (u8)rc;
            if (status[i]) buf.clear();
            at[i] = part[c].size();
            chunk_of[i] = (u32)c;
            part[c].insert(part[c].end(), buf.begin(), buf.end());
            off[i + 1] = buf.size();  // lengths first, prefix-summed below
        }
    });
    for (u64 i = 0; i < n; i++) off[i + 1] += off[i];
    u8* p = (u8*)std::malloc(std::max<u64>(n ? off[n] : 0, 1));
    if (!p) { kd::set_error("kd_odb_read_batch: out of memory"); return KD_EINVAL; }
    par_items(nch, nt, [&](size_t c, int) {
        for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++)
            if (off[i + 1] > off[i]) memcpy(p + off[i], part[chunk_of[i]].data() + at[i], off[i + 1] - off[i]);
    });
    *data = p;
    return KD_OK;
}

// ---------------------------------------------------------------------------------------------
// the batched read with the arena in HBM (kd_inflate.hip inflates the plain packed blobs; with
// KD_RBD_DELTAS kd_delta.hip rebuilds delta chains level by level from the plan made here)
// ---------------------------------------------------------------------------------------------
namespace kd {
// kd_inflate.hip: upload the gathered sources, one launch of k_inf_streams, the status bytes back
int inflate_from_host(kd_ctx* ctx, const uint8_t* h_src, const uint64_t* h_src_off, const uint8_t* h_kind, uint64_t n,
                      uint8_t* d_dst, const uint64_t* h_dst_off, uint64_t* d_dst_off, uint8_t* h_status);
}

namespace {
// the most a deflate stream of `size` bytes is taken to occupy (a stored block's 5 bytes per 16 KiB
// and the wrapper, with room); a stream that is longer fails on the device and is read on the host
inline u64 inf_bound(u64 size) { return size + (size >> 12) + (size >> 14) + (size >> 25) + 13; }

struct DevItem {
    u64 key = ~0ull;  // pack << 48 | offset, or ~0: read by id
    u64 data = 0;     // device class: where the stream starts in its pack
    u64 size = 0;     // inflated size (host class: what the read gave)
    u8 dev = 0;       // device class: 1 a plain stream, 2 (KD_RBD_DELTAS) rebuilt from its delta chain
    u32 node = ~0u;   // KD_RBD_DELTAS: the entry's node in the delta forest, if it is one
};

// One entry of the delta forest: a requested delta, or an ancestor of one (KD_RBD_DELTAS).
struct DlNode {
    u64 key = ~0ull;   // pack << 48 | offset
    u64 pkey = ~0ull;  // the base's key (~0: a plain entry, the chain's root)
    u64 data = 0;      // where the stream starts in its pack
    u64 zsize = 0;     // the stream's inflated size (entry header)
    u64 rsize = 0;     // the object's size
    u64 bsize = 0;     // a delta: the base size its payload states
    u32 parent = ~0u;
    u32 level = 0;     // 0 for the plain base
    u8 delta = 0;
    u8 bad = 0;        // cannot be rebuilt on the device (the reason is the host route's to find)
    u8 ok = 0;         // this entry and its whole chain can
    // per pass
    u8 in_ws = 0;      // the result lives in workspace (nobody requested it)
    u64 at = 0;        // where the result is (arena or workspace) and where the payload is (workspace)
    u64 pay = 0;
    u32 st = 0, pst = 0;  // status indices of the result and of the payload
};

using Clock = std::chrono::steady_clock;
inline int64_t us_since(Clock::time_point t0) {
    return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - t0).count();
}

// at most `cap` bytes from the front of the zlib stream at src (the Reader's z_stream: libdeflate
// cannot stop early); *got <- how many came out
bool peek_stream(Reader& rd, const u8* src, size_t avail, u8* out, size_t cap, size_t* got) {
    *got = 0;
    if (!rd.zok || inflateReset(&rd.z) != Z_OK) return false;
    rd.z.next_in = (Bytef*)src;
    rd.z.avail_in = (uInt)std::min<size_t>(avail, 0xFFFFFFFFu);
    rd.z.next_out = out;
    rd.z.avail_out = (uInt)cap;
    const int r = inflate(&rd.z, Z_SYNC_FLUSH);
    if (r != Z_OK && r != Z_STREAM_END && r != Z_BUF_ERROR) return false;
    *got = cap - rd.z.avail_out;
    return true;
}

u32 find_node(const std::vector<DlNode>& nodes, u64 key) {
    auto it = std::lower_bound(nodes.begin(), nodes.end(), key, [](const DlNode& a, u64 k) { return a.key < k; });
    return it != nodes.end() && it->key == key ? (u32)(it - nodes.begin()) : ~0u;
}

// want_type: the object type the ids must name (OBJ_BLOB for the public entry points, OBJ_TREE for kd_walk_device's
// leaf trees); status 2 for anything else
int read_batch_device_impl(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags, kd_blobs* out,
                           uint8_t* status, uint64_t st8[8], int want_type = OBJ_BLOB,
                           int64_t* phase_us = nullptr) {
    const bool deltas = (flags & KD_RBD_DELTAS) != 0;
    const auto t_start = Clock::now();
    out->n = n;
    out->data = nullptr;
    out->off = nullptr;
    out->mem = KD_MEM_DEVICE;
    out->size_hint = 0;
    u64 st4[4] = {0, 0, 0, 0};
    const int nt = default_threads(threads);
    constexpr u64 CH = 256;
    const u64 nch = (n + CH - 1) / CH;
    std::lock_guard<std::mutex> dev_lock(odb->dev_mu);  // (the pinned staging is the store's)
    std::vector<std::unique_ptr<Reader>> rds(nt);
    auto reader = [&](int tid) -> Reader& {
        if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
        return *rds[tid];
    };
    // 1 + 2: every id located, its entry header parsed, its class decided
    std::vector<DevItem> it(n);
    // KD_RBD_DELTAS: the entries of every requested delta's chain, found by the thread that meets them
    // first (a thread stops walking up at an entry it has already listed: chains share their tails)
    std::vector<std::unordered_set<u64>> seen(deltas ? nt : 0);
    std::vector<std::vector<DlNode>> recs(deltas ? nt : 0);
    auto discover = [&](Reader& rd, int tid, long p, u64 o) {
        const Pack& pk = *odb->packs[p];
        u64 cur = o;
        for (int hop = 0; hop < MAX_CHAIN; hop++) {
            DlNode nd;
            nd.key = (u64)p << 48 | cur;
            if (!seen[tid].insert(nd.key).second) return;
            int t;
            u64 sz, data, boff = 0;
            const u8* boid = nullptr;
            if (cur >= (1ull << 48) || rd.entry_header(pk, cur, &t, &sz, &data, &boff, &boid) != RD_OK || data >= pk.pack.n - 20 ||
                sz > KD_INF_MAX) {
                nd.bad = 1;
                recs[tid].push_back(nd);
                return;
            }
            nd.data = data;
            nd.zsize = sz;
            if (t == OBJ_OFS_DELTA) {
                cur = boff;
            } else if (t == OBJ_REF_DELTA) {
                if (!pk.find(boid, &cur)) nd.bad = 1;  // the base is in another pack, loose, or nowhere
            } else {
                nd.rsize = sz;
                nd.bad = t != want_type;
                recs[tid].push_back(nd);
                return;
            }
            nd.delta = 1;
            if (!nd.bad) nd.pkey = (u64)p << 48 | cur;
            recs[tid].push_back(nd);
            if (nd.bad) return;
        }
    };
    par_items(nch, nt, [&](size_t c, int tid) {
        Reader& rd = reader(tid);
        for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
            u64 o;
            const long p = rd.locate(oids + 20 * i, &o);
            if (p < 0 || p >= 0xFFFF || o >= (1ull << 48)) continue;
            it[i].key = (u64)p << 48 | o;
            int type;
            u64 size, data, boff = 0;
            const u8* boid = nullptr;
            const Pack& pk = *odb->packs[p];
            if (rd.entry_header(pk, o, &type, &size, &data, &boff, &boid) != RD_OK) continue;
            if (type == want_type && size <= KD_INF_MAX && data < pk.pack.n - 20) {
                it[i].dev = 1;
                it[i].data = data;
                it[i].size = size;
            } else if (deltas && (type == OBJ_OFS_DELTA || type == OBJ_REF_DELTA)) {
                it[i].dev = 2;
                discover(rd, tid, p, o);
            }
        }
    });
    // the forest: unique entries in key order, parents linked, sizes peeked, levels and chains decided
    std::vector<DlNode> nodes;
    std::vector<u32> par;  // every entry's parent, apart from the entries (the walk up a chain touches nothing else)
    int64_t peek_us = 0;
    if (deltas) {
        {
            // (the keys are sorted, not the entries: 16 bytes move per comparison instead of a whole DlNode)
            // and every thread's list on its own first, then merged pairwise)
            std::vector<std::pair<u64, const DlNode*>> ks;
            std::vector<size_t> seg{0};
            for (auto& v : recs) {
                for (const DlNode& nd : v) ks.push_back({nd.key, &nd});
                seg.push_back(ks.size());
            }
            auto less = [](const auto& a, const auto& b) { return a.first < b.first; };
            par_items(seg.size() - 1, nt, [&](size_t t, int) { std::sort(ks.begin() + seg[t], ks.begin() + seg[t + 1], less); });
            while (seg.size() > 2) {
                const size_t pairs = (seg.size() - 1) / 2;
                par_items(pairs, nt, [&](size_t q, int) {
                    std::inplace_merge(ks.begin() + seg[2 * q], ks.begin() + seg[2 * q + 1], ks.begin() + seg[2 * q + 2], less);
                });
                std::vector<size_t> next;
                for (size_t q = 0; q < seg.size(); q += 2) next.push_back(seg[q]);
                if (next.back() != seg.back()) next.push_back(seg.back());
                seg.swap(next);
            }
            ks.erase(std::unique(ks.begin(), ks.end(), [](const auto& a, const auto& b) { return a.first == b.first; }), ks.end());
            nodes.resize(ks.size());
            par_items((ks.size() + CH - 1) / CH, nt, [&](size_t c, int) {
                for (u64 k = c * CH; k < std::min<u64>(ks.size(), (c + 1) * CH); k++) nodes[k] = *ks[k].second;
            });
        }
        const u64 nn = nodes.size(), nnch = (nn + CH - 1) / CH;
        // a delta's result size and its base's are the two varints at the front of its inflated payload
        const auto t_peek = Clock::now();
        par_items(nnch, nt, [&](size_t c, int tid) {
            Reader& rd = reader(tid);
            for (u64 k = c * CH; k < std::min(nn, (c + 1) * CH); k++) {
                DlNode& nd = nodes[k];
                if (!nd.delta || nd.bad) continue;
                nd.parent = find_node(nodes, nd.pkey);
                const Pack& pk = *odb->packs[nd.key >> 48];
                u8 hb[20];
                size_t got = 0, pos = 0;
                if (nd.parent == ~0u || !peek_stream(rd, pk.pack.p + nd.data, pk.pack.n - 20 - nd.data, hb, (size_t)std::min<u64>(20, nd.zsize), &got) ||
                    !kd_dl::size_varint(hb, got, &pos, &nd.bsize) || !kd_dl::size_varint(hb, got, &pos, &nd.rsize) || nd.rsize > KD_INF_MAX)
                    nd.bad = 1;
            }
        });
        peek_us = us_since(t_peek);
        std::vector<u8> state(nn, 0);  // 1 on the stack, 2 decided
        std::vector<u32> stack;
        for (u64 s = 0; s < nn; s++) {
            stack.clear();
            for (u32 c = (u32)s; state[c] == 0;) {
                state[c] = 1;
                stack.push_back(c);
                if (nodes[c].parent == ~0u) break;
                c = nodes[c].parent;
            }
            for (size_t k = stack.size(); k-- > 0;) {
                DlNode& nd = nodes[stack[k]];
                if (!nd.delta) {
                    nd.ok = !nd.bad;
                } else if (!nd.bad && state[nd.parent] == 2) {  // (a parent still on the stack: a cycle of REF_DELTAs)
                    const DlNode& pa = nodes[nd.parent];
                    nd.level = pa.level + 1;
                    nd.ok = pa.ok && nd.bsize == pa.rsize && nd.level <= KD_DL_MAX_DEPTH;
                }
                state[stack[k]] = 2;
            }
        }
        par_items(nch, nt, [&](size_t c, int) {
            for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
                if (!it[i].dev) continue;
                it[i].node = find_node(nodes, it[i].key);
                if (it[i].dev == 2) {
                    if (it[i].node != ~0u && nodes[it[i].node].ok) it[i].size = nodes[it[i].node].rsize;
                    else it[i].dev = 0;  // host class: the host route gives it its bytes or its status
                }
            }
        });
        par.resize(nn);
        for (u64 k = 0; k < nn; k++) par[k] = nodes[k].parent;
    }
    const int64_t plan_us = us_since(t_start);
    int64_t host_us = 0, device_us = 0;
    std::vector<u64> soff2, woff, level_start;
    std::vector<kd::DlItem> ditems;
    std::vector<kd::DlCopy> copies;
    std::vector<u32> wsitem;
    std::vector<u8> need;          // per pass: the entry is on a delta-class request's chain
    std::vector<int64_t> home;     // per pass: the first request that names the entry
    std::vector<u8> hst;
    std::vector<u8> forced(n, 0);  // device items the device refused and the host could not read either
    std::vector<u64> off(n + 1), soff(n + 1);
    std::vector<u8> kind(n), dstat(n);
    for (int pass = 0;; pass++) {
        const auto t_pass = Clock::now();
        // host class: read by the Reader, threaded and in pack order (as kd_odb_read_batch reads)
        std::vector<std::pair<u64, u64>> ord;
        for (u64 i = 0; i < n; i++)
            if (!it[i].dev || forced[i]) ord.push_back({it[i].key, i});
        std::sort(ord.begin(), ord.end());
        const u64 nh = ord.size(), nhch = (nh + CH - 1) / CH;
        std::vector<std::vector<u8>> part(nhch);
        std::vector<u64> at(n);
        std::vector<u32> chunk_of(n);
        par_items(nhch, nt, [&](size_t c, int tid) {
            Reader& rd = reader(tid);
            std::vector<u8> buf;
            for (u64 s = c * CH; s < std::min(nh, (c + 1) * CH); s++) {
                const u64 key = ord[s].first, i = ord[s].second;
                int type = 0;
                const int rc = key != ~0ull ? rd.read_packed(*odb->packs[key >> 48], key & ((1ull << 48) - 1), &type, buf)
                                            : rd.read(oids + 20 * i, &type, buf);
                status[i] = rc == RD_OK && type != want_type ? 2 : (u8)rc;
                if (status[i]) buf.clear();
                at[i] = part[c].size();
                chunk_of[i] = (u32)c;
                part[c].insert(part[c].end(), buf.begin(), buf.end());
                it[i].size = buf.size();
            }
        });
        // 3: sizes -> off; the sources' offsets (a device item's span is clipped to the pack's trailer)
        off[0] = soff[0] = 0;
        u64 ndev = 0, comp = 0;
        for (u64 i = 0; i < n; i++) {
            const u8 cls = forced[i] ? 0 : it[i].dev;
            u64 span = it[i].size;
            if (cls == 1) {
                const Pack& pk = *odb->packs[it[i].key >> 48];
                span = std::min(inf_bound(it[i].size), pk.pack.n - 20 - it[i].data);
                ndev++;
                comp += span;
            } else if (cls == 2) {
                span = 0;  // (rebuilt by k_dl_apply: a raw item without a source, which the inflate launch leaves alone)
            }
            kind[i] = cls == 1 ? 0 : cls == 2 ? 2 : 1;
            off[i + 1] = off[i] + it[i].size;
            soff[i + 1] = soff[i] + span;
        }
        // KD_RBD_DELTAS: the levels.  Needed entries: every delta-class request's chain.  An entry's home is
        // the first request that names it; one nobody requested lives in workspace, as every payload does
        u64 m = 0, ws_bytes = 0, ndelta = 0;
        u32 depth = 0;
        if (deltas) {
            const u64 nn = nodes.size();
            need.assign(nn, 0);
            home.assign(nn, -1);
            copies.clear();
            for (u64 i = 0; i < n; i++) {
                if (kind[i] != 2) continue;
                ndelta++;
                for (u32 k = it[i].node; k != ~0u && !need[k]; k = par[k]) need[k] = 1;
            }
            for (u64 i = 0; i < n; i++) {
                if (kind[i] == 1 || it[i].node == ~0u || !need[it[i].node]) continue;
                int64_t& h = home[it[i].node];
                if (h < 0) h = (int64_t)i;
                else if (kind[i] == 2) copies.push_back({0, off[i], it[i].size, 0, (u32)h});  // (src: the home, below)
            }
            // launch 2's items: unrequested chain bases, then every payload; unrequested results behind them.
            // Entries are taken in key order, which is pack order: neighbours in a launch are neighbours in the pack
            wsitem.clear();
            for (u64 k = 0; k < nn; k++)
                if (need[k] && !nodes[k].delta && home[k] < 0) wsitem.push_back((u32)k);
            const u64 nbase = wsitem.size();
            for (u64 k = 0; k < nn; k++)
                if (need[k] && nodes[k].delta) {
                    wsitem.push_back((u32)k);
                    depth = std::max(depth, nodes[k].level);
                }
            m = wsitem.size();
            soff2.assign(m + 1, 0);
            woff.assign(m + 1, 0);
            for (u64 j = 0; j < m; j++) {
                DlNode& nd = nodes[wsitem[j]];
                const Pack& pk = *odb->packs[nd.key >> 48];
                soff2[j + 1] = soff2[j] + std::min(inf_bound(nd.zsize), pk.pack.n - 20 - nd.data);
                woff[j + 1] = woff[j] + nd.zsize;
                if (j < nbase) {
                    nd.in_ws = 1;
                    nd.at = woff[j];
                    nd.st = (u32)(n + j);
                } else {
                    nd.pay = woff[j];
                    nd.pst = (u32)(n + j);
                }
            }
            comp += soff2[m];
            ws_bytes = woff[m];
            // the delta entries in level order
            level_start.assign(depth + 2, 0);
            for (u64 j = nbase; j < m; j++) level_start[nodes[wsitem[j]].level + 1]++;
            for (u32 l = 1; l <= depth + 1; l++) level_start[l] += level_start[l - 1];
            ditems.assign(m - nbase, kd::DlItem{});
            std::vector<u64> fill(level_start.begin(), level_start.end());
            std::vector<u32> order(m - nbase);
            for (u64 j = nbase; j < m; j++) order[fill[nodes[wsitem[j]].level]++] = wsitem[j];
            for (u64 j = 0; j < order.size(); j++) {
                DlNode& nd = nodes[order[j]];
                nd.st = (u32)(n + m + j);
                nd.in_ws = home[order[j]] < 0;
                if (nd.in_ws) {
                    nd.at = ws_bytes;
                    ws_bytes += nd.rsize;
                } else {
                    nd.at = off[home[order[j]]];
                }
            }
            for (u64 k = 0; k < nn; k++)
                if (need[k] && !nodes[k].delta && home[k] >= 0) {
                    nodes[k].in_ws = 0;
                    nodes[k].at = off[home[k]];
                    nodes[k].st = (u32)home[k];
                }
            for (u64 j = 0; j < order.size(); j++) {
                const DlNode& nd = nodes[order[j]];
                const DlNode& pa = nodes[nd.parent];
                kd::DlItem& d = ditems[j];
                d.base_at = pa.at;
                d.delta_at = nd.pay;
                d.dst_at = nd.at;
                d.base_len = (u32)pa.rsize;
                d.delta_len = (u32)nd.zsize;
                d.dst_len = (u32)nd.rsize;
                d.where = (pa.in_ws ? 1u : 0u) | 2u | (nd.in_ws ? 4u : 0u);
                d.base_st = pa.st;
                d.delta_st = nd.pst;
                d.out_st = nd.st;
            }
            for (kd::DlCopy& c : copies) {
                const DlNode& nd = nodes[it[c.pad].node];  // (pad carried the home request)
                c.src_at = nd.at;
                c.src_ws = 0;
                c.pad = 0;
            }
            // level_start as delta_read_from_host takes it: [l - 1] .. [l] is level l
            level_start.erase(level_start.begin());
            hst.assign(n + m + ditems.size(), 0);
        }
        // 4: gather into the pinned staging (grow-only, 8 bytes of padding behind the last source).
        // It holds every source of the call at once: about the arena's size, page-locked until the
        // store is closed (kartdiff.h says so; chunking it through two buffers would bound it)
        const u64 need = soff[n] + (deltas ? soff2[m] : 0) + 8;
        if (odb->pin_cap < need) {
            if (odb->pin) kd_host_free(odb->pin);
            odb->pin = nullptr;
            odb->pin_cap = 0;
            const u64 want = need + need / 4;
            void* p = nullptr;
            if (int rc = kd_host_alloc(want, &p)) return rc;
            odb->pin = (u8*)p;
            odb->pin_cap = want;
        }
        u8* pin = odb->pin;
        par_items(nch, nt, [&](size_t c, int) {
            for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
                const u64 len = soff[i + 1] - soff[i];
                if (!len) continue;
                if (kind[i] == 0) memcpy(pin + soff[i], odb->packs[it[i].key >> 48]->pack.p + it[i].data, len);
                else memcpy(pin + soff[i], part[chunk_of[i]].data() + at[i], len);
            }
        });
        if (deltas) {
            const u64 mch = (m + CH - 1) / CH;
            par_items(mch, nt, [&](size_t c, int) {
                for (u64 j = c * CH; j < std::min(m, (c + 1) * CH); j++) {
                    const DlNode& nd = nodes[wsitem[j]];
                    memcpy(pin + soff[n] + soff2[j], odb->packs[nd.key >> 48]->pack.p + nd.data, soff2[j + 1] - soff2[j]);
                }
            });
        }
        memset(pin + need - 8, 0, 8);
        host_us += us_since(t_pass);
        const auto t_dev = Clock::now();
        // 5: the arena and its offsets in HBM, one upload, one launch (KD_RBD_DELTAS: two, and one per level)
        void *d_data = nullptr, *d_off = nullptr;
        int rc = kd_malloc(ctx, off[n] + 16, &d_data);  // (the tree join reads up to 8 bytes past the last object)
        if (!rc) rc = kd_malloc(ctx, 8 * (n + 1), &d_off);
        if (!rc && !deltas)
            rc = kd::inflate_from_host(ctx, pin, soff.data(), kind.data(), n, (u8*)d_data, off.data(), (u64*)d_off, dstat.data());
        if (!rc && deltas) {
            for (u64 i = 0; i < n; i++) kind[i] = kind[i] != 0;  // (what k_inf_streams takes)
            kd::DlPlan pl{};
            pl.h_src = pin;
            pl.n = n;
            pl.soff1 = soff.data();
            pl.kind1 = kind.data();
            pl.off = off.data();
            pl.m = m;
            pl.soff2 = soff2.data();
            pl.woff = woff.data();
            pl.ws_bytes = ws_bytes;
            pl.items = ditems.data();
            pl.n_items = ditems.size();
            pl.level_start = level_start.data();
            pl.depth = depth;
            pl.copies = copies.data();
            pl.n_copies = copies.size();
            pl.h_status = hst.data();
            pl.d_dst = (u8*)d_data;
            pl.d_dst_off = (u64*)d_off;
            rc = kd::delta_read_from_host(ctx, pl);
            // a request's device status: its own inflate's, or its entry's after the levels
            for (u64 i = 0; i < n && !rc; i++) {
                const bool dl = !forced[i] && it[i].dev == 2;
                dstat[i] = dl ? hst[nodes[it[i].node].st] : hst[i];
                if (dl) kind[i] = 0;  // (below: a device item)
            }
        }
        device_us += us_since(t_dev);
        // 6: a device item with a nonzero status is read on the host: its bytes go into its place,
        // or (the object is corrupt for the host too) it becomes a failed host item of another pass
        u64 nfix = 0, nfixd = 0, nbad = 0;
        if (!rc) {
            Reader& rd = reader(0);
            std::vector<u8> buf;
            for (u64 i = 0; i < n && !rc; i++) {
                if (kind[i] == 0) {
                    status[i] = 0;
                    if (dstat[i] == 0) continue;
                    nfix++;
                    if (!forced[i] && it[i].dev == 2) nfixd++;
                    int type = 0;
                    const int hr = rd.read_packed(*odb->packs[it[i].key >> 48], it[i].key & ((1ull << 48) - 1), &type, buf);
                    if (hr == RD_OK && type == want_type && buf.size() == it[i].size) {
                        if (it[i].size) {
                            rc = kd_memcpy(ctx, (u8*)d_data + off[i], buf.data(), it[i].size, KD_COPY_H2D);
                            if (!rc) rc = kd_sync(ctx);  // (before buf is read into again; a rare path)
                        }
                    } else {
                        forced[i] = 1;
                        nbad++;
                    }
                } else if (dstat[i] != 0) {  // a raw copy cannot fail on ranges this function laid out
                    kd::set_error("kd_odb_read_batch_device: raw item %llu: device status %u", (unsigned long long)i, dstat[i]);
                    rc = KD_EINVAL;
                }
            }
        }
        st4[0] += ndev - (nfix - nfixd);
        st4[2] += comp;
        st4[3] += nfix;
        if (rc || (nbad && pass == 0)) {
            kd_mfree(ctx, d_data);
            kd_mfree(ctx, d_off);
            if (rc) return rc;
            st4[0] = st4[2] = st4[3] = 0;  // the second pass counts again
            continue;
        }
        if (nbad) { kd::set_error("kd_odb_read_batch_device: unreadable items after the host pass"); kd_mfree(ctx, d_data); kd_mfree(ctx, d_off); return KD_EINVAL; }
        st4[1] = nh;
        out->data = (const u8*)d_data;
        out->off = (const u64*)d_off;
        memcpy(st8, st4, sizeof st4);
        st8[4] = ndelta - nfixd;
        st8[5] = ditems.size();
        st8[6] = depth;
        st8[7] = ws_bytes;
        break;
    }
    if (phase_us) {  // (kd_walk_device sums its batches' phases)
        phase_us[0] += plan_us;
        phase_us[1] += host_us;
        phase_us[2] += device_us;
    }
    if (deltas) {
        odb->rbd_us[0] = plan_us;
        odb->rbd_us[1] = peek_us;
        odb->rbd_us[2] = host_us;
        odb->rbd_us[3] = device_us;
    }
    return KD_OK;
}
}  // namespace

extern "C" int kd_odb_read_batch_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, kd_blobs* out,
                                        uint8_t* status, uint64_t stats[4]) {
    if (!ctx || !odb || !out || (n && (!oids || !status))) { kd::set_error("kd_odb_read_batch_device: NULL"); return KD_EINVAL; }
    u64 st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = read_batch_device_impl(ctx, odb, oids, n, threads, 0, out, status, st8);
    if (!rc && stats) memcpy(stats, st8, 4 * sizeof(u64));
    return rc;
}

extern "C" int kd_odb_read_batch_device_ex(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags,
                                           kd_blobs* out, uint8_t* status, uint64_t stats[8]) {
    if (!ctx || !odb || !out || (n && (!oids || !status))) { kd::set_error("kd_odb_read_batch_device_ex: NULL"); return KD_EINVAL; }
    if (flags & ~KD_RBD_DELTAS) { kd::set_error("kd_odb_read_batch_device_ex: unknown flags %u", flags); return KD_EINVAL; }
    if (n >= (1ull << 30)) { kd::set_error("kd_odb_read_batch_device_ex: too many ids"); return KD_EINVAL; }
    u64 st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = read_batch_device_impl(ctx, odb, oids, n, threads, flags, out, status, st8);
    if (!rc && stats) memcpy(stats, st8, sizeof st8);
    return rc;
}

namespace {
// the walked tree of each root: peel commits, then follow `subpath`
int walk_top(kd_odb* odb, Reader& rd0, const uint8_t* roots, int k, const char* subpath, const char* who, Item& top) {
    std::string msg;
    for (int r = 0; r < k && r < KMAX; r++) {
        int rc = peel_to_tree(rd0, roots + 20 * r, top.oid[r], msg);
        if (rc) { kd::set_error("%s: %s", who, msg.c_str()); return rc; }
        top.has[r] = 1;
        top.mode[r] = 040000;
    }
    top.tree = true;
    const std::string sp = subpath ? subpath : "";
    size_t a = 0;
    std::vector<u8> buf;
    std::vector<TEnt> ents;
    while (a < sp.size()) {
        size_t b = sp.find('/', a);
        if (b == std::string::npos) b = sp.size();
        if (b > a) {
            const std::string comp = sp.substr(a, b - a);
            for (int r = 0; r < k && r < KMAX; r++) {
                if (!top.has[r]) continue;
                int type = 0;
                const int rc = rd0.read(top.oid[r], &type, buf);
                if (rc || type != OBJ_TREE || !parse_tree(buf, ents)) {
                    char hx[41];
                    hex40(top.oid[r], hx);
                    kd::set_error("%s: cannot read tree %s", who, hx);
                    return rc == RD_MISSING ? KD_ENOTFOUND : KD_EINVAL;
                }
                top.has[r] = 0;
                for (const TEnt& e : ents)
                    if (e.tree() && e.nlen == comp.size() && !memcmp(e.name, comp.data(), e.nlen)) {
                        memcpy(top.oid[r], e.oid, 20);
                        top.has[r] = 1;
                        break;
                    }
            }
        }
        a = b + 1;
    }
    return KD_OK;
}

// one level of breadth-first expansion, in parallel: every subtree item replaced by its children
void walk_expand_level(kd_odb* odb, Walk& W, std::vector<Item>& items, int nt) {
    std::vector<std::vector<Item>> kids(items.size());
    std::vector<std::unique_ptr<Reader>> rds(nt);
    par_items(items.size(), nt, [&](size_t i, int tid) {
        if (!items[i].tree) { kids[i].push_back(items[i]); return; }
        if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
        W.expand(*rds[tid], items[i], [&](const Item& c) { kids[i].push_back(c); });
    });
    if (W.err) return;
    std::vector<Item> next;
    for (auto& v : kids)
        for (auto& c : v) next.push_back(std::move(c));
    items.swap(next);
}

// every item's outputs stitched in item order into one block per root
int walk_stitch(const std::vector<Item>& items, const std::vector<WalkOut>& outs, int k, const Item& top, int nt, const char* who,
                kd_leaves** out) {
    for (int r = 0; r < k && r < KMAX; r++) {
        u64 n = 0, bytes = 0;
        for (size_t i = 0; i < items.size(); i++) {
            n += outs[i * k + r].end.size();
            bytes += outs[i * k + r].path.size();
        }
        // one block: header, path_off[n+1], mode[n], oid[20n], path bytes (kd_free)
        const size_t hsz = (sizeof(kd_leaves) + 15) & ~(size_t)15;
        const size_t total = hsz + 8 * (n + 1) + 4 * n + 20 * n + bytes + 16;
        u8* blk = (u8*)std::malloc(total);
        if (!blk) {
            for (int q = 0; q < r; q++) { std::free(out[q]); out[q] = nullptr; }
            kd::set_error("%s: out of memory (%llu leaves)", who, (unsigned long long)n);
            return KD_EINVAL;
        }
        kd_leaves* L = (kd_leaves*)blk;
        L->n = n;
        L->path_off = (uint64_t*)(blk + hsz);
        L->mode = (uint32_t*)(L->path_off + n + 1);
        L->oid = (uint8_t*)(L->mode + n);
        L->path = L->oid + 20 * n;
        L->present = top.has[r];
        L->path_off[0] = 0;
        // per-item bases, then parallel copies
        std::vector<u64> lbase(items.size() + 1, 0), bbase(items.size() + 1, 0);
        for (size_t i = 0; i < items.size(); i++) {
            lbase[i + 1] = lbase[i] + outs[i * k + r].end.size();
            bbase[i + 1] = bbase[i] + outs[i * k + r].path.size();
        }
        par_items(items.size(), nt, [&](size_t i, int) {
            const WalkOut& o = outs[i * k + r];
            const u64 m = o.end.size();
            if (!m) return;
            memcpy(L->path + bbase[i], o.path.data(), o.path.size());
            memcpy(L->oid + 20 * lbase[i], o.oid.data(), 20 * m);
            memcpy(L->mode + lbase[i], o.mode.data(), 4 * m);
            for (u64 j = 0; j < m; j++) L->path_off[lbase[i] + j + 1] = bbase[i] + o.end[j];
        });
        out[r] = L;
    }
    return KD_OK;
}
}  // namespace

extern "C" int kd_walk(kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1, int threads,
                       kd_leaves** out) {
    if (!odb || !roots || !out || k < 1 || k > KMAX) { kd::set_error("kd_walk: bad arguments"); return KD_EINVAL; }
    if ((cmp0 < 0) != (cmp1 < 0) || cmp0 >= k || cmp1 >= k || (cmp0 >= 0 && cmp0 == cmp1)) {
        kd::set_error("kd_walk: compare roots %d/%d of %d", cmp0, cmp1, k);
        return KD_EINVAL;
    }
    for (int r = 0; r < k && r < KMAX; r++) out[r] = nullptr;
    const int nt = default_threads(threads);
    Walk W;
    W.k = k;
    W.c0 = cmp0 < 0 ? -1 : cmp0;
    W.c1 = cmp1 < 0 ? -1 : cmp1;
    Reader rd0(odb);
    Item top;
    if (int rc = walk_top(odb, rd0, roots, k, subpath, "kd_walk", top)) return rc;
    // ---- items: the top expanded breadth-first (in parallel) until there is work for every thread ----
    std::vector<Item> items;
    if (!W.pruned(top) && std::any_of(top.has, top.has + k, [](u8 h) { return h != 0; })) items.push_back(top);
    for (int level = 0; level < 4; level++) {
        size_t ntree = 0;
        for (auto& it : items) ntree += it.tree;
        if (ntree == 0 || ntree >= (size_t)nt * 16) break;
        walk_expand_level(odb, W, items, nt);
        if (W.err) break;
    }
    // ---- every item walked by some thread into its own outputs; then stitched in item order ----
    std::vector<WalkOut> outs;
    if (!W.err) {
        outs.resize(items.size() * k);
        std::vector<std::unique_ptr<Reader>> rds(nt);
        par_items(items.size(), nt, [&](size_t i, int tid) {
            WalkOut* o = &outs[i * k];
            if (!items[i].tree) { W.emit(items[i], o); return; }
            if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
            W.walk_item(*rds[tid], items[i], o);
        });
    }
    if (W.err) {
        kd::set_error("kd_walk: %s", W.emsg.c_str());
        return W.err.load();
    }
    return walk_stitch(items, outs, k, top, nt, "kd_walk", out);
}

// ---------------------------------------------------------------------------------------------
// kd_walk with its lowest level on the GPU: the host expands `depth` levels, the subtree items left at
// that depth become tasks of kd_tree_join_batch over trees read by the batched device read
// ---------------------------------------------------------------------------------------------
namespace {
struct OidKey {
    u8 b[20];
    bool operator<(const OidKey& o) const { return memcmp(b, o.b, 20) < 0; }
    bool operator==(const OidKey& o) const { return memcmp(b, o.b, 20) == 0; }
};

// what a packed or loose tree costs a batch: the compressed span the device read ships for it, or the bytes the
// host reads for it (the entry header's size either way; 4 KiB where unknown).  For a delta entry the header's
// size is the delta's, not the tree's (that is known only after the plan's peek): on a repacked repository a
// batch's arena and outputs can be several times walk_batch_bytes (kartdiff.h says so)
u64 tree_cost(kd_odb* odb, Reader& rd, const u8* oid) {
    u64 o;
    const long p = rd.locate(oid, &o);
    int type;
    u64 size, data, boff = 0;
    const u8* boid = nullptr;
    if (p < 0 || rd.entry_header(*odb->packs[p], o, &type, &size, &data, &boff, &boid) != RD_OK) return 4096;
    return inf_bound(size);
}
}  // namespace

extern "C" int kd_walk_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1,
                              int threads, int depth, uint32_t flags, kd_leaves** out, uint64_t* stats) {
    if (!ctx || !odb || !roots || !out || k < 1 || k > KMAX || depth < 0 || depth > 64) {
        kd::set_error("kd_walk_device: bad arguments");
        return KD_EINVAL;
    }
    if ((cmp0 < 0) != (cmp1 < 0) || cmp0 >= k || cmp1 >= k || (cmp0 >= 0 && cmp0 == cmp1)) {
        kd::set_error("kd_walk_device: compare roots %d/%d of %d", cmp0, cmp1, k);
        return KD_EINVAL;
    }
    if (flags & ~KD_RBD_DELTAS) { kd::set_error("kd_walk_device: unknown flags %u", flags); return KD_EINVAL; }
    for (int r = 0; r < k; r++) out[r] = nullptr;
    u64 st[KD_WD_STATS];
    memset(st, 0, sizeof st);
    const int nt = default_threads(threads);
    Walk W;
    W.k = k;
    W.c0 = cmp0 < 0 ? -1 : cmp0;
    W.c1 = cmp1 < 0 ? -1 : cmp1;
    Reader rd0(odb);
    Item top;
    const auto t_call = Clock::now();
    auto t0 = Clock::now();
    if (int rc = walk_top(odb, rd0, roots, k, subpath, "kd_walk_device", top)) return rc;
    // ---- host expansion: `depth` levels below the walked tree, breadth-first, pruned ----
    std::vector<Item> items;
    if (!W.pruned(top) && std::any_of(top.has, top.has + k, [](u8 h) { return h != 0; })) items.push_back(top);
    for (int level = 0; level < depth && !W.err; level++) {
        if (std::none_of(items.begin(), items.end(), [](const Item& it) { return it.tree; })) break;
        walk_expand_level(odb, W, items, nt);
    }
    if (W.err) {
        kd::set_error("kd_walk_device: %s", W.emsg.c_str());
        return W.err.load();
    }
    st[10] = (u64)us_since(t0);
    // ---- tasks: every subtree item left; a blob item is the host's, emitted as kd_walk emits it ----
    std::vector<WalkOut> outs(items.size() * k);
    std::vector<size_t> task_item;
    for (size_t i = 0; i < items.size(); i++) {
        if (items[i].tree) task_item.push_back(i);
        else W.emit(items[i], &outs[i * k]);
    }
    const u64 ntask = task_item.size();
    st[0] = ntask;
    std::vector<u8> on_host(ntask, 0);
    u64 batch_bytes;
    {
        std::lock_guard<std::mutex> lk(odb->dev_mu);
        batch_bytes = odb->walk_batch_bytes;
    }
    int rc = KD_OK;
    int64_t read_us[3] = {0, 0, 0};  // the batched reads' plan, host reads + gather, device
    // what each task costs a batch, by every thread (a locate and an entry header per tree)
    t0 = Clock::now();
    std::vector<u64> task_cost(ntask, 0);
    {
        constexpr u64 CH = 256;
        std::vector<std::unique_ptr<Reader>> rds(nt);
        par_items((ntask + CH - 1) / CH, nt, [&](size_t c, int tid) {
            if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
            for (u64 t = c * CH; t < std::min(ntask, (c + 1) * CH); t++) {
                const Item& it = items[task_item[t]];
                for (int r = 0; r < k; r++)
                    if (it.has[r]) task_cost[t] += tree_cost(odb, *rds[tid], it.oid[r]);
            }
        });
    }
    st[11] += (u64)us_since(t0);
    for (u64 lo = 0; lo < ntask && !rc;) {
        // ---- one batch: tasks [lo, hi), their trees made unique ----
        t0 = Clock::now();
        std::vector<OidKey> uniq;
        u64 hi = lo, cost = 0;
        for (; hi < ntask; hi++) {
            const Item& it = items[task_item[hi]];
            const u64 c = task_cost[hi];
            if (hi > lo && cost + c > batch_bytes) break;
            cost += c;
            for (int r = 0; r < k; r++)
                if (it.has[r]) {
                    OidKey q;
                    memcpy(q.b, it.oid[r], 20);
                    uniq.push_back(q);
                }
        }
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        const u64 nu = uniq.size();
        st[3] += nu;
        st[9]++;
        st[11] += (u64)us_since(t0);
        t0 = Clock::now();
        // ---- the trees read through the batched device read (expected type: tree) ----
        std::vector<u8> rstat(std::max<u64>(nu, 1), 0);
        const int64_t read_before = read_us[0] + read_us[1] + read_us[2];
        kd_blobs arena{};
        u64 st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        rc = read_batch_device_impl(ctx, odb, (const u8*)uniq.data(), nu, threads, flags, &arena, rstat.data(), st8, OBJ_TREE, read_us);
        if (rc) break;
        st[4] += st8[0];
        st[5] += st8[1];
        st[6] += st8[3];
        st[7] += st8[2];
        st[8] += st8[4];
        std::vector<u64> off(nu + 1);
        rc = kd_memcpy(ctx, off.data(), arena.off, 8 * (nu + 1), KD_COPY_D2H);
        if (!rc) rc = kd_sync(ctx);
        st[17] += (u64)std::max<int64_t>(0, us_since(t0) - ((read_us[0] + read_us[1] + read_us[2]) - read_before));  // (the offsets back)
        t0 = Clock::now();
        // ---- device tasks: every tree read, none above KD_INF_MAX; the join's own bound on a call ----
        std::vector<u32> tix;         // [nd * k]
        std::vector<u64> dtask;       // the batch's device tasks (indices into task_item)
        std::vector<u64> poff{0};
        std::string pfx;
        u64 cap_n[KMAX] = {0, 0, 0}, cap_b[KMAX] = {0, 0, 0}, bound = 0;
        for (u64 t = lo; t < hi && !rc; t++) {
            const Item& it = items[task_item[t]];
            u32 ix[KMAX] = {KD_NONE, KD_NONE, KD_NONE};
            bool dev = true;
            u64 tb = 0;
            for (int r = 0; r < k; r++) {
                if (!it.has[r]) continue;
                OidKey q;
                memcpy(q.b, it.oid[r], 20);
                const u64 u = (u64)(std::lower_bound(uniq.begin(), uniq.end(), q) - uniq.begin());
                const u64 L = off[u + 1] - off[u];
                if (rstat[u] != 0 || L > KD_INF_MAX) dev = false;
                ix[r] = (u32)u;
                tb += L + (L / 23) * (it.path.size() + 2);
            }
            if (!dev || bound + tb >= (1ull << 31)) {  // (a batch that large: the rest of it is the host's)
                on_host[t] = 1;
                continue;
            }
            bound += tb;
            for (int r = 0; r < k; r++) {
                tix.push_back(ix[r]);
                if (ix[r] == KD_NONE) continue;
                const u64 L = off[ix[r] + 1] - off[ix[r]];
                cap_n[r] += L / 23;
                cap_b[r] += L + (L / 23) * (it.path.size() + 1);
            }
            dtask.push_back(t);
            pfx += it.path;
            poff.push_back(pfx.size());
        }
        const u64 nd = dtask.size();
        // ---- the join on the device, its results back ----
        std::vector<u32> cnt(std::max<u64>(nd * k, 1), 0);
        std::vector<u8> jst(std::max<u64>(nd, 1), 0);
        std::vector<u64> tot(2 * KMAX, 0);
        std::vector<std::vector<u8>> hpath(k), hoid(k);
        std::vector<std::vector<u64>> hpoff(k);
        std::vector<std::vector<u32>> hmode(k);
        if (!rc && nd) {
            std::vector<void*> dev;
            auto dalloc = [&](u64 bytes, const void* src) -> void* {
                void* p = nullptr;
                if (rc) return p;
                rc = kd_malloc(ctx, std::max<u64>(bytes, 16), &p);
                if (!rc) dev.push_back(p);
                if (!rc && src && bytes) rc = kd_memcpy(ctx, p, src, bytes, KD_COPY_H2D);
                return p;
            };
            void* d_tix = dalloc(4 * nd * k, tix.data());
            void* d_pfx = dalloc(pfx.size(), pfx.data());
            void* d_poff = dalloc(8 * (nd + 1), poff.data());
            void* d_cnt = dalloc(4 * nd * k, nullptr);
            void* d_st = dalloc(nd, nullptr);
            void* d_tot = dalloc(16 * KMAX, nullptr);
            kd_tj_out jo[KMAX];
            memset(jo, 0, sizeof jo);
            for (int r = 0; r < k; r++) {
                jo[r].cap_n = cap_n[r];
                jo[r].cap_bytes = cap_b[r];
                jo[r].path_off = (uint64_t*)dalloc(8 * (cap_n[r] + 1), nullptr);
                jo[r].mode = (uint32_t*)dalloc(4 * cap_n[r], nullptr);
                jo[r].oid = (uint8_t*)dalloc(20 * cap_n[r], nullptr);
                jo[r].path = (uint8_t*)dalloc(cap_b[r], nullptr);
            }
            if (!rc) rc = kd_sync(ctx);  // (the uploads read pageable vectors)
            st[15] += (u64)us_since(t0);
            t0 = Clock::now();
            if (!rc)
                rc = kd_tree_join_batch(ctx, arena.data, arena.off, nu, (const u32*)d_tix, (const u8*)d_pfx, (const u64*)d_poff, nd, k,
                                        cmp0, cmp1, jo, (u32*)d_cnt, (u8*)d_st, (u64*)d_tot, KD_MEM_DEVICE);
            if (!rc) rc = kd_memcpy(ctx, tot.data(), d_tot, 16 * k, KD_COPY_D2H);
            if (!rc) rc = kd_memcpy(ctx, cnt.data(), d_cnt, 4 * nd * k, KD_COPY_D2H);
            if (!rc) rc = kd_memcpy(ctx, jst.data(), d_st, nd, KD_COPY_D2H);
            if (!rc) rc = kd_sync(ctx);
            st[16] += (u64)us_since(t0);  // (the kernels and three small copies behind them)
            t0 = Clock::now();
            for (int r = 0; r < k && !rc; r++) {
                const u64 n = tot[2 * r], nbytes = tot[2 * r + 1];
                if (n > cap_n[r] || nbytes > cap_b[r]) {  // (the capacities are upper bounds)
                    kd::set_error("kd_walk_device: the join kept more than its trees hold");
                    rc = KD_EINVAL;
                    break;
                }
                hpoff[r].resize(n + 1);
                hmode[r].resize(n);
                hoid[r].resize(20 * n);
                hpath[r].resize(nbytes);
                rc = kd_memcpy(ctx, hpoff[r].data(), jo[r].path_off, 8 * (n + 1), KD_COPY_D2H);
                if (!rc && n) rc = kd_memcpy(ctx, hmode[r].data(), jo[r].mode, 4 * n, KD_COPY_D2H);
                if (!rc && n) rc = kd_memcpy(ctx, hoid[r].data(), jo[r].oid, 20 * n, KD_COPY_D2H);
                if (!rc && nbytes) rc = kd_memcpy(ctx, hpath[r].data(), jo[r].path, nbytes, KD_COPY_D2H);
            }
            if (!rc) rc = kd_sync(ctx);
            else kd_sync(ctx);
            for (void* p : dev) kd_mfree(ctx, p);
        }
        kd_mfree(ctx, (void*)arena.data);
        kd_mfree(ctx, (void*)arena.off);
        st[17] += (u64)us_since(t0);
        if (rc) break;
        // ---- a device task's entries into its item's outputs (a refused task is the host's) ----
        t0 = Clock::now();
        for (int r = 0; r < k; r++) {
            std::vector<u64> first(nd + 1, 0);
            for (u64 j = 0; j < nd; j++) first[j + 1] = first[j] + cnt[j * k + r];
            par_items(nd, nt, [&](size_t j, int) {
                if (jst[j] != KD_TJ_OK || !cnt[j * k + r]) return;
                WalkOut& o = outs[task_item[dtask[j]] * k + r];
                const u64 e0 = first[j], e1 = first[j + 1], b0 = hpoff[r][e0];
                o.path.assign((const char*)hpath[r].data() + b0, hpoff[r][e1] - b0);
                o.end.resize(e1 - e0);
                for (u64 e = e0; e < e1; e++) o.end[e - e0] = hpoff[r][e + 1] - b0;
                o.oid.assign(hoid[r].begin() + 20 * e0, hoid[r].begin() + 20 * e1);
                o.mode.assign(hmode[r].begin() + e0, hmode[r].begin() + e1);
            });
        }
        for (u64 j = 0; j < nd; j++)
            if (jst[j] != KD_TJ_OK) on_host[dtask[j]] = 1;
        st[18] += (u64)us_since(t0);
        lo = hi;
    }
    if (rc) return rc;
    // ---- host-class tasks: the existing walk of the item ----
    t0 = Clock::now();
    std::vector<size_t> hostq;
    for (u64 t = 0; t < ntask; t++)
        if (on_host[t]) hostq.push_back(task_item[t]);
    st[2] = hostq.size();
    st[1] = ntask - hostq.size();
    {
        std::vector<std::unique_ptr<Reader>> rds(nt);
        par_items(hostq.size(), nt, [&](size_t q, int tid) {
            if (!rds[tid]) rds[tid] = std::make_unique<Reader>(odb);
            W.walk_item(*rds[tid], items[hostq[q]], &outs[hostq[q] * k]);
        });
    }
    st[19] = (u64)us_since(t0);
    if (W.err) {
        kd::set_error("kd_walk_device: %s", W.emsg.c_str());
        return W.err.load();
    }
    t0 = Clock::now();
    rc = walk_stitch(items, outs, k, top, nt, "kd_walk_device", out);
    st[18] += (u64)us_since(t0);
    st[12] = (u64)read_us[0];
    st[13] = (u64)read_us[1];
    st[14] = (u64)read_us[2];
    st[20] = (u64)us_since(t_call);  // the whole call: what [10..19] leave of it is vectors built and freed, allocations
    if (!rc && stats) memcpy(stats, st, sizeof st);
    return rc;
}
