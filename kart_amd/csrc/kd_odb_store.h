// kd_odb_store.h — what the object-store units share (library internal): the mapped packs, struct kd_odb,
// one thread's Reader, and the small helpers every unit uses.
//
//   kd_odb.cpp          the store itself: open / close / options, the Reader, kd_odb_read, kd_odb_read_batch
//   kd_odb_walk.cpp     the leaf walk over it: kd_walk, kd_walk_device
//   kd_odb_plan.cpp     the host-only plan of the batched device read (kd_odb_plan.h)
//   kd_odb_devread.cpp  the plan carried out on the device: kd_odb_read_batch_device, .._ex
//
// Formats follow git's documented ones (Documentation/technical/pack-format.txt): idx v2 = magic,
// fanout[256], sha[n], crc[n], off32[n] (MSB -> index into off64[]); pack entries = type/size varint
// header, zlib stream; OFS_DELTA base = this offset - (offset varint).
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kartdiff.h"

namespace kd {
void set_error(const char* fmt, ...);
}

namespace kd_store {

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

    bool open(const std::string& idx_path, const std::string& pack_path);
    // offset of `oid` in the pack, or false
    bool find(const u8* oid, u64* off) const;
};

struct Reader;

}  // namespace kd_store

struct kd_odb {
    std::vector<std::string> objdirs;  // objects/ and its alternates
    std::vector<std::unique_ptr<kd_store::Pack>> packs;
    // idle readers (zlib stream + base cache) reused by single-object reads: building one costs
    // more than reading a small object (ctypes drops the GIL, so calls may be concurrent)
    std::mutex pool_mu;
    std::vector<kd_store::Reader*> pool;
    // options (kd_odb_set_option; kd_odb_open seeds them from the environment)
    int zlib_only = 0;  // "zlib" [KD_ODB_ZLIB]: 1 = inflate with zlib even when libdeflate is present (A/B)
    // "walk_batch_bytes" [KD_WALK_BATCH_BYTES]: kd_walk_device reads its leaf trees in batches of about this
    // many compressed and host-read bytes (what bounds the pinned staging and the device arena of a walk)
    uint64_t walk_batch_bytes = 64ull << 20;
    // kd_odb_read_batch_device: the pinned staging its sources are gathered into (grow-only), one call at a time
    std::mutex dev_mu;
    uint8_t* pin = nullptr;
    uint64_t pin_cap = 0;
    // the last kd_odb_read_batch_device_ex call's host phases in microseconds (kd_odb_get_option "rbd_*_us")
    int64_t rbd_us[4] = {0, 0, 0, 0};  // plan (all of it), peek (the header peeks in it), host reads + gather, device
};

namespace kd_store {

// One thread's reader: a zlib stream, a delta-base cache, scratch buffers.  (Defined in kd_odb.cpp.)
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

    explicit Reader(const kd_odb* d);
    ~Reader();
    Reader(const Reader&) = delete;

    // inflate one zlib stream starting at src into exactly `size` bytes
    int inflate_exact(const u8* src, size_t avail, u8* dst, size_t size);
    // entry header at `off`: type, inflated size, start of the zlib data (after the delta base)
    int entry_header(const Pack& pk, u64 off, int* type, u64* size, u64* data, u64* base_off, const u8** base_oid);
    // object at `off` of `pk` (delta chains resolved) into out
    int read_packed(const Pack& pk, u64 off, int* type, std::vector<u8>& out, int depth = 0);
    // the pack holding oid, or -1 (the packs that held the last few objects are searched first)
    long locate(const u8* oid, u64* off);
    // the object `oid`, packed or loose
    int read(const u8* oid, int* type, std::vector<u8>& out, int depth = 0);

    static constexpr int MRU = 4;
    size_t mru[MRU] = {~size_t(0), ~size_t(0), ~size_t(0), ~size_t(0)};

private:
    Slot& slot(u64 off) { return cache[(off * 0x9E3779B97F4A7C15ull) >> 54 & (CACHE_SLOTS - 1)]; }
    void remember(const Pack* pk, u64 off, int type, const std::vector<u8>& data);
    int rebuild(const std::vector<u8>& base, const std::vector<u8>& delta, std::vector<u8>& out);
    int parse_loose(const std::vector<u8>& raw, int* type, std::vector<u8>& out);
    int read_loose(const u8* oid, int* type, std::vector<u8>& out);
};

// a per-thread set of readers for one parallel region, each built when its thread first asks for it
struct Readers {
    const kd_odb* db;
    std::vector<std::unique_ptr<Reader>> rds;
    Readers(const kd_odb* d, int nt) : db(d), rds((size_t)nt) {}
    Reader& operator[](int tid) {
        if (!rds[tid]) rds[tid] = std::make_unique<Reader>(db);
        return *rds[tid];
    }
};

inline void hex40(const u8* oid, char* out) {
    static const char hx[] = "0123456789abcdef";
    for (int i = 0; i < 20; i++) {
        out[2 * i] = hx[oid[i] >> 4];
        out[2 * i + 1] = hx[oid[i] & 15];
    }
    out[40] = 0;
}

inline bool unhex40(const u8* s, u8* oid) {
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

// the most a deflate stream of `size` bytes is taken to occupy (a stored block's 5 bytes per 16 KiB
// and the wrapper, with room); a stream that is longer fails on the device and is read on the host
inline u64 inf_bound(u64 size) { return size + (size >> 12) + (size >> 14) + (size >> 25) + 13; }

// a request's or a forest entry's place: pack << 48 | offset (~0: not in a pack this key can name)
constexpr u64 KEY_NONE = ~0ull;
inline u64 pack_key(long p, u64 off) { return (u64)p << 48 | off; }
inline size_t key_pack(u64 key) { return (size_t)(key >> 48); }
inline u64 key_off(u64 key) { return key & ((1ull << 48) - 1); }

// fn(i, tid) for every i < n, by at most `threads` threads taking the next i in turn
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

inline int default_threads(int threads) {
    if (threads > 0) return std::min(threads, 256);
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hc ? hc : 1u, 16u));
}

using Clock = std::chrono::steady_clock;
inline int64_t us_since(Clock::time_point t0) {
    return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - t0).count();
}

// ---------------------------------------------------------------------------------------------
// kd_odb_devread.cpp, for kd_walk_device's leaf trees
// ---------------------------------------------------------------------------------------------
// the counters of one batched device read, in the order kartdiff.h gives stats[4] and stats[8]
struct ReadStats {
    u64 device = 0, host = 0, compressed = 0, fixups = 0, deltas = 0, links = 0, depth = 0, scratch = 0;
};
static_assert(sizeof(ReadStats) == 8 * sizeof(u64), "stats[8] is a view of ReadStats");

// kd_odb_read_batch_device_ex behind its argument checks.  want_type: the object type the ids must name
// (status 2 for anything else); phase_us: [3] plan, host reads + gather, device are added to it
int read_batch_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags, kd_blobs* out,
                      uint8_t* status, ReadStats* stats, int want_type, int64_t* phase_us);

}  // namespace kd_store
