// kd_odb.cpp — the git object database read natively: loose objects, pack v2 with idx v1/v2, zlib,
// OFS/REF delta chains.
//
// Replaces what Kart gets from libgit2 (koordinates fork @ bb69c8fa, vendor/libgit2/Makefile:1-3)
// on the diff path: the blob reads of BaseDataset.get_blob_at (kart/base_dataset.py:230-265) and the
// object reads under the feature-tree iteration of Dataset3 (the walk itself is kd_odb_walk.cpp).
//
// Host code (no GPU).  Formats follow git's documented ones (Documentation/technical/pack-format.txt,
// see kd_odb_store.h); a delta = src/dst size varints + copy/insert ops, decoded by kd_delta.h.
#include <dirent.h>
#include <dlfcn.h>

#include <cstdlib>

#include "kd_delta.h"
#include "kd_odb_store.h"

namespace kd_store {

bool Pack::open(const std::string& idx_path, const std::string& pack_path) {
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

bool Pack::find(const u8* oid, u64* off) const {
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

}  // namespace

// ---------------------------------------------------------------------------------------------
// Reader
// ---------------------------------------------------------------------------------------------
Reader::Reader(const kd_odb* d) : db(d), cache(CACHE_SLOTS) {
    memset(&z, 0, sizeof z);
    zok = inflateInit(&z) == Z_OK;
    if (!d->zlib_only && deflate_lib().ok()) dec = deflate_lib().alloc();
}

Reader::~Reader() {
    if (zok) inflateEnd(&z);
    if (dec) deflate_lib().release(dec);
}

int Reader::inflate_exact(const u8* src, size_t avail, u8* dst, size_t size) {
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

int Reader::entry_header(const Pack& pk, u64 off, int* type, u64* size, u64* data, u64* base_off, const u8** base_oid) {
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

// git's delta applied to `base`: kd_delta.h decodes and bounds every op, memcpy moves its bytes
int Reader::rebuild(const std::vector<u8>& base, const std::vector<u8>& delta, std::vector<u8>& out) {
    const u8* d = delta.data();
    const u64 dlen = delta.size(), blen = base.size();
    u64 pos = 0, src, dst;
    if (!kd_dl::size_varint(d, dlen, &pos, &src) || !kd_dl::size_varint(d, dlen, &pos, &dst) || src != blen) return RD_CORRUPT;
    out.resize(dst);
    for (u64 w = 0;;) {
        u32 kind, len;
        u64 from;
        if (kd_dl::next_op(d, dlen, blen, dst, w, &pos, &kind, &from, &len) != KD_DL_OK) return RD_CORRUPT;
        if (kind == kd_dl::OP_END) return RD_OK;
        memcpy(out.data() + w, (kind == kd_dl::OP_COPY ? base.data() : d) + from, len);
        w += len;
    }
}

int Reader::read_packed(const Pack& pk, u64 off, int* type, std::vector<u8>& out, int depth) {
    struct Link { u64 off, data, size; };
    std::vector<Link> chain;
    u64 cur = off;
    int btype = 0;
    for (;;) {
        Slot& s = slot(cur);
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
        if (rebuild(out, dbuf, tmp)) return RD_CORRUPT;
        out.swap(tmp);
        // every resolved link, the object itself included: in a batch read in pack order the
        // next object is usually a delta against this one (fast-import and repack chains)
        remember(&pk, L.off, btype, out);
    }
    *type = btype;
    return RD_OK;
}

void Reader::remember(const Pack* pk, u64 off, int type, const std::vector<u8>& data) {
    if (data.size() > CACHE_MAX_OBJ) return;
    Slot& s = slot(off);
    s.pk = pk;
    s.off = off;
    s.type = type;
    s.data = data;
}

// one loose object file: zlib("<type> <size>\0" + content)
int Reader::parse_loose(const std::vector<u8>& raw, int* type, std::vector<u8>& out) {
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
int Reader::read_loose(const u8* oid, int* type, std::vector<u8>& out) {
    char name[41];
    hex40(oid, name);
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

// The packs that held the last few objects are searched first, most recent first: a batch's objects
// tend to share packs, a compare walk alternates between its roots' packs (one per side and subtree
// in a repository written by parallel imports), and every miss is a binary search of another index
long Reader::locate(const u8* oid, u64* off) {
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

int Reader::read(const u8* oid, int* type, std::vector<u8>& out, int depth) {
    u64 off;
    const long p = locate(oid, &off);
    if (p >= 0) return read_packed(*db->packs[p], off, type, out, depth);
    return read_loose(oid, type, out);
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

}  // namespace kd_store

using namespace kd_store;

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
    Readers rds(odb, nt);
    par_items(nch, nt, [&](size_t c, int tid) {
        Reader& rd = rds[tid];
        for (u64 i = c * CH; i < std::min(n, (c + 1) * CH); i++) {
            u64 o;
            const long p = rd.locate(oids + 20 * i, &o);
            ord[i] = {p >= 0 && p < 0xFFFF && o < (1ull << 48) ? pack_key(p, o) : KEY_NONE, i};
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
        Reader& rd = rds[tid];
        std::vector<u8> buf;
        for (u64 s = c * CH; s < std::min(n, (c + 1) * CH); s++) {
            const u64 key = ord[s].first, i = ord[s].second;
            int type = 0;
            const int rc = key != KEY_NONE ? rd.read_packed(*odb->packs[key_pack(key)], key_off(key), &type, buf)
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
