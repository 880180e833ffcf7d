// kd_odb_walk.cpp — Dataset3's leaf walk over the object store (kd_odb.cpp), with tree-OID pruning.
//
// Replaces, on the diff path, the feature-tree iteration of Dataset3 (kart/dataset3.py:26-35,225-231) and
// the subtree pruning of tree-to-tree diff (pygit2 Tree.diff_to_tree, called at
// kart/rich_base_dataset.py:212-232): a subtree whose OID is the same in both trees is never opened.
//
// The walk feeds the packer (kd_pack_*_keys, kd_sort_side): its output is the flat (path arena, offsets,
// OIDs) layout those take.  kd_walk is host code; kd_walk_device hands its lowest level to the GPU.
#include <cstdlib>

#include "kd_odb_store.h"

namespace kd_store {
namespace {

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

// (laxer than kd_treeparse.h, which refuses what git's fsck refuses: whatever that one refuses comes here)
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

    Walk(int k_, int cmp0, int cmp1) : k(k_), c0(cmp0 < 0 ? -1 : cmp0), c1(cmp1 < 0 ? -1 : cmp1) {}

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

    // the joined entries e as an item without its path; -> the first root's entry that is present
    const TEnt* child_entries(const TEnt* const* e, Item& c) const {
        const TEnt* e0 = nullptr;
        for (int r = 0; r < k && r < KMAX; r++)
            if (e[r]) {
                e0 = e0 ? e0 : e[r];
                c.has[r] = 1;
                c.mode[r] = e[r]->mode;
                memcpy(c.oid[r], e[r]->oid, 20);
            }
        c.tree = e0->tree();
        return e0;
    }

    Item child(const std::string& parent, const TEnt* const* e) const {
        Item c;
        const TEnt* e0 = child_entries(e, c);
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
                Item c;  // (child's entries; its path is `path`, in place)
                child_entries(e, c);
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

// what kd_walk and kd_walk_device both ask of their arguments
int check_walk_args(const char* who, const kd_odb* odb, const uint8_t* roots, int k, int cmp0, int cmp1, kd_leaves** out) {
    if (!odb || !roots || !out || k < 1 || k > KMAX) { kd::set_error("%s: bad arguments", who); return KD_EINVAL; }
    if ((cmp0 < 0) != (cmp1 < 0) || cmp0 >= k || cmp1 >= k || (cmp0 >= 0 && cmp0 == cmp1)) {
        kd::set_error("%s: compare roots %d/%d of %d", who, cmp0, cmp1, k);
        return KD_EINVAL;
    }
    return KD_OK;
}

// the walked tree of each root: peel commits, then follow `subpath`
int walk_top(Reader& rd0, const uint8_t* roots, int k, const char* subpath, const char* who, Item& top) {
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

// the walk's first items: the top itself, unless it is pruned or absent from every root
std::vector<Item> walk_start(const Walk& W, const Item& top) {
    std::vector<Item> items;
    if (!W.pruned(top) && std::any_of(top.has, top.has + W.k, [](u8 h) { return h != 0; })) items.push_back(top);
    return items;
}

// one level of breadth-first expansion, in parallel: every subtree item replaced by its children
void walk_expand_level(kd_odb* odb, Walk& W, std::vector<Item>& items, int nt) {
    std::vector<std::vector<Item>> kids(items.size());
    Readers rds(odb, nt);
    par_items(items.size(), nt, [&](size_t i, int tid) {
        if (!items[i].tree) { kids[i].push_back(items[i]); return; }
        W.expand(rds[tid], items[i], [&](const Item& c) { kids[i].push_back(c); });
    });
    if (W.err) return;
    std::vector<Item> next;
    for (auto& v : kids)
        for (auto& c : v) next.push_back(std::move(c));
    items.swap(next);
}

// the host walk of items[q[..]], each into its own outputs, by every thread
void walk_items(kd_odb* odb, Walk& W, const std::vector<Item>& items, const std::vector<size_t>& q, std::vector<WalkOut>& outs,
                int nt) {
    Readers rds(odb, nt);
    par_items(q.size(), nt, [&](size_t j, int tid) {
        const size_t i = q[j];
        if (!items[i].tree) W.emit(items[i], &outs[i * W.k]);
        else W.walk_item(rds[tid], items[i], &outs[i * W.k]);
    });
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
}  // namespace kd_store

using namespace kd_store;

extern "C" int kd_walk(kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1, int threads,
                       kd_leaves** out) {
    if (int rc = check_walk_args("kd_walk", odb, roots, k, cmp0, cmp1, out)) return rc;
    for (int r = 0; r < k; r++) out[r] = nullptr;
    const int nt = default_threads(threads);
    Walk W(k, cmp0, cmp1);
    Reader rd0(odb);
    Item top;
    if (int rc = walk_top(rd0, roots, k, subpath, "kd_walk", top)) return rc;
    // ---- items: the top expanded breadth-first (in parallel) until there is work for every thread ----
    std::vector<Item> items = walk_start(W, top);
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
        std::vector<size_t> all(items.size());
        for (size_t i = 0; i < all.size(); i++) all[i] = i;
        walk_items(odb, W, items, all, outs, nt);
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
namespace kd_store {
namespace {

struct OidKey {
    u8 b[20];
    explicit OidKey(const u8* oid) { memcpy(b, oid, 20); }
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

// device allocations of one batch's join, freed together
struct DevAllocs {
    kd_ctx* ctx;
    std::vector<void*> ptrs;
    int rc = KD_OK;  // the first failure; nothing is allocated or uploaded after it
    explicit DevAllocs(kd_ctx* c) : ctx(c) {}
    DevAllocs(const DevAllocs&) = delete;
    ~DevAllocs() {
        for (void* p : ptrs) kd_mfree(ctx, p);
    }
    // `bytes` on the device (at least 16), src uploaded into them if given
    void* get(u64 bytes, const void* src = nullptr) {
        void* p = nullptr;
        if (rc) return p;
        rc = kd_malloc(ctx, std::max<u64>(bytes, 16), &p);
        if (!rc) ptrs.push_back(p);
        if (!rc && src && bytes) rc = kd_memcpy(ctx, p, src, bytes, KD_COPY_H2D);
        return p;
    }
};

// the whole device walk's state: what the phases below share
struct DeviceWalk {
    kd_ctx* ctx;
    kd_odb* odb;
    Walk& W;
    int k, cmp0, cmp1, threads, nt;
    uint32_t flags;
    const std::vector<Item>& items;
    std::vector<size_t> task_item;  // the tasks: the subtree items left after the host expansion
    std::vector<u64> task_cost;
    std::vector<u8> on_host;        // [task] the host walks it after all
    std::vector<WalkOut>& outs;
    u64* st;                        // KD_WD_STATS counters
    int64_t read_us[3] = {0, 0, 0}; // the batched reads' plan, host reads + gather, device
};

// one batch: tasks [lo, hi), their trees read into the arena, the join's inputs and results
struct WalkBatch {
    u64 lo, hi;
    std::vector<OidKey> uniq;  // the batch's trees
    kd_blobs arena{};
    std::vector<u8> rstat;     // [uniq] the read's status
    std::vector<u64> off;      // [uniq + 1] the arena's offsets, on the host
    // build_tasks
    std::vector<u64> dtask;    // the device tasks (indices into task_item)
    std::vector<u32> tix;      // [dtask * k] each task's tree per root, or KD_NONE
    std::string pfx;           // each task's path prefix
    std::vector<u64> poff{0};
    u64 cap_n[KMAX] = {0, 0, 0}, cap_b[KMAX] = {0, 0, 0};  // upper bounds of the join's outputs per root
    // run_join / download
    std::vector<u32> cnt;      // [dtask * k] entries kept
    std::vector<u8> jst;       // [dtask] KD_TJ_*
    std::vector<u64> tot;
    std::vector<u8> hpath[KMAX], hoid[KMAX];
    std::vector<u64> hpoff[KMAX];
    std::vector<u32> hmode[KMAX];
};

// what each task costs a batch, by every thread (a locate and an entry header per tree)
void task_costs(DeviceWalk& D) {
    const u64 ntask = D.task_item.size();
    D.task_cost.assign(ntask, 0);
    constexpr u64 CH = 256;
    Readers rds(D.odb, D.nt);
    par_items((ntask + CH - 1) / CH, D.nt, [&](size_t c, int tid) {
        for (u64 t = c * CH; t < std::min(ntask, (c + 1) * CH); t++) {
            const Item& it = D.items[D.task_item[t]];
            for (int r = 0; r < D.k; r++)
                if (it.has[r]) D.task_cost[t] += tree_cost(D.odb, rds[tid], it.oid[r]);
        }
    });
}

// the batch that starts at task lo: tasks up to about batch_bytes of cost, their trees made unique
void cut_batch(const DeviceWalk& D, u64 lo, u64 batch_bytes, WalkBatch& B) {
    B.lo = lo;
    u64 hi = lo, cost = 0;
    for (; hi < D.task_item.size(); hi++) {
        const Item& it = D.items[D.task_item[hi]];
        const u64 c = D.task_cost[hi];
        if (hi > lo && cost + c > batch_bytes) break;
        cost += c;
        for (int r = 0; r < D.k; r++)
            if (it.has[r]) B.uniq.push_back(OidKey(it.oid[r]));
    }
    B.hi = hi;
    std::sort(B.uniq.begin(), B.uniq.end());
    B.uniq.erase(std::unique(B.uniq.begin(), B.uniq.end()), B.uniq.end());
}

// the trees read through the batched device read (expected type: tree)
int read_trees(DeviceWalk& D, WalkBatch& B) {
    const u64 nu = B.uniq.size();
    B.rstat.assign(std::max<u64>(nu, 1), 0);
    ReadStats rs;
    if (int rc = read_batch_device(D.ctx, D.odb, (const u8*)B.uniq.data(), nu, D.threads, D.flags, &B.arena, B.rstat.data(), &rs,
                                   OBJ_TREE, D.read_us))
        return rc;
    D.st[4] += rs.device;
    D.st[5] += rs.host;
    D.st[6] += rs.fixups;
    D.st[7] += rs.compressed;
    D.st[8] += rs.deltas;
    return KD_OK;
}

// device tasks: every tree read, none above KD_INF_MAX, and the join's own bound of 2^31 bytes on a call
// (a batch that large: the rest of it is the host's)
void build_tasks(DeviceWalk& D, WalkBatch& B) {
    u64 bound = 0;
    for (u64 t = B.lo; t < B.hi; t++) {
        const Item& it = D.items[D.task_item[t]];
        u32 ix[KMAX] = {KD_NONE, KD_NONE, KD_NONE};
        bool dev = true;
        u64 tb = 0;
        for (int r = 0; r < D.k; r++) {
            if (!it.has[r]) continue;
            const u64 u = (u64)(std::lower_bound(B.uniq.begin(), B.uniq.end(), OidKey(it.oid[r])) - B.uniq.begin());
            const u64 L = B.off[u + 1] - B.off[u];
            if (B.rstat[u] != 0 || L > KD_INF_MAX) dev = false;
            ix[r] = (u32)u;
            tb += L + (L / 23) * (it.path.size() + 2);
        }
        if (!dev || bound + tb >= (1ull << 31)) {
            D.on_host[t] = 1;
            continue;
        }
        bound += tb;
        for (int r = 0; r < D.k; r++) {
            B.tix.push_back(ix[r]);
            if (ix[r] == KD_NONE) continue;
            const u64 L = B.off[ix[r] + 1] - B.off[ix[r]];
            B.cap_n[r] += L / 23;
            B.cap_b[r] += L + (L / 23) * (it.path.size() + 1);
        }
        B.dtask.push_back(t);
        B.pfx += it.path;
        B.poff.push_back(B.pfx.size());
    }
}

// the join's arrays on the device
struct JoinDev {
    void *tix = nullptr, *pfx = nullptr, *poff = nullptr;  // the task lists, uploaded
    void *cnt = nullptr, *st = nullptr, *tot = nullptr;    // per-task counts and statuses, the totals
    kd_tj_out jo[KMAX];                                    // each root's outputs at their capacities
};

// the join's inputs uploaded, its outputs allocated
int alloc_join(const DeviceWalk& D, const WalkBatch& B, DevAllocs& dev, JoinDev& J) {
    const u64 nd = B.dtask.size();
    J.tix = dev.get(4 * nd * D.k, B.tix.data());
    J.pfx = dev.get(B.pfx.size(), B.pfx.data());
    J.poff = dev.get(8 * (nd + 1), B.poff.data());
    J.cnt = dev.get(4 * nd * D.k);
    J.st = dev.get(nd);
    J.tot = dev.get(16 * KMAX);
    memset(J.jo, 0, sizeof J.jo);
    for (int r = 0; r < D.k; r++) {
        J.jo[r].cap_n = B.cap_n[r];
        J.jo[r].cap_bytes = B.cap_b[r];
        J.jo[r].path_off = (uint64_t*)dev.get(8 * (B.cap_n[r] + 1));
        J.jo[r].mode = (uint32_t*)dev.get(4 * B.cap_n[r]);
        J.jo[r].oid = (uint8_t*)dev.get(20 * B.cap_n[r]);
        J.jo[r].path = (uint8_t*)dev.get(B.cap_b[r]);
    }
    return dev.rc ? dev.rc : kd_sync(D.ctx);  // (the uploads read pageable vectors)
}

// the join in HBM, its totals, counts and statuses back (the kernels and three small copies behind them)
int run_join(const DeviceWalk& D, WalkBatch& B, JoinDev& J) {
    const u64 nd = B.dtask.size();
    int rc = kd_tree_join_batch(D.ctx, B.arena.data, B.arena.off, B.uniq.size(), (const u32*)J.tix, (const u8*)J.pfx,
                                (const u64*)J.poff, nd, D.k, D.cmp0, D.cmp1, J.jo, (u32*)J.cnt, (u8*)J.st, (u64*)J.tot, KD_MEM_DEVICE);
    if (!rc) rc = kd_memcpy(D.ctx, B.tot.data(), J.tot, 16 * D.k, KD_COPY_D2H);
    if (!rc) rc = kd_memcpy(D.ctx, B.cnt.data(), J.cnt, 4 * nd * D.k, KD_COPY_D2H);
    if (!rc) rc = kd_memcpy(D.ctx, B.jst.data(), J.st, nd, KD_COPY_D2H);
    if (!rc) rc = kd_sync(D.ctx);
    return rc;
}

// what the join kept, back on the host.  rc: what the steps before gave; after a failure nothing is copied,
// but the stream is still drained before the join's arrays are freed
int download(const DeviceWalk& D, WalkBatch& B, const kd_tj_out* jo, int rc) {
    for (int r = 0; r < D.k && !rc; r++) {
        const u64 n = B.tot[2 * r], nbytes = B.tot[2 * r + 1];
        if (n > B.cap_n[r] || nbytes > B.cap_b[r]) {  // (the capacities are upper bounds)
            kd::set_error("kd_walk_device: the join kept more than its trees hold");
            rc = KD_EINVAL;
            break;
        }
        B.hpoff[r].resize(n + 1);
        B.hmode[r].resize(n);
        B.hoid[r].resize(20 * n);
        B.hpath[r].resize(nbytes);
        rc = kd_memcpy(D.ctx, B.hpoff[r].data(), jo[r].path_off, 8 * (n + 1), KD_COPY_D2H);
        if (!rc && n) rc = kd_memcpy(D.ctx, B.hmode[r].data(), jo[r].mode, 4 * n, KD_COPY_D2H);
        if (!rc && n) rc = kd_memcpy(D.ctx, B.hoid[r].data(), jo[r].oid, 20 * n, KD_COPY_D2H);
        if (!rc && nbytes) rc = kd_memcpy(D.ctx, B.hpath[r].data(), jo[r].path, nbytes, KD_COPY_D2H);
    }
    if (!rc) rc = kd_sync(D.ctx);
    else kd_sync(D.ctx);
    return rc;
}

// a device task's entries into its item's outputs (a refused task is the host's)
void stitch_batch(DeviceWalk& D, WalkBatch& B) {
    const u64 nd = B.dtask.size();
    const int k = D.k;
    for (int r = 0; r < k; r++) {
        std::vector<u64> first(nd + 1, 0);
        for (u64 j = 0; j < nd; j++) first[j + 1] = first[j] + B.cnt[j * k + r];
        par_items(nd, D.nt, [&](size_t j, int) {
            if (B.jst[j] != KD_TJ_OK || !B.cnt[j * k + r]) return;
            WalkOut& o = D.outs[D.task_item[B.dtask[j]] * k + r];
            const u64 e0 = first[j], e1 = first[j + 1], b0 = B.hpoff[r][e0];
            o.path.assign((const char*)B.hpath[r].data() + b0, B.hpoff[r][e1] - b0);
            o.end.resize(e1 - e0);
            for (u64 e = e0; e < e1; e++) o.end[e - e0] = B.hpoff[r][e + 1] - b0;
            o.oid.assign(B.hoid[r].begin() + 20 * e0, B.hoid[r].begin() + 20 * e1);
            o.mode.assign(B.hmode[r].begin() + e0, B.hmode[r].begin() + e1);
        });
    }
    for (u64 j = 0; j < nd; j++)
        if (B.jst[j] != KD_TJ_OK) D.on_host[B.dtask[j]] = 1;
}

// one batch from its first task `lo`; *next <- the first task behind it
int run_batch(DeviceWalk& D, u64 lo, u64 batch_bytes, u64* next) {
    u64* st = D.st;
    auto t0 = Clock::now();
    WalkBatch B;
    cut_batch(D, lo, batch_bytes, B);
    st[3] += B.uniq.size();
    st[9]++;
    st[11] += (u64)us_since(t0);
    t0 = Clock::now();
    const int64_t read_before = D.read_us[0] + D.read_us[1] + D.read_us[2];
    if (int rc = read_trees(D, B)) return rc;
    B.off.resize(B.uniq.size() + 1);
    int rc = kd_memcpy(D.ctx, B.off.data(), B.arena.off, 8 * B.off.size(), KD_COPY_D2H);
    if (!rc) rc = kd_sync(D.ctx);
    st[17] += (u64)std::max<int64_t>(0, us_since(t0) - ((D.read_us[0] + D.read_us[1] + D.read_us[2]) - read_before));  // (the offsets back)
    t0 = Clock::now();
    if (!rc) build_tasks(D, B);
    const u64 nd = B.dtask.size();
    B.cnt.assign(std::max<u64>(nd * D.k, 1), 0);
    B.jst.assign(std::max<u64>(nd, 1), 0);
    B.tot.assign(2 * KMAX, 0);
    if (!rc && nd) {
        DevAllocs dev(D.ctx);
        JoinDev J;
        rc = alloc_join(D, B, dev, J);
        st[15] += (u64)us_since(t0);
        t0 = Clock::now();
        if (!rc) rc = run_join(D, B, J);
        st[16] += (u64)us_since(t0);
        t0 = Clock::now();
        rc = download(D, B, J.jo, rc);
    }
    kd_mfree(D.ctx, (void*)B.arena.data);
    kd_mfree(D.ctx, (void*)B.arena.off);
    st[17] += (u64)us_since(t0);
    if (rc) return rc;
    t0 = Clock::now();
    stitch_batch(D, B);
    st[18] += (u64)us_since(t0);
    *next = B.hi;
    return KD_OK;
}

}  // namespace
}  // namespace kd_store

extern "C" int kd_walk_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1,
                              int threads, int depth, uint32_t flags, kd_leaves** out, uint64_t* stats) {
    if (!ctx || depth < 0 || depth > 64) { kd::set_error("kd_walk_device: bad arguments"); return KD_EINVAL; }
    if (int rc = check_walk_args("kd_walk_device", odb, roots, k, cmp0, cmp1, out)) return rc;
    if (flags & ~KD_RBD_DELTAS) { kd::set_error("kd_walk_device: unknown flags %u", flags); return KD_EINVAL; }
    for (int r = 0; r < k; r++) out[r] = nullptr;
    u64 st[KD_WD_STATS];
    memset(st, 0, sizeof st);
    const int nt = default_threads(threads);
    Walk W(k, cmp0, cmp1);
    Reader rd0(odb);
    Item top;
    const auto t_call = Clock::now();
    auto t0 = Clock::now();
    if (int rc = walk_top(rd0, roots, k, subpath, "kd_walk_device", top)) return rc;
    // ---- host expansion: `depth` levels below the walked tree, breadth-first, pruned ----
    std::vector<Item> items = walk_start(W, top);
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
    DeviceWalk D{ctx, odb, W, k, cmp0, cmp1, threads, nt, flags, items, {}, {}, {}, outs, st};
    for (size_t i = 0; i < items.size(); i++) {
        if (items[i].tree) D.task_item.push_back(i);
        else W.emit(items[i], &outs[i * k]);
    }
    const u64 ntask = D.task_item.size();
    st[0] = ntask;
    D.on_host.assign(ntask, 0);
    u64 batch_bytes;
    {
        std::lock_guard<std::mutex> lk(odb->dev_mu);
        batch_bytes = odb->walk_batch_bytes;
    }
    t0 = Clock::now();
    task_costs(D);
    st[11] += (u64)us_since(t0);
    for (u64 lo = 0; lo < ntask;)
        if (int rc = run_batch(D, lo, batch_bytes, &lo)) return rc;
    // ---- host-class tasks: the existing walk of the item ----
    t0 = Clock::now();
    std::vector<size_t> hostq;
    for (u64 t = 0; t < ntask; t++)
        if (D.on_host[t]) hostq.push_back(D.task_item[t]);
    st[2] = hostq.size();
    st[1] = ntask - hostq.size();
    walk_items(odb, W, items, hostq, outs, nt);
    st[19] = (u64)us_since(t0);
    if (W.err) {
        kd::set_error("kd_walk_device: %s", W.emsg.c_str());
        return W.err.load();
    }
    t0 = Clock::now();
    int rc = walk_stitch(items, outs, k, top, nt, "kd_walk_device", out);
    st[18] += (u64)us_since(t0);
    st[12] = (u64)D.read_us[0];
    st[13] = (u64)D.read_us[1];
    st[14] = (u64)D.read_us[2];
    st[20] = (u64)us_since(t_call);  // the whole call: what [10..19] leave of it is vectors built and freed, allocations
    if (!rc && stats) memcpy(stats, st, sizeof st);
    return rc;
}
