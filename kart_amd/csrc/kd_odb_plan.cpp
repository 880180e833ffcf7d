// kd_odb_plan.cpp — the plan of the batched device read, phase by phase (kd_odb_plan.h).  Host code only:
// pack arithmetic, the Reader for entry headers, header peeks and host-class reads.
#include "kd_odb_plan.h"

namespace kd_store {

namespace {

constexpr u64 CH = 256;  // requests (or entries) per parallel task
inline u64 chunks(u64 n) { return (n + CH - 1) / CH; }

// the entries of the chain above pack p's entry at o, listed by the thread that meets them first (a
// thread stops walking up at an entry it has already listed: chains share their tails)
void discover(const Batch& b, Reader& rd, long p, u64 o, std::unordered_set<u64>& seen, std::vector<DlNode>& recs) {
    const Pack& pk = *b.odb->packs[p];
    u64 cur = o;
    for (int hop = 0; hop < MAX_CHAIN; hop++) {
        DlNode nd;
        nd.key = pack_key(p, cur);
        if (!seen.insert(nd.key).second) return;
        int t;
        u64 sz, data, boff = 0;
        const u8* boid = nullptr;
        if (cur >= (1ull << 48) || rd.entry_header(pk, cur, &t, &sz, &data, &boff, &boid) != RD_OK || data >= pk.pack.n - 20 ||
            sz > KD_INF_MAX) {
            nd.bad = 1;
            recs.push_back(nd);
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
            nd.bad = t != b.want_type;
            recs.push_back(nd);
            return;
        }
        nd.delta = 1;
        if (!nd.bad) nd.pkey = pack_key(p, cur);
        recs.push_back(nd);
        if (nd.bad) return;
    }
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

// One peek's output, kept together and on cache lines of its own.  The loop is sensitive to where these 36 bytes
// lie in its frame: as three plain locals (`u8 hb[20]`, got, pos) where the compiler first put them, the peek
// phase of 1.05M entries took 33 ms on 16 threads; in this struct it takes 16 ms, against the 12-14 ms of the same
// loop before it was moved here (profiles/odb_split/).  Why is not known, nor where the last 2 ms go: moving the
// buffer 512 bytes along the stack, or merely grouping the three in an unaligned struct, had the same effect in
// a host-only test, so the alignment is a way of pinning the placement down, not a claim about the cause.
struct alignas(64) PeekScratch {
    u8 hb[20];
    size_t got = 0;
    u64 pos = 0;
};

u32 find_node(const std::vector<DlNode>& nodes, u64 key) {
    auto it = std::lower_bound(nodes.begin(), nodes.end(), key, [](const DlNode& a, u64 k) { return a.key < k; });
    return it != nodes.end() && it->key == key ? (u32)(it - nodes.begin()) : ~0u;
}

// every thread's list sorted on its own, the lists merged pairwise, duplicates dropped -> nodes in key order
// (the keys are sorted, not the entries: 16 bytes move per comparison instead of a whole DlNode)
void merge_unique(const std::vector<std::vector<DlNode>>& recs, int nt, std::vector<DlNode>& nodes) {
    std::vector<std::pair<u64, const DlNode*>> ks;
    std::vector<size_t> seg{0};
    for (auto& v : recs) {
        for (const DlNode& nd : v) ks.push_back({nd.key, &nd});
        seg.push_back(ks.size());
    }
    auto less = [](const auto& x, const auto& y) { return x.first < y.first; };
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
    ks.erase(std::unique(ks.begin(), ks.end(), [](const auto& x, const auto& y) { return x.first == y.first; }), ks.end());
    nodes.resize(ks.size());
    par_items(chunks(ks.size()), nt, [&](size_t c, int) {
        for (u64 k = c * CH; k < std::min<u64>(ks.size(), (c + 1) * CH); k++) nodes[k] = *ks[k].second;
    });
}

// levels and `ok`, every chain decided from its root down (each entry once)
void decide_chains(std::vector<DlNode>& nodes) {
    const u64 nn = nodes.size();
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
}

}  // namespace

void classify_requests(const Batch& b, Readers& rds, std::vector<DevItem>& it, ChainLists& ch) {
    it.assign(b.n, DevItem{});
    ch.recs.assign(b.deltas ? b.nt : 0, {});
    ch.seen.assign(b.deltas ? b.nt : 0, {});
    par_items(chunks(b.n), b.nt, [&](size_t c, int tid) {
        Reader& rd = rds[tid];
        for (u64 i = c * CH; i < std::min(b.n, (c + 1) * CH); i++) {
            u64 o;
            const long p = rd.locate(b.oids + 20 * i, &o);
            if (p < 0 || p >= 0xFFFF || o >= (1ull << 48)) continue;
            it[i].key = pack_key(p, o);
            int type;
            u64 size, data, boff = 0;
            const u8* boid = nullptr;
            const Pack& pk = *b.odb->packs[p];
            if (rd.entry_header(pk, o, &type, &size, &data, &boff, &boid) != RD_OK) continue;
            if (type == b.want_type && size <= KD_INF_MAX && data < pk.pack.n - 20) {
                it[i].cls = CLS_STREAM;
                it[i].data = data;
                it[i].size = size;
            } else if (b.deltas && (type == OBJ_OFS_DELTA || type == OBJ_REF_DELTA)) {
                it[i].cls = CLS_DELTA;
                discover(b, rd, p, o, ch.seen[tid], ch.recs[tid]);
            }
        }
    });
}

void build_forest(const Batch& b, Readers& rds, const ChainLists& ch, Forest& f) {
    std::vector<DlNode>& nodes = f.nodes;
    merge_unique(ch.recs, b.nt, nodes);
    const u64 nn = nodes.size();
    // a delta's result size and its base's are the two varints at the front of its inflated payload
    const auto t_peek = Clock::now();
    par_items(chunks(nn), b.nt, [&](size_t c, int tid) {
        Reader& rd = rds[tid];
        for (u64 k = c * CH; k < std::min(nn, (c + 1) * CH); k++) {
            DlNode& nd = nodes[k];
            if (!nd.delta || nd.bad) continue;
            nd.parent = find_node(nodes, nd.pkey);
            const Pack& pk = *b.odb->packs[key_pack(nd.key)];
            PeekScratch s;
            if (nd.parent == ~0u ||
                !peek_stream(rd, pk.pack.p + nd.data, pk.pack.n - 20 - nd.data, s.hb, (size_t)std::min<u64>(20, nd.zsize), &s.got) ||
                !kd_dl::size_varint(s.hb, s.got, &s.pos, &nd.bsize) || !kd_dl::size_varint(s.hb, s.got, &s.pos, &nd.rsize) ||
                nd.rsize > KD_INF_MAX)
                nd.bad = 1;
        }
    });
    f.peek_us = us_since(t_peek);
    decide_chains(nodes);
    f.par.resize(nn);
    for (u64 k = 0; k < nn; k++) f.par[k] = nodes[k].parent;
}

void resolve_requests(const Batch& b, const Forest& f, std::vector<DevItem>& it) {
    par_items(chunks(b.n), b.nt, [&](size_t c, int) {
        for (u64 i = c * CH; i < std::min(b.n, (c + 1) * CH); i++) {
            if (it[i].cls == CLS_HOST) continue;
            it[i].node = find_node(f.nodes, it[i].key);
            if (it[i].cls == CLS_DELTA) {
                if (it[i].node != ~0u && f.nodes[it[i].node].ok) it[i].size = f.nodes[it[i].node].rsize;
                else it[i].cls = CLS_HOST;  // the host route gives it its bytes or its status
            }
        }
    });
}

// host class: read by the Reader, threaded and in pack order (as kd_odb_read_batch reads)
void read_host_class(const Batch& b, Readers& rds, std::vector<DevItem>& it, u8* status, PassPlan& p) {
    std::vector<std::pair<u64, u64>> ord;
    for (u64 i = 0; i < b.n; i++)
        if (it[i].cls == CLS_HOST) ord.push_back({it[i].key, i});
    std::sort(ord.begin(), ord.end());
    const u64 nh = ord.size();
    p.n_host = nh;
    p.part.assign(chunks(nh), {});
    p.at.assign(b.n, 0);
    p.chunk_of.assign(b.n, 0);
    par_items(chunks(nh), b.nt, [&](size_t c, int tid) {
        Reader& rd = rds[tid];
        std::vector<u8> buf;
        for (u64 s = c * CH; s < std::min(nh, (c + 1) * CH); s++) {
            const u64 key = ord[s].first, i = ord[s].second;
            int type = 0;
            const int rc = key != KEY_NONE ? rd.read_packed(*b.odb->packs[key_pack(key)], key_off(key), &type, buf)
                                           : rd.read(b.oids + 20 * i, &type, buf);
            status[i] = rc == RD_OK && type != b.want_type ? 2 : (u8)rc;
            if (status[i]) buf.clear();
            p.at[i] = p.part[c].size();
            p.chunk_of[i] = (u32)c;
            p.part[c].insert(p.part[c].end(), buf.begin(), buf.end());
            it[i].size = buf.size();
        }
    });
}

// sizes -> off; launch 1's source offsets (a stream's span is clipped to the pack's trailer)
void layout_arena(const Batch& b, const std::vector<DevItem>& it, PassPlan& p) {
    const u64 n = b.n;
    p.off.resize(n + 1);
    p.soff.resize(n + 1);
    p.kind1.resize(n);
    p.off[0] = p.soff[0] = 0;
    p.n_stream = p.n_delta = p.compressed = 0;
    for (u64 i = 0; i < n; i++) {
        u64 span = it[i].size;  // host class: its bytes, raw
        if (it[i].cls == CLS_STREAM) {
            const Pack& pk = *b.odb->packs[key_pack(it[i].key)];
            span = std::min(inf_bound(it[i].size), pk.pack.n - 20 - it[i].data);
            p.n_stream++;
            p.compressed += span;
        } else if (it[i].cls == CLS_DELTA) {
            span = 0;  // (rebuilt by k_dl_apply: a raw item without a source, which the inflate launch leaves alone)
            p.n_delta++;
        }
        p.kind1[i] = it[i].cls != CLS_STREAM;
        p.off[i + 1] = p.off[i] + it[i].size;
        p.soff[i + 1] = p.soff[i] + span;
    }
    p.dstat.resize(n);
}

namespace {

// Needed entries: every delta-class request's chain.  An entry's home is the first request that names
// it; a later delta-class request of it is a copy of its home
void mark_needed(const Batch& b, const std::vector<DevItem>& it, const Forest& f, PassPlan& p) {
    p.need.assign(f.nodes.size(), 0);
    p.home.assign(f.nodes.size(), -1);
    p.copy_req.clear();
    for (u64 i = 0; i < b.n; i++) {
        if (it[i].cls != CLS_DELTA) continue;
        for (u32 k = it[i].node; k != ~0u && !p.need[k]; k = f.par[k]) p.need[k] = 1;
    }
    for (u64 i = 0; i < b.n; i++) {
        if (it[i].cls == CLS_HOST || it[i].node == ~0u || !p.need[it[i].node]) continue;
        int64_t& h = p.home[it[i].node];
        if (h < 0) h = (int64_t)i;
        else if (it[i].cls == CLS_DELTA) p.copy_req.push_back({i, (u64)h});
    }
}

// launch 2's items: unrequested chain bases, then every payload, all into workspace.  Entries are taken
// in key order, which is pack order: neighbours in a launch are neighbours in the pack
void layout_launch2(const Batch& b, Forest& f, PassPlan& p) {
    std::vector<DlNode>& nodes = f.nodes;
    const u64 nn = nodes.size();
    p.wsitem.clear();
    p.depth = 0;
    for (u64 k = 0; k < nn; k++)
        if (p.need[k] && !nodes[k].delta && p.home[k] < 0) p.wsitem.push_back((u32)k);
    p.n_base = p.wsitem.size();
    for (u64 k = 0; k < nn; k++)
        if (p.need[k] && nodes[k].delta) {
            p.wsitem.push_back((u32)k);
            p.depth = std::max(p.depth, nodes[k].level);
        }
    const u64 m = p.m = p.wsitem.size();
    p.soff2.assign(m + 1, 0);
    p.woff.assign(m + 1, 0);
    for (u64 j = 0; j < m; j++) {
        DlNode& nd = nodes[p.wsitem[j]];
        const Pack& pk = *b.odb->packs[key_pack(nd.key)];
        p.soff2[j + 1] = p.soff2[j] + std::min(inf_bound(nd.zsize), pk.pack.n - 20 - nd.data);
        p.woff[j + 1] = p.woff[j] + nd.zsize;
        if (j < p.n_base) {
            nd.in_ws = 1;
            nd.at = p.woff[j];
            nd.st = (u32)(b.n + j);
        } else {
            nd.pay = p.woff[j];
            nd.pst = (u32)(b.n + j);
        }
    }
    p.compressed += p.soff2[m];
    p.ws_bytes = p.woff[m];
}

// the delta entries in level order, each result at its home in the arena or (nobody requested it) behind
// launch 2's results in workspace; -> the entries in that order
std::vector<u32> place_results(const Batch& b, Forest& f, PassPlan& p) {
    std::vector<DlNode>& nodes = f.nodes;
    const u64 nd_items = p.m - p.n_base;
    p.level_start.assign(p.depth + 2, 0);
    for (u64 j = p.n_base; j < p.m; j++) p.level_start[nodes[p.wsitem[j]].level + 1]++;
    for (u32 l = 1; l <= p.depth + 1; l++) p.level_start[l] += p.level_start[l - 1];
    std::vector<u64> fill(p.level_start.begin(), p.level_start.end());
    std::vector<u32> order(nd_items);
    for (u64 j = p.n_base; j < p.m; j++) order[fill[nodes[p.wsitem[j]].level]++] = p.wsitem[j];
    for (u64 j = 0; j < order.size(); j++) {
        DlNode& nd = nodes[order[j]];
        nd.st = (u32)(b.n + p.m + j);
        nd.in_ws = p.home[order[j]] < 0;
        if (nd.in_ws) {
            nd.at = p.ws_bytes;
            p.ws_bytes += nd.rsize;
        } else {
            nd.at = p.off[p.home[order[j]]];
        }
    }
    for (u64 k = 0; k < nodes.size(); k++)
        if (p.need[k] && !nodes[k].delta && p.home[k] >= 0) {  // a requested chain base: launch 1 inflates it
            nodes[k].in_ws = 0;
            nodes[k].at = p.off[p.home[k]];
            nodes[k].st = (u32)p.home[k];
        }
    // level_start as delta_read_from_host takes it: [l - 1] .. [l] is level l
    p.level_start.erase(p.level_start.begin());
    return order;
}

}  // namespace

void layout_deltas(const Batch& b, const std::vector<DevItem>& it, Forest& f, PassPlan& p) {
    mark_needed(b, it, f, p);
    layout_launch2(b, f, p);
    const std::vector<u32> order = place_results(b, f, p);
    p.items.assign(order.size(), kd::DlItem{});
    for (u64 j = 0; j < order.size(); j++) {
        const DlNode& nd = f.nodes[order[j]];
        const DlNode& pa = f.nodes[nd.parent];
        kd::DlItem& d = p.items[j];
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
    p.copies.resize(p.copy_req.size());
    for (u64 j = 0; j < p.copy_req.size(); j++) {
        const CopyReq& c = p.copy_req[j];
        p.copies[j] = {p.off[c.home], p.off[c.req], it[c.req].size, 0, 0};  // (a home is in the arena)
    }
    p.hst.assign(b.n + p.m + p.items.size(), 0);
}

// every source into the staging (8 bytes of padding behind the last).  It holds every source of the call at
// once: about the arena's size (chunking it through two buffers would bound it)
void gather(const Batch& b, const std::vector<DevItem>& it, const Forest& f, const PassPlan& p, u8* staging) {
    par_items(chunks(b.n), b.nt, [&](size_t c, int) {
        for (u64 i = c * CH; i < std::min(b.n, (c + 1) * CH); i++) {
            const u64 len = p.soff[i + 1] - p.soff[i];
            if (!len) continue;
            if (it[i].cls == CLS_STREAM) memcpy(staging + p.soff[i], b.odb->packs[key_pack(it[i].key)]->pack.p + it[i].data, len);
            else memcpy(staging + p.soff[i], p.part[p.chunk_of[i]].data() + p.at[i], len);
        }
    });
    if (b.deltas) {
        u8* src2 = staging + p.soff[b.n];
        par_items(chunks(p.m), b.nt, [&](size_t c, int) {
            for (u64 j = c * CH; j < std::min(p.m, (c + 1) * CH); j++) {
                const DlNode& nd = f.nodes[p.wsitem[j]];
                memcpy(src2 + p.soff2[j], b.odb->packs[key_pack(nd.key)]->pack.p + nd.data, p.soff2[j + 1] - p.soff2[j]);
            }
        });
    }
    memset(staging + p.src_bytes(), 0, 8);
}

void request_status(const Batch& b, const std::vector<DevItem>& it, const Forest& f, PassPlan& p) {
    for (u64 i = 0; i < b.n; i++) p.dstat[i] = it[i].cls == CLS_DELTA ? p.hst[f.nodes[it[i].node].st] : p.hst[i];
}

kd::DlPlan PassPlan::dl_plan() {
    kd::DlPlan pl{};
    pl.n = kind1.size();
    pl.soff1 = soff.data();
    pl.kind1 = kind1.data();
    pl.off = off.data();
    pl.m = m;
    pl.soff2 = soff2.data();
    pl.woff = woff.data();
    pl.ws_bytes = ws_bytes;
    pl.items = items.data();
    pl.n_items = items.size();
    pl.level_start = level_start.data();
    pl.depth = depth;
    pl.copies = copies.data();
    pl.n_copies = copies.size();
    pl.h_status = hst.data();
    return pl;
}

}  // namespace kd_store
