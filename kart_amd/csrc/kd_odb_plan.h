// kd_odb_plan.h — the host-only half of the batched device read (library internal): where every request's
// bytes come from and where on the device they go, as plain arithmetic over the mapped packs.
//
// kd_odb_devread.cpp carries a plan out (kd_inflate.hip, kd_delta.hip); tests/odb_plan_host_check.cpp
// carries the same plan out on the CPU under the sanitizers, in heap blocks of exactly the planned sizes.
// Nothing here touches a device: every range k_inf_streams and k_dl_apply read or write is laid out here
// and can be checked before anything is launched.
//
// One call plans in this order (the parallel loops are par_items over chunks of 256):
//   classify_requests   every id located, its entry header parsed, its class decided; with KD_RBD_DELTAS the
//                       entries of every requested delta's chain are listed per thread
//   build_forest        those lists sorted, merged and made unique; parents linked, the size varints at the
//                       front of each payload peeked, levels and `ok` decided            -> Forest
//   resolve_requests    request -> node; a delta request whose chain is not `ok` becomes host class
// and then once per pass (a second pass only after an item failed on the device and on the host):
//   read_host_class     the host-class requests read by the Reader, threaded and in pack order
//   layout_arena        off, soff, kind1 (what k_inf_streams takes)
//   layout_deltas       need, home, launch 2's items and the workspace, the items in level order, the copies
//   gather              every source into the staging
#pragma once
#include <unordered_set>
#include <vector>

#include "kd_delta.h"
#include "kd_odb_store.h"

namespace kd_store {

// a request's class: who produces its bytes
enum Cls : u8 {
    CLS_HOST = 0,    // the Reader; its bytes travel as a raw item
    CLS_STREAM = 1,  // a plain packed entry of the wanted type: one zlib stream for k_inf_streams
    CLS_DELTA = 2,   // (KD_RBD_DELTAS) a delta entry whose whole chain can be rebuilt by k_dl_apply
};

// what one call reads
struct Batch {
    const kd_odb* odb;
    const u8* oids;  // [20 n]
    u64 n;
    int nt;          // threads
    int want_type;   // OBJ_BLOB, or OBJ_TREE for kd_walk_device's leaf trees
    bool deltas;     // KD_RBD_DELTAS
};

struct DevItem {
    u64 key = KEY_NONE;  // pack_key, or KEY_NONE: read by id
    u64 data = 0;        // CLS_STREAM: where the stream starts in its pack
    u64 size = 0;        // inflated size (host class: what the read gave)
    u8 cls = CLS_HOST;   // fixed while a pass is planned and run; an item that failed on the device and on the
                         // host is demoted to CLS_HOST for the second pass
    u32 node = ~0u;      // KD_RBD_DELTAS: the entry's node in the delta forest, if it is one
};

// One entry of the delta forest: a requested delta, or an ancestor of one (KD_RBD_DELTAS).
struct DlNode {
    u64 key = KEY_NONE;   // pack_key
    u64 pkey = KEY_NONE;  // the base's key (KEY_NONE: a plain entry, the chain's root)
    u64 data = 0;         // where the stream starts in its pack
    u64 zsize = 0;        // the stream's inflated size (entry header)
    u64 rsize = 0;        // the object's size
    u64 bsize = 0;        // a delta: the base size its payload states
    u32 parent = ~0u;
    u32 level = 0;        // 0 for the plain base
    u8 delta = 0;
    u8 bad = 0;           // cannot be rebuilt on the device (the reason is the host route's to find)
    u8 ok = 0;            // this entry and its whole chain can
    // per pass (layout_deltas)
    u8 in_ws = 0;         // the result lives in workspace (nobody requested it)
    u64 at = 0;           // where the result is (arena or workspace) and where the payload is (workspace)
    u64 pay = 0;
    u32 st = 0, pst = 0;  // status indices of the result and of the payload
};

// KD_RBD_DELTAS: what the threads of classify_requests found walking up the requested deltas' chains.  It
// lives until the call ends (tearing down 1.6M set entries costs as much as a phase, and no phase pays it)
struct ChainLists {
    std::vector<std::unordered_set<u64>> seen;  // per thread: the keys it has listed
    std::vector<std::vector<DlNode>> recs;      // per thread: the entries, in the order met
};

struct Forest {
    std::vector<DlNode> nodes;  // unique entries in key order (which is pack order)
    std::vector<u32> par;       // every entry's parent, apart from the entries (the walk up a chain touches nothing else)
    int64_t peek_us = 0;        // the header peeks' share of build_forest
};

// a further request of an entry that already has a home: request `req` is a copy of request `home`
struct CopyReq {
    u64 req, home;
};

// One pass's plan.  The vectors keep their storage from pass to pass.
struct PassPlan {
    // read_host_class: request i's bytes are part[chunk_of[i]] at at[i], it[i].size of them
    u64 n_host = 0;
    std::vector<std::vector<u8>> part;
    std::vector<u64> at;
    std::vector<u32> chunk_of;
    // layout_arena
    std::vector<u64> off, soff;  // [n + 1] the arena's offsets; launch 1's source offsets in the staging
    std::vector<u8> kind1;       // [n] what k_inf_streams takes: 0 a zlib stream, 1 raw bytes (none for CLS_DELTA)
    u64 n_stream = 0, n_delta = 0;
    u64 compressed = 0;          // source bytes of every zlib stream shipped (both launches)
    // layout_deltas (all empty or 0 without KD_RBD_DELTAS)
    std::vector<u8> need;         // [nodes] the entry is on a delta-class request's chain
    std::vector<int64_t> home;    // [nodes] the first request that names the entry, or -1
    std::vector<u32> wsitem;      // [m] launch 2's entries: n_base unrequested chain bases, then every payload
    u64 n_base = 0, m = 0;
    std::vector<u64> soff2, woff; // [m + 1] launch 2's sources (behind launch 1's) and workspace offsets
    u64 ws_bytes = 0;             // launch 2's results, then the unrequested delta results
    std::vector<kd::DlItem> items;    // in level order
    std::vector<u64> level_start;     // [depth + 1]: items[level_start[l - 1] .. level_start[l]) is level l
    u32 depth = 0;
    std::vector<CopyReq> copy_req;
    std::vector<kd::DlCopy> copies;   // copy_req as the device takes it
    std::vector<u8> hst;              // [n + m + items] every device status of the pass
    // after the pass ran
    std::vector<u8> dstat;  // [n] each request's device status: its own inflate's, or its entry's after the levels

    // the staging: launch 1's sources, launch 2's, 8 bytes of padding
    u64 src_bytes() const { return soff.back() + (soff2.empty() ? 0 : soff2.back()); }
    u64 staging_bytes() const { return src_bytes() + 8; }
    // the plan as kd_delta.hip takes it, minus h_src and the device pointers
    kd::DlPlan dl_plan();
};

void classify_requests(const Batch& b, Readers& rds, std::vector<DevItem>& it, ChainLists& ch);
void build_forest(const Batch& b, Readers& rds, const ChainLists& ch, Forest& f);
void resolve_requests(const Batch& b, const Forest& f, std::vector<DevItem>& it);

void read_host_class(const Batch& b, Readers& rds, std::vector<DevItem>& it, u8* status, PassPlan& p);
void layout_arena(const Batch& b, const std::vector<DevItem>& it, PassPlan& p);
void layout_deltas(const Batch& b, const std::vector<DevItem>& it, Forest& f, PassPlan& p);
// staging: p.staging_bytes() bytes
void gather(const Batch& b, const std::vector<DevItem>& it, const Forest& f, const PassPlan& p, u8* staging);

// KD_RBD_DELTAS, after the pass ran: p.hst -> p.dstat
void request_status(const Batch& b, const std::vector<DevItem>& it, const Forest& f, PassPlan& p);

}  // namespace kd_store
