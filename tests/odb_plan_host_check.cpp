// odb_plan_host_check — the batched device read's plan (kart_amd/csrc/kd_odb_plan.cpp) made, checked and
// carried out on the CPU, for a sanitizer build (tests/test_odb_plan_host.py):
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I kart_amd/csrc
//       tests/odb_plan_host_check.cpp kart_amd/csrc/kd_odb.cpp kart_amd/csrc/kd_odb_plan.cpp -lz -ldl -pthread
//
// usage: odb_plan_host_check <gitdir> <ids> <out>
// ids:   20-byte object ids, one after the other.
// out:   three sections, little-endian.  One per plan, first with KD_RBD_DELTAS, then without:
//          u64 counters[8] (device, host, compressed, fixups, deltas, links, depth, scratch), u64 passes,
//          then per request u8 class (the last pass's), u8 status, u64 length, the bytes.
//        Then what Reader::read gives for every id: u8 result (0 ok, 1 missing, 2 corrupt), u8 type,
//        u64 length, the bytes.
//
// Each plan goes through what kd_odb_devread.cpp does with it, with the device replaced by the host: the
// staging, the arena and the workspace are heap blocks of exactly the planned sizes, zlib runs the two
// inflate launches over exactly the planned source spans, kd_delta.h's next_op with memcpy runs the levels,
// then the copies.  Before anything runs, the plan's own invariants are checked (check_plan): a violation
// prints what failed and exits with 3.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "kd_odb_plan.h"

using namespace kd_store;

namespace kd {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace kd
extern "C" int kd_host_alloc(uint64_t bytes, void** hptr) {
    *hptr = malloc(bytes);
    return *hptr ? KD_OK : KD_EINVAL;
}
extern "C" int kd_host_free(void* hptr) {
    free(hptr);
    return KD_OK;
}

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "plan invariant failed: %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fputc('\n', stderr);                                  \
            exit(3);                                              \
        }                                                         \
    } while (0)

struct Span {
    u64 at, len;
    bool operator<(const Span& o) const { return at < o.at; }
};

// nonempty ranges pairwise disjoint and inside [0, total)
static void check_disjoint(std::vector<Span> v, u64 total, const char* what) {
    std::sort(v.begin(), v.end());
    u64 end = 0;
    for (const Span& s : v) {
        CHECK(s.at >= end, "%s: a range at %llu overlaps the one before (ends at %llu)", what, (unsigned long long)s.at, (unsigned long long)end);
        CHECK(s.len <= total && s.at <= total - s.len, "%s: a range at %llu + %llu leaves %llu", what, (unsigned long long)s.at,
              (unsigned long long)s.len, (unsigned long long)total);
        end = s.at + s.len;
    }
}

static void check_plan(const Batch& b, const std::vector<DevItem>& it, const Forest& f, const PassPlan& p) {
    const u64 n = b.n, arena = p.off[n];
    CHECK(p.off.size() == n + 1 && p.soff.size() == n + 1 && p.kind1.size() == n, "launch 1 arrays");
    std::vector<Span> wa, ww;  // what is written in the arena and in the workspace
    for (u64 i = 0; i < n; i++) {
        CHECK(p.off[i + 1] == p.off[i] + it[i].size && p.soff[i + 1] >= p.soff[i], "request %llu", (unsigned long long)i);
        CHECK(p.kind1[i] == (it[i].cls != CLS_STREAM), "kind1 of request %llu", (unsigned long long)i);
        const u64 span = p.soff[i + 1] - p.soff[i];
        if (it[i].cls == CLS_HOST) CHECK(span == it[i].size, "raw request %llu ships %llu of %llu bytes", (unsigned long long)i, (unsigned long long)span, (unsigned long long)it[i].size);
        if (it[i].cls == CLS_STREAM) {  // gather reads the span from the mapped pack, which no sanitizer watches
            const Pack& pk = *b.odb->packs[key_pack(it[i].key)];
            CHECK(it[i].data < pk.pack.n - 20 && span <= pk.pack.n - 20 - it[i].data, "stream request %llu: its span leaves the pack", (unsigned long long)i);
        }
        if (it[i].cls == CLS_DELTA) CHECK(span == 0 && b.deltas, "delta request %llu has a source", (unsigned long long)i);
        else if (it[i].size) wa.push_back({p.off[i], it[i].size});
    }
    if (!b.deltas) return;
    const u64 m = p.m, ni = p.items.size(), nst = n + m + ni;
    CHECK(p.soff2.size() == m + 1 && p.woff.size() == m + 1 && p.wsitem.size() == m && p.n_base <= m, "launch 2 arrays");
    CHECK(p.hst.size() == nst, "status array");
    for (u64 j = 0; j < m; j++) {
        CHECK(p.soff2[j + 1] >= p.soff2[j] && p.woff[j + 1] >= p.woff[j], "launch 2 item %llu", (unsigned long long)j);
        const DlNode& nd = f.nodes[p.wsitem[j]];
        const Pack& pk = *b.odb->packs[key_pack(nd.key)];
        CHECK(nd.data < pk.pack.n - 20 && p.soff2[j + 1] - p.soff2[j] <= pk.pack.n - 20 - nd.data, "launch 2 item %llu: its span leaves the pack", (unsigned long long)j);
        if (p.woff[j + 1] > p.woff[j]) ww.push_back({p.woff[j], p.woff[j + 1] - p.woff[j]});
    }
    CHECK(p.woff[m] <= p.ws_bytes, "launch 2's results leave the workspace");
    // level_start: non-decreasing, ends at n_items
    CHECK(p.level_start.size() == (size_t)p.depth + 1 && p.level_start[0] == 0 && p.level_start[p.depth] == ni, "level_start");
    std::vector<u32> level(ni, 0);
    for (u32 l = 1; l <= p.depth; l++) {
        CHECK(p.level_start[l - 1] <= p.level_start[l], "level_start decreases at %u", l);
        for (u64 q = p.level_start[l - 1]; q < p.level_start[l]; q++) level[q] = l;
    }
    for (u64 q = 0; q < ni; q++) {
        const kd::DlItem& d = p.items[q];
        const unsigned long long Q = q;
        CHECK(d.pad == 0 && d.where < 8 && (d.where & 2), "item %llu where", Q);
        CHECK(d.base_st < nst && d.delta_st < nst && d.out_st == n + m + q, "item %llu status indices", Q);
        // every range inside the allocation its `where` bit names
        const u64 bcap = d.where & 1 ? p.ws_bytes : arena, ocap = d.where & 4 ? p.ws_bytes : arena;
        CHECK(d.base_len <= bcap && d.base_at <= bcap - d.base_len, "item %llu base range", Q);
        CHECK(d.delta_len <= p.ws_bytes && d.delta_at <= p.ws_bytes - d.delta_len, "item %llu delta range", Q);
        CHECK(d.dst_len <= ocap && d.dst_at <= ocap - d.dst_len, "item %llu dst range", Q);
        if (d.dst_len) (d.where & 4 ? ww : wa).push_back({d.dst_at, d.dst_len});
        // the payload is one of launch 2's results
        CHECK(d.delta_st >= n + p.n_base && d.delta_st < n + m, "item %llu payload status", Q);
        const u64 pj = d.delta_st - n;
        CHECK(d.delta_at == p.woff[pj] && d.delta_len == p.woff[pj + 1] - p.woff[pj], "item %llu payload place", Q);
        // the base is an inflate result, or the dst of an item at a strictly lower level
        if (d.base_st < n) {
            const u64 i = d.base_st;
            CHECK(it[i].cls == CLS_STREAM && !(d.where & 1) && d.base_at == p.off[i] && d.base_len == it[i].size, "item %llu base in launch 1", Q);
        } else if (d.base_st < n + m) {
            const u64 j = d.base_st - n;
            CHECK(j < p.n_base && (d.where & 1) && d.base_at == p.woff[j] && d.base_len == p.woff[j + 1] - p.woff[j], "item %llu base in launch 2", Q);
        } else {
            const u64 q0 = d.base_st - n - m;
            const kd::DlItem& pa = p.items[q0];
            CHECK(level[q0] < level[q] && d.base_at == pa.dst_at && d.base_len == pa.dst_len && (d.where & 1u) == ((pa.where >> 2) & 1u),
                  "item %llu base at level %u, its own %u", Q, level[q0], level[q]);
        }
    }
    // every copy's source is its node's home
    CHECK(p.copies.size() == p.copy_req.size(), "copies");
    for (u64 c = 0; c < p.copies.size(); c++) {
        const kd::DlCopy& k = p.copies[c];
        const CopyReq& r = p.copy_req[c];
        CHECK(r.req < n && r.home < n && it[r.req].cls == CLS_DELTA && it[r.req].node != ~0u, "copy %llu request", (unsigned long long)c);
        CHECK(p.home[it[r.req].node] == (int64_t)r.home && it[r.home].node == it[r.req].node && r.home != r.req, "copy %llu home", (unsigned long long)c);
        CHECK(k.src_ws == 0 && k.pad == 0 && k.src_at == p.off[r.home] && k.dst_at == p.off[r.req] && k.len == it[r.req].size &&
                  k.len == it[r.home].size, "copy %llu ranges", (unsigned long long)c);
        if (k.len) wa.push_back({k.dst_at, k.len});
    }
    check_disjoint(wa, arena, "arena");
    check_disjoint(ww, p.ws_bytes, "workspace");
}

// k_inf_streams' part on the host: exactly `span` source bytes into exactly `size` bytes
static u8 host_inflate(const u8* src, u64 span, u8* dst, u64 size) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit(&z) != Z_OK) abort();
    u8 dummy;
    z.next_in = (Bytef*)src;
    z.avail_in = (uInt)span;
    z.next_out = size ? dst : &dummy;
    z.avail_out = (uInt)size;
    const int r = inflate(&z, Z_FINISH);
    const bool ok = r == Z_STREAM_END && z.total_out == size;
    inflateEnd(&z);
    return ok ? 0 : 1;
}

static u8 host_apply(const u8* base, u64 bl, const u8* d, u64 dl, u8* dst, u64 ol) {
    u64 pos, w = 0, iterations = 0;
    u32 st = kd_dl::parse_header(d, dl, bl, ol, &pos);
    while (st == KD_DL_OK) {
        u32 kind, len;
        u64 src;
        if (++iterations > dl + 1) abort();
        st = kd_dl::next_op(d, dl, bl, ol, w, &pos, &kind, &src, &len);
        if (st != KD_DL_OK || kind == kd_dl::OP_END) break;
        memcpy(dst + w, (kind == kd_dl::OP_COPY ? base : d) + src, len);
        w += len;
    }
    return (u8)st;
}

// the pass carried out: staging -> arena (and workspace); every status into p.hst / p.dstat
static void run_on_host(const Batch& b, const std::vector<DevItem>& it, const Forest& f, PassPlan& p, const u8* staging, u8* arena,
                        u8* ws) {
    const u64 n = b.n;
    u8* st1 = b.deltas ? p.hst.data() : p.dstat.data();
    for (u64 i = 0; i < n; i++) {
        const u64 span = p.soff[i + 1] - p.soff[i];
        if (p.kind1[i] == 0) st1[i] = host_inflate(staging + p.soff[i], span, arena + p.off[i], p.off[i + 1] - p.off[i]);
        else {
            if (span) memcpy(arena + p.off[i], staging + p.soff[i], span);
            st1[i] = 0;
        }
    }
    if (!b.deltas) return;
    const u8* src2 = staging + p.soff[n];
    for (u64 j = 0; j < p.m; j++)
        p.hst[n + j] = host_inflate(src2 + p.soff2[j], p.soff2[j + 1] - p.soff2[j], ws + p.woff[j], p.woff[j + 1] - p.woff[j]);
    for (u32 l = 1; l <= p.depth; l++)
        for (u64 q = p.level_start[l - 1]; q < p.level_start[l]; q++) {
            const kd::DlItem& d = p.items[q];
            if (p.hst[d.base_st] || p.hst[d.delta_st]) {
                p.hst[d.out_st] = KD_DL_EPARENT;
                continue;
            }
            p.hst[d.out_st] = host_apply((d.where & 1 ? ws : arena) + d.base_at, d.base_len, ws + d.delta_at, d.delta_len,
                                         (d.where & 4 ? ws : arena) + d.dst_at, d.dst_len);
        }
    for (const kd::DlCopy& c : p.copies)
        if (c.len) memcpy(arena + c.dst_at, (c.src_ws ? ws : arena) + c.src_at, c.len);
    request_status(b, it, f, p);
}

static void put64(FILE* f, u64 v) { fwrite(&v, 8, 1, f); }

// one whole read as kd_odb_devread.cpp drives it: plan, passes, host fix-ups
static void run_read(kd_odb* odb, const std::vector<u8>& ids, bool deltas, FILE* out) {
    const u64 n = ids.size() / 20;
    const Batch b{odb, ids.data(), n, 3, OBJ_BLOB, deltas};
    Readers rds(odb, b.nt);
    std::vector<DevItem> it;
    Forest forest;
    ChainLists chains;
    classify_requests(b, rds, it, chains);
    if (deltas) {
        build_forest(b, rds, chains, forest);
        resolve_requests(b, forest, it);
    }
    std::vector<u8> status(n + 1, 0xEE);
    PassPlan p;
    for (u64 pass = 0;; pass++) {
        if (pass > 1) { fprintf(stderr, "a third pass\n"); exit(3); }
        read_host_class(b, rds, it, status.data(), p);
        layout_arena(b, it, p);
        if (deltas) layout_deltas(b, it, forest, p);
        check_plan(b, it, forest, p);
        u8* staging = (u8*)malloc(p.staging_bytes());
        u8* arena = (u8*)malloc(p.off[n]);
        u8* ws = (u8*)malloc(p.ws_bytes);
        if (!staging || !arena || !ws) abort();
        gather(b, it, forest, p, staging);
        for (u64 k = 0; k < 8; k++)
            if (staging[p.src_bytes() + k] != 0) { fprintf(stderr, "the staging's padding is not zero\n"); exit(3); }
        run_on_host(b, it, forest, p, staging, arena, ws);
        u64 nfix = 0, nfixd = 0, nbad = 0;
        std::vector<u8> buf;
        for (u64 i = 0; i < n; i++) {
            if (it[i].cls == CLS_HOST) {
                if (p.dstat[i]) { fprintf(stderr, "raw item %llu failed\n", (unsigned long long)i); exit(3); }
                continue;
            }
            status[i] = 0;
            if (p.dstat[i] == 0) continue;
            nfix++;
            nfixd += it[i].cls == CLS_DELTA;
            int type = 0;
            const int hr = rds[0].read_packed(*odb->packs[key_pack(it[i].key)], key_off(it[i].key), &type, buf);
            if (hr != RD_OK || type != b.want_type || buf.size() != it[i].size) {
                it[i].cls = CLS_HOST;
                nbad++;
            } else if (it[i].size) {
                memcpy(arena + p.off[i], buf.data(), it[i].size);
            }
        }
        if (!nbad) {
            const u64 counters[8] = {p.n_stream - (nfix - nfixd), p.n_host, p.compressed, nfix, p.n_delta - nfixd, p.items.size(), p.depth, p.ws_bytes};
            fwrite(counters, 8, 8, out);
            put64(out, pass + 1);
            for (u64 i = 0; i < n; i++) {
                fputc(it[i].cls, out);
                fputc(status[i], out);
                put64(out, p.off[i + 1] - p.off[i]);
                if (p.off[i + 1] > p.off[i]) fwrite(arena + p.off[i], 1, p.off[i + 1] - p.off[i], out);
            }
        }
        free(ws);
        free(arena);
        free(staging);
        if (!nbad) return;
    }
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <gitdir> <ids> <out>\n", argv[0]);
        return 2;
    }
    std::vector<u8> ids;
    {
        FILE* in = fopen(argv[2], "rb");
        if (!in) { perror("ids"); return 2; }
        u8 buf[4096];
        size_t r;
        while ((r = fread(buf, 1, sizeof buf, in)) > 0) ids.insert(ids.end(), buf, buf + r);
        fclose(in);
        if (ids.size() % 20) return 2;
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) { perror("out"); return 2; }
    kd_odb* odb = nullptr;
    if (kd_odb_open(argv[1], &odb)) return 2;
    run_read(odb, ids, true, out);
    run_read(odb, ids, false, out);
    {
        Reader rd(odb);
        std::vector<u8> buf;
        for (u64 i = 0; i < ids.size() / 20; i++) {
            int type = 0;
            const int rc = rd.read(ids.data() + 20 * i, &type, buf);
            if (rc) buf.clear();
            fputc(rc, out);
            fputc(rc ? 0 : type, out);
            put64(out, buf.size());
            if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), out);
        }
    }
    kd_odb_close(odb);
    return fclose(out) == 0 ? 0 : 2;
}
