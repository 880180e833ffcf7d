// kd_odb_devread.cpp — the batched read with the arena in HBM: kd_odb_plan.cpp's plan carried out on the
// device.  kd_inflate.hip inflates the plain packed blobs; with KD_RBD_DELTAS kd_delta.hip rebuilds delta
// chains level by level.  What the device refuses is read on the host and patched in; what the host cannot
// read either becomes a failed host item of one more pass.
#include "kd_odb_plan.h"

namespace kd {
// kd_inflate.hip: upload the gathered sources, one launch of k_inf_streams, the status bytes back
int inflate_from_host(kd_ctx* ctx, const uint8_t* h_src, const uint64_t* h_src_off, const uint8_t* h_kind, uint64_t n,
                      uint8_t* d_dst, const uint64_t* h_dst_off, uint64_t* d_dst_off, uint8_t* h_status);
}

namespace kd_store {

namespace {

// the store's pinned staging grown to `bytes` (grow-only, page-locked until the store is closed: kartdiff.h
// says so)
int grow_staging(kd_odb* odb, u64 bytes) {
    if (odb->pin_cap >= bytes) return KD_OK;
    if (odb->pin) kd_host_free(odb->pin);
    odb->pin = nullptr;
    odb->pin_cap = 0;
    const u64 want = bytes + bytes / 4;
    void* p = nullptr;
    if (int rc = kd_host_alloc(want, &p)) return rc;
    odb->pin = (u8*)p;
    odb->pin_cap = want;
    return KD_OK;
}

// the arena and its offsets in HBM, one upload, one launch (KD_RBD_DELTAS: two, and one per level)
int run_on_device(kd_ctx* ctx, const Batch& b, const std::vector<DevItem>& it, const Forest& f, const u8* staging, PassPlan& p,
                  void** d_data, void** d_off) {
    int rc = kd_malloc(ctx, p.off[b.n] + 16, d_data);  // (the tree join reads up to 8 bytes past the last object)
    if (!rc) rc = kd_malloc(ctx, 8 * (b.n + 1), d_off);
    if (rc) return rc;
    if (!b.deltas)
        return kd::inflate_from_host(ctx, staging, p.soff.data(), p.kind1.data(), b.n, (u8*)*d_data, p.off.data(), (u64*)*d_off,
                                     p.dstat.data());
    kd::DlPlan pl = p.dl_plan();
    pl.h_src = staging;
    pl.d_dst = (u8*)*d_data;
    pl.d_dst_off = (u64*)*d_off;
    rc = kd::delta_read_from_host(ctx, pl);
    if (!rc) request_status(b, it, f, p);
    return rc;
}

struct FixUps {
    u64 n = 0, n_delta = 0;  // device items read on the host after all; the delta class among them
    u64 n_bad = 0;           // ... of which the host could not read either (demoted for another pass)
};

// a device item with a nonzero status is read on the host: its bytes go into its place, or (the object
// is corrupt for the host too) it becomes a failed host item of another pass
int fix_up(kd_ctx* ctx, const Batch& b, Reader& rd, std::vector<DevItem>& it, const PassPlan& p, u8* d_data, u8* status,
           FixUps* fx) {
    std::vector<u8> buf;
    for (u64 i = 0; i < b.n; i++) {
        const u8 dst = p.dstat[i];
        if (it[i].cls == CLS_HOST) {
            if (dst == 0) continue;  // a raw copy cannot fail on ranges the plan laid out
            kd::set_error("kd_odb_read_batch_device: raw item %llu: device status %u", (unsigned long long)i, dst);
            return KD_EINVAL;
        }
        status[i] = 0;
        if (dst == 0) continue;
        fx->n++;
        if (it[i].cls == CLS_DELTA) fx->n_delta++;
        int type = 0;
        const int hr = rd.read_packed(*b.odb->packs[key_pack(it[i].key)], key_off(it[i].key), &type, buf);
        if (hr != RD_OK || type != b.want_type || buf.size() != it[i].size) {
            it[i].cls = CLS_HOST;
            fx->n_bad++;
        } else if (it[i].size) {
            int rc = kd_memcpy(ctx, d_data + p.off[i], buf.data(), it[i].size, KD_COPY_H2D);
            if (!rc) rc = kd_sync(ctx);  // (before buf is read into again; a rare path)
            if (rc) return rc;
        }
    }
    return KD_OK;
}

}  // namespace

int read_batch_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags, kd_blobs* out,
                      uint8_t* status, ReadStats* stats, int want_type, int64_t* phase_us) {
    const auto t_start = Clock::now();
    out->n = n;
    out->data = nullptr;
    out->off = nullptr;
    out->mem = KD_MEM_DEVICE;
    out->size_hint = 0;
    const Batch b{odb, oids, n, default_threads(threads), want_type, (flags & KD_RBD_DELTAS) != 0};
    std::lock_guard<std::mutex> dev_lock(odb->dev_mu);  // (the pinned staging is the store's)
    Readers rds(odb, b.nt);
    std::vector<DevItem> it;
    ChainLists chains;
    Forest forest;
    classify_requests(b, rds, it, chains);
    if (b.deltas) {
        build_forest(b, rds, chains, forest);
        resolve_requests(b, forest, it);
    }
    const int64_t plan_us = us_since(t_start);
    int64_t host_us = 0, device_us = 0;
    PassPlan p;
    for (int pass = 0;; pass++) {
        const auto t_pass = Clock::now();
        read_host_class(b, rds, it, status, p);
        layout_arena(b, it, p);
        if (b.deltas) layout_deltas(b, it, forest, p);
        if (int rc = grow_staging(odb, p.staging_bytes())) return rc;
        gather(b, it, forest, p, odb->pin);
        host_us += us_since(t_pass);
        const auto t_dev = Clock::now();
        void *d_data = nullptr, *d_off = nullptr;
        int rc = run_on_device(ctx, b, it, forest, odb->pin, p, &d_data, &d_off);
        device_us += us_since(t_dev);
        FixUps fx;
        if (!rc) rc = fix_up(ctx, b, rds[0], it, p, (u8*)d_data, status, &fx);
        if (!rc && fx.n_bad && pass > 0) {
            kd::set_error("kd_odb_read_batch_device: unreadable items after the host pass");
            rc = KD_EINVAL;
        }
        if (rc || fx.n_bad) {
            kd_mfree(ctx, d_data);
            kd_mfree(ctx, d_off);
            if (rc) return rc;
            continue;  // (the second pass plans and counts again)
        }
        out->data = (const u8*)d_data;
        out->off = (const u64*)d_off;
        stats->device = p.n_stream - (fx.n - fx.n_delta);
        stats->host = p.n_host;
        stats->compressed = p.compressed;
        stats->fixups = fx.n;
        stats->deltas = p.n_delta - fx.n_delta;
        stats->links = p.items.size();
        stats->depth = p.depth;
        stats->scratch = p.ws_bytes;
        break;
    }
    if (phase_us) {  // (kd_walk_device sums its batches' phases)
        phase_us[0] += plan_us;
        phase_us[1] += host_us;
        phase_us[2] += device_us;
    }
    if (b.deltas) {
        odb->rbd_us[0] = plan_us;
        odb->rbd_us[1] = forest.peek_us;
        odb->rbd_us[2] = host_us;
        odb->rbd_us[3] = device_us;
    }
    return KD_OK;
}

}  // namespace kd_store

using namespace kd_store;

extern "C" int kd_odb_read_batch_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, kd_blobs* out,
                                        uint8_t* status, uint64_t stats[4]) {
    if (!ctx || !odb || !out || (n && (!oids || !status))) { kd::set_error("kd_odb_read_batch_device: NULL"); return KD_EINVAL; }
    ReadStats st;
    const int rc = read_batch_device(ctx, odb, oids, n, threads, 0, out, status, &st, OBJ_BLOB, nullptr);
    if (!rc && stats) memcpy(stats, &st, 4 * sizeof(u64));
    return rc;
}

extern "C" int kd_odb_read_batch_device_ex(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags,
                                           kd_blobs* out, uint8_t* status, uint64_t stats[8]) {
    if (!ctx || !odb || !out || (n && (!oids || !status))) { kd::set_error("kd_odb_read_batch_device_ex: NULL"); return KD_EINVAL; }
    if (flags & ~KD_RBD_DELTAS) { kd::set_error("kd_odb_read_batch_device_ex: unknown flags %u", flags); return KD_EINVAL; }
    if (n >= (1ull << 30)) { kd::set_error("kd_odb_read_batch_device_ex: too many ids"); return KD_EINVAL; }
    ReadStats st;
    const int rc = read_batch_device(ctx, odb, oids, n, threads, flags, out, status, &st, OBJ_BLOB, nullptr);
    if (!rc && stats) memcpy(stats, &st, sizeof st);
    return rc;
}
