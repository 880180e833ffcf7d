"""Engine: one libkartdiff context per GPU, with numpy-in / numpy-out calls.

Every method goes through the HIP library; there is no CPU implementation here.  Device-resident
pipelines (bench.py) keep their buffers in HBM through the library's own allocator
(``kart_amd.device``).
"""
import ctypes
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

from . import _native as N

_TRACE = os.environ.get("KD_TRACE_HOST") == "1"  # (diagnosis: host phase times to stderr)

# placeholder a native call gets for an empty host array: a module-level array, alive for every call
_PAD = np.zeros(16, np.uint8)


@dataclass
class Diff2Result:
    n_insert: int
    n_update: int
    n_delete: int
    delta: np.ndarray  # uint32 [n_delta, 2] (base sorted index | NONE, target sorted index | NONE)
    upd: np.ndarray  # uint32 [n_update, 2]

    def type_counts(self):
        out = {}
        for name, v in (("inserts", self.n_insert), ("updates", self.n_update), ("deletes", self.n_delete)):
            if v:
                out[name] = v
        return out


@dataclass
class Merge3Result:
    n_clean: int
    conflict: np.ndarray  # uint32 [n, 3] (ancestor, ours, theirs) sorted indices | NONE
    mdelta: np.ndarray  # uint32 [n, 2] (ours | NONE, theirs | NONE): take theirs


class Engine:
    def __init__(self, device=0):
        self.L = N.lib()
        self.ctx = ctypes.c_void_p()
        N.check(self.L.kd_init(int(device), ctypes.byref(self.ctx)), "kd_init")
        self.device = device

    def set_option(self, name, value):
        """a tuning option of the context (kd_set_option: the A/B switches of kartdiff.h)"""
        N.check(self.L.kd_set_option(self.ctx, name.encode(), int(value)), "kd_set_option")

    def get_option(self, name):
        v = ctypes.c_int64()
        N.check(self.L.kd_get_option(self.ctx, name.encode(), ctypes.byref(v)), "kd_get_option")
        return int(v.value)

    def close(self):
        if self.ctx:
            self.L.kd_fini(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---------------------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        N.check(self.L.kd_set_stream(self.ctx, stream_handle), "kd_set_stream")

    def sync(self):
        N.check(self.L.kd_sync(self.ctx), "kd_sync")

    def device_sync(self):
        """hipDeviceSynchronize (every stream of the device) + profiling flush"""
        N.check(self.L.kd_device_sync(self.ctx), "kd_device_sync")

    # ---- multi-GPU (RCCL owned by the library) ---------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_uint8 * N.KD_COMM_ID_BYTES)()
        N.check(N.lib().kd_comm_unique_id(buf), "kd_comm_unique_id")
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (ctypes.c_uint8 * N.KD_COMM_ID_BYTES).from_buffer_copy(uid)
        N.check(self.L.kd_comm_init(self.ctx, int(nranks), int(rank), buf), "kd_comm_init")
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_info(self):
        """{"count": ncclCommCount, "rank": ncclCommUserRank, "device": ncclCommCuDevice} of the
        library's communicator"""
        out = (ctypes.c_int32 * 3)()
        N.check(self.L.kd_comm_info(self.ctx, out), "kd_comm_info")
        return {"count": int(out[0]), "rank": int(out[1]), "device": int(out[2])}

    def comm_fini(self):
        N.check(self.L.kd_comm_fini(self.ctx), "kd_comm_fini")

    def reserve(self, max_entries, max_updates=0):
        N.check(self.L.kd_reserve(self.ctx, int(max_entries), int(max_updates)), "kd_reserve")

    def prof_enable(self, on=True):
        N.check(self.L.kd_prof_enable(self.ctx, 1 if on else 0), "kd_prof_enable")

    def prof_select(self, names=None):
        """time only these kernels (iterable of names; None = all)"""
        arg = ",".join(names).encode() if names else None
        N.check(self.L.kd_prof_select(self.ctx, arg), "kd_prof_select")

    def prof_reset(self):
        N.check(self.L.kd_prof_reset(self.ctx), "kd_prof_reset")

    def prof_get(self, name):
        launches = ctypes.c_uint64()
        ms = ctypes.c_double()
        N.check(self.L.kd_prof_get(self.ctx, name.encode(), ctypes.byref(launches), ctypes.byref(ms)), "kd_prof_get")
        return int(launches.value), float(ms.value)

    # ---------------------------------------------------------------------------------------
    def diff2(self, base, target, flags=0) -> Diff2Result:
        """base/target: PackedSide (host) -> key-ordered delta set (kd_diff2).  A side packed on the
        GPU with its rows in walk order (PackedSide.dperm) joins through its order on the device
        (kd_diff2_device_perm: no OID or filename gather)."""
        if base.walk_rows or target.walk_rows:
            return self._diff2_perm(base, target, flags)
        t0 = time.perf_counter() if _TRACE else 0
        sa, sb = base.kd_side(), target.kd_side()
        res = ctypes.POINTER(N.KdDiffResult)()
        if _TRACE:
            print(f"[kd] engine.diff2 kd_side    {1e3 * (time.perf_counter() - t0):9.3f} ms", file=sys.stderr)
        N.check(self.L.kd_diff2(self.ctx, ctypes.byref(sa), ctypes.byref(sb), flags, ctypes.byref(res)), "kd_diff2")
        if _TRACE:
            print(f"[kd] engine.diff2 call       {1e3 * (time.perf_counter() - t0):9.3f} ms", file=sys.stderr)
        try:
            r = res.contents
            nd, nu = int(r.n_delta), int(r.n_update)
            delta = np.ctypeslib.as_array(r.delta, (nd * 2,)).reshape(nd, 2).copy() if nd else np.zeros((0, 2), np.uint32)
            upd = np.ctypeslib.as_array(r.upd, (nu * 2,)).reshape(nu, 2).copy() if nu else np.zeros((0, 2), np.uint32)
            return Diff2Result(int(r.n_insert), nu, int(r.n_delete), delta, upd)
        finally:
            self.L.kd_free(res)

    def _diff2_perm(self, base, target, flags):
        from .device import DevBuf, perm_dev

        (sa, oa, ka), (sb, ob, kb) = perm_dev(self, base), perm_dev(self, target)
        n = base.n + target.n
        d_delta, d_upd, d_c = DevBuf(self, 8 * (n + 1)), DevBuf(self, 8 * (n + 1)), DevBuf(self, 64)
        N.check(self.L.kd_diff2_device_perm(self.ctx, ctypes.byref(sa), ctypes.byref(sb), oa.ptr, ob.ptr, flags,
                                            d_delta.ptr, d_upd.ptr, d_c.ptr, d_c.ptr + 32), "kd_diff2_device_perm")
        c = d_c.download(np.uint64, 5)
        err = int(c[4]) & 0xFFFFFFFF
        if err:
            raise N.Unsupported(N.KD_EUNSUPPORTED, "kd_diff2: " + ("side keys not strictly ascending" if err & 1 else
                                                                   "hash key collision between different filenames"))
        nd, nu = int(c[3]), int(c[1])
        delta = d_delta.download(np.uint32, 2 * nd).reshape(nd, 2)
        upd = d_upd.download(np.uint32, 2 * nu).reshape(nu, 2)
        del ka, kb
        return Diff2Result(int(c[0]), nu, int(c[2]), delta, upd)

    def _merge3_perm(self, ancestor, ours, theirs, flags):
        from .device import DevBuf, perm_dev

        ds = [perm_dev(self, s) for s in (ancestor, ours, theirs)]
        n = ancestor.n + ours.n + theirs.n
        d_conf, d_md, d_c = DevBuf(self, 12 * (n + 1)), DevBuf(self, 8 * (ours.n + theirs.n + 1)), DevBuf(self, 64)
        N.check(self.L.kd_merge3_device_perm(self.ctx, *(ctypes.byref(d[0]) for d in ds), *(d[1].ptr for d in ds),
                                             flags, d_conf.ptr, d_md.ptr, d_c.ptr, d_c.ptr + 32),
                "kd_merge3_device_perm")
        c = d_c.download(np.uint64, 5)
        err = int(c[4]) & 0xFFFFFFFF
        if err:
            raise N.Unsupported(N.KD_EUNSUPPORTED,
                                "kd_merge3: err=0x%x (%s)" % (err, "keys not strictly ascending" if err & 1 else
                                                              "hash key collision" if err & 2 else "tile overflow"))
        nc, nm = int(c[1]), int(c[2])
        conf = d_conf.download(np.uint32, 3 * nc).reshape(nc, 3)
        md = d_md.download(np.uint32, 2 * nm).reshape(nm, 2)
        return Merge3Result(int(c[0]), conf, md)

    @staticmethod
    def diff2_sharded(engines, base, target, bucket_bits, flags=0) -> Diff2Result:
        """One process, len(engines) GPUs: kd_diff2_sharded cuts base/target (host PackedSides) into
        bucket ranges, diffs each on its GPU and all-gathers the records over RCCL."""
        ctxs = (ctypes.c_void_p * len(engines))(*[e.ctx.value for e in engines])
        sa, sb = base.kd_side(), target.kd_side()
        L = engines[0].L
        res = ctypes.POINTER(N.KdDiffResult)()
        N.check(L.kd_diff2_sharded(ctxs, len(engines), ctypes.byref(sa), ctypes.byref(sb), int(bucket_bits), flags,
                                   ctypes.byref(res)), "kd_diff2_sharded")
        try:
            r = res.contents
            nd, nu = int(r.n_delta), int(r.n_update)
            delta = np.ctypeslib.as_array(r.delta, (nd * 2,)).reshape(nd, 2).copy() if nd else np.zeros((0, 2), np.uint32)
            upd = np.ctypeslib.as_array(r.upd, (nu * 2,)).reshape(nu, 2).copy() if nu else np.zeros((0, 2), np.uint32)
            return Diff2Result(int(r.n_insert), nu, int(r.n_delete), delta, upd)
        finally:
            L.kd_free(res)

    def delta_pk_order(self, base, target, records):
        """records uint32 [n, 2] (classify2's (base | NONE, target | NONE) deltas or updates) of two
        KD_KEY_INT PackedSides -> (pks ascending int64 [n], record index of each uint32 [n]): the
        order DeltaDiff.sorted_items yields (kd_delta_pk_order; the sides' keys are uploaded)"""
        from . import packing
        from .device import DevBuf, DevSide

        records = np.ascontiguousarray(records, np.uint32).reshape(-1, 2)
        n = records.shape[0]
        if n == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.uint32)
        lo, hi = [], []
        for side in (base, target):
            if side.n:
                info = side.info if side.info is not None else packing.keys_scan(side.key, side.key_mode)
                lo.append(int(info.pk_min))
                hi.append(int(info.pk_max))
        A, B = DevSide(self, base, keys_only=True), DevSide(self, target, keys_only=True)  # (the pass reads keys only)
        sa, sb = A.kd_side(), B.kd_side()
        d_rec = DevBuf.from_numpy(self, records.reshape(-1))
        d_n = DevBuf.from_numpy(self, np.array([n], np.uint64))
        d_pk, d_perm = DevBuf(self, 8 * n), DevBuf(self, 4 * n)
        N.check(self.L.kd_delta_pk_order(self.ctx, ctypes.byref(sa), ctypes.byref(sb), d_rec.ptr, None, n, d_n.ptr,
                                         min(lo), max(hi), d_pk.ptr, d_perm.ptr), "kd_delta_pk_order")
        return d_pk.download(np.int64, n), d_perm.download(np.uint32, n)

    def find_renames(self, base, target, delta):
        """delta uint32 [n, 2] (the (base | NONE, target | NONE) records of a two-way diff of the two
        PackedSides, in its order) -> uint32 [k, 2]: (delta index of a delete, delta index of the insert
        with the same blob OID), ascending by the delete (kd_find_renames: at most one pair per OID, the
        last delete with the last insert, as WorkingCopy.find_renames pairs them)"""
        delta = np.ascontiguousarray(delta, np.uint32).reshape(-1, 2)
        n = int(delta.shape[0])
        if n < 2:
            return np.zeros((0, 2), np.uint32)
        if base.walk_rows or target.walk_rows:  # OIDs in walk order: read through the sort orders
            from .device import DevBuf, perm_dev

            (sa, oa, ka), (sb, ob, kb) = perm_dev(self, base), perm_dev(self, target)
            d_delta = DevBuf.from_numpy(self, delta.reshape(-1))
            d_ren, d_n = DevBuf(self, 8 * (n // 2 + 1)), DevBuf(self, 8)
            N.check(self.L.kd_find_renames(self.ctx, ctypes.byref(sa), ctypes.byref(sb), oa.ptr, ob.ptr, d_delta.ptr, n,
                                           None, N.KD_MEM_DEVICE, d_ren.ptr, d_n.ptr, N.KD_MEM_DEVICE), "kd_find_renames")
            k = int(d_n.download(np.uint64, 1)[0])
            del ka, kb
            return d_ren.download(np.uint32, 2 * k).reshape(k, 2)
        sa, sb = base.kd_side(), target.kd_side()
        ren = np.zeros((n // 2 + 1, 2), np.uint32)
        k = ctypes.c_uint64()
        N.check(self.L.kd_find_renames(self.ctx, ctypes.byref(sa), ctypes.byref(sb), None, None, N.ptr(delta), n, None,
                                       N.KD_MEM_HOST, N.ptr(ren), ctypes.byref(k), N.KD_MEM_HOST), "kd_find_renames")
        return ren[:int(k.value)].copy()

    def tree_hash(self, names, name_off, oids, seg, kind, rank=False, bodies=False, body_cap=None):
        """The ids of one level of git trees (kd_tree_hash).  Tree t consists of entries
        seg[t] .. seg[t+1]: names uint8 arena with name_off uint64 [n+1], oids uint8 [n, 20], all of
        one ``kind`` (KD_TE_BLOB / KD_TE_TREE); ``rank``: the entries of a run come in any order
        (blobs, runs of up to 512).  Returns (ids uint8 [n_trees, 20], status uint8 [n_trees]) plus
        (body uint8, body_off uint64 [n_trees+1]) with ``bodies`` (``body_cap``: the room for them in
        bytes, by default what the entries can need).  numpy arrays in: numpy arrays
        out.  If any input is a DevBuf the others are uploaded, the call is the device form and the
        results are DevBufs (the ids are the next level's ``oids`` as they stand)."""
        from .device import DevBuf

        ins = [names, name_off, oids, seg]
        flags = N.KD_TH_RANK_NAMES if rank else 0
        e = N.KdTreeEntries()
        e.kind = int(kind)
        if any(isinstance(x, DevBuf) for x in ins):
            dts = (np.uint8, np.uint64, np.uint8, np.uint64)
            d = [x if isinstance(x, DevBuf) else DevBuf.from_numpy(self, np.ascontiguousarray(x, dt).reshape(-1))
                 for x, dt in zip(ins, dts)]
            n, nt = d[2].nbytes // 20, d[3].nbytes // 8 - 1
            if d[1].nbytes != 8 * (n + 1) or nt < 0:
                raise ValueError("tree_hash: name_off must hold n + 1 offsets, seg n_trees + 1")
            e.n, e.name, e.name_off, e.oid, e.mem = n, d[0].ptr, d[1].ptr, d[2].ptr, N.KD_MEM_DEVICE
            ids, status = DevBuf(self, 20 * nt), DevBuf(self, nt)
            cap = 28 * n + d[0].nbytes if body_cap is None else int(body_cap)
            body, body_off = (DevBuf(self, cap), DevBuf(self, 8 * (nt + 1))) if bodies else (None, None)
            N.check(self.L.kd_tree_hash(self.ctx, ctypes.byref(e), d[3].ptr, nt, flags, ids.ptr, status.ptr,
                                        body.ptr if bodies else None, body_off.ptr if bodies else None, cap,
                                        N.KD_MEM_DEVICE), "kd_tree_hash")
            if any(x is not y for x, y in zip(ins, d)):
                self.sync()  # (the uploaded copies are freed on return)
            return (ids, status, body, body_off) if bodies else (ids, status)
        names = np.ascontiguousarray(names, np.uint8).reshape(-1)
        name_off = np.ascontiguousarray(name_off, np.uint64)
        oids = np.ascontiguousarray(oids, np.uint8).reshape(-1, 20)
        seg = np.ascontiguousarray(seg, np.uint64)
        n, nt = int(oids.shape[0]), int(seg.shape[0]) - 1
        if name_off.shape[0] != n + 1 or nt < 0:
            raise ValueError("tree_hash: name_off must hold n + 1 offsets, seg n_trees + 1")
        e.n, e.name, e.name_off, e.mem = n, N.ptr(names) if names.size else N.ptr(_PAD), N.ptr(name_off), N.KD_MEM_HOST
        e.oid = N.ptr(oids) if n else N.ptr(_PAD)
        ids, status = np.zeros((max(nt, 1), 20), np.uint8), np.zeros(max(nt, 1), np.uint8)
        cap = 28 * n + int(names.size) if body_cap is None else int(body_cap)
        body = np.zeros(max(cap, 1), np.uint8) if bodies else None
        body_off = np.zeros(nt + 1, np.uint64) if bodies else None
        N.check(self.L.kd_tree_hash(self.ctx, ctypes.byref(e), N.ptr(seg), nt, flags, N.ptr(ids), N.ptr(status),
                                    N.ptr(body), N.ptr(body_off), cap, N.KD_MEM_HOST), "kd_tree_hash")
        if bodies:
            return ids[:nt], status[:nt], body[:int(body_off[nt])], body_off
        return ids[:nt], status[:nt]

    def fielddiff(self, old_data, old_off, new_data, new_off, pairs, maps, size_hint=0):
        """Blob arenas (uint8 data, uint64 off[n+1]) per side; pairs uint32 [n, 2] (old blob,
        new blob) or None (blob u on both sides); maps: schema.FieldMaps; size_hint: the typical
        blob size in bytes (kd_blobs.size_hint; 0 = the arenas' mean), which picks the window shape.
        A side may be a device.DevBlobs (an arena already in HBM, e.g. ObjectDB.read_batch_device's)
        in place of its data, with None for its off.
        Returns (masks uint64 [n, words], status uint8 [n])."""
        from .device import DevBlobs

        sides, arrays = [], []  # (arrays: the converted host arrays, alive until the call has returned)
        for d, o in ((old_data, old_off), (new_data, new_off)):
            if isinstance(d, DevBlobs):
                b = d.kd_blobs()
                if size_hint:
                    b.size_hint = int(size_hint)
            else:
                d = np.ascontiguousarray(d, np.uint8)
                o = np.ascontiguousarray(o, np.uint64)
                arrays += [d, o]
                b = N.KdBlobs()
                b.n = int(o.shape[0]) - 1
                b.data = N.ptr(d) if d.size else N.ptr(_PAD)
                b.off = N.ptr(o)
                b.mem = N.KD_MEM_HOST
                b.size_hint = int(size_hint)
            sides.append(b)
        ob, nb = sides
        n = int(pairs.shape[0]) if pairs is not None else int(ob.n)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, np.uint32)
        masks = np.zeros((max(n, 1), maps.words), np.uint64)
        status = np.zeros(max(n, 1), np.uint8)
        km = maps.kd_maps()
        N.check(
            self.L.kd_fielddiff(self.ctx, ctypes.byref(ob), ctypes.byref(nb), N.ptr(pairs), n, None, N.KD_MEM_HOST,
                                ctypes.byref(km), N.ptr(masks), N.ptr(status), N.KD_MEM_HOST),
            "kd_fielddiff",
        )
        return masks[:n], status[:n]

    def inflate(self, src, src_off, dst_off, kind=None):
        """zlib streams inflated on the GPU (kd_inflate_batch, host form): item i is
        src[src_off[i]:src_off[i+1]] -> data[dst_off[i]:dst_off[i+1]], its inflated size the dst range
        exactly; kind[i] = 1 copies the item as it is.  Returns (data uint8 [dst_off[-1]], status
        uint8 [n] of KD_INF_* codes); a failed item's bytes are unspecified."""
        src = np.ascontiguousarray(src, np.uint8)
        src_off = np.ascontiguousarray(src_off, np.uint64)
        dst_off = np.ascontiguousarray(dst_off, np.uint64)
        n = int(src_off.shape[0]) - 1
        if n < 0 or dst_off.shape[0] != n + 1:
            raise ValueError("inflate: src_off and dst_off must hold n + 1 offsets")
        if n and int(src_off[-1]) > src.size:
            raise ValueError("inflate: src_off runs past src")
        if kind is not None:
            kind = np.ascontiguousarray(kind, np.uint8)
            if kind.shape[0] != n:
                raise ValueError("inflate: kind must hold n bytes")
        data = np.zeros(max(int(dst_off[-1]), 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        N.check(self.L.kd_inflate_batch(self.ctx, N.ptr(src) if src.size else N.ptr(_PAD), N.ptr(src_off), N.ptr(kind), n,
                                        N.ptr(data), N.ptr(dst_off), N.ptr(status), N.KD_MEM_HOST), "kd_inflate_batch")
        return data[:int(dst_off[-1])], status[:n]

    def apply_deltas(self, base, base_off, base_idx, delta, delta_off, dst_off):
        """one level of git deltas applied on the GPU (kd_delta_apply_batch, host form): item i patches
        base[base_off[b]:base_off[b+1]], b = base_idx[i], with delta[delta_off[i]:delta_off[i+1]] into
        data[dst_off[i]:dst_off[i+1]]; the delta's two sizes must be the base and dst ranges' lengths.
        Returns (data uint8 [dst_off[-1]], status uint8 [n] of KD_DL_* codes); a failed item's bytes are
        unspecified."""
        base = np.ascontiguousarray(base, np.uint8)
        delta = np.ascontiguousarray(delta, np.uint8)
        base_off = np.ascontiguousarray(base_off, np.uint64)
        base_idx = np.ascontiguousarray(base_idx, np.uint32)
        delta_off = np.ascontiguousarray(delta_off, np.uint64)
        dst_off = np.ascontiguousarray(dst_off, np.uint64)
        n, nb = int(delta_off.shape[0]) - 1, int(base_off.shape[0]) - 1
        if n < 0 or nb < 0 or dst_off.shape[0] != n + 1 or base_idx.shape[0] != n:
            raise ValueError("apply_deltas: delta_off and dst_off must hold n + 1 offsets, base_idx n, base_off nb + 1")
        if int(base_off[-1]) > base.size or int(delta_off[-1]) > delta.size:
            raise ValueError("apply_deltas: offsets run past their arena")
        data = np.zeros(max(int(dst_off[-1]), 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        N.check(self.L.kd_delta_apply_batch(self.ctx, N.ptr(base) if base.size else N.ptr(_PAD), N.ptr(base_off), nb,
                                            N.ptr(base_idx) if n else N.ptr(_PAD), N.ptr(delta) if delta.size else N.ptr(_PAD),
                                            N.ptr(delta_off), n, N.ptr(data), N.ptr(dst_off), N.ptr(status), N.KD_MEM_HOST),
                "kd_delta_apply_batch")
        return data[:int(dst_off[-1])], status[:n]

    def tree_join(self, data, off, tree, pfx, pfx_off, k, compare=None):
        """changed leaf trees parsed, joined and pruned on the GPU (kd_tree_join_batch, host form): tree i
        is data[off[i]:off[i+1]], task t names tree[t, r] (or KD_NONE) for each of the k roots and the path
        prefix pfx[pfx_off[t]:pfx_off[t+1]]; ``compare=(i, j)`` drops every name roots i and j agree on.
        Returns ([(paths uint8, path_off uint64 [n+1], oids uint8 [n, 20], modes uint32 [n]) per root],
        count uint32 [n_task, k], status uint8 [n_task] of KD_TJ_* codes): what kd_walk lists under those
        trees; a task with a nonzero status contributes nothing."""
        data = np.ascontiguousarray(data, np.uint8)
        pfx = np.ascontiguousarray(pfx, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        pfx_off = np.ascontiguousarray(pfx_off, np.uint64)
        tree = np.ascontiguousarray(tree, np.uint32).reshape(-1, k)
        nt, ntrees = int(tree.shape[0]), int(off.shape[0]) - 1
        if ntrees < 0 or pfx_off.shape[0] != nt + 1:
            raise ValueError("tree_join: off must hold n_trees + 1 offsets, pfx_off n_task + 1")
        if int(off[-1]) > data.size or int(pfx_off[-1]) > pfx.size:
            raise ValueError("tree_join: offsets run past their arena")
        c0, c1 = compare if compare is not None else (N.KD_WALK_ALL, N.KD_WALK_ALL)
        # what a root can keep at most: every entry of its trees (23 bytes at least), each under its prefix
        lens = np.diff(off).astype(np.int64)
        lead = np.diff(pfx_off).astype(np.int64) + 1
        outs, arrays = (N.KdTjOut * k)(), []
        for r in range(k):
            idx = tree[:, r].astype(np.int64)
            ok = (idx != N.KD_NONE) & (idx < ntrees)
            ln = np.where(ok, lens[np.where(ok, idx, 0)] if ntrees else 0, 0)
            cap_n = int((ln // 23).sum())
            cap_b = int((ln + (ln // 23) * lead).sum())
            a = (np.zeros(cap_n + 1, np.uint64), np.zeros(max(cap_n, 1), np.uint32), np.zeros((max(cap_n, 1), 20), np.uint8),
                 np.zeros(max(cap_b, 1), np.uint8))
            arrays.append(a)
            outs[r].cap_n, outs[r].cap_bytes = cap_n, cap_b
            outs[r].path_off, outs[r].mode, outs[r].oid, outs[r].path = (x.ctypes.data for x in a)
        count = np.zeros((max(nt, 1), k), np.uint32)
        status = np.zeros(max(nt, 1), np.uint8)
        N.check(self.L.kd_tree_join_batch(self.ctx, N.ptr(data) if data.size else N.ptr(_PAD), N.ptr(off), ntrees,
                                          N.ptr(tree) if nt else N.ptr(_PAD), N.ptr(pfx) if pfx.size else N.ptr(_PAD),
                                          N.ptr(pfx_off), nt, k, c0, c1, outs, N.ptr(count), N.ptr(status), None,
                                          N.KD_MEM_HOST), "kd_tree_join_batch")
        res = []
        for r in range(k):
            n, nb = int(outs[r].n), int(outs[r].bytes)
            po, mo, oo, pa = arrays[r]
            res.append((pa[:nb], po[:n + 1], oo[:n], mo[:n]))
        return res, count[:nt], status[:nt]

    def pack_keys(self, d_paths, d_off, n, encoding):
        """join keys and the side scan of a path arena that is in HBM (kd_pack_keys_device): ``d_paths`` /
        ``d_off`` DevBufs (or device addresses) of the arena and its n + 1 uint64 offsets, ``encoding`` the
        dataset's PathEncoding.  Returns (keys DevBuf uint64 [n], status DevBuf uint8 [n], KdKeysInfo of the
        keys as written, bad, first_bad); the one read-back is the 56-byte info record."""
        from .device import DevBuf

        n = int(n)
        hex_ = 1 if encoding.encoding == "hex" else 0
        if encoding.key_mode == N.KD_KEY_HASH and ((hex_ and encoding.branches != 256) or (not hex_ and encoding.branches != 64)):
            from .packing import PackError

            raise PackError(f"unsupported path structure {encoding}")
        keys, status, info = DevBuf(self, 8 * n), DevBuf(self, n), DevBuf(self, ctypes.sizeof(N.KdKeypackInfo))
        N.check(self.L.kd_pack_keys_device(self.ctx, getattr(d_paths, "ptr", d_paths), getattr(d_off, "ptr", d_off), n,
                                           int(encoding.key_mode), int(encoding.levels), hex_, keys.ptr, status.ptr,
                                           info.ptr), "kd_pack_keys_device")
        raw = info.download(np.uint8, ctypes.sizeof(N.KdKeypackInfo))
        r = N.KdKeypackInfo.from_buffer_copy(raw.tobytes())
        ki = N.KdKeysInfo.from_buffer_copy(bytes(r.info))
        return keys, status, ki, int(r.bad), int(r.first_bad)

    def merge3(self, ancestor, ours, theirs, flags=0) -> Merge3Result:
        """three PackedSides -> conflicts / merge deltas in path order (kd_merge3; sides packed on the
        GPU with walk-order rows through kd_merge3_device_perm)"""
        if ancestor.walk_rows or ours.walk_rows or theirs.walk_rows:
            return self._merge3_perm(ancestor, ours, theirs, flags)
        sa, so, st = ancestor.kd_side(), ours.kd_side(), theirs.kd_side()
        res = ctypes.POINTER(N.KdMergeResult)()
        N.check(self.L.kd_merge3(self.ctx, ctypes.byref(sa), ctypes.byref(so), ctypes.byref(st), flags,
                                 ctypes.byref(res)), "kd_merge3")
        try:
            r = res.contents
            nc, nm = int(r.n_conflict), int(r.n_mdelta)
            conf = np.ctypeslib.as_array(r.conflict, (nc * 3,)).reshape(nc, 3).copy() if nc else np.zeros((0, 3), np.uint32)
            md = np.ctypeslib.as_array(r.mdelta, (nm * 2,)).reshape(nm, 2).copy() if nm else np.zeros((0, 2), np.uint32)
            return Merge3Result(int(r.n_clean), conf, md)
        finally:
            self.L.kd_free(res)

    def envelopes(self, data, off, filt_env, bits=20):
        """GPKG geometry blobs -> (match u8[n], enc u8[n, bits/2], enc_ok u8[n], n_candidates)."""
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = int(off.shape[0]) - 1
        g = N.KdBlobs()
        g.n = n
        g.data = N.ptr(data) if data.size else N.ptr(_PAD)
        g.off = N.ptr(off)
        g.mem = N.KD_MEM_HOST
        nb = bits // 2
        match = np.zeros(max(n, 1), np.uint8)
        enc = np.zeros((max(n, 1), nb), np.uint8)
        ok = np.zeros(max(n, 1), np.uint8)
        fe = (ctypes.c_double * 4)(*[float(x) for x in filt_env])
        ncand = ctypes.c_uint64()
        N.check(self.L.kd_envelopes(self.ctx, ctypes.byref(g), fe, int(bits), N.ptr(match), N.ptr(enc), N.ptr(ok),
                                    N.KD_MEM_HOST, ctypes.byref(ncand)), "kd_envelopes")
        return match[:n], enc[:n], ok[:n], int(ncand.value)

    def hex_encode(self, data, off, mode):
        """Blob arena -> (hex u8[2*off[n]], start u32[n], status u8[n]) via kd_hex_encode (host buffers).
        Blob i's string is hex[2*(off[i] + start[i]) : 2*off[i+1]]."""
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = int(off.shape[0]) - 1
        g = N.KdBlobs()
        g.n = n
        g.data = N.ptr(data) if data.size else N.ptr(_PAD)
        g.off = N.ptr(off)
        g.mem = N.KD_MEM_HOST
        nbytes = int(off[-1]) if n >= 0 and off.size else 0
        hexbuf = np.zeros(max(2 * nbytes, 1), np.uint8)
        start = np.zeros(max(n, 1), np.uint32)
        status = np.zeros(max(n, 1), np.uint8)
        N.check(self.L.kd_hex_encode(self.ctx, ctypes.byref(g), int(mode), N.ptr(hexbuf), N.ptr(start), N.ptr(status),
                                     N.KD_MEM_HOST), "kd_hex_encode")
        return hexbuf[: 2 * nbytes], start[:n], status[:n]

    def env_overlap(self, enc, bits, q):
        enc = np.ascontiguousarray(enc, np.uint8)
        n = enc.shape[0]
        out = np.zeros(max(n, 1), np.uint8)
        qq = (ctypes.c_double * 4)(*[float(x) for x in q])
        N.check(self.L.kd_env_overlap(self.ctx, N.ptr(enc) if enc.size else N.ptr(_PAD), n, int(bits),
                                      qq, N.ptr(out), N.KD_MEM_HOST), "kd_env_overlap")
        return out[:n]
