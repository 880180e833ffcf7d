"""ctypes binding of libkartdiff.so (include/kartdiff.h).

The product path has no CPU fallback of its own: if the HIP library is missing or fails to load,
every engine call raises ``NativeUnavailable`` loudly.  (The reference-style CPU path that callers
fall back to on ``KD_EUNSUPPORTED`` is the caller's, i.e. Kart's own code, not ours.)
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KART_AMD_LIB", os.path.join(HERE, "libkartdiff.so"))

KD_OK = 0
KD_EINVAL = -1
KD_EHIP = -2
KD_EUNSUPPORTED = -3
KD_ENOTFOUND = -4
KD_WALK_ALL = -1
KD_NONE = 0xFFFFFFFF
KD_MEM_HOST = 0
KD_MEM_DEVICE = 1
KD_TE_BLOB = 0
KD_TE_TREE = 1
KD_TH_RANK_NAMES = 1
KD_KEY_INT = 0
KD_KEY_HASH = 1
KD_DIFF_UNORDERED = 0x1
KD_HEX_BYTES = 0
KD_HEX_GPKG_WKB = 1
KD_COPY_H2D = 1
KD_COPY_D2H = 2
KD_COPY_D2D = 3
KD_COMM_ID_BYTES = 128
KD_GH_GEOM, KD_GH_NULL, KD_GH_FALLBACK = 0, 2, 3
KD_GF_RECT = 0x1
KD_GF_DELTA_HEADS = 0x2  # the geometry heads are in delta order (slot d = delta d)
KD_GF_EXACT = 0x4  # kd_geom_refine: decide what FP64 cannot certify in exact arithmetic
# kd_inflate_batch's status of one stream (kartdiff.h KD_INF_*)
(KD_INF_OK, KD_INF_EHEADER, KD_INF_EBTYPE, KD_INF_ESTORED, KD_INF_ELENS, KD_INF_ESYMBOL, KD_INF_EDIST, KD_INF_EOVER,
 KD_INF_ESHORT, KD_INF_ESRC, KD_INF_EADLER, KD_INF_ERANGE) = range(12)
KD_INF_MAX = 256 << 10  # the largest blob kd_odb_read_batch_device inflates on the device
# kd_delta_apply_batch's status of one item (kartdiff.h KD_DL_*)
(KD_DL_OK, KD_DL_EHEADER, KD_DL_EBASE, KD_DL_ESIZE, KD_DL_EOP, KD_DL_ETRUNC, KD_DL_ECOPY, KD_DL_EOVER, KD_DL_ESHORT,
 KD_DL_EPARENT) = range(10)
KD_DL_ERANGE = 11
KD_DL_MAX_DEPTH = 64  # the deepest chain kd_odb_read_batch_device_ex rebuilds on the device
KD_RBD_DELTAS = 1     # kd_odb_read_batch_device_ex flag: delta chains rebuilt on the device
# kd_tree_join_batch's status of one task (kartdiff.h KD_TJ_*)
(KD_TJ_OK, KD_TJ_EMODE, KD_TJ_ENAME, KD_TJ_EOID, KD_TJ_ETREE, KD_TJ_EORDER, KD_TJ_EBIG, KD_TJ_ECAP) = range(8)
KD_TJ_ERANGE = 11
KD_TJ_MAX_BYTES = 1 << 30  # the largest tree the join takes
KD_WD_STATS = 24           # kd_walk_device's counters

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_i16p = ctypes.POINTER(ctypes.c_int16)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_dblp = ctypes.POINTER(ctypes.c_double)


class NativeUnavailable(RuntimeError):
    pass


class KdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkartdiff error {code}: {msg}")
        self.code = code


class Unsupported(KdError):
    """KD_EUNSUPPORTED: this input needs the reference CPU path."""


class NotFound(KdError):
    """KD_ENOTFOUND: a git object is not in the object database."""


class KdLeaves(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("path_off", c_u64p),
        ("mode", c_u32p),
        ("oid", c_u8p),
        ("path", c_u8p),
        ("present", ctypes.c_int32),
    ]


class KdTjOut(ctypes.Structure):
    """kd_tj_out (kd_tree_join_batch): one root's kept entries in kd_leaves layout, caller-owned arrays"""
    _fields_ = [
        ("cap_n", ctypes.c_uint64),
        ("cap_bytes", ctypes.c_uint64),
        ("path_off", ctypes.c_void_p),
        ("mode", ctypes.c_void_p),
        ("oid", ctypes.c_void_p),
        ("path", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64),
    ]


class KdSide(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("key", ctypes.c_void_p),
        ("oid", ctypes.c_void_p),
        ("name", ctypes.c_void_p),
        ("name_off", ctypes.c_void_p),
        ("mem", ctypes.c_uint32),
        ("key_mode", ctypes.c_uint32),
    ]


class KdTreeEntries(ctypes.Structure):
    """kd_tree_entries (kd_tree_hash): the (name, oid) entries of one level of git trees"""
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("name", ctypes.c_void_p),
        ("name_off", ctypes.c_void_p),
        ("oid", ctypes.c_void_p),
        ("kind", ctypes.c_uint32),
        ("mem", ctypes.c_uint32),
    ]


class KdBlobs(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("data", ctypes.c_void_p),
        ("off", ctypes.c_void_p),
        ("mem", ctypes.c_uint32),
        ("size_hint", ctypes.c_uint32),
    ]


class KdLegendMaps(ctypes.Structure):
    _fields_ = [
        ("n_keys", ctypes.c_int32),
        ("words", ctypes.c_int32),
        ("n_leg_old", ctypes.c_int32),
        ("n_leg_new", ctypes.c_int32),
        ("leg_old_hex", ctypes.c_void_p),
        ("map_old", ctypes.c_void_p),
        ("leg_new_hex", ctypes.c_void_p),
        ("map_new", ctypes.c_void_p),
        ("cmp_mask", ctypes.c_void_p),
    ]


class KdStep(ctypes.Structure):
    """kd_step (kd_diff2_step): the join's, the field diff's and the pk order's arguments"""
    _fields_ = [
        ("base", ctypes.POINTER(KdSide)),
        ("target", ctypes.POINTER(KdSide)),
        ("base_order", ctypes.c_void_p),
        ("target_order", ctypes.c_void_p),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("d_delta", ctypes.c_void_p),
        ("d_upd", ctypes.c_void_p),
        ("d_delta_key", ctypes.c_void_p),
        ("d_upd_key", ctypes.c_void_p),
        ("d_counts", ctypes.c_void_p),
        ("d_err", ctypes.c_void_p),
        ("old_blobs", ctypes.POINTER(KdBlobs)),
        ("new_blobs", ctypes.POINTER(KdBlobs)),
        ("d_pairs", ctypes.c_void_p),
        ("upd_cap", ctypes.c_uint64),
        ("maps", ctypes.POINTER(KdLegendMaps)),
        ("d_masks", ctypes.c_void_p),
        ("d_status", ctypes.c_void_p),
        ("pk_lo", ctypes.c_int64),
        ("pk_hi", ctypes.c_int64),
        ("delta_cap", ctypes.c_uint64),
        ("d_delta_pk", ctypes.c_void_p),
        ("d_delta_perm", ctypes.c_void_p),
        ("d_upd_pk", ctypes.c_void_p),
        ("d_upd_perm", ctypes.c_void_p),
    ]


class KdGeomCols(ctypes.Structure):
    _fields_ = [
        ("n_leg_old", ctypes.c_int32),
        ("n_leg_new", ctypes.c_int32),
        ("leg_old_hex", ctypes.c_void_p),
        ("gidx_old", ctypes.c_void_p),
        ("leg_new_hex", ctypes.c_void_p),
        ("gidx_new", ctypes.c_void_p),
    ]


class KdFilterPoly(ctypes.Structure):
    """kd_filter_poly: the filter polygon's closed rings (host memory)"""
    _fields_ = [
        ("xy", ctypes.c_void_p),
        ("ring_off", ctypes.c_void_p),
        ("n_ring", ctypes.c_uint64),
        ("n_vert", ctypes.c_uint64),
    ]


class KdKeysInfo(ctypes.Structure):
    _fields_ = [
        ("vary", ctypes.c_uint64),
        ("key0", ctypes.c_uint64),
        ("pk_min", ctypes.c_int64),
        ("pk_max", ctypes.c_int64),
        ("ascending", ctypes.c_int32),
        ("seg_max", ctypes.c_int32),  # longest run of keys sharing their top 24 (bucket) bits; -1: buckets descend
    ]


class KdKeypackInfo(ctypes.Structure):
    """kd_keypack_info (kd_pack_keys_device): the scan of the keys as written and the refused entries"""
    _fields_ = [
        ("info", KdKeysInfo),
        ("bad", ctypes.c_uint64),
        ("first_bad", ctypes.c_uint64),  # 2**64 - 1 when bad == 0
    ]


class KdDiffResult(ctypes.Structure):
    _fields_ = [
        ("n_insert", ctypes.c_uint64),
        ("n_update", ctypes.c_uint64),
        ("n_delete", ctypes.c_uint64),
        ("n_delta", ctypes.c_uint64),
        ("delta", c_u32p),
        ("upd", c_u32p),
    ]


class KdMergeResult(ctypes.Structure):
    _fields_ = [
        ("n_clean", ctypes.c_uint64),
        ("n_conflict", ctypes.c_uint64),
        ("n_mdelta", ctypes.c_uint64),
        ("conflict", c_u32p),
        ("mdelta", c_u32p),
    ]


# name -> (restype, argtypes); every symbol include/kartdiff.h declares
SIGNATURES = {
    "kd_abi_version": (ctypes.c_int, []),
    "kd_last_error": (ctypes.c_char_p, []),
    "kd_init": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "kd_fini": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "kd_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "kd_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "kd_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]),
    "kd_free": (None, [ctypes.c_void_p]),
    "kd_diff2": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_uint32,
         ctypes.POINTER(ctypes.POINTER(KdDiffResult))],
    ),
    "kd_diff2_device": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_uint32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_fielddiff": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdBlobs), ctypes.POINTER(KdBlobs), ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(KdLegendMaps),
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_find_renames": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint32],
    ),
    "kd_tree_hash": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdTreeEntries), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32],
    ),
    "kd_merge3": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.POINTER(KdSide),
         ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(KdMergeResult))],
    ),
    "kd_merge3_device": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.POINTER(KdSide),
         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_merge3_device_perm": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "kd_envelopes": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdBlobs), c_dblp, ctypes.c_int, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, c_u64p],
    ),
    "kd_env_overlap": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, c_dblp, ctypes.c_void_p,
         ctypes.c_uint32],
    ),
    "kd_geom_heads": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "kd_geom_filter_heads": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, c_dblp,
         ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint32],
    ),
    "kd_geom_filter_deltas": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(KdBlobs),
         ctypes.POINTER(KdBlobs), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, c_dblp, ctypes.c_uint32, ctypes.c_int,
         ctypes.c_void_p, ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_geom_refine": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdFilterPoly), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_uint32, ctypes.POINTER(KdBlobs), ctypes.POINTER(KdBlobs), ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_orient2d_exact_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "kd_shard_cuts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kd_sf_index_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                          ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    "kd_sf_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     c_dblp, ctypes.c_void_p, ctypes.c_uint32]),
    "kd_sf_index_free": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_geom_filter": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdBlobs), ctypes.POINTER(KdBlobs), ctypes.c_void_p, ctypes.c_uint64,
         ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(KdGeomCols), c_dblp, ctypes.c_uint32, ctypes.c_int,
         ctypes.c_void_p, ctypes.c_void_p, c_u64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_hex_encode": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdBlobs), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_sort_side": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_void_p]),
    "kd_diff2_device_perm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "kd_sort_side_into": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.POINTER(KdKeysInfo)]),
    "kd_keys_scan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(KdKeysInfo)]),
    "kd_sort_segmented_into": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "kd_delta_pk_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide),
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "kd_diff2_device_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    "kd_diff2_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(KdStep)]),
    "kd_malloc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "kd_mfree": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "kd_host_alloc": (ctypes.c_int, [ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "kd_host_free": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_memcpy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]),
    "kd_memset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64]),
    "kd_device_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_comm_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "kd_comm_fini": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_comm_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "kd_allgather_u64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "kd_diff2_gather": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_uint64, ctypes.c_uint64,
         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_diff2_gather_begin": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_uint64, ctypes.c_uint64,
         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_diff2_gather_end": (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    ),
    "kd_diff2_sharded": (
        ctypes.c_int,
        [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(KdSide), ctypes.POINTER(KdSide), ctypes.c_int,
         ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(KdDiffResult))],
    ),
    "kd_pack_int_keys": (
        ctypes.c_int64,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_pack_hash_keys": (
        ctypes.c_int64,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
         ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_int_keys_to_pks": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "kd_pack_keys_device": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kd_odb_open": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]),
    "kd_odb_close": (ctypes.c_int, [ctypes.c_void_p]),
    "kd_odb_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "kd_odb_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    "kd_odb_read": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(c_u8p), c_u64p],
    ),
    "kd_odb_read_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(c_u8p), ctypes.c_void_p,
         ctypes.c_void_p],
    ),
    "kd_inflate_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_odb_read_batch_device": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(KdBlobs),
         ctypes.c_void_p, c_u64p],
    ),
    "kd_delta_apply_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_odb_read_batch_device_ex": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32,
         ctypes.POINTER(KdBlobs), ctypes.c_void_p, c_u64p],
    ),
    "kd_walk": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
         ctypes.POINTER(ctypes.POINTER(KdLeaves))],
    ),
    "kd_walk_device": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
         ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(KdLeaves)), c_u64p],
    ),
    "kd_tree_join_batch": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
         ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(KdTjOut),
         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32],
    ),
    "kd_prof_enable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "kd_prof_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "kd_prof_get": (
        ctypes.c_int,
        [ctypes.c_void_p, ctypes.c_char_p, c_u64p, c_dblp],
    ),
    "kd_prof_reset": (ctypes.c_int, [ctypes.c_void_p]),
}

_lib = None


def lib():
    """Load libkartdiff.so once; raise NativeUnavailable (never silently fall back).  The library
    needs no GPU framework: it allocates, copies and communicates itself (kd_malloc, kd_memcpy,
    kd_comm_*)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(
                f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
            )
        try:
            L = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise NativeUnavailable(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc == KD_OK:
        return
    msg = lib().kd_last_error().decode(errors="replace")
    if rc == KD_EUNSUPPORTED:
        raise Unsupported(rc, f"{what}: {msg}")
    if rc == KD_ENOTFOUND:
        raise NotFound(rc, f"{what}: {msg}")
    raise KdError(rc, f"{what}: {msg}")


def ptr(a):
    """data pointer of a numpy array (or None)"""
    if a is None:
        return None
    return a.ctypes.data
