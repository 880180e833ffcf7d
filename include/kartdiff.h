/*
 * kartdiff.h — C ABI of libkartdiff.so, the MI355X (gfx950) bulk feature-diff engine.
 *
 * Drop-in boundary.  Each entry point replaces one reference interface:
 *
 *   kd_diff2       <- libgit2 tree-to-tree diff as consumed by RichBaseDataset.diff_feature
 *                     (/root/reference/kart/rich_base_dataset.py:205-300; the FFI call is
 *                     Tree.diff_to_tree at :212-232).  Returns the insert/update/delete delta set.
 *   kd_fielddiff   <- Dataset3.get_feature (kart/dataset3.py:185-223) + Schema.feature_from_raw_dict
 *                     (kart/schema.py:288-293) + the per-field Python `==` compare of
 *                     TextDiffWriter.write_feature_delta (kart/text_diff_writer.py:135-145).
 *   kd_find_renames <- WorkingCopy.find_renames (kart/working_copy/base.py:829-854) for a commit<>commit
 *                     diff, the TODO at kart/rich_base_dataset.py:233: deletes and inserts whose blob
 *                     OIDs are equal (Schema.hash_feature(.., without_pk=True), kart/schema.py:314-335)
 *                     paired on the GPU, at any size (the reference caps its pass at 400 deltas, :688).
 *   kd_merge3      <- repo.merge_trees(ancestor, ours, theirs) (kart/merge.py:99-100; libgit2
 *                     git_merge_trees) feeding MergeIndex.from_pygit2_index (kart/merge_util.py:92-103).
 *   kd_tree_hash   <- index.write_tree(repo) (kart/merge.py:122; libgit2 git_index_write_tree): the ids
 *                     and bodies of one level of git tree objects, SHA-1 on the GPU.
 *   kd_envelopes   <- SpatialFilter.matches envelope quick-check (kart/spatial_filter/__init__.py:534-590,
 *                     709-734) + get_envelope_for_indexing/EnvelopeEncoder.encode for an identity
 *                     CRS (kart/spatial_filter/index.py:485-579,639-707).
 *   kd_env_overlap <- sf_filter_blob decode + cyclic_range_overlaps
 *                     (vendor/spatial-filter/spatial_filter.cpp:170-260).
 *   kd_sf_index_build / kd_sf_filter
 *                  <- sf_filter_blob (vendor/spatial-filter/spatial_filter.cpp:212-260): the clone-time
 *                     spatial filter over a batch of object ids against feature_envelopes.
 *   kd_geom_filter <- BaseDiffWriter.filtered_ds_feature_deltas (kart/base_diff_writer.py:279-329):
 *                     the geometry of each delta's old/new feature blob, envelope-tested, kept
 *                     deltas compacted on the GPU.  kd_geom_heads + kd_geom_filter_heads: the same
 *                     from 48-byte geometry heads the blob reader extracts on the host.
 *   kd_geom_refine <- SpatialFilter.matches' exact test (kart/spatial_filter/__init__.py:534-590, the
 *                     prepared filter polygon's Intersects): the filter's candidates decided on the
 *                     GPU wherever FP64 certifies the answer, the rest left to the caller.
 *   kd_hex_encode  <- Geometry.to_hex_wkb / gpkg_geom_to_hex_wkb (kart/geometry.py:346-375) and
 *                     bytes.hex(v), as feature_as_json formats them (kart/feature_output.py:34-56).
 *   kd_diff2_sharded / kd_diff2_gather
 *                  <- the same diff split by dataset3 path-bucket range over several GPUs (the
 *                     reference's own sharding idea: kart/fast_import.py:289-337), counts and
 *                     compacted delta records all-gathered over RCCL (xGMI).
 *   kd_malloc / kd_memcpy / kd_host_alloc ...
 *                  device HBM and pinned host staging for callers without a GPU framework.
 *   kd_pack_*      <- Dataset3.decode_path_to_1pk / PathEncoder (kart/dataset3.py:250-259,
 *                     kart/dataset3_paths.py:202-215,292-299): host-side key packing.
 *   kd_odb_* / kd_walk
 *                  <- libgit2's ODB reads and tree iteration under Dataset3 (kart/dataset3.py:
 *                     26-35,225-231; kart/base_dataset.py:230-265), with diff_to_tree's subtree
 *                     pruning: the leaves the packer above consumes, read natively.
 *
 * Conventions: plain pointers and sizes only; return 0 on success, KD_EINVAL (-1) on bad
 * arguments, KD_EHIP (-2) on a HIP runtime error, KD_EUNSUPPORTED (-3) when the input needs
 * the CPU path (caller falls back); kd_last_error() gives a thread-local message.  One kd_ctx per
 * GPU; calls on one context are serialised by the caller.  Index arrays are uint32 (a side may
 * hold at most 2^32-2 entries per GPU); KD_NONE marks "absent".
 */
#ifndef KARTDIFF_H
#define KARTDIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KD_ABI_VERSION 1

#define KD_OK 0
#define KD_EINVAL (-1)
#define KD_EHIP (-2)
#define KD_EUNSUPPORTED (-3)

#define KD_NONE 0xFFFFFFFFu

/* where a buffer lives */
#define KD_MEM_HOST 0u
#define KD_MEM_DEVICE 1u

/* key modes (see DESIGN.md "join key") */
#define KD_KEY_INT 0u  /* IntPathEncoder: key = rank24(bucket) | wrap34 | frank(pk), bijective with
                          pk and ascending in git's tree order (DESIGN.md "join key")            */
#define KD_KEY_HASH 1u /* MsgpackHashPathEncoder: key = rank-mapped bucket bits | FNV-1a(filename)
                          bits; matched keys are verified against the filename bytes           */

typedef struct kd_ctx kd_ctx;

/* One commit's dataset feature tree, flattened: n leaf entries sorted by strictly ascending key.
 * KD_KEY_INT keys of a tree walk's leaves are ascending as listed (git tree order), unless a leaf
 * tree mixes pks of different 2^30 wraps; KD_KEY_HASH leaves need kd_sort_segmented_into. */
typedef struct kd_side {
    uint64_t n;
    const uint64_t* key;      /* [n] join keys, strictly ascending                                 */
    const uint8_t* oid;       /* [n*20] git blob OIDs (raw bytes)                                  */
    const uint8_t* name;      /* KD_KEY_HASH only: concatenated filenames (may be NULL for INT)    */
    const uint64_t* name_off; /* [n+1] offsets into name (KD_KEY_HASH only)                        */
    uint32_t mem;             /* KD_MEM_HOST or KD_MEM_DEVICE: where the arrays above live         */
    uint32_t key_mode;        /* KD_KEY_INT or KD_KEY_HASH                                         */
} kd_side;

/* A blob arena: blob b = data[off[b] .. off[b+1]).  Feature blobs are msgpack
 * [legend_hex40, [values...]] (kart/dataset3.py:185-215); geometry blobs are GPKG binary. */
typedef struct kd_blobs {
    uint64_t n;
    const uint8_t* data;
    const uint64_t* off; /* [n+1] */
    uint32_t mem;
    uint32_t size_hint; /* typical (mean) blob size in bytes (0 = unknown); sizes the LDS staging pool */
} kd_blobs;

/* Legend -> union-key maps for kd_fielddiff (host memory).  Union keys are the old schema's
 * column names in order, then the new schema's names not in the old one
 * (BaseDiffWriter._all_feature_keys, kart/base_diff_writer.py:181-187).
 * map[l*n_keys + k] = value index in legend l's non-pk array, or
 *   -1 key not in that side's schema (_NULL), -2 column absent from the legend (None),
 *   -3 the primary-key column (value from the path). */
typedef struct kd_legend_maps {
    int32_t n_keys;
    int32_t words;            /* ceil(n_keys / 64): uint64 mask words per update */
    int32_t n_leg_old;
    int32_t n_leg_new;
    const uint8_t* leg_old_hex; /* [n_leg_old*40] legend hexhash strings */
    const int16_t* map_old;     /* [n_leg_old*n_keys] */
    const uint8_t* leg_new_hex;
    const int16_t* map_new;
    const uint64_t* cmp_mask;   /* [words] keys to compare ("__"-prefixed keys are excluded) */
} kd_legend_maps;

typedef struct kd_diff_result {
    uint64_t n_insert, n_update, n_delete, n_delta;
    uint32_t* delta;  /* [2*n_delta] (base index | KD_NONE, target index | KD_NONE), key order */
    uint32_t* upd;    /* [2*n_update] (base index, target index) of the updates, key order     */
} kd_diff_result;

typedef struct kd_merge_result {
    uint64_t n_clean;     /* merged entries present without conflict                          */
    uint64_t n_conflict;
    uint64_t n_mdelta;    /* entries where the merge result differs from ours                 */
    uint32_t* conflict;   /* [3*n_conflict] (ancestor, ours, theirs) index | KD_NONE          */
    uint32_t* mdelta;     /* [2*n_mdelta] (ours | KD_NONE, theirs | KD_NONE): take theirs     */
} kd_merge_result;

/* -------- context -------- */
int kd_abi_version(void);
const char* kd_last_error(void);
/* Creates the context and warms the first-diff path (runtime copy kernels, DMA queues, the pinned
 * staging chunks, one 1 + 1-entry classify2), so a one-shot process's first diff runs warm. */
int kd_init(int device_ordinal, kd_ctx** out);
int kd_fini(kd_ctx* ctx);
/* Launch on an external HIP stream (e.g. torch's current stream); NULL = the context's own. */
int kd_set_stream(kd_ctx* ctx, void* hip_stream);
/* Tuning options of a context (A/B switches of the measured alternatives; defaults are the measured
 * optima).  kd_init seeds each from the environment variable in brackets, once; kd_set_option changes
 * it for later calls on the context.  Unknown names: KD_EINVAL.
 *   merge3_join    [KD_MERGE3_JOIN]    1: one-pass three-way join (k_join3b); 0: classify2 + k_resolve3
 *   j2_oidlds_min  [KD_J2_OIDLDS_MIN]  k_join2 stages OIDs in LDS from this many entries (2^26)
 *   j2_walk        [KD_J2_WALK]        the join tile's work out of LDS: 1 (default) guided split search (a verified
 *                                      bracket around the proportional guess, the blind search when a wave's
 *                                      bracket fails), a walk without per-item guards in full waves, and in
 *                                      k_join2 the complete order check as straight-line reads issued with
 *                                      the search's first; 0: the blind 4-ary search, guarded walk and looped
 *                                      check.  Same results either way
 *   fd_stream      [KD_FD_STREAM]      -1 auto, 0 windowed, 1 streamed field diff (contiguous arenas)
 *   fd_walk        [KD_FD_WALK]        -1 / 0 off, 1 the walked field diff (A/B)
 *   pkm_max_blocks [KD_PKM_MAX_BLOCKS] largest pk range (64-pk blocks) kd_delta_pk_order places by bitmap
 *   trace_host     [KD_TRACE_HOST]     1: stream-synced wall-clock marks of host phases to stderr
 *   step_overlap   [KD_STEP_OVERLAP]   kd_diff2_step's schedule: 0 every kernel on the context's stream, in
 *                                      the order of the separate calls; 1 / 2: the placement and the pk order
 *                                      on a side stream beside the field diff, which is queued first (1) or
 *                                      after them (2).  Default 1
 *   step_overlap_min [KD_STEP_OVERLAP_MIN] the side stream is used from this many entries of both sides
 *                                      together (2^26: below, the two cross-stream waits cost more than a
 *                                      short field diff hides)
 *   step_count     [KD_STEP_COUNT]     1 (default): where kd_diff2_step uses the side stream and the field diff
 *                                      reads update-order arenas, the field diff takes the update count from
 *                                      partial counters the join leaves and is queued directly behind the join;
 *                                      the group scan leads the side stream.  0: the scan in front of the fork
 *   pkm_wave       [KD_PKM_WAVE]       the bitmap pk order's scans in their LDS-free one-wave-per-chunk form:
 *                                      -1 on kd_diff2_step's side stream only, 0 never, 1 always */
int kd_set_option(kd_ctx* ctx, const char* name, int64_t value);
int kd_get_option(kd_ctx* ctx, const char* name, int64_t* value);
int kd_sync(kd_ctx* ctx);
/* Pre-size device workspaces so the first timed call does not allocate. */
int kd_reserve(kd_ctx* ctx, uint64_t max_entries_per_side, uint64_t max_updates);
void kd_free(void* p); /* frees kd_diff_result / kd_merge_result and their arrays */

/* -------- two-way diff: classify2 (+ optional fused field diff) -------- */
/* Host-convenience form: sides may be host or device; results are host memory (kd_free). */
int kd_diff2(kd_ctx* ctx, const kd_side* base, const kd_side* target, uint32_t flags,
             kd_diff_result** out);
/* flags for kd_diff2 / kd_diff2_device */
#define KD_DIFF_UNORDERED 0x1u /* device form only: deltas/updates grouped per 1024-pair tile, tiles in
                                  completion order (each tile key-ordered) — skips the ordering
                                  scan + scatter; the delta SET is identical                      */

/* Device form: everything device-resident, asynchronous on the context stream.
 * d_delta / d_upd capacity must cover the worst case (base.n + target.n pairs).
 * d_counts[4] <- inserts, updates, deletes, deltas.  d_err <- nonzero if a side is not strictly
 * ascending (1) or a KD_KEY_HASH key matched two different filenames (2). */
int kd_diff2_device(kd_ctx* ctx, const kd_side* base, const kd_side* target, uint32_t flags,
                    uint32_t* d_delta, uint32_t* d_upd, uint64_t* d_counts, uint32_t* d_err);

/* Late-materialised form, what follows kd_sort_side_into(..., d_oid_out = NULL, ...): each side's
 * keys are sorted but its OIDs (and KD_KEY_HASH filename offsets) are still in the order the tree
 * walk produced them; row order[i] belongs to sorted entry i.  The join reads OIDs through the order
 * (one extra coalesced 4-B load per matched entry), so no side's OIDs are ever permuted.  Results are
 * identical to kd_diff2_device on the permuted sides (indices are sorted-entry indices). */
int kd_diff2_device_perm(kd_ctx* ctx, const kd_side* base, const kd_side* target, const uint32_t* base_order,
                         const uint32_t* target_order, uint32_t flags, uint32_t* d_delta, uint32_t* d_upd,
                         uint64_t* d_counts, uint32_t* d_err);

/* kd_diff2_device / kd_diff2_device_perm with more outputs: base_order / target_order (both or
 * NULL) as kd_diff2_device_perm; d_delta_key [cap] / d_upd_key [cap] (optional, device) <- the join key
 * of every delta / update record, written beside the lists (what kd_delta_pk_order reads instead of
 * gathering them from the sides). */
int kd_diff2_device_ex(kd_ctx* ctx, const kd_side* base, const kd_side* target, const uint32_t* base_order,
                       const uint32_t* target_order, uint32_t flags, uint32_t* d_delta, uint32_t* d_upd,
                       uint64_t* d_delta_key, uint64_t* d_upd_key, uint64_t* d_counts, uint32_t* d_err);

/* -------- field diff -------- */
/* For each update u: old blob = old->data[old->off[pu[2u]] ..], new blob = neu->...[pu[2u+1]]
 * (pu = the (base, target) update pairs, or NULL: blob u on both sides).  masks[u*words + w]
 * bit k set iff union key k changed under Python `==`.  status[u]: 0 ok, 1 malformed blob,
 * 2 unknown legend, 3 too many values, 4 unsupported value (nested container, invalid ext 'G'):
 * nonzero -> the caller recomputes that update on the CPU path.  masks[u] is all zero wherever
 * status[u] != 0, whatever was found before the failure.  A compared key whose value index lies
 * at or beyond the blob's value count gives status 1 (after status 4: a malformed value or
 * trailing bytes win).
 * pairs_mem / out_mem say where pu and masks/status live.  Device form: with d_n_upd != NULL the
 * update count is read from that device counter (no host sync between classify and diff), pu
 * and the outputs must be device memory, and n_upd is the capacity — an upper bound of *d_n_upd
 * used to size the grid (0 = unknown). */
int kd_fielddiff(kd_ctx* ctx, const kd_blobs* old_blobs, const kd_blobs* new_blobs,
                 const uint32_t* pu, uint64_t n_upd, const uint64_t* d_n_upd, uint32_t pairs_mem,
                 const kd_legend_maps* maps, uint64_t* masks, uint8_t* status, uint32_t out_mem);

/* -------- renames: deletes and inserts paired by blob OID -------- */
/* <- WorkingCopy.find_renames (kart/working_copy/base.py:829-854) for a commit<>commit diff, the TODO
 * at kart/rich_base_dataset.py:233: blob OID == Schema.hash_feature(.., without_pk=True)
 * (kart/schema.py:314-335; a V3 feature blob is msg_pack([legend hash, non-pk values]), the pk lives in
 * the path: kart/dataset3.py:261-272), for features stored under the current legend.
 *
 * delta [n_delta] = the (base index | KD_NONE, target index | KD_NONE) records of a two-way diff in its
 * key order.  A delete has only a base index, an insert only a target index; updates, and records whose
 * index lies outside its side, are ignored.  For every OID (all 20 bytes) that occurs on at least one
 * delete and at least one insert, the delete with the largest delta index is paired with the insert
 * with the largest delta index (the reference's two dicts, filled in iteration order); every other
 * delta of that OID stays.  ren[k] = (delta index of the delete, delta index of the insert), ascending
 * by the delete's delta index; *n_ren = the number of pairs.  A pure function of the inputs, bitwise
 * reproducible.  A caller diffing in reverse swaps the pair columns: the pairing is symmetric.
 *
 * Only n, oid and mem of the sides are read (oid 4-byte aligned).  base_order / target_order (both or
 * NULL, in the memory of their side) as kd_diff2_device_perm: the OID of sorted entry i is
 * oid[order[i]].  list_mem / out_mem say where delta and ren / n_ren live; host lists and outputs are
 * staged by the library (the call then returns with the results).  With d_n_delta != NULL the count is
 * read on the device, n_delta is the capacity (it sizes the grid and the workspace), delta, ren and
 * n_ren must be device memory and the call is asynchronous; no record beyond the device count
 * influences the result.  ren needs room for min(deletes, inserts) pairs (n_delta / 2 always does).
 * Workspace (grow-only, kept by the context): 20 bytes per delta of n_delta for the lists and a
 * table of 16 bytes times the power of two at or above 2 * min(n_delta, base->n), so pass the
 * tightest n_delta the caller knows.
 * KD_EINVAL: NULL where a pointer is required, one order without the other, n_delta > 2^32 - 2. */
int kd_find_renames(kd_ctx* ctx, const kd_side* base, const kd_side* target,
                    const uint32_t* base_order, const uint32_t* target_order,
                    const uint32_t* delta, uint64_t n_delta, const uint64_t* d_n_delta, uint32_t list_mem,
                    uint32_t* ren, uint64_t* n_ren, uint32_t out_mem);

/* -------- git tree objects: ids and bodies of one level of trees -------- */
/* <- index.write_tree(repo) (kart/merge.py:122).  Tree t consists of entries seg[t] .. seg[t+1] of e.
 * Its body is the concatenation of "<mode> <name>\0<20 oid bytes>" over them, mode "100644" for
 * KD_TE_BLOB and "40000" for KD_TE_TREE (one kind per call); its id is
 * SHA1("tree " + decimal(len(body)) + "\0" + body).  An empty run gives git's empty tree,
 * 4b825dc642cb6eb9a060e54bf8d69288fbee4904.  A pure function of the inputs, bitwise reproducible.
 *
 * status[t]: 0 ok; 1 the run is not strictly ascending in git's order (without KD_TH_RANK_NAMES);
 * 2 two entries of the run share a name (with it); 3 a name is empty, longer than 255 bytes, or holds
 * '/' or NUL.  Where several apply the largest is reported.  Where status is non-zero the id is 20
 * zero bytes, the body is empty and body_off[t+1] == body_off[t].
 * Git's order: names compare as unsigned bytes; a blob's name as if it ended in NUL (a prefix comes
 * first: a, a-, a0, ab), a tree's as if it ended in '/' (a-, a, a0, ab).  The rule of e->kind is used.
 * KD_TH_RANK_NAMES (KD_TE_BLOB only, else KD_EINVAL): the entries of a run arrive in any order and are
 * ordered by the blob rule before formatting (a KD_KEY_HASH side in key order is grouped by leaf tree
 * but not in filename order inside one); runs of up to 512 entries, a longer one: KD_EUNSUPPORTED.
 * Without the flag a run may have any length.
 *
 * name_off[n+1] are byte offsets into name, ascending; oid and tree_oid are 4-byte aligned, and
 * tree_oid has the layout of kd_tree_entries.oid, so a device-resident level is the next level's
 * oid array as it stands.  seg lives where e's arrays live (e->mem); out_mem says where tree_oid,
 * status, body and body_off live.  body / body_off (both or neither): the object payloads without
 * the "tree <len>\0" header, tree t's at body[body_off[t] .. body_off[t+1]]; KD_EINVAL when body_cap is
 * below body_off[n_trees].  Host arrays are staged by the library and the call returns with the
 * results.  With device outputs the hashing is queued on the context's stream and the call returns
 * without waiting for it; every call waits once, after the sizing kernels, for 32 bytes (the arena's
 * size, the body bytes, the long-run flag) that size the arena and decide the two errors above.
 * Host seg and name_off are checked (KD_EINVAL if they descend or run past n); device ones are
 * clamped to the entries and the name bytes there are.
 * Workspace (grow-only, kept by the context): 4 bytes per entry (8 with KD_TH_RANK_NAMES), 44 bytes
 * per tree, and an arena of every object padded to SHA-1's 64-byte blocks: the body bytes plus
 * between 16 and 98 bytes per tree; host arrays add their device copies.
 * KD_EINVAL: NULL where a pointer is required, an unknown kind or flag, body without body_off,
 * n or n_trees above 2^32 - 2. */
#define KD_TE_BLOB 0u        /* every entry is "100644 <name>\0<oid>" */
#define KD_TE_TREE 1u        /* every entry is "40000 <name>\0<oid>"  */
#define KD_TH_RANK_NAMES 1u  /* entries of a run may arrive in any order (KD_TE_BLOB only) */

typedef struct kd_tree_entries {
    uint64_t n;
    const uint8_t* name;
    const uint64_t* name_off; /* [n+1] */
    const uint8_t* oid;       /* [n*20], 4-byte aligned */
    uint32_t kind;            /* KD_TE_BLOB | KD_TE_TREE, one kind per call */
    uint32_t mem;             /* KD_MEM_HOST | KD_MEM_DEVICE */
} kd_tree_entries;

int kd_tree_hash(kd_ctx* ctx, const kd_tree_entries* e, const uint64_t* seg, uint64_t n_trees, uint32_t flags,
                 uint8_t* tree_oid, uint8_t* status, uint8_t* body, uint64_t* body_off, uint64_t body_cap,
                 uint32_t out_mem);

/* -------- three-way merge classification -------- */
int kd_merge3(kd_ctx* ctx, const kd_side* ancestor, const kd_side* ours, const kd_side* theirs,
              uint32_t flags, kd_merge_result** out);
/* Device form of kd_merge3 (no host sync): all three sides in device memory; d_conflict
 * [(a.n + o.n + t.n) * 3] <- conflict triples (ancestor, ours, theirs index, 0xFFFFFFFF = absent)
 * in path order, d_mdelta [(o.n + t.n) * 2] <- merge deltas, d_counts[4] <- clean entries,
 * conflicts, merge deltas, 0; d_err <- 1 unsorted side, 2 hash key collision, 8 tile overflow. */
int kd_merge3_device(kd_ctx* ctx, const kd_side* ancestor, const kd_side* ours, const kd_side* theirs,
                     uint32_t flags, uint32_t* d_conflict, uint32_t* d_mdelta, uint64_t* d_counts,
                     uint32_t* d_err);

/* Late-materialised form (after kd_sort_segmented_into / kd_sort_side_into without OIDs): keys
 * sorted, each side's OIDs and KD_KEY_HASH filename offsets still in walk order, row order[i]
 * belonging to sorted entry i.  Results identical to kd_merge3_device on the permuted sides. */
int kd_merge3_device_perm(kd_ctx* ctx, const kd_side* ancestor, const kd_side* ours, const kd_side* theirs,
                          const uint32_t* ancestor_order, const uint32_t* ours_order, const uint32_t* theirs_order,
                          uint32_t flags, uint32_t* d_conflict, uint32_t* d_mdelta, uint64_t* d_counts,
                          uint32_t* d_err);

/* -------- spatial -------- */
/* Per geometry blob (GPKG; length 0 = null geometry):
 *   match[i]: 0 NON_MATCHING, 1 CANDIDATE (bbox passed; exact GEOS test is the caller's),
 *             2 MATCHING (null geometry), 3 FALLBACK (needs the CPU path)
 *   enc[i*bits/2 ..] EnvelopeEncoder bytes of the identity-CRS index envelope; enc_ok[i]=1 when
 *   the spatial indexer would store a row.
 * filt_env = (min-x, max-x, min-y, max-y) of the filter (SpatialFilter.filter_env). */
int kd_envelopes(kd_ctx* ctx, const kd_blobs* geoms, const double filt_env[4], int bits,
                 uint8_t* match, uint8_t* enc, uint8_t* enc_ok, uint32_t out_mem,
                 uint64_t* n_candidates);
/* Decode n encoded envelopes (bits/2 bytes each) and test them against q = (w, s, e, n):
 * out[i] = cyclic(w,e) && range(s,n) overlap (spatial_filter.cpp:187-260). */
int kd_env_overlap(kd_ctx* ctx, const uint8_t* enc, uint64_t n, int bits, const double q[4],
                   uint8_t* out, uint32_t mem);

/* -------- clone-time spatial filter -------- */
/* sf_filter_blob (vendor/spatial-filter/spatial_filter.cpp:212-260) for a batch of objects.  The
 * feature_envelopes table (blob id -> EnvelopeEncoder bytes, bits/2 each: bits = 8 * bytes / 4 as
 * the reference derives it) is loaded once into HBM: oid [n*20] and env [n*bits/2] in any row order
 * (mem: where they live).  kd_sf_filter answers m objects: oid [m*20] (4-byte aligned), is_feature
 * [m] (may be NULL = all are feature blobs: 1 when the object's path contains
 * "/.table-dataset/feature/" or "/.sno-dataset/feature/"), q = (w, s, e, n) of the filter;
 * result[i] = 0 MATCH (not a feature, not in the index, or the envelope overlaps), 1 NOT_MATCHED,
 * 2 ERROR (an inverted range reached by range_overlaps, per object as the reference decides it: a
 * query with south > north errors only the objects whose longitude range overlaps). */
typedef struct kd_sf_index kd_sf_index;
int kd_sf_index_build(kd_ctx* ctx, const uint8_t* oid, const uint8_t* env, uint64_t n, int bits, uint32_t mem,
                      kd_sf_index** out);
int kd_sf_filter(kd_ctx* ctx, const kd_sf_index* index, const uint8_t* oid, const uint8_t* is_feature, uint64_t m,
                 const double q[4], uint8_t* result, uint32_t mem);
int kd_sf_index_free(kd_sf_index* index);

/* -------- spatially filtered diff -------- */
/* BaseDiffWriter.filtered_ds_feature_deltas (kart/base_diff_writer.py:279-329) with
 * SpatialFilter.matches (kart/spatial_filter/__init__.py:534-605): for every delta, the geometry
 * column is located in the old and new feature blobs (legend -> value position), its GPKG
 * envelope (or point) tested against the filter envelope in FP64.  Per side (match[2d], match[2d+1]):
 *   0 NON_MATCHING, 1 CANDIDATE (bbox passes: the exact Intersects is the caller's),
 *   2 MATCHING (null geometry / no geometry column / inside a KD_GF_RECT filter),
 *   3 FALLBACK (the caller decides on the CPU: unknown legend, nested value, envelope needs OGR),
 *   4 NONEXISTENT (KD_NONE side).  Empty geometries are NON_MATCHING (Intersects(empty) is false).
 * keep[0..*n_keep) <- the delta indices (in delta order) with either side 1, 2 or 3.
 * enc/enc_ok (optional, NULL): the new side's spatial-index envelope (EnvelopeEncoder, bits/2
 * bytes per delta), as kd_envelopes computes it.  pairs = (old blob | KD_NONE, new blob | KD_NONE)
 * per delta — classify2's delta list with the arenas indexed by sorted entry.  With d_n the count
 * is read on the device (pairs and outputs device memory, n = capacity: an upper bound of the
 * count, the kernels do not clamp).  match must be 2-B aligned.
 * Validation: kd_geom_filter locates the geometry value in a blob and reads nothing after that
 * value's last byte.  A blob malformed only behind it (trailing bytes, a truncated later value) is
 * answered as its well-formed twin; damage at or before that byte is 3 FALLBACK.  The heads forms
 * (kd_geom_heads validates the whole blob, as msgpack.unpackb does) answer 3 for both. */
#define KD_GF_RECT 0x1u /* the filter geometry is its own envelope (an axis-aligned rectangle) */
/* kd_geom_filter_heads / kd_geom_filter_deltas: the heads are already in delta order — heads_old[d] /
 * heads_new[d] belong to delta d (an absent side's slot is never read), as the drop-in's blob reader
 * lays them out after classification; pairs then give each side's presence and its blob in the
 * arenas (the slow path).  n_old and n_new must each cover whole 64-delta chunks of the capacity
 * (>= ceil(n / 64) * 64; heads device memory in kd_geom_filter_deltas). */
#define KD_GF_DELTA_HEADS 0x2u
typedef struct kd_geom_cols {
    int32_t n_leg_old, n_leg_new;
    const uint8_t* leg_old_hex; /* [n_leg_old*40] legend hexhashes (host memory) */
    const int16_t* gidx_old;    /* [n_leg_old] value index of the geometry column, -1 none */
    const uint8_t* leg_new_hex;
    const int16_t* gidx_new;
} kd_geom_cols;
int kd_geom_filter(kd_ctx* ctx, const kd_blobs* old_blobs, const kd_blobs* new_blobs, const uint32_t* pairs,
                   uint64_t n, const uint64_t* d_n, uint32_t pairs_mem, const kd_geom_cols* cols,
                   const double filt_env[4], uint32_t flags, int bits, uint8_t* match, uint32_t* keep,
                   uint64_t* n_keep, uint8_t* enc, uint8_t* enc_ok, uint32_t out_mem);

/* Geometry heads (host, multithreaded): the filtered diff from 48 contiguous bytes per blob.  For
 * each feature blob (msgpack [legend_hex, [values]]) the geometry column's value is located as
 * msgpack.unpackb + Dataset3.get_feature would (kart/dataset3.py:185-223; the whole blob validated:
 * nested values skipped, trailing bytes refused) and its GPKG bytes summarised: */
#define KD_GH_GEOM 0u     /* a geometry: gpkg[] = its first min(glen, 40) bytes (header + XY envelope) */
#define KD_GH_NULL 2u     /* null geometry, or no geometry column in the blob's legend (MATCHING)    */
#define KD_GH_FALLBACK 3u /* malformed blob, unknown legend, value not an ext 'G': the caller decides */
typedef struct kd_geom_head {
    uint8_t gpkg[40];
    uint32_t glen;        /* GPKG value length                                                        */
    uint32_t goff_status; /* (status << 24) | offset of the GPKG value in its blob (< 2^24)           */
} kd_geom_head;
/* n_leg legends (40-byte hex each) with gidx[l] = the geometry value's index (-1: none); threads
 * 0 = up to 16.  Blob i = data[off[i] .. off[i+1]) (host memory). */
int kd_geom_heads(const uint8_t* data, const uint64_t* off, uint64_t n, int n_leg, const uint8_t* leg_hex,
                  const int16_t* gidx, int threads, kd_geom_head* out);
/* kd_geom_filter from the heads: same codes, keep list and index envelopes.  heads_old [n_old] /
 * heads_new [n_new] in heads_mem; pairs index them.  A geometry whose decode needs bytes past its
 * head (an XYZ/XYM/XYZM envelope, a NaN envelope) is read from old_blobs / new_blobs (the arenas
 * the heads came from, device or host); with NULL arenas such a side is 3 FALLBACK. */
int kd_geom_filter_heads(kd_ctx* ctx, const kd_geom_head* heads_old, uint64_t n_old, const kd_geom_head* heads_new,
                         uint64_t n_new, uint32_t heads_mem, const kd_blobs* old_blobs, const kd_blobs* new_blobs,
                         const uint32_t* pairs, uint64_t n, const uint64_t* d_n, uint32_t pairs_mem,
                         const double filt_env[4], uint32_t flags, int bits, uint8_t* match, uint32_t* keep,
                         uint64_t* n_keep, uint8_t* enc, uint8_t* enc_ok, uint32_t out_mem);

/* kd_geom_filter_heads over classify2's delta list on the device (all buffers device memory, the delta
 * count *d_n on the device, cap the list's capacity): filtered from heads in delta order (the layout
 * the drop-in's blob reader produces: it reads the deltas' blobs after classification); a geometry
 * whose head cannot decide it is read from old_blobs / new_blobs at the delta's own blob (the pairs).
 * With KD_GF_DELTA_HEADS in flags the heads are given in delta order; without it heads_old [n_old] /
 * heads_new [n_new] are indexed like the arenas (per entry) and first gathered into delta order.
 * Outputs as kd_geom_filter_heads (match [cap * 2], keep [cap], n_keep, enc, enc_ok: device). */
int kd_geom_filter_deltas(kd_ctx* ctx, const kd_geom_head* heads_old, uint64_t n_old, const kd_geom_head* heads_new,
                          uint64_t n_new, const kd_blobs* old_blobs, const kd_blobs* new_blobs, const uint32_t* pairs,
                          uint64_t cap, const uint64_t* d_n, const double filt_env[4], uint32_t flags, int bits,
                          uint8_t* match, uint32_t* keep, uint64_t* n_keep, uint8_t* enc, uint8_t* enc_ok);

/* The exact stage behind the envelope test: Intersects(feature, filter polygon) for the sides the
 * filter left 1 CANDIDATE, decided on the device: wherever FP64 can prove the answer (the default), or,
 * with KD_GF_EXACT in flags, for every supported geometry whose coordinates are within range.
 *
 * Filter: closed rings of finite XY doubles (host memory); its region is the even-odd interior of
 * all rings together, boundary included — a valid OGC polygon's or multipolygon's point set.  Up to
 * 2^20 vertices (more: KD_EUNSUPPORTED).  Its device copy is kept in the context and written again
 * only when the pointer, the sizes or a hash of the bytes change.
 *
 * Feature: the WKB behind the GPKG header, either byte order per sub-geometry, ISO types 1-6 and
 * their +1000 / +2000 / +3000 variants (extra ordinates ignored); a polygon is the even-odd interior
 * of its own rings, boundary included.  Intersects holds when a vertex of the feature lies in the
 * filter, a segment of the feature meets a boundary segment of the filter, or the feature is areal
 * and the first vertex of a filter ring lies in it.  Every decision is an exact comparison of
 * doubles or the sign of det = (ax-cx)(by-cy) - (ay-cy)(bx-cx).
 *
 * Without KD_GF_EXACT the sign is taken in FP64 and counts only when
 * |det| > (3 + 16 eps) eps (|(ax-cx)(by-cy)| + |(ay-cy)(bx-cx)|), eps = 2^-53, the sum >= 1e-290 and
 * every operand finite.  A witness makes the side 2 MATCHING; no witness and nothing undecided
 * 0 NON_MATCHING; anything else stays 1 for the caller's exact test — every touching configuration
 * (shared vertex, shared edge, point on the boundary, collinear overlap) among them, and near
 * misses inside the bound.
 *
 * With KD_GF_EXACT a second pass takes the sides the first left 1: the same bound first (what it
 * certifies keeps its answer), and where it fails the exact sign of det by floating-point expansion
 * arithmetic (kd_orient2d_exact_batch computes the same on the host).  Touching then is a witness:
 * a point equal to an edge's end, on a horizontal edge's span, or on an edge by an exactly zero
 * determinant; two segments whose closed boxes overlap and whose end points are not strictly on
 * one side of each other; the first vertex of a filter ring on the feature's boundary.  Such a side
 * is 2, a side without witness 0, and 1 remains only where a determinant has an operand outside the
 * expansion's range: a non-zero coordinate must satisfy 2^-485 <= |v| < 2^510 (below, the rounding
 * error of a product of two coordinates would underflow; above, the sum of the six products could
 * overflow), which degrees and projected metres do by hundreds of binades.  No decision of either
 * mode contradicts rational arithmetic.  The flag changes nothing for a side the first pass decides.
 *
 * In both modes type 7 and above, EWKB flag bits, a count that runs past the value and a non-finite
 * coordinate stay 1 (counted unsupported).  No byte outside the GPKG value [goff, goff + glen) of
 * the blob is read.
 *
 * heads / pairs / blobs as in kd_geom_filter_heads, flags & KD_GF_DELTA_HEADS as in
 * kd_geom_filter_deltas, flags & KD_GF_EXACT as above (KD_GF_RECT is ignored); NULL heads: KD_EUNSUPPORTED (the geometry is not
 * located from legends here), the arenas are required.  A side whose code is not 1, or whose head is
 * not KD_GH_GEOM, is left untouched.  match [n * 2] is updated in place, keep [n] / *n_keep are
 * rebuilt in delta order from the codes (either side 1, 2 or 3), stats[4] <- candidate sides decided
 * true, decided false, left undecided, unsupported or malformed (their sum is the number of candidate
 * sides in either mode; a side the exact pass decides counts as true or false).  Host buffers (out_mem, pairs_mem,
 * heads_mem, blobs->mem = KD_MEM_HOST), or everything device memory with the delta count read from
 * *d_n on the device (n = capacity; match 2-B, stats 8-B aligned). */
#define KD_GF_EXACT 0x4u /* kd_geom_refine: decide what FP64 cannot certify in exact arithmetic */
typedef struct kd_filter_poly {
    const double* xy;         /* [n_vert][2], each ring closed (first vertex == last)          */
    const uint64_t* ring_off; /* [n_ring + 1]: ring r = vertices ring_off[r] .. ring_off[r+1]  */
    uint64_t n_ring, n_vert;
} kd_filter_poly;
int kd_geom_refine(kd_ctx* ctx, const kd_filter_poly* filter, const kd_geom_head* heads_old, uint64_t n_old,
                   const kd_geom_head* heads_new, uint64_t n_new, uint32_t heads_mem, const kd_blobs* old_blobs,
                   const kd_blobs* new_blobs, const uint32_t* pairs, uint64_t n, const uint64_t* d_n, uint32_t pairs_mem,
                   uint32_t flags, uint8_t* match, uint32_t* keep, uint64_t* n_keep, uint64_t* stats, uint32_t out_mem);
/* The exact orientation behind KD_GF_EXACT on the host (no context, no device): out[i] <- the sign
 * of det((a - c), (b - c)) for abc[i] = (ax, ay, bx, by, cx, cy): -1, 0 or +1, or 2 when a coordinate
 * is outside the range above (NaN and infinities included). */
int kd_orient2d_exact_batch(const double* abc /* [n][6] */, uint64_t n, int8_t* out);

/* -------- writer formatting -------- */
#define KD_HEX_BYTES 0u    /* bytes.hex(v): lowercase hex of every byte of every blob                */
#define KD_HEX_GPKG_WKB 1u /* gpkg_geom_to_hex_wkb: uppercase hex of the WKB after the GPKG header   */
/* hex[2*off[n]]: the hex of arena byte p lands at hex[2p], so blob i's string is
 * hex[2*(off[i] + start[i]) .. 2*off[i+1]) (start = 0 in KD_HEX_BYTES mode; start/status may then
 * be NULL).  KD_HEX_GPKG_WKB: start[i] = WKB offset in blob i (8 + envelope size), status[i] =
 * 0 ok, 1 null geometry (length 0: the reference returns None), 3 needs the CPU path (invalid
 * GPKG or empty WKB: the reference raises; big-endian WKB: the reference re-encodes via OGR).
 * blobs->mem says where the arena lives, out_mem where hex/start/status live. */
int kd_hex_encode(kd_ctx* ctx, const kd_blobs* blobs, uint32_t mode, uint8_t* hex, uint32_t* start,
                  uint8_t* status, uint32_t out_mem);

/* -------- packing on the GPU (the sort that follows the leaf-path decode) -------- */
/* Sort one side's n entries by join key on the device: an onesweep LSD radix sort over the keys'
 * varying bits (LDS-ranked, LDS-reordered tiles, decoupled look-back; stable).  d_key [n] is sorted in place; d_order [n] <- original index of
 * sorted entry k; d_oid [n*20] (may be NULL) is permuted in place.  *h_dup (may be NULL) <- 1 when
 * the sorted keys are not strictly ascending (two entries share a key: the caller's fallback).
 * Replaces the host sort of the packer (Dataset3 leaves arrive in git path order, not key order). */
int kd_sort_side(kd_ctx* ctx, uint64_t* d_key, uint8_t* d_oid, uint32_t* d_order, uint64_t n, uint32_t* h_dup);
/* What a sort needs to know about a side's keys (host scan, kd_keys_scan): the bits that vary
 * (OR of key[i] ^ key[0]) and key[0]; whether the keys are strictly ascending already (a walk-order
 * KD_KEY_INT side usually is: no sort); for KD_KEY_INT the smallest and largest pk; seg_max: the
 * longest run of consecutive keys sharing their top 24 bits (the leaf tree: a walk lists each leaf
 * tree's entries together), or -1 when those bits descend somewhere — a side with 0 < seg_max <= 512
 * that is not ascending sorts per leaf tree (kd_sort_segmented_into, seg_bits 24). */
typedef struct kd_keys_info {
    uint64_t vary;
    uint64_t key0;
    int64_t pk_min, pk_max; /* KD_KEY_INT only */
    int32_t ascending;
    int32_t seg_max;
} kd_keys_info;
int kd_keys_scan(const uint64_t* keys, uint64_t n, uint32_t key_mode, kd_keys_info* out);
/* Out-of-place form (what a device pipeline runs): d_key_in / d_oid_in hold the side in walk order
 * and are left unchanged; d_key_out [n] <- the keys ascending, d_oid_out [n*20] <- the OIDs in that
 * order (both oid pointers NULL to skip: kd_diff2_device_perm then reads them through the order),
 * d_order [n] <- input index of sorted entry k.  d_dup (device, may be NULL: a following
 * kd_diff2_device checks strict order anyway) <- 1 when two entries share a key.  Outputs must not
 * alias inputs.  info (host, from kd_keys_scan) sizes the passes; with NULL one 16-byte read-back
 * finds the varying bits.  Otherwise asynchronous on the context stream.  This is the fallback of a
 * side whose walk order is not key order (a leaf tree mixing pk wraps). */
int kd_sort_side_into(kd_ctx* ctx, const uint64_t* d_key_in, const uint8_t* d_oid_in, uint64_t* d_key_out,
                      uint8_t* d_oid_out, uint32_t* d_order, uint64_t n, uint32_t* d_dup, const kd_keys_info* info);
/* A side in walk order whose keys ascend in their top seg_bits bucket bits (KD_KEY_HASH: inside a leaf
 * tree the leaves are in filename order, not FNV order; KD_KEY_INT: a leaf tree mixing pk wraps):
 * each bucket's entries ordered by key.
 * d_key_out [n] <- keys ascending, d_order [n] <- walk index of sorted entry k (the OIDs and
 * filenames stay in walk order: kd_diff2_device_perm / kd_merge3_device_perm read through it).
 * *d_err |= 1 on a duplicate key or descending bucket bits, 4 on a bucket of more than 512 entries
 * (then sort with kd_sort_side_into).  max_seg: the longest bucket the caller knows of (kd_keys_scan's
 * seg_max; 0 = unknown): at most 128 stages a smaller halo per tile.  One kernel, no host sync. */
int kd_sort_segmented_into(kd_ctx* ctx, const uint64_t* d_key_in, uint64_t* d_key_out, uint32_t* d_order,
                           uint64_t n, int seg_bits, int max_seg, uint32_t* d_err);
/* The deltas in pk order (DeltaDiff.sorted_items, kart/diff_structs.py:442-458; classify2 emits them in
 * git walk order): for KD_KEY_INT device sides and a device record list d_delta [cap] of (base | KD_NONE,
 * target | KD_NONE) records (classify2's deltas or updates) with *d_n of them, d_pk [cap] <- their pks
 * ascending, d_perm [cap] <- the record index of pk rank k.  d_keys (optional, device): the records'
 * keys as kd_diff2_device_ex wrote them (else each is gathered from the sides).  pk_lo / pk_hi bound
 * every pk of both sides (kd_keys_scan's pk_min / pk_max): a range of at most 2^26 64-pk blocks is
 * placed through a bitmap (one mask per block: every pk occurs once), a wider one radix-sorted with
 * passes sized by the range — no read-back either way.  Stable, asynchronous. */
int kd_delta_pk_order(kd_ctx* ctx, const kd_side* base, const kd_side* target, const uint32_t* d_delta,
                      const uint64_t* d_keys, uint64_t cap, const uint64_t* d_n, int64_t pk_lo, int64_t pk_hi,
                      int64_t* d_pk, uint32_t* d_perm);

/* -------- the whole step in one call -------- */
/* kd_diff2_device_ex, kd_fielddiff (device form, the update count read from d_counts[1]) and
 * kd_delta_pk_order of the deltas and of the updates, with those calls' arguments:
 *   the join       base, target, base_order / target_order (both or NULL), flags, d_delta, d_upd (optional),
 *                  d_delta_key / d_upd_key (optional), d_counts, d_err
 *   the field diff old_blobs NULL: none.  d_pairs NULL: update u's blobs at index u of both arenas; else the
 *                  device update pairs (d_upd).  upd_cap bounds the update count (0 = unknown); maps,
 *                  d_masks, d_status as kd_fielddiff's
 *   the pk order   d_delta_pk NULL: the deltas are not ordered; d_upd_pk NULL: nor the updates (they need
 *                  d_upd).  pk_lo / pk_hi bound every pk; delta_cap / upd_cap are the lists' capacities;
 *                  the records' keys are read from d_delta_key / d_upd_key when given. */
typedef struct kd_step {
    const kd_side* base;
    const kd_side* target;
    const uint32_t* base_order;
    const uint32_t* target_order;
    uint32_t flags;
    uint32_t reserved;
    uint32_t* d_delta;
    uint32_t* d_upd;
    uint64_t* d_delta_key;
    uint64_t* d_upd_key;
    uint64_t* d_counts;
    uint32_t* d_err;
    const kd_blobs* old_blobs;
    const kd_blobs* new_blobs;
    const uint32_t* d_pairs;
    uint64_t upd_cap;
    const kd_legend_maps* maps;
    uint64_t* d_masks;
    uint8_t* d_status;
    int64_t pk_lo;
    int64_t pk_hi;
    uint64_t delta_cap;
    int64_t* d_delta_pk;
    uint32_t* d_delta_perm;
    int64_t* d_upd_pk;
    uint32_t* d_upd_perm;
} kd_step;
/* Results are those of the separate calls in sequence, bit for bit.  The library owns the schedule: with
 * the step_overlap option the placement (k_place2) and the pk order run on a stream of the context's own
 * beside the field diff, which needs neither (a field diff given d_pairs reads the placed updates: then
 * only the pk order runs beside it; KD_DIFF_UNORDERED, or nothing to overlap: one stream), and with the
 * step_count option the group scan that writes d_counts runs there too.  The context's
 * stream waits for that work before the call returns, so whatever is queued on it next — kd_sync
 * included — comes after the whole step.  Asynchronous. */
int kd_diff2_step(kd_ctx* ctx, const kd_step* step);

/* -------- device memory and copies (no GPU framework needed by the caller) -------- */
#define KD_COPY_H2D 1u
#define KD_COPY_D2H 2u
#define KD_COPY_D2D 3u
int kd_malloc(kd_ctx* ctx, uint64_t bytes, void** dptr);   /* HBM of the context's device      */
int kd_mfree(kd_ctx* ctx, void* dptr);
int kd_host_alloc(uint64_t bytes, void** hptr);            /* pinned (page-locked) host memory */
int kd_host_free(void* hptr);
/* asynchronous on the context stream (host buffers should be pinned for a true async copy) */
int kd_memcpy(kd_ctx* ctx, void* dst, const void* src, uint64_t bytes, uint32_t kind);
int kd_memset(kd_ctx* ctx, void* dst, int value, uint64_t bytes);
int kd_device_sync(kd_ctx* ctx);                           /* hipDeviceSynchronize + profiling */

/* -------- multi-GPU: bucket-range shards, RCCL all-gather -------- */
#define KD_COMM_ID_BYTES 128
/* One process per GPU: rank 0 makes the id, the caller broadcasts it (any channel), every rank
 * calls kd_comm_init with it.  The library owns the communicator (RCCL, loaded at first use). */
int kd_comm_unique_id(uint8_t id[KD_COMM_ID_BYTES]);
int kd_comm_init(kd_ctx* ctx, int nranks, int rank, const uint8_t id[KD_COMM_ID_BYTES]);
int kd_comm_fini(kd_ctx* ctx);
/* the communicator's own view, from RCCL: out[0] = ncclCommCount (ranks that joined), out[1] =
 * ncclCommUserRank, out[2] = ncclCommCuDevice (the HIP device it drives) */
int kd_comm_info(kd_ctx* ctx, int32_t out[3]);
/* d_recv[nranks * n] <- every rank's d_send[n] (device buffers, context stream) */
int kd_allgather_u64(kd_ctx* ctx, const uint64_t* d_send, uint64_t* d_recv, uint64_t n);
/* One rank's step of a sharded diff: kd_diff2_device on this rank's shard (device sides holding
 * the global sorted entries [base_off, base_off + base.n) / [target_off, ...) of one bucket range),
 * its delta records rebased to global indices, then all-gathered with the counts:
 *   d_all_counts / h_all_counts [nranks * 8]: rank r's inserts, updates, deletes, deltas, error word;
 *   d_all_delta [all_cap * 2]: rank r's records at 2 * r * stride, stride = max_r deltas(r).
 * Ranks hold consecutive bucket ranges, so the gathered records in rank order are key-ordered.
 * One host sync (the record stride).  d_upd may be NULL. */
int kd_diff2_gather(kd_ctx* ctx, const kd_side* base, const kd_side* target, uint64_t base_off,
                    uint64_t target_off, uint32_t flags, uint32_t* d_delta, uint32_t* d_upd,
                    uint64_t* d_counts, uint32_t* d_err, uint32_t* d_all_delta, uint64_t all_cap,
                    uint64_t* d_all_counts, uint64_t* h_all_counts);
/* kd_diff2_gather in two halves, so the caller can queue work between them (the shard's
 * kd_fielddiff): _begin queues the join, the rebase and the counts' all-gather (no host wait);
 * _end waits for the counts, queues the records' all-gather on the context's communication
 * stream (overlapping the work queued in between) and makes the context stream wait for it.
 * kd_diff2_gather = _begin + _end. */
int kd_diff2_gather_begin(kd_ctx* ctx, const kd_side* base, const kd_side* target, uint64_t base_off,
                          uint64_t target_off, uint32_t flags, uint32_t* d_delta, uint32_t* d_upd,
                          uint64_t* d_counts, uint32_t* d_err, uint64_t* d_all_counts);
int kd_diff2_gather_end(kd_ctx* ctx, const uint32_t* d_delta, uint32_t* d_all_delta, uint64_t all_cap,
                        uint64_t* h_all_counts);
/* One process driving g GPUs (one context each): host sides are cut into g bucket ranges of about
 * equal entry count (bucket = the key's top bucket_bits bits: 24 for KD_KEY_INT, 6 per tree level
 * for base64 hash paths, 8 per level for hex), each shard diffed on its GPU, and the records
 * all-gathered over a communicator the library keeps on ctxs[0].  Result as kd_diff2. */
int kd_diff2_sharded(kd_ctx** ctxs, int g, const kd_side* base, const kd_side* target, int bucket_bits,
                     uint32_t flags, kd_diff_result** out);
/* The cut kd_diff2_sharded uses (host only, no GPU): cut [g+1] bucket edges, shard s = buckets
 * [cut[s], cut[s+1]), each cut the smallest bucket with at least total*s/g entries of both sorted
 * key arrays before it; a_lo / b_lo [g+1] the matching entry ranges of each side. */
int kd_shard_cuts(const uint64_t* key_a, uint64_t n_a, const uint64_t* key_b, uint64_t n_b, int g, int bucket_bits,
                  uint64_t* cut, uint64_t* a_lo, uint64_t* b_lo);

/* -------- host-side key packing (CPU, multithreaded) -------- */
/* KD_KEY_INT: filenames b64(msgpack([pk])) -> keys (entries may be whole relative paths
 * "c/c/c/c/<filename>": the part after the last '/' is decoded).  status[i] = 0 ok / 1 not an int
 * pk / 2 pk outside [-2^63, 2^63).  Returns number of bad entries. */
int64_t kd_pack_int_keys(const uint8_t* names, const uint64_t* name_off, uint64_t n,
                         uint64_t* keys, uint8_t* status);
/* KD_KEY_HASH: "c1/../cL/<filename>" relative paths -> keys (levels, hex=0 base64 / 1 hex). */
int64_t kd_pack_hash_keys(const uint8_t* paths, const uint64_t* path_off, uint64_t n, int levels,
                          int hex, uint64_t* keys, uint8_t* status);
/* Inverse of the KD_KEY_INT key: pk = ((wrap - 2^33) * 2^24 + bucket) * 64 + low6, bucket and low6
 * through the inverse rank maps. */
int kd_int_keys_to_pks(const uint64_t* keys, uint64_t n, int64_t* pks);

/* -------- key packing and the side scan on the GPU -------- */
/* kd_pack_int_keys / kd_pack_hash_keys and kd_keys_scan in one asynchronous call on device memory
 * (Dataset3.decode_path_to_1pk, kart/dataset3.py:250-259, and the path encoders,
 * kart/dataset3_paths.py:202-215,283-299, decoded by the same code as the host entries): a path arena
 * d_paths with its offsets d_path_off [n+1] — what kd_tree_join_batch's device form writes — becomes
 * d_keys [n] and d_status [n] (0 ok / 1 not packable / 2 pk outside [-2^63, 2^63); the key of a refused
 * entry is 0), and *d_info: info = what kd_keys_scan returns for the keys as written, bad = the refused
 * entries, first_bad = the smallest refused index (UINT64_MAX when bad == 0).  n == 0: ascending = 1,
 * bad = 0, everything else of info zero.  Every pointer is device memory; no host wait, nothing read
 * back.  levels / hex are the hash path structure (ignored for KD_KEY_INT); 64 or more bucket bits, a
 * NULL pointer or another key_mode: KD_EINVAL.  The arena is read inside [off[0], off[n]) only (in
 * aligned 16-byte pieces holding at least one such byte); an entry with off[i+1] < off[i], or outside
 * that range, gets status 1 and is not read.  Options: kp_tile [KD_KP_TILE] 512 / 1024 entries per
 * workgroup, kp_lds_bytes [KD_KP_LDS_BYTES] the largest tile staged in LDS (longer ones decode from
 * HBM); read-only kp_hbm_tiles: the tiles of the last call that did. */
typedef struct kd_keypack_info {
    kd_keys_info info;
    uint64_t bad;
    uint64_t first_bad;
} kd_keypack_info; /* 56 bytes */
int kd_pack_keys_device(kd_ctx* ctx, const uint8_t* d_paths, const uint64_t* d_path_off, uint64_t n,
                        uint32_t key_mode, int levels, int hex, uint64_t* d_keys, uint8_t* d_status,
                        kd_keypack_info* d_info);

/* -------- git object database + leaf walk (host, no GPU) -------- */
/* Replaces libgit2's ODB and tree iteration under Dataset3 (kart/dataset3.py:26-35,225-231,
 * kart/base_dataset.py:230-265) and the subtree pruning of Tree.diff_to_tree
 * (kart/rich_base_dataset.py:212-232).  Loose objects, pack v2 (idx v1/v2), zlib, OFS/REF delta
 * chains, objects/info/alternates.  The pack set is read at open: reopen to see new packs. */
#define KD_ENOTFOUND (-4) /* object not in the odb (missing, or promised by a partial clone) */
typedef struct kd_odb kd_odb;
int kd_odb_open(const char* gitdir, kd_odb** out);
/* Options of an object store (A/B switches; kd_odb_open seeds each from the environment variable in
 * brackets).  Unknown names: KD_EINVAL.
 *   zlib           [KD_ODB_ZLIB]       1: inflate with zlib even when libdeflate.so.0 is present
 *   walk_batch_bytes [KD_WALK_BATCH_BYTES]  kd_walk_device reads its leaf trees in batches of about this many
 *                  compressed and host-read bytes (default 64 MiB): the bound of a walk's pinned staging and
 *                  device arena.  A batch always holds at least one task.
 * Read-only (kd_odb_get_option), microseconds of the last kd_odb_read_batch_device_ex call with
 * KD_RBD_DELTAS: rbd_plan_us (classes, forest, peeks, levels), rbd_peek_us (the header peeks in it),
 * rbd_host_us (host reads, layout, gather), rbd_device_us (upload, launches, statuses back). */
int kd_odb_set_option(kd_odb* odb, const char* name, int64_t value);
int kd_odb_get_option(kd_odb* odb, const char* name, int64_t* value);
int kd_odb_close(kd_odb* odb);
/* One object (*type 1 commit, 2 tree, 3 blob, 4 tag); *data malloc'd (kd_free). */
int kd_odb_read(kd_odb* odb, const uint8_t oid[20], int* type, uint8_t** data, uint64_t* len);
/* n blobs into one arena *data (kd_free): blob i = (*data)[off[i] .. off[i+1]) (off [n+1]);
 * status[i] 0 ok, 1 missing (empty), 2 corrupt / not a blob (empty).  threads 0 = up to 16. */
int kd_odb_read_batch(kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint8_t** data,
                      uint64_t* off, uint8_t* status);

/* -------- device inflate: zlib streams decoded on the GPU (opt-in route of the batched read) -------- */
/* Kart imports with `git fast-import --depth=0` (kart/fast_import.py:204,273): a feature blob of an
 * imported layer is a plain deflate stream in the pack, its inflated size in the entry header.  The
 * decoder (kart_amd/csrc/kd_inflate.h, written from RFC 1950 / RFC 1951) handles the zlib header
 * (CM = 8, window <= 32 KiB, FCHECK, no FDICT), stored / fixed / dynamic blocks and the Adler-32
 * trailer.  Status of one stream: */
#define KD_INF_OK 0u
#define KD_INF_EHEADER 1u  /* bad zlib header                                                        */
#define KD_INF_EBTYPE 2u   /* reserved block type                                                    */
#define KD_INF_ESTORED 3u  /* stored LEN / NLEN mismatch                                             */
#define KD_INF_ELENS 4u    /* bad code lengths: over-subscribed; incomplete (other than one code of one
                              bit, or an empty distance set); a repeat with no previous length or running
                              past HLIT + HDIST; no end-of-block code; HLIT > 286 or HDIST > 30      */
#define KD_INF_ESYMBOL 5u  /* literal/length 286 / 287, distance 30 / 31, or a code the set leaves out */
#define KD_INF_EDIST 6u    /* a distance reaching before the stream's own output                     */
#define KD_INF_EOVER 7u    /* more output than the expected size                                     */
#define KD_INF_ESHORT 8u   /* end of stream before the expected size                                 */
#define KD_INF_ESRC 9u     /* source exhausted: a bit needed at or beyond the stream's bound         */
#define KD_INF_EADLER 10u  /* Adler-32 mismatch                                                      */
#define KD_INF_ERANGE 11u  /* device offsets only: an item's offsets descend or pass off[n]          */
#define KD_INF_MAX (256u << 10) /* the largest blob kd_odb_read_batch_device inflates on the device  */
/* Item i: src[src_off[i] .. src_off[i+1]) -> dst[dst_off[i] .. dst_off[i+1]), status[i] = KD_INF_*.
 * kind[i] (NULL: all 0): 0 a zlib stream whose inflated size is its dst range exactly — the src range
 * only bounds the stream, bytes after its end are ignored; 1 raw bytes copied as they are (the ranges'
 * sizes must agree: KD_INF_ESRC / KD_INF_EOVER).  A failing item stops at its first error: the bytes of
 * its own dst range are unspecified, nothing outside that range is written.  One launch of
 * k_inf_streams, one lane per item.
 * mem = KD_MEM_HOST: every array is host memory, staged by the library (workspace: the context's
 * grow-only slots), offsets are checked (descending: KD_EINVAL) and the call returns with the results.
 * mem = KD_MEM_DEVICE: every array is device memory, src readable up to src_off[n] + 8 bytes, and the
 * call is queued on the context's stream. */
int kd_inflate_batch(kd_ctx* ctx, const uint8_t* src, const uint64_t* src_off, const uint8_t* kind, uint64_t n,
                     uint8_t* dst, const uint64_t* dst_off, uint8_t* status, uint32_t mem);
/* kd_odb_read_batch with the arena in HBM: out->data / out->off (kd_malloc'd, mem = KD_MEM_DEVICE, the
 * caller kd_mfree's both) hold what kd_odb_read_batch returns in *data / off, status (host, [n]) its
 * codes, for every input.  A packed, non-delta blob of at most KD_INF_MAX bytes is shipped compressed
 * (the span from its data to size + size/4096 + size/16384 + size/2^25 + 13 bytes on, clipped to the
 * pack's trailer) and inflated by kd_inflate_batch; every other object (deltas, loose objects, larger
 * blobs, ids no pack holds) is read on the host as before and uploaded as a raw item of the same
 * launch.  A device item that fails is read again on the host, so the result does not rest on that
 * bound.  stats: streams inflated on the device, objects read on the host, compressed bytes uploaded,
 * device items that needed the host read.  Returns after the results are complete.
 * Costs to know: the sources of one call are gathered into one pinned (page-locked) host buffer the
 * store keeps and only grows until kd_odb_close — the largest call's compressed spans plus host-read
 * bytes, plus a quarter (about 1.3 GB after a read of 4M blobs of 240 B).  A raw item is copied by one
 * lane, a byte at a time, whatever its size: a host-class blob of many megabytes holds its wave for as
 * long as that takes. */
int kd_odb_read_batch_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, kd_blobs* out,
                             uint8_t* status, uint64_t stats[4]);

/* -------- device deltas: git deltas applied on the GPU (opt-in route of the batched read) -------- */
/* After a clone, fetch, gc or repack most feature blobs are OFS_DELTA / REF_DELTA entries against an
 * earlier version of the same feature.  The decoder (kart_amd/csrc/kd_delta.h, written from git's pack
 * format documentation) handles the two size varints, copy ops (up to 4 offset and 3 size bytes, size 0
 * = 0x10000) and insert ops.  Status of one item: */
#define KD_DL_OK 0u
#define KD_DL_EHEADER 1u  /* a size varint truncated or longer than 10 bytes                          */
#define KD_DL_EBASE 2u    /* base size != the base range's length                                     */
#define KD_DL_ESIZE 3u    /* result size != the dst range's length                                    */
#define KD_DL_EOP 4u      /* opcode 0                                                                 */
#define KD_DL_ETRUNC 5u   /* an op's argument bytes or literals run past the delta                    */
#define KD_DL_ECOPY 6u    /* a copy reaching past the base                                            */
#define KD_DL_EOVER 7u    /* more output than the result size                                         */
#define KD_DL_ESHORT 8u   /* delta exhausted before the result size                                   */
#define KD_DL_EPARENT 9u  /* chained use: the base or the delta payload of this item did not come out OK */
#define KD_DL_ERANGE 11u  /* device offsets that descend or leave their arena; base_idx[i] >= nb       */
#define KD_DL_MAX_DEPTH 64u /* the deepest chain kd_odb_read_batch_device_ex rebuilds on the device   */
/* One level of deltas: item i patches base[base_off[b] .. base_off[b+1]), b = base_idx[i] < nb (many items
 * may share one base), with delta[delta_off[i] .. delta_off[i+1]) into dst[dst_off[i] .. dst_off[i+1]);
 * status[i] = KD_DL_*.  The header's sizes must equal the base and dst ranges' lengths.  A failing item
 * stops at its first error: the bytes of its own dst range are unspecified, nothing outside that range
 * is written, and no byte outside the item's base and delta ranges is read.  One launch of k_dl_apply,
 * 16 lanes per item.  base, delta and dst must not overlap.
 * mem = KD_MEM_HOST: every array is host memory, staged by the library (workspace: the context's
 * grow-only slots), offsets are checked (descending: KD_EINVAL) and the call returns with the results.
 * mem = KD_MEM_DEVICE: every array is device memory and the call is queued on the context's stream. */
int kd_delta_apply_batch(kd_ctx* ctx, const uint8_t* base, const uint64_t* base_off, uint64_t nb,
                         const uint32_t* base_idx, const uint8_t* delta, const uint64_t* delta_off, uint64_t n,
                         uint8_t* dst, const uint64_t* dst_off, uint8_t* status, uint32_t mem);
/* kd_odb_read_batch_device with flags.  flags = 0 is kd_odb_read_batch_device itself (stats[4..7] = 0).
 * KD_RBD_DELTAS: a requested OFS_DELTA / REF_DELTA object whose whole chain lies in its own pack, ends
 * in a blob, is at most KD_DL_MAX_DEPTH links deep and has no stream or result above KD_INF_MAX is
 * rebuilt on the device: the chain's base and every link's payload are inflated by k_inf_streams, then
 * one k_dl_apply launch per level patches each link against its parent (results nobody requested and
 * all payloads live in workspace).  The sizes a layout needs are read on the host by inflating at most
 * the first 20 bytes of each link's payload.  A link that fails on the device fails every link below
 * it; each requested one is read on the host and uploaded in place (a fixup).  out, status: as
 * kd_odb_read_batch's, for every input.
 * stats: [0] plain streams inflated on the device, [1] objects read on the host, [2] compressed bytes
 * uploaded, [3] fixups, [4] requested objects rebuilt from a chain on the device, [5] unique delta links
 * applied, [6] the deepest level launched, [7] workspace bytes (payloads and unrequested results);
 * [0] + [4] + [1] + [3] == n. */
#define KD_RBD_DELTAS 1u
int kd_odb_read_batch_device_ex(kd_ctx* ctx, kd_odb* odb, const uint8_t* oids, uint64_t n, int threads, uint32_t flags,
                                kd_blobs* out, uint8_t* status, uint64_t stats[8]);
/* A walk's leaves for one root, one block (kd_free): leaf i = path[path_off[i] .. path_off[i+1])
 * relative to the walked tree, '/'-separated, in git path order (what `git ls-tree -r` lists). */
typedef struct kd_leaves {
    uint64_t n;
    uint64_t* path_off; /* [n+1] */
    uint32_t* mode;     /* [n] git file modes (0100644, 0100755, 0120000, 0160000)  */
    uint8_t* oid;       /* [n*20] */
    uint8_t* path;
    int32_t present;    /* 0: the walked tree does not exist in this root */
} kd_leaves;
#define KD_WALK_ALL (-1)
/* Walk the tree at `subpath` ("" or NULL = the root) of k roots (commit, tag or tree OIDs, 20 raw
 * bytes each, k <= 3) into out[0..k).  cmp0/cmp1 (root indices) prune: an entry (subtree or leaf)
 * identical in roots cmp0 and cmp1 — same mode and OID, or absent from both — is skipped in every
 * root and a pruned subtree is never read.  KD_WALK_ALL (both) lists everything.  The first levels
 * are expanded breadth-first, then subtrees are walked depth-first by `threads` (0 = up to 16). */
int kd_walk(kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1,
            int threads, kd_leaves** out);

/* -------- device leaf join: changed leaf trees parsed, joined and pruned on the GPU -------- */
/* The lowest level of a pruned walk: at a high edit rate every leaf tree of both sides has changed and
 * each one is parsed and joined entry by entry.  The decoder (kart_amd/csrc/kd_treeparse.h, written
 * from git's tree format: <octal mode> SP <name> NUL <20 OID bytes>, repeated) defines the device class
 * of a tree — stricter than the host walk's parser, never laxer.  Status of one task (the status of the
 * first of its roots' trees that is refused): */
#define KD_TJ_OK 0u
#define KD_TJ_EMODE 1u   /* a mode byte that is no octal digit, no digits, more than 11 digits or a value
                            above 2^32 - 1, or the tree ends inside a mode                              */
#define KD_TJ_ENAME 2u   /* an empty name, or no NUL before the end of the tree                         */
#define KD_TJ_EOID 3u    /* fewer than 20 bytes behind a name's NUL                                      */
#define KD_TJ_ETREE 4u   /* an entry of mode 040000 (a subtree at leaf depth is the host walk's)         */
#define KD_TJ_EORDER 5u  /* a name not strictly above the one before it (unsigned bytes, then length)    */
#define KD_TJ_EBIG 6u    /* a tree above KD_TJ_MAX_BYTES, or a task whose kept paths of one root pass
                            2^32 - 1 bytes                                                               */
#define KD_TJ_ECAP 7u    /* mem = KD_MEM_DEVICE only: the task's output ranges pass cap_n / cap_bytes     */
#define KD_TJ_ERANGE 11u /* tree[] names no tree of the arena; offsets that descend or pass their end    */
#define KD_TJ_MAX_BYTES (1u << 30) /* the largest tree the join takes                                    */
/* One root's output of kd_tree_join_batch, in kd_leaves layout.  The caller owns the arrays: path_off
 * [cap_n + 1], mode [cap_n], oid [20 * cap_n], path [cap_bytes].  n and bytes are results (host words
 * with mem = KD_MEM_HOST; with KD_MEM_DEVICE they are written to totals, see below). */
typedef struct kd_tj_out {
    uint64_t cap_n, cap_bytes;
    uint64_t* path_off;
    uint32_t* mode;
    uint8_t* oid;
    uint8_t* path;
    uint64_t n, bytes;
} kd_tj_out;
/* n_task tasks over an arena of inflated tree objects: tree i = data[off[i] .. off[i+1]) (off [n_trees +
 * 1], 64-bit, a tree may start at any byte; trees are read 8 bytes at a time at byte addresses, so with
 * mem = KD_MEM_DEVICE data must be readable up to off[n_trees] + 8 bytes; what lies there is never used).  Task t names up to k <= 3 trees, one per root: tree[t*k + r], or KD_NONE where root r
 * has no tree at this path, and a path prefix pfx[pfx_off[t] .. pfx_off[t+1]).  The k entry lists are
 * merged by name exactly as kd_walk joins a level (Walk::join + Walk::pruned restricted to non-tree
 * entries): a name is dropped in every root when roots cmp0 and cmp1 agree on it (both lack it, or both
 * have it with equal mode and OID; KD_WALK_ALL for both: nothing is dropped), every other entry is kept
 * in each root that has it.  out[r] receives root r's kept entries in task order and name order:
 * path = prefix + '/' + name (no '/' after an empty prefix), path_off (path_off[0] = 0), mode, oid;
 * count[t*k + r] the entries task t kept in root r; status[t] = KD_TJ_*.  A task with a nonzero status
 * contributes nothing and nothing of it is written (its counts are 0).
 * Three steps: k_tj_count (one lane per task: every tree validated, then the join counted), the
 * project's k_gf_scan over the counts, k_tj_emit (the same join again, writing at the scanned
 * positions): positions are deterministic, no atomic decides one.  All kept entries and path bytes of one
 * call, over all roots together, must stay below 2^32 (the scan is 32-bit): kd_walk_device-style callers
 * batch far below that.
 * mem = KD_MEM_HOST: every array is host memory, staged by the library; offsets are checked (descending:
 * KD_EINVAL), totals above a root's cap_n / cap_bytes are KD_EINVAL with nothing written, and the call
 * returns with the results.  totals is ignored.
 * mem = KD_MEM_DEVICE: every array (out[r]'s arrays too; out itself is host memory) is device memory and
 * the call is queued on the context's stream; totals [2*k] (device) <- (n, bytes) per root; a task whose
 * ranges pass a cap gets KD_TJ_ECAP and writes nothing. */
int kd_tree_join_batch(kd_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n_trees, const uint32_t* tree,
                       const uint8_t* pfx, const uint64_t* pfx_off, uint64_t n_task, int k, int cmp0, int cmp1,
                       kd_tj_out* out, uint32_t* count, uint8_t* status, uint64_t* totals, uint32_t mem);

/* kd_walk with its lowest level on the GPU (an opt-in route): out[0..k) is what kd_walk returns for the
 * same roots, subpath and compare roots, byte for byte (n, path_off, mode, oid, path, present), and a
 * missing or corrupt tree gives the code kd_walk gives.  The host peels the roots, follows `subpath` and
 * expands `depth` levels below the walked tree breadth-first, in parallel, with pruning (depth = the number
 * of path components above the trees handed over; 0 hands over the walked tree itself; Kart passes its
 * path encoding's levels).  A blob met above `depth` is emitted by the host; every subtree item left at
 * `depth` is a task.  Tasks go in batches of about walk_batch_bytes (each tree counted as the compressed
 * span the device read ships for it: its entry's size + size/4096 + size/16384 + size/2^25 + 13; 4 KiB for
 * a loose tree): a batch's tree ids are made unique, read through the batched device read with trees as
 * the expected type (flags: KD_RBD_DELTAS rebuilds delta-compressed trees on the device too) and joined
 * by kd_tree_join_batch in HBM.  A task is host class — walked by kd_walk's own code, with the same
 * result — when one of its trees is above KD_INF_MAX, is missing or corrupt, or gets a KD_TJ_* status
 * (a subtree at that depth, names out of order, ...).
 * A delta-compressed tree is counted by its delta's size (the tree's is known only after the read's plan): on
 * a repacked repository a batch's arena and outputs can be several times walk_batch_bytes, and where a
 * batch's join could keep 2^31 entries and path bytes the rest of that batch's tasks are host class (seen
 * in stats[2] only).  The trees' costs are taken by every thread (a locate and an entry header per tree); a
 * batch's ids are sorted and made unique on one: stats[11].
 * stats [KD_WD_STATS] (may be NULL): [0] tasks, [1] tasks joined on the device, [2] host-class tasks
 * ([1] + [2] == [0]), [3] unique trees requested (summed over batches), [4] trees inflated on the device,
 * [5] trees read on the host, [6] fixups, [7] compressed bytes uploaded, [8] trees rebuilt from a delta
 * chain on the device, [9] batches; microseconds of [10] the host expansion, [11] forming the batches,
 * the reads' [12] locate / plan, [13] host reads and gather, [14] upload, inflate / delta kernels and
 * statuses back, the join's [15] task lists, allocations and upload, [16] kernels (to the counts' arrival),
 * [17] downloads (offsets, results) and frees, [18] stitching, [19] host-class walks, [20] the whole call (what [10..19] leave of
 * it: per-batch vectors built and freed, device allocations and frees between the timed spans); [21..23] 0. */
#define KD_WD_STATS 24
int kd_walk_device(kd_ctx* ctx, kd_odb* odb, const uint8_t* roots, int k, const char* subpath, int cmp0, int cmp1,
                   int threads, int depth, uint32_t flags, kd_leaves** out, uint64_t* stats);

/* -------- profiling (hipEvents around every launch on the context stream) -------- */
int kd_prof_enable(kd_ctx* ctx, int on);
/* Time only the named kernels ("k_join2,k_fielddiff"; NULL or "" = every kernel): each timed
 * launch adds two events to the stream, so a bench times just the kernels it reports. */
int kd_prof_select(kd_ctx* ctx, const char* names);
/* name = kernel name; returns launches and summed milliseconds since the last reset. */
int kd_prof_get(kd_ctx* ctx, const char* name, uint64_t* launches, double* total_ms);
int kd_prof_reset(kd_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* KARTDIFF_H */
