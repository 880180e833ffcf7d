"""kd_pack_keys_device against the host packer and the host scan: exact keys, statuses and info, 0xA5
canaries behind every output.

Every case uploads a path arena with its offsets, packs it on the device into buffers of this test's own
and compares entry by entry with kd_pack_int_keys / kd_pack_hash_keys on the same bytes; the info record
must be kd_keys_scan of the keys as downloaded, zeros of refused entries included.  T is the tile (one
workgroup's entries), read from the context's option.
"""
import ctypes

import numpy as np
import pytest

import keypack_craft as K
import tree_craft as C
from kart_amd import _native as N
from kart_amd import packing, synth, walkkey
from kart_amd.device import DevBuf, DevPermSide, DevSide

pytestmark = pytest.mark.gpu

CAN = 64
FILL = 0xA5
INFO = ctypes.sizeof(N.KdKeypackInfo)
NOBAD = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------
# running one call
# ---------------------------------------------------------------------------------------------
def _canaried(engine, nbytes):
    b = DevBuf(engine, nbytes + CAN)
    b.upload(np.full(nbytes + CAN, FILL, np.uint8))
    return b


def _body(buf, nbytes, what):
    raw = buf.download(np.uint8, nbytes + CAN)
    assert (raw[nbytes:] == FILL).all(), f"canary behind {what} overwritten"
    return raw[:nbytes]


def _info_tuple(i):
    return (int(i.vary), int(i.key0), int(i.pk_min), int(i.pk_max), int(i.ascending), int(i.seg_max))


def run(engine, d_paths, off, cfg):
    """one call on an arena that is in HBM; (keys, status, info tuple, bad, first_bad, hbm tiles)"""
    off = np.ascontiguousarray(off, np.uint64)
    n = off.shape[0] - 1
    d_off = DevBuf.from_numpy(engine, off)
    d_keys, d_status, d_info = _canaried(engine, 8 * n), _canaried(engine, n), _canaried(engine, INFO)
    N.check(engine.L.kd_pack_keys_device(engine.ctx, d_paths.ptr, d_off.ptr, n, cfg[0], cfg[1], cfg[2], d_keys.ptr,
                                         d_status.ptr, d_info.ptr), "kd_pack_keys_device")
    engine.sync()
    keys = _body(d_keys, 8 * n, "keys").view(np.uint64)
    status = _body(d_status, n, "status")
    r = N.KdKeypackInfo.from_buffer_copy(_body(d_info, INFO, "info").tobytes())
    return keys, status, _info_tuple(r.info), int(r.bad), int(r.first_bad), engine.get_option("kp_hbm_tiles")


def check(engine, entries, cfg, lead=0):
    """pack `entries` on the device (the arena starts `lead` bytes into its buffer) and compare with the
    host packer and the host scan; returns what run() returns"""
    data, off = K.arena(entries)
    buf = np.concatenate([np.full(lead, ord("/"), np.uint8), data, np.zeros(16, np.uint8)])
    d_paths = DevBuf.from_numpy(engine, buf)
    got = run(engine, d_paths, off + np.uint64(lead), cfg)
    _compare(got, data, off, cfg)
    return got


def _compare(got, data, off, cfg):
    keys, status, info, bad, first_bad, _ = got
    hk, hs = K.host_pack(None, cfg, data, off)
    assert np.array_equal(status, hs), f"status differs first at {np.nonzero(status != hs)[0][:5]}"
    assert np.array_equal(keys, hk), f"keys differ first at {np.nonzero(keys != hk)[0][:5]}"
    nz = np.nonzero(hs)[0]
    assert bad == nz.size and first_bad == (int(nz[0]) if nz.size else NOBAD)
    assert info == _info_tuple(packing.keys_scan(keys, cfg[0]))


def T(engine):
    t = engine.get_option("kp_tile")
    assert t in (512, 1024)
    return t


def int_entries(pks):
    arena, off = synth.int_pk_paths(np.asarray(pks, np.int64))
    return [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(pks))]


def wide_entry(pk):
    """any int64 pk under its own tree levels"""
    b = (pk // 64) % (1 << 24)
    lead = "/".join(chr(walkkey.B64[(b >> (18 - 6 * k)) & 63]) for k in range(4))
    return (lead + "/" + walkkey.filename(pk)).encode()


# ---------------------------------------------------------------------------------------------
# the CPU test's inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [K.INT, K.HASH64, K.HASHHEX], ids=["int", "hash64", "hashhex"])
def test_crafted_entries_and_mutations(engine, cfg):
    g = K.group(cfg)
    entries = [x[0] for x in g] + K.mutations(cfg)
    keys, status, _, bad, _, _ = check(engine, entries, cfg)
    assert keys[:len(g)].tolist() == [k for _, k, _ in g] and status[:len(g)].tolist() == [s for _, _, s in g]
    assert 0 < bad < len(entries)


# ---------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------
def test_entry_counts(engine):
    t = T(engine)
    pks = walkkey.walk_order_pks(4 * t)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 5):
        e = int_entries(pks[:n])
        keys, status, info, bad, first_bad, _ = check(engine, e, K.INT)
        assert bad == 0 and first_bad == NOBAD and info[4] == 1
        if n == 0:
            assert info == (0, 0, 0, 0, 1, 0)
        if n > 2:  # ... and with two refusals in it, one of them the last entry
            e[n // 2], e[n - 1] = b"A/A/A/A/k!", b""
            _, _, info, bad, first_bad, _ = check(engine, e, K.INT)
            assert (bad, first_bad) == (2, n // 2) and info[4] == 0


def test_start_offsets(engine):
    e = int_entries(walkkey.walk_order_pks(700)) + [K.hash_valid(K.HASH64)[5]]
    for lead in range(16):
        check(engine, e[lead:], K.INT, lead=lead)
        check(engine, [K.hash_valid(K.HASH64)[j % 9] for j in range(lead, 300)], K.HASH64, lead=lead)


def test_arena_offsets_beyond_4g(engine):
    """a sparse arena: off[0] beyond 2^32, nothing below it ever touched"""
    t = T(engine)
    e = int_entries(walkkey.walk_order_pks(2 * t + 9))
    data, off = K.arena(e)
    base = (1 << 32) + 5
    buf = DevBuf(engine, base + data.size + 16)
    buf.upload(data, offset=base)
    got = run(engine, buf, off + np.uint64(base), K.INT)
    _compare(got, data, off, K.INT)
    assert got[3] == 0 and got[2][4] == 1


def test_descending_offsets_are_refused(engine):
    e = int_entries(walkkey.walk_order_pks(600))
    data, off = K.arena(e)
    d_paths = DevBuf.from_numpy(engine, np.concatenate([data, np.zeros(16, np.uint8)]))
    bad_off = off.copy()
    bad_off[300] = bad_off[302]  # entry 299 runs into 301's, entry 300 = [off[302], off[301]) descends
    keys, status, info, bad, first_bad, _ = run(engine, d_paths, bad_off, K.INT)
    assert status[300] == 1 and keys[300] == 0 and first_bad in (299, 300)
    hk, hs = K.host_pack(None, K.INT, data, off)
    keep = np.ones(600, bool)
    keep[299:301] = False
    assert np.array_equal(keys[keep], hk[keep]) and not status[keep].any()


# ---------------------------------------------------------------------------------------------
# the scan
# ---------------------------------------------------------------------------------------------
def _bucket_runs(runs):
    """int entries whose buckets (first, second, ...) have the given run lengths: each run one bucket
    held by as many pk wraps as it takes, so the keys ascend inside a run wherever they can"""
    pks = []
    for b, ln in enumerate(runs):
        blk = walkkey.walk_order_range(64 * (b + 1), 64 * (b + 2))
        w = 0
        while ln > 0:
            take = min(ln, 64)
            pks += [int(p) + (w << 30) for p in blk[:take]]
            ln -= take
            w += 1
    return [wide_entry(p) for p in pks]


def test_info_at_tile_seams(engine):
    t = T(engine)
    asc = int_entries(walkkey.walk_order_pks(3 * t))
    _, _, info, _, _, _ = check(engine, asc, K.INT)
    assert info[4] == 1 and info[5] == 64
    only_seam = list(asc)
    only_seam[t - 1], only_seam[t] = asc[t], asc[t - 1]
    keys, _, info, _, _, _ = check(engine, only_seam, K.INT)
    assert info[4] == 0 and (keys[1:t] > keys[:t - 1]).all() and (keys[t + 1:] > keys[t:-1]).all()
    dup = list(asc)
    dup[2 * t] = dup[2 * t - 1]
    keys, _, info, _, _, _ = check(engine, dup, K.INT)
    assert info[4] == 0 and keys[2 * t] == keys[2 * t - 1]


def test_bucket_runs_across_seams(engine):
    t = T(engine)
    long = 3 * t + 7
    for runs in ([long], [long, 5, 9], [5, 9, long], [5, long, 9], [t - 3, 7, t + 1, 2]):
        _, _, info, _, _, _ = check(engine, _bucket_runs(runs), K.INT)
        assert info[5] == max(runs), runs
    # the bucket bits descend at a seam only: tile 0 holds buckets 1..k ascending, tile 1 starts over
    e = _bucket_runs([64] * (t // 64)) * 2
    _, _, info, _, _, _ = check(engine, e, K.INT)
    assert info[5] == -1 and info[4] == 0
    # ... and at a seam they merely repeat: one run of 128 across it
    e = _bucket_runs([64] * (t // 64 - 1) + [128] + [64] * 3)
    _, _, info, _, _, _ = check(engine, e, K.INT)
    assert info[5] == 128


def test_pk_extremes_and_hash_range(engine):
    pks = [-(1 << 63), (1 << 63) - 1, 0, -1, 1 << 30, -(1 << 30)]
    _, _, info, _, _, _ = check(engine, [wide_entry(p) for p in pks], K.INT)
    assert info[2:4] == (-(1 << 63), (1 << 63) - 1)
    _, _, info, _, _, _ = check(engine, K.hash_valid(K.HASH64), K.HASH64)
    assert info[2:4] == (0, 0)


# ---------------------------------------------------------------------------------------------
# hash mode and the beyond-LDS branch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [K.HASH64, K.HASHHEX], ids=["hash64", "hashhex"])
def test_hash_filename_lengths(engine, cfg):
    rng = np.random.default_rng(9)
    lead = [b"3f/a0/", b"00/ff/"] if cfg[2] else [b"-/_/A/z/", b"A/0/a/Z/"]
    for ln in (0, 1, 15, 16, 17, 255, 1000, 70000):
        e = [lead[j % 2] + bytes(rng.integers(0, 256, ln, dtype=np.uint8)) for j in range(3 if ln == 70000 else 40)]
        e[1:1] = [x for _, x, _ in K.hash_refused(cfg)]
        keys, status, _, bad, _, hbm = check(engine, e, cfg)
        assert bad == len(K.hash_refused(cfg))
        assert (hbm >= 1) is (ln >= 1000), f"filenames of {ln} bytes: {hbm} tiles decoded from HBM"


def test_small_budget_takes_the_hbm_branch(engine):
    """the same entries through both branches (the LDS budget lowered by the context's option)"""
    t = T(engine)
    e = int_entries(walkkey.walk_order_pks(2 * t + 5))
    e[7] = b"A/A/A/A/k!"
    full = engine.get_option("kp_lds_bytes")
    try:
        a = check(engine, e, K.INT)
        engine.set_option("kp_lds_bytes", 16)
        b = check(engine, e, K.INT)
        h = check(engine, K.hash_valid(K.HASH64) * 30, K.HASH64)
    finally:
        engine.set_option("kp_lds_bytes", full)
    assert a[5] == 0 and b[5] == 3 and h[5] >= 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:5] == b[2:5]


def test_other_tile_size(engine):
    t = T(engine)
    other = 1536 - t
    e = _bucket_runs([other + 3, 70, 2 * other + 1]) + int_entries(walkkey.walk_order_pks(100))
    try:
        a = check(engine, e, K.INT)
        engine.set_option("kp_tile", other)
        b = check(engine, e, K.INT)
    finally:
        engine.set_option("kp_tile", t)
    assert np.array_equal(a[0], b[0]) and a[2:5] == b[2:5]


def test_bad_arguments(engine):
    d = DevBuf(engine, 256)
    L, c = engine.L, engine.ctx
    assert L.kd_pack_keys_device(c, None, d.ptr, 0, 0, 4, 0, d.ptr, d.ptr, d.ptr) == N.KD_EINVAL
    assert L.kd_pack_keys_device(c, d.ptr, d.ptr, 0, 0, 4, 0, d.ptr, d.ptr, None) == N.KD_EINVAL
    assert L.kd_pack_keys_device(c, d.ptr, d.ptr, 0, 2, 4, 0, d.ptr, d.ptr, d.ptr) == N.KD_EINVAL
    assert L.kd_pack_keys_device(c, d.ptr, d.ptr, 0, N.KD_KEY_HASH, 8, 1, d.ptr, d.ptr, d.ptr) == N.KD_EINVAL  # 64 bits
    assert L.kd_pack_keys_device(c, d.ptr, d.ptr, 0, N.KD_KEY_HASH, 11, 0, d.ptr, d.ptr, d.ptr) == N.KD_EINVAL  # 66 bits
    assert L.kd_pack_keys_device(c, d.ptr, d.ptr, 0, N.KD_KEY_INT, 99, 1, d.ptr, d.ptr, d.ptr) == N.KD_OK  # (ignored)


# ---------------------------------------------------------------------------------------------
# scale
# ---------------------------------------------------------------------------------------------
def test_a_million_int_paths(engine):
    pks = walkkey.walk_order_pks(1_000_000)
    data, off = synth.int_pk_paths(pks)
    got = run(engine, DevBuf.from_numpy(engine, np.concatenate([data, np.zeros(16, np.uint8)])), off, K.INT)
    _compare(got, data, off, K.INT)
    assert got[2][4] == 1 and got[2][2:4] == (0, 999_999) and got[5] == 0


def test_a_million_hash_paths(engine):
    n = 1_000_000
    paths, plen = synth.text_pk_paths(*synth.text_pks(np.arange(n, dtype=np.int64)))
    data, off = synth._arena(paths, plen, synth._walk_order(paths))
    got = run(engine, DevBuf.from_numpy(engine, np.concatenate([data, np.zeros(16, np.uint8)])), off, K.HASH64)
    _compare(got, data, off, K.HASH64)
    assert got[3] == 0 and got[2][4] == 0 and 0 < got[2][5] <= 512


# ---------------------------------------------------------------------------------------------
# sides born in HBM
# ---------------------------------------------------------------------------------------------
def test_tree_join_to_diff_without_a_download(engine):
    """kd_tree_join_batch (device form, k = 2) -> DevSide.from_leaves on both roots -> kd_diff2_device: the
    deltas and counts of the route through the host's pack_side of the same leaves"""
    rng = np.random.default_rng(12)
    trees, tasks, prefixes = [], [], []
    for b in (3, 4, 70, 71, 4097):
        pks = walkkey.walk_order_range(64 * b, 64 * b + 64)
        full = [(0o100644, walkkey.filename(int(p)).encode(), bytes(rng.integers(0, 256, 20, dtype=np.uint8))) for p in pks]
        a = [e for e in full if rng.random() < 0.9]  # (filename order = the order of walk_order_range)
        b_ = [(m, nm, bytes(rng.integers(0, 256, 20, dtype=np.uint8)) if rng.random() < 0.3 else o)
              for m, nm, o in full if rng.random() < 0.9]
        trees += [C.mk(a), C.mk(b_)]
        tasks.append([len(trees) - 2, len(trees) - 1])
        prefixes.append(wide_entry(64 * b).rsplit(b"/", 1)[0])
    order = np.argsort(walkkey.rank_digits(np.array([3, 4, 70, 71, 4097], np.uint64)), kind="stable")  # walk order
    tasks, prefixes = [tasks[i] for i in order], [prefixes[i] for i in order]
    want = C.join_batch(trees, tasks, prefixes, 2, (0, 1))
    data, off = C.arena(trees)
    pfx, pfx_off = C.arena(prefixes)
    d_in = [DevBuf.from_numpy(engine, x) for x in (np.concatenate([data, np.zeros(16, np.uint8)]), off,
                                                   np.array(tasks, np.uint32), np.concatenate([pfx, np.zeros(16, np.uint8)]), pfx_off)]
    outs, bufs = (N.KdTjOut * 2)(), []
    for r in range(2):
        cn, cb = len(want[0][r][3]), len(want[0][r][0])
        b = [DevBuf(engine, s) for s in (8 * (cn + 1), 4 * cn, 20 * cn, cb + 16)]
        bufs.append(b)
        outs[r].cap_n, outs[r].cap_bytes = cn, cb
        outs[r].path_off, outs[r].mode, outs[r].oid, outs[r].path = (x.ptr for x in b)
    nt = len(tasks)
    d_count, d_status, d_tot = DevBuf(engine, 8 * nt), DevBuf(engine, nt), DevBuf(engine, 32)
    N.check(engine.L.kd_tree_join_batch(engine.ctx, d_in[0].ptr, d_in[1].ptr, len(trees), d_in[2].ptr, d_in[3].ptr, d_in[4].ptr,
                                        nt, 2, 0, 1, outs, d_count.ptr, d_status.ptr, d_tot.ptr, N.KD_MEM_DEVICE),
            "kd_tree_join_batch")
    sides, hosts = [], []
    for r in range(2):
        n = len(want[0][r][3])
        assert n > 10
        s = DevSide.from_leaves(engine, bufs[r][3], bufs[r][0], bufs[r][2], n, packing.INT_PK_ENCODING)
        assert isinstance(s, DevSide) and s.oid is bufs[r][2] and s.info.ascending
        sides.append(s)
        wp, wo, wi, _ = want[0][r]
        hosts.append(packing.pack_side(np.frombuffer(bytes(wp), np.uint8), wi, packing.INT_PK_ENCODING, rel_off=wo))
    cap = sides[0].n + sides[1].n + 1
    d_delta, d_upd, d_c = DevBuf(engine, 8 * cap), DevBuf(engine, 8 * cap), DevBuf(engine, 64)
    d_c.zero()
    sa, sb = sides[0].kd_side(), sides[1].kd_side()
    N.check(engine.L.kd_diff2_device(engine.ctx, ctypes.byref(sa), ctypes.byref(sb), 0, d_delta.ptr, d_upd.ptr, d_c.ptr,
                                     d_c.ptr + 32), "kd_diff2_device")
    c = d_c.download(np.uint64, 5)
    ref = engine.diff2(hosts[0], hosts[1])
    assert int(c[4]) & 0xFFFFFFFF == 0
    assert [int(x) for x in c[:4]] == [ref.n_insert, ref.n_update, ref.n_delete, ref.delta.shape[0]] and ref.n_update > 0
    assert np.array_equal(d_delta.download(np.uint32, 2 * int(c[3])).reshape(-1, 2), ref.delta)
    assert np.array_equal(d_upd.download(np.uint32, 2 * int(c[1])).reshape(-1, 2), ref.upd)


def _same_side(a, b):
    assert np.array_equal(a.key, b.key) and np.array_equal(a.oid, b.oid) and np.array_equal(a.order, b.order)
    assert a.key_mode == b.key_mode and a.walk_rows == b.walk_rows
    assert _info_tuple(a.info) == _info_tuple(b.info)
    for x, y in ((a.name, b.name), (a.name_off, b.name_off)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))


def _oids(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 20), dtype=np.uint8)


def test_pack_side_device_keys_equals_the_host_route(engine):
    cases = {
        "ascending int": ([e.decode() for e in int_entries(walkkey.walk_order_pks(3000))], packing.INT_PK_ENCODING),
        # two wraps inside every leaf tree, listed in filename order: the segmented sort
        "wraps inside leaf trees": (sorted(wide_entry(p + w).decode() for p in range(640) for w in (0, 1 << 30)),
                                    packing.INT_PK_ENCODING),
        # one leaf tree of 640 entries (ten wraps, the negative ones listed behind the others): the radix sort
        "a long leaf tree": (sorted(wide_entry(p + w * (1 << 30)).decode() for p in range(64, 128) for w in range(-5, 5)),
                             packing.INT_PK_ENCODING),
        "hash": (sorted(set(e.decode("latin-1") for e in K.hash_valid(K.HASH64) if len(e) < 300 and b"\0" not in e)),
                 packing.GENERAL_ENCODING),
    }
    for name, (paths, enc) in cases.items():
        paths = [p.encode("latin-1") for p in paths]
        oids = _oids(len(paths), 3)
        host = packing.pack_side(paths, oids, enc, engine=engine)
        dev = packing.pack_side(paths, oids, enc, engine=engine, device_keys=True)
        _same_side(dev, host)
        plain = packing.pack_side(paths, oids, enc)  # the sorted form, without an engine
        assert np.array_equal(dev.materialised().key, plain.key) and np.array_equal(dev.materialised().oid, plain.oid), name
        if name == "ascending int":
            assert dev.dev is not None and dev.dperm is None and dev.timing["sort_on"] == "none"
            r = engine.diff2(dev, host)
            assert r.delta.shape[0] == 0
        else:
            assert isinstance(dev.dperm, DevPermSide) and dev.timing["sort_on"] == "gpu", name
            r = engine.diff2(dev, host)
            assert r.delta.shape[0] == 0, name
    seg = cases["wraps inside leaf trees"]
    info = packing.pack_side([p.encode() for p in seg[0]], _oids(len(seg[0]), 3), seg[1]).info
    assert 0 < info.seg_max <= packing.SEG_SORT_MAX and not info.ascending
    assert packing.pack_side([p.encode() for p in cases["a long leaf tree"][0]], _oids(640, 3), seg[1]).info.seg_max == 640
    # without an engine, or with no leaf, the option changes nothing
    paths = [p.encode() for p in cases["ascending int"][0]]
    assert packing.pack_side(paths, _oids(3000, 3), packing.INT_PK_ENCODING, device_keys=True).dev is None
    assert packing.pack_side([], np.zeros((0, 20), np.uint8), packing.INT_PK_ENCODING, engine=engine, device_keys=True).n == 0


def test_pack_errors_carry_the_host_route_s_text(engine):
    paths = [e for e in int_entries(walkkey.walk_order_pks(900))]
    paths[700], paths[800] = b"A/A/A/A/!!", b"A/A/A/A/kc8="
    oids = _oids(900, 4)
    with pytest.raises(packing.PackError) as host:
        packing.pack_side(paths, oids, packing.INT_PK_ENCODING)
    with pytest.raises(packing.PackError) as dev:
        packing.pack_side(paths, oids, packing.INT_PK_ENCODING, engine=engine, device_keys=True)
    assert str(dev.value) == str(host.value) and "2 feature paths not packable" in str(host.value)
    paths = int_entries(walkkey.walk_order_pks(900))
    paths[10] = paths[600]
    with pytest.raises(packing.PackError) as host:
        packing.pack_side(paths, oids, packing.INT_PK_ENCODING)
    with pytest.raises(packing.PackError) as dev:
        packing.pack_side(paths, oids, packing.INT_PK_ENCODING, engine=engine, device_keys=True)
    assert str(dev.value) == str(host.value) == "duplicate join keys within one side"

