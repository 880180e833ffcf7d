"""Field diff on hand-built blobs: every kernel variant against the C oracle bit for bit (masks and
status, failed rows included) and against Python's own decode and ``==``.

The CPU half holds the oracle to Python on every crafted set, which is what lets the GPU half use
the oracle as its bit-exact reference.  The sets (tests/fd_craft.py) are built once per process and
shared by every test and every kernel parametrisation.

Kernels: ``win`` with size_hint 64 is k_fielddiff<S,1> (up to 64 union keys) or <S,4>; with 512 it
is k_fielddiff<L,1> / <L,4>; ``stream`` is k_fielddiff_s, ``walk`` is k_fdwalk; tables above 16 KiB
take k_fielddiff_g whatever the options say.
"""
import numpy as np
import pytest

import fd_craft as F

SMALL_TABLE, BIG_TABLE = F.SMALL_TABLE, F.BIG_TABLE

# (name, factory, statuses that must occur, table bound)
SETS = {
    "semantics": (F.semantics_set, {0}),
    "position": (F.position_set, {0}),
    "payload": (F.payload_set, {0}),
    "queue": (F.queue_set, {0}),
    "wide70": (lambda: F.wide_set(70), {0, 1, 4}),
    "wide300": (lambda: F.wide_set(300), {0, 1, 4}),
    "legends8": (lambda: F.legends_set(8, 4), {0}),
    "legends8s": (lambda: F.legends_set(8, 4, True), {0}),
    "headers": (F.headers_set, {0, 1, 2}),
    "malformed": (F.malformed_set, {0, 1, 4}),
    "tiles": (F.tiles_set, {0}),
}
# the same rows under tables of 24 KiB and more (320 more legends that no blob names): k_fielddiff_g
BIG_SETS = {
    "legends300": (lambda: F.legends_set(300, 14), {0}),
    "legends300s": (lambda: F.legends_set(300, 14, True), {0}),
    "semantics_big": (lambda: F.semantics_set(big=True), {0}),
    "wide300_big": (lambda: F.wide_set(300, big=True), {0, 1, 4}),
    "headers_big": (lambda: F.headers_set(big=True), {0, 1, 2}),
    "malformed_big": (lambda: F.malformed_set(big=True), {0, 1, 4}),
    "maxvals_big": (lambda: F.maxvals_set(big=True), {0, 3}),
}
# (fd_stream / fd_walk selection as in test_gpu_parity, kd_blobs.size_hint)
KERNELS = {"winS": ("win", 64), "winL": ("win", 512), "stream": ("stream", 512), "walk": ("walk", 512)}


def _get(name):
    return {**SETS, **BIG_SETS}[name][0]()


def check_against_python(S, masks, status):
    """status 0: the changed names are Python's.  Any other status: Python raises too, or the row
    holds a nested container (a documented refusal); and no mask bit of a failed row is set"""
    exp = S.expected
    names = S.maps.changed_names_rows(masks)
    for u in range(len(S)):
        if status[u] == 0:
            assert exp[u] is not None, (S.name, u, "Python raises, status 0")
            assert names[u] == exp[u], (S.name, u, names[u], exp[u])
        else:
            assert exp[u] is None or u in S.nested, (S.name, u, int(status[u]), exp[u])
            assert not masks[u].any(), (S.name, u, int(status[u]), "mask bits on a failed row")


def check_gpu(engine, S, hint):
    gm, gs = engine.fielddiff(*S.old_arena, *S.new_arena, None, S.maps, size_hint=hint)
    om, ost = S.oracle
    bad = np.flatnonzero((gs != ost) | (gm != om).any(axis=1))
    first = bad[:8]  # (rows, both statuses, both name lists of the first rows that differ)
    assert bad.size == 0, (S.name, first.tolist(), gs[first].tolist(), ost[first].tolist(),
                           [S.maps.changed_names(gm[u]) for u in first[:4]],
                           [S.maps.changed_names(om[u]) for u in first[:4]])
    check_against_python(S, gm, gs)


def _kernel(engine, request, kern):
    from test_gpu_parity import _fd_kernel

    _fd_kernel(engine, request, KERNELS[kern][0])
    return KERNELS[kern][1]


# ------------------------------------------------------------------------------------------
# CPU half: the oracle against Python


@pytest.mark.parametrize("name", list(SETS) + list(BIG_SETS))
def test_oracle_equals_python(name):
    """kdo_fielddiff == py_feature + py_changed_fields on a crafted set; the statuses the set is
    built to reach all occur; the device tables sit well on their side of the 16 KiB selector"""
    S = _get(name)
    masks, status = S.oracle
    check_against_python(S, masks, status)
    assert set(np.unique(status).tolist()) == {**SETS, **BIG_SETS}[name][1]
    if name in BIG_SETS:
        assert S.table_bytes() >= BIG_TABLE
    else:
        assert S.table_bytes() <= SMALL_TABLE


def test_oracle_equals_python_value_limit():
    """4,096 values are accepted, 4,097 give status 3 (Python raises: the legend has 4,096 columns);
    the schema maps value indices 0-2 only, so the tables stay under 2 KiB (the big-table form of
    the same rows is in BIG_SETS)"""
    S = F.maxvals_set()
    masks, status = S.oracle
    check_against_python(S, masks, status)
    assert status.tolist() == [0, 0, 3, 3, 3, 0]
    assert S.maps.changed_names(masks[1]) == ["n1"]
    assert S.table_bytes() <= SMALL_TABLE


def test_oracle_equals_python_arena_ends():
    S = [F.arena_end_set(r) for r in range(16)]
    assert sorted(int(s.old_arena[1][-1]) % 16 for s in S) == list(range(16))
    assert sorted(int(s.new_arena[1][-1]) % 16 for s in S) == list(range(16))
    for s in S:
        check_against_python(s, *s.oracle)
        assert not s.oracle[1].any()


def test_semantics_matrix_shape():
    """the matrix holds every header form: each type byte msgpack defines for a field value occurs"""
    vm = F.value_matrix()
    assert len({b for _, b in vm}) == len(vm) >= 200
    seen = {b[0] for _, b in vm}
    want = set(range(0xC4, 0xDC)) | {0xC0, 0xC2, 0xC3}
    assert want <= seen, sorted(hex(t) for t in want - seen)
    assert any(t < 0x80 for t in seen) and any(t >= 0xE0 for t in seen) and any(0xA0 <= t < 0xC0 for t in seen)


def test_engine_answers_where_python_raises():
    """the accepted divergences, pinned: more values than the legend holds (either side, both sides)
    and invalid UTF-8 in a str make Python raise; the engine compares the mapped values (a str by
    its bytes) and answers status 0"""
    S, want = F.divergence_set()
    masks, status = S.oracle
    assert S.expected == [None] * len(S)
    assert not status.any()
    assert [S.maps.changed_names(m) for m in masks] == want


# ------------------------------------------------------------------------------------------
# GPU half: every kernel against the oracle and Python

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_semantics(engine, request, kern):
    """every encoding of every value against every other, as the middle value of three (lockstep
    path of k_fielddiff<S,1>, <L,1>, k_fielddiff_s, k_fdwalk): fast_eq on equal type bytes —
    floats with NaN and the two zeros, every int width, str / bin / ext raw bytes — and decode_w +
    scalar_eq + payload_eq on mixed type bytes (int vs float, widths of one str, ext 'G' vs bin)"""
    check_gpu(engine, F.semantics_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_position(engine, request, kern):
    """six value kinds swept through the head window, across its end, between the windows, into the
    tail window and onto the blob's last byte, the two sides 0-15 B apart (rd12's window / global
    split and lds_bytes_eq / the queue / glb_bytes_eq of k_fielddiff<S,1> and <L,1>; the tile image
    of k_fielddiff_s; h_ld16 of k_fdwalk); rows whose paddings differ in presence cross legends and
    take the general path (seek_value_w)"""
    check_gpu(engine, F.position_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_payloads(engine, request, kern):
    """bin payloads of 13 B to 70,000 B outside both windows at every relative skew: task_put's
    refusals (under 16 B, 64 KiB and more) into glb_bytes_eq, coop_differs_u around its 512-B pass,
    k_fdwalk's in-register compare up to 32 B; first / last / middle byte different, and neighbours
    outside the payload that must not count"""
    check_gpu(engine, F.payload_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_queue_overflow(engine, request, kern):
    """three queued payloads per update: a round of k_fielddiff<L,1> (64 updates, 64 slots),
    <S,1> (32, 32) or k_fdwalk (64, 64) overflows its queue and the late lanes compare alone
    (glb_bytes_eq / the walk's own loop)"""
    check_gpu(engine, F.queue_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("cols", [70, 300])
def test_gpu_wide_schema(engine, request, cols, kern):
    """71 and 301 union keys: k_fielddiff<S,4> / <L,4> (mask words in registers), the in-place
    mask words past 256 keys and their clearing on the failed row, keys >= 64 refused by task_put,
    dc / dd array headers; k_fielddiff_s and k_fdwalk with their own register word counts"""
    check_gpu(engine, F.wide_set(cols), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("same", [False, True])
def test_gpu_cross_legend_small_tables(engine, request, same, kern):
    """reordered, dropped and added columns under small tables: the general path of diff_body (map
    codes -1, -2, -3, seek_value_w's backward restarts) in every LDS-table kernel"""
    check_gpu(engine, F.legends_set(8, 4, same), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("name", list(BIG_SETS))
def test_gpu_big_tables(engine, name):
    """tables of 24 KiB and more, so k_fielddiff_g (dv_decode, py_eq, diff_one, seek_value): 300 keys
    x 14 legends with reordered, dropped and added columns (its general path, map codes -1 / -2 /
    -3); the whole value matrix (every int width, floats and NaN, str / bin / ext forms, mixed
    pairs); 301 keys with failing rows behind set bits of the fifth mask word (store_masks' clearing
    of the words kept in place); every header form, unknown legends; the malformed rows — short
    value counts on both sides and on one, status 4 over status 1; 4,096 / 4,097 values"""
    S = _get(name)
    assert S.table_bytes() >= BIG_TABLE
    check_gpu(engine, S, 0)


@gpu
def test_gpu_big_tables_accepted_divergences(engine):
    """surplus values and invalid UTF-8 through k_fielddiff_g: status 0, as the oracle"""
    S, want = F.divergence_set(big=True)
    assert S.table_bytes() >= BIG_TABLE
    gm, gs = engine.fielddiff(*S.old_arena, *S.new_arena, None, S.maps)
    assert not gs.any()
    assert np.array_equal(gm, S.oracle[0])
    assert [S.maps.changed_names(m) for m in gm] == want


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_headers(engine, request, kern):
    """legend headers d9 / da / db and array headers 9x / dc / dd on either side (head_fast's
    fallback into parse_header_w + rd_legend), an unknown legend (status 2), a wrong first byte,
    blobs of 0, 43 and 44 bytes (status 1 and the empty value array)"""
    check_gpu(engine, F.headers_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_value_limit(engine, request, kern):
    """4,096 values pass, 4,097 give status 3, in every LDS-table kernel"""
    check_gpu(engine, F.maxvals_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_malformed(engine, request, kern):
    """statuses 1 and 4 among good rows of the same round: nested values, c1, an ext 'G' that is no
    GeoPackage, truncation, the trailing-byte check, value counts short of the legend (the aligned
    table's value count sends them from the lockstep path to the general one, which reports the
    missing value), each first, last and behind a payload whose compare was already queued — the failed rows' masks come back clear (s_res included)"""
    check_gpu(engine, F.malformed_set(), _kernel(engine, request, kern))


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_accepted_divergences(engine, request, kern):
    """surplus values and invalid UTF-8: the kernels answer as the oracle does (status 0)"""
    S, want = F.divergence_set()
    gm, gs = engine.fielddiff(*S.old_arena, *S.new_arena, None, S.maps, size_hint=_kernel(engine, request, kern))
    assert not gs.any()
    assert np.array_equal(gm, S.oracle[0])
    assert [S.maps.changed_names(m) for m in gm] == want


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_arena_ends(engine, request, kern):
    """arenas of every length mod 16 whose last blob ends, with a payload, at the arena's end:
    k_fdwalk's guarded loads, the tail windows of k_fielddiff, the last chunk of k_fielddiff_s"""
    hint = _kernel(engine, request, kern)
    for r in range(16):
        check_gpu(engine, F.arena_end_set(r), hint)


@gpu
@pytest.mark.parametrize("kern", list(KERNELS))
def test_gpu_stream_tiles(engine, request, kern):
    """32-update tiles whose spans reach the 16,384-B tile buffer of k_fielddiff_s inside a header,
    inside a value and at a blob's end, +-0 / 1 / 15 / 16 / 17 B: its residency test and the
    global-memory form of the blobs past the buffer (the other kernels run the same rows)"""
    check_gpu(engine, F.tiles_set(), _kernel(engine, request, kern))
