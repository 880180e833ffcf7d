"""The geometry filter (kd_geomfilter.hip) on crafted inputs (tests/gf_craft.py): the register
window of ``decode_side`` at every start residue and at the arena's end, GPKG headers and envelopes
at every decision edge, legend tables at their limits, msgpack header forms, damaged blobs, and
delta lists around the wave, round, tile and scan seams.

The CPU half pins the oracle (``O.geom_filter``, the C restatement) to its Python restatement on
every set and checks that each set reaches what it is built for.  The GPU half runs every set
through every form of the filter — the blob arenas (k_gf_match), per-entry heads with and without
arenas (k_gf_heads + k_gf_fb), delta-order heads (k_gf_dense), and the three device forms with the
delta count in a device word — and demands the oracle's codes, kept list, ``enc_ok`` and index
envelopes, at bits 0, 2, 6, 20 and 32.

One stated difference: the arena form reads a 112-byte window and does not walk a blob behind its
geometry value, so a blob damaged only *after* that value is answered as its well-formed twin
(include/kartdiff.h at kd_geom_filter); the heads forms refuse it as the reference does.  The
``tails`` set pins exactly that rule, row by row.
"""
import numpy as np
import pytest

import gf_craft as C
from kart_amd import _native as N
from kart_amd import spatial as S
from oracle import oracle as O

BITS = (0, 2, 6, 20, 32)
# the codes each set must reach (0 NON_MATCHING, 1 CANDIDATE, 2 MATCHING, 3 FALLBACK, 4 NONEXISTENT)
REACH = {"window": {0, 1, 2, 3, 4}, "window_end": {0, 1, 2, 4}, "gpkg": {0, 1, 2, 3, 4}, "legends": {0, 2, 3, 4},
         "headers": {2, 3, 4}, "tiles": {0, 1, 2, 3, 4}, "tails": {2, 3, 4}}


def calls_of(name):
    return C.tails_set()[:1] if name == "tails" else C.SETS[name]()


def mismatch(call, got, want, what):
    """the first rows that differ: set, row, note, start residues, both values"""
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[:6]
    return [(what, call.describe(int(r)), np.asarray(got)[r].tolist(), np.asarray(want)[r].tolist()) for r in bad]


def check(call, got, want, bits, form):
    """codes, kept list, enc_ok, and enc where enc_ok, equal ``want``"""
    codes, keep, enc, ok = got
    wc, wk, wenc, wok = want
    assert codes.shape == wc.shape, (call.name, form, bits, codes.shape, wc.shape)
    assert np.array_equal(codes, wc), (form, bits, mismatch(call, codes, wc, "codes"))
    assert np.array_equal(keep, wk), (form, bits, call.name, keep[:8].tolist(), wk[:8].tolist(), len(keep), len(wk))
    if bits:
        assert np.array_equal(ok, wok), (form, bits, mismatch(call, ok, wok, "enc_ok"))
        m = wok == 1
        assert np.array_equal(enc[m], wenc[m]), (form, bits, mismatch(call, enc * m[:, None], wenc * m[:, None], "enc"))


# ------------------------------------------------------------------------------------------
# CPU half


@pytest.mark.parametrize("name", list(REACH))
def test_oracle_c_equals_python(name):
    """kdo_geom_filter == the msgpack.unpackb restatement on every crafted call, at every index
    envelope width; the set reaches the codes it is built for, with and without an index envelope"""
    seen, oks = set(), set()
    for call in calls_of(name) + (C.tails_set()[1:] if name == "tails" else []):
        if name == "tiles" and call.n > 300:
            bits_here = (20,)  # (the big calls repeat the small calls' seven blobs: one width for the Python walk)
        else:
            bits_here = BITS[1:]
        for bits in bits_here:
            c, p = call.oracle(bits), call.oracle(bits, py=True)
            for x, y, what in zip(c, p, ("codes", "keep", "enc", "ok")):
                assert np.array_equal(x, y), (bits, mismatch(call, x, y, what) if what != "keep" else call.name)
        codes, _, _, ok = call.oracle(20)
        seen |= set(np.unique(codes).tolist())
        oks |= set(np.unique(ok).tolist())
    assert seen >= REACH[name], (name, seen)
    assert oks == {0, 1}, (name, oks)


def test_window_reaches_every_residue_and_arena_end():
    """each layout of ``window`` starts at every residue 0..15 on both sides (asserted while laying
    out), a delta's two blobs never at the same one; every value-header / ext form occurs, so the
    geometry payload starts at blob bytes 47, 48, 49, 50 and 52; ``window_end`` has a last blob at
    every (distance from the arena's end, residue), on both sides of the register-window switch"""
    (W,) = C.window_set()
    r = np.array([(W.residue(d, 0), W.residue(d, 1)) for d in range(W.n)])
    both = (r >= 0).all(axis=1)
    assert both.sum() > 1000 and (r[both, 0] != r[both, 1]).all()
    q = set()
    for note, b in C.window_layouts():
        parts = note.split("/")
        if len(parts) == 3 and parts[1] in ("e8", "e16", "e32"):
            p = 44 if parts[0] == "fix" else 46
            q.add(p + {"e8": 3, "e16": 4, "e32": 6}[parts[1]])
            assert b[p] in (0xc7, 0xc8, 0xc9)
    assert q == {47, 48, 49, 50, 52}
    assert {len(b) for n, b in C.window_layouts() if n.startswith("len")} == {51, 52, 53}
    cov = C.end_coverage()
    assert cov == {(d, res) for d in C.END_DIST for res in range(16)}
    fast = {(d, res) for d, res in cov if d + (res & 3) >= 112}
    assert fast and cov - fast and {res for _, res in fast} == set(range(16))
    assert min(d for d, _ in fast) == 109 and max(d for d, _ in cov - fast) == 111


def test_gpkg_values_cover_every_header():
    vals = dict(C.gpkg_values(C.G_FILT))
    flags = {g[3] for n, g in vals.items() if n.startswith("flags")}
    assert flags == set(range(0x40))


@pytest.mark.parametrize("name", ["headers", "tails", "window"])
def test_geom_heads_equal_oracle_feature_geometry(name):
    """kd_geom_heads (the host pass behind every heads form) against O.feature_geometry: status,
    GPKG length, its first 40 bytes and its offset, blob by blob under each side's own table"""
    seen = set()
    for call in calls_of(name):
        for s, heads in enumerate(call.heads()):
            for i, b in enumerate(call.blobs[s]):
                st, g = call.geometry(s, i)
                hs = int(heads["goff_status"][i]) >> 24
                where = (call.name, s, i)
                if st:
                    assert hs == N.KD_GH_FALLBACK, where
                elif g is None:
                    assert hs == N.KD_GH_NULL, where
                else:
                    assert hs == N.KD_GH_GEOM and int(heads["glen"][i]) == len(g), where
                    assert heads["gpkg"][i].tobytes()[:min(40, len(g))] == g[:40], where
                    goff = int(heads["goff_status"][i]) & 0xFFFFFF
                    assert bytes(b[goff:goff + len(g)]) == g, where
                seen.add(hs)
    assert seen == {N.KD_GH_GEOM, N.KD_GH_NULL, N.KD_GH_FALLBACK}


def test_tails_rows_are_damaged_and_their_twins_are_not():
    """the oracle refuses (3) every damaged row, and answers each row's W with something else:
    otherwise the row would prove nothing"""
    T, TW = C.tails_set()
    codes, wcodes = T.oracle(20)[0], TW.oracle(20)[0]
    rows = C.tail_rows()
    assert {r[3] for r in rows} == {"twin", "after", "before"}
    for d in range(T.n):
        for s in range(2):
            if T.pairs[d, s] == C.NONE:
                continue
            assert wcodes[d, s] not in (3, 4), T.describe(d)
            assert (codes[d, s] == wcodes[d, s]) if T.where[d] == "twin" else (codes[d, s] == 3), T.describe(d)
    exp = C.tails_arena_expected(20)[0]
    after = np.array([w == "after" for w in T.where])
    assert (exp[after] != codes[after]).any(axis=1).all() and np.array_equal(exp[~after], codes[~after])


def test_tiles_patterns():
    """the kept patterns are what they say (rows the specials overwrite aside)"""
    for n in (64, 256):  # (no specials below 257 deltas)
        want = {"all": n, "none": 0, "alternating": n // 2, "last-lane": n // 64, "last-delta": 1}
        for call in C.tiles_set():
            _, cnt, pat = call.name.split("/")
            if int(cnt) == n:
                assert len(call.oracle(20)[1]) == want[pat], call.name
    big = [c for c in C.tiles_set() if c.name.startswith("tiles/8193/")]
    for call in big:
        codes = call.oracle(20)[0]
        assert codes[4095].tolist() == [0, 4] and codes[4096].tolist() == [0, 0]  # deferred, then NON_MATCHING
        nb = call.needs_blob()
        assert nb[4095, 0] and nb[4096, 1] and nb[4092].all()
    assert sum(len(c.hand) for c in C.tiles_set()) == 20


# ------------------------------------------------------------------------------------------
# GPU half

def run_arena(engine, call, bits):
    return S.geom_filter(engine, *call.arenas, call.pairs, call.geom_cols(), call.filt, call.rect, bits)


def run_heads(engine, call, bits, arenas=True, delta=False):
    heads = call.heads()
    pairs = call.pairs
    if delta:
        heads = C.delta_order_heads(heads, pairs, max((call.n + 63) // 64 * 64, 64))
    return S.geom_filter_heads(engine, heads[0], heads[1], pairs, call.filt, call.rect, bits,
                               arenas=call.arenas if arenas else None, delta_heads=delta)


def want_of(name, call, bits, form):
    """the oracle's answer; on ``tails`` the arena forms answer a row damaged after its geometry
    value as its well-formed twin"""
    if name == "tails" and form in ("arena", "dev-arena"):
        return C.tails_arena_expected(bits or 20)
    return call.oracle(bits)


def without_arenas(call, want):
    """exactly the sides whose head needs its blob read 3; the new side's index envelope is then absent"""
    codes, _, enc, ok = want
    nb = call.needs_blob()
    codes = np.where(nb, 3, codes).astype(np.uint8)
    keep = np.nonzero(((codes >= 1) & (codes <= 3)).any(axis=1))[0].astype(np.uint32)
    return codes, keep, enc, np.where(nb[:, 1], 0, ok).astype(np.uint8)


HOST_FORMS = ("arena", "heads", "heads-noarena", "delta-heads")


@pytest.mark.gpu
@pytest.mark.parametrize("form", HOST_FORMS)
@pytest.mark.parametrize("name", list(REACH))
def test_gpu_forms_equal_oracle(engine, name, form):
    """every call of the set through one form of the filter, at every index-envelope width"""
    needed = False
    for call in calls_of(name):
        for bits in BITS:
            want = want_of(name, call, bits, form)
            if form == "arena":
                got = run_arena(engine, call, bits)
            elif form == "heads":
                got = run_heads(engine, call, bits)
            elif form == "delta-heads":
                got = run_heads(engine, call, bits, delta=True)
            else:
                got = run_heads(engine, call, bits, arenas=False)
                needed |= bool(call.needs_blob().any())
                want = without_arenas(call, want)
            check(call, got, want, bits, form)
    if form == "heads-noarena" and name in ("window", "gpkg", "tiles"):
        assert needed  # the set holds heads that need their blob


DEV_FORMS = ("arena", "gather", "delta")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["full", "zero", "below"])
@pytest.mark.parametrize("form", DEV_FORMS)
@pytest.mark.parametrize("name", ["tiles", "window", "window_end", "gpkg", "tails"])
def test_gpu_device_forms_equal_oracle(engine, name, form, mode):
    """the device forms (delta count in a device word): count = capacity, count 0, and a count
    below a capacity two tiles larger with poisoned pairs beyond it — every output at or beyond the
    count (beyond n_keep for the kept list) keeps its sentinel"""
    calls = calls_of(name)
    if mode != "full":
        calls = calls[::7] if name == "window_end" else calls  # (208 small arenas: the count's handling is the same in each)
    for call in calls:
        for bits in BITS:
            got = C.device_filter(engine, call, bits, form, mode)
            assert got[4], (call.name, form, mode, bits, "an output beyond the count was written")
            if mode == "zero":
                assert got[0].shape[0] == 0 and got[1].size == 0
                continue
            check(call, got[:4], want_of(name, call, bits, "dev-" + form), bits, f"dev-{form}/{mode}")


@pytest.mark.gpu
def test_gpu_too_many_legends_refused(engine):
    """65 legends on a side: KD_EUNSUPPORTED, the caller takes the reference path"""
    call = C.too_many_legends()
    with pytest.raises(N.Unsupported):
        run_arena(engine, call, 20)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["arena", "delta"])
def test_gpu_scan_carry(engine, form):
    """8,193 tiles: k_gf_scan's second pass carries the first pass's total.  All deltas are
    (NONE, NONE) but five whose new side is a null geometry — delta 0, the last of tile 0, the last
    of tile 8191, the first of tile 8192 and the last delta: exactly those are kept, in order"""
    codes, keep = C.scan_device(engine, form)
    want = np.full((C.SCAN_N, 2), 4, np.uint8)
    want[list(C.SCAN_ROWS), 1] = 2
    assert keep.tolist() == list(C.SCAN_ROWS), (form, keep[:8].tolist())
    assert np.array_equal(codes, want), (form, np.argwhere(codes != want)[:5].tolist())


def test_scan_expectation_is_the_oracles():
    """the oracle over the scan set's pairs (host arrays; no kernel): the rows stated above"""
    pairs = np.full((C.SCAN_N, 2), C.NONE, np.uint32)
    pairs[list(C.SCAN_ROWS)] = (C.NONE, 0)
    nd, no = C.arena(C.scan_blobs())
    codes, keep, _, _ = O.geom_filter(np.zeros(0, np.uint8), np.zeros(1, np.uint64), nd, no, pairs, dict(C.TAB), dict(C.TAB),
                                      C.W_FILT, True, 20)
    assert keep.tolist() == list(C.SCAN_ROWS) and (codes[keep, 1] == 2).all() and (codes[:, 0] == 4).all()
    assert int((codes[:, 1] == 4).sum()) == C.SCAN_N - len(C.SCAN_ROWS)
