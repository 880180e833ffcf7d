"""The three-way join at its seams: crafted merges that land on each data-dependent fork of
k_join3b, k_apart3b and k_partition2<384> (kd_classify2.hip).  The CPU tests assert, from a host
model of the tile geometry (tests/j3_craft.py), that every input still reaches the seam its builder
names, and hold the oracle to a pure-Python classify3; the GPU tests hold engine.merge3 to the
oracle bit for bit, order included, for int and hash keys, in sorted form and through walk orders,
with the one-pass join and with the two-step path (merge3_join = 0)."""
import ctypes
import functools

import numpy as np
import pytest

import j3_craft as C
from j3_craft import ACAP, GROUP, HALO, NAME_CH, TILE, Case
from oracle import oracle as O

from kart_amd import _native as N

gpu = pytest.mark.gpu
S = 16  # key spacing: room for ancestor-only keys between two paths
CANARY = 0xA5
LENS = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33] + list(range(60, 69)) + [100, 200]
PAIRS = ["same", "omod", "tmod", "conf", "bothmod"]  # kinds that ours and theirs both hold


def _keys(n, first=1):
    return S * (first + np.arange(n, dtype=np.uint64))


# ---------------------------------------------------------------------------------------------
# the crafted inputs (CPU; each is built once)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def seam1():
    """seam 1, ancestor search at every width: 330 full tiles of ours-only rows; tile t < 329 holds
    t ancestor keys in its key range (every other one a key of ours, the rest in the gaps between
    ours' keys) and sees one lookahead key, tile 328 holds 329 and sees none, the last tile holds
    none: nk = 1..329 and 0"""
    nt = 330
    ko = _keys(nt * TILE)
    key, va = [ko], [np.full(ko.size, -1, np.int64)]
    for t in range(nt - 1):
        c = t if t < nt - 2 else t + 1  # (the last of them has no lookahead key: no ancestor key follows its own)
        m = np.arange(c)
        x = t * TILE + (m * TILE) // max(c, 1)
        on = m % 2 == 0
        va[0][x[on]] = np.where(m[on] % 4 == 0, 1, 0)  # the ancestor's OID equals ours (merge delta) or not (conflict)
        key.append(ko[x[~on]] + np.uint64(8))
        va.append(np.zeros(int((~on).sum()), np.int64))
    key, va = np.concatenate(key), np.concatenate(va)
    o = np.argsort(key)
    vo = np.concatenate([np.ones(ko.size, np.int64), np.full(key.size - ko.size, -1, np.int64)])
    return Case(key[o], va[o], vo[o], np.full(key.size, -1, np.int64), lens=6)


SEAM2_NDIF = [0, 1, 191, 192, 192, 193, 383, 384, 384]


@functools.lru_cache(None)
def seam2():
    """seam 2, compaction passes and the clean count: one tile each of 0 (192 unchanged pairs), 1, 191,
    192 (every pair a conflict), 192, 193, 383 and 384 (ours-only additions; then mixed one-sided
    paths) differing paths, each tile's kinds shuffled, with a few ancestor-only keys"""
    rng = np.random.default_rng(2)
    changed, kept = ["omod", "tmod", "conf", "addconf"], ["same", "addadd", "bothmod"]
    single = ["oadd", "tadd", "odel", "tdel", "odel_tmod", "omod_tdel"]
    cyc = lambda names, n: [names[x % len(names)] for x in range(n)]
    blocks = [cyc(kept, 192), cyc(kept, 191) + ["conf"], cyc(changed, 191) + ["same"], ["conf"] * 192, cyc(changed, 192),
              cyc(changed, 191) + cyc(single, 2), ["tmod"] + cyc(single, 382), ["oadd"] * 384, cyc(single, 384)]
    kinds = []
    for b in blocks:
        b = b + ["bothdel"] * 5
        kinds += [b[x] for x in rng.permutation(len(b))]
    return Case.of_kinds(_keys(len(kinds)), kinds)


def _pairs(n, start=0):
    return [PAIRS[(start + x) % len(PAIRS)] for x in range(n)]


@functools.lru_cache(None)
def seam3():
    """seam 3, straddling pairs and ragged ends at the 384-item tile: {name: Case}"""
    out = {"insert_first": Case.of_kinds(_keys(601), ["tadd"] + _pairs(600)),
           "delete_first": Case.of_kinds(_keys(601), ["oadd"] + _pairs(600))}
    for rem in (1, 2, 3, 191, 193, 383):
        e = 2 + rem % 2
        m = (TILE + rem - e) // 2
        for one in ("tadd", "oadd"):
            kinds = _pairs(m, rem)
            for at in (m, m // 2, 0)[:e]:
                kinds.insert(at, one)
            out["rem%d_%s" % (rem, one)] = Case.of_kinds(_keys(len(kinds)), kinds)
    base = np.array([C.KINDS[k] for k in (PAIRS + ["oadd", "tadd", "odel", "tdel", "addconf"]) * 60], np.int64)
    for role, name in enumerate(("anc", "ours", "theirs")):
        for keep in (0, 1):
            v = base.copy()
            v[:, role] = -1
            if keep:
                v[250, role] = 3
            out["%s_%d" % (name, keep)] = Case(_keys(len(v)), v[:, 0], v[:, 1], v[:, 2])
    out["anc_only"] = Case.of_kinds(_keys(5), ["bothdel"] * 5)
    return out


@functools.lru_cache(None)
def seam4():
    """seam 4, k_apart3b's guess: 4,000 ancestor keys that both sides deleted, below, above and amid
    2,000 paths of which ours and theirs hold ~700 each; an ancestor of under 256 keys; ours empty"""
    rng = np.random.default_rng(4)

    def live(n, p_anc=1.0, p_ours=0.35):
        va = np.where(rng.random(n) < p_anc, 0, -1)
        vo = np.where(rng.random(n) < p_ours, rng.integers(0, 2, n), -1)
        vt = np.where(rng.random(n) < 0.35, 2 * rng.integers(0, 2, n), -1)
        return np.stack([va, vo, vt], 1)

    dead = np.tile(np.array([[0, -1, -1]]), (4000, 1))
    sets = {"below": [dead, live(2000)], "above": [live(2000), dead], "middle": [live(1000), dead, live(1000)],
            "small_k": [live(2000, p_anc=0.05)], "ours_empty": [live(3000, p_ours=0.0)]}
    out = {}
    for name, parts in sets.items():
        v = np.concatenate(parts)
        out[name] = Case(_keys(len(v)), v[:, 0], v[:, 1], v[:, 2])
    return out


CAP_TARGETS = [NAME_CH - 1, NAME_CH, NAME_CH + 1, NAME_CH + 2]


@functools.lru_cache(None)
def seam5_cap(perm):
    """seam 5, the name staging cap: four full tiles of matched pairs, then four of ours-only rows;
    the model picks each tile's name length L and how many of its rows carry L + 1 so that the
    tile's staged chunks come to 999, 1000, 1001 and 1002 (sorted form: 385 staged rows; through
    walk orders: 417 with the halo)"""
    kinds = _pairs(4 * 192) + ["oadd"] * (4 * TILE)
    case = Case.of_kinds(_keys(len(kinds)), kinds)
    rows = [(192 * t, 192 * (t + 1)) for t in range(4)] + [(768 + TILE * t, 768 + TILE * (t + 1)) for t in range(4)]
    lens = np.full(len(kinds), 20, np.int64)

    g = C.geometry(*case.k, perm)  # (the staged rows do not depend on the lengths)

    def ch(t):
        offO, offT = (np.concatenate([[0], np.cumsum(lens[i])]) for i in case.idx[1:])
        return int(C.chunks(offO[g.rA0[t]], offO[g.rA1[t]]) + C.chunks(offT[g.rB0[t]], offT[g.rB1[t]]))

    for _ in range(4):  # (a tile's lookahead and halo rows belong to its neighbours: later passes settle them)
        for t, (a, b) in enumerate(rows):
            want = CAP_TARGETS[t % 4]
            for L in range(32, 48):
                lens[a:b] = L + 1
                if ch(t) >= want:
                    break
            lo, hi = 0, b - a  # the smallest r whose last r rows at L + 1 reach the target
            while lo < hi:
                r = (lo + hi) // 2
                lens[a:b] = L
                lens[b - r:b] = L + 1
                lo, hi = (lo, r) if ch(t) >= want else (r + 1, hi)
            lens[a:b] = L
            lens[b - lo:b] = L + 1
    return Case.of_kinds(case.key, kinds, lens=lens)


@functools.lru_cache(None)
def seam5_mixed():
    """seam 5, one mixed-length input: 4,000 paths of every kind with names of every length in LENS"""
    rng = np.random.default_rng(5)
    names = list(C.KINDS)
    w = np.array([3.0 if k in ("odel", "odel_tmod", "omod", "conf") else 1.0 for k in names])
    kinds = rng.choice(names, size=4000, p=w / w.sum()).tolist()
    lw = np.array([0.25 if x >= 100 else 1.0 for x in LENS])
    return Case.of_kinds(_keys(4000), kinds, lens=rng.choice(LENS, size=4000, p=lw / lw.sum()), seed=55)


def _sites(case):
    """the paths at each of the three filename compare sites, as (path mask, side whose name meets
    the first: 1 ours | 2 theirs, first side: 1 ours | 0 the ancestor)"""
    p = C.paths(case)
    return p, {"ours_theirs": (p.matched, 2, 1),
               "anc_ours": (p.differ & (p.ia >= 0) & (p.io >= 0), 1, 0),
               "anc_theirs": (p.differ & (p.ia >= 0) & (p.io < 0) & (p.it >= 0), 2, 0)}


SEAM6_KINDS = ["same", "omod", "tmod", "conf", "odel", "omod_tdel", "addadd", "oadd",
               "same", "conf", "bothmod", "odel_tmod", "odel", "tdel", "addconf", "tadd"]
HALO_TARGETS = ("lo-1", "lo", "hi-1", "hi")


def _halo_hits(case, order):
    """{(side, 'pair' | 'path', target)}: a matched pair's / a differing path's walk row on that side is
    exactly the first row before the staged rows, the first staged, the last staged, the first after"""
    g = C.case_geometry(case, True, order)
    p, hits = C.paths(case), set()
    with_anc = p.differ & (p.ia >= 0)
    for side, x, r0, r1, path in (("ours", p.io, g.rA0, g.rA1, with_anc & (p.io >= 0)),
                                  ("theirs", p.it, g.rB0, g.rB1, with_anc & (p.io < 0) & (p.it >= 0))):
        row = np.asarray(order[1 if side == "ours" else 2])[np.maximum(x, 0)]
        for what, mask in (("pair", p.matched), ("path", path)):
            for name, v in zip(HALO_TARGETS, (r0 - 1, r0, r1 - 1, r1)):
                if (mask & (row == v[p.tile])).any():
                    hits.add((side, what, name))
    return hits


HALO_ALL = {(s, w, t) for s in ("ours", "theirs") for w in ("pair", "path") for t in HALO_TARGETS}


@functools.lru_cache(None)
def seam6():
    """seam 6, walk rows around the halo: (Case, orders); every order is the identity except for one
    reversed segment of length 8, 9, 10, 17 or 64 across each tile's first row on ours, on theirs
    and at the tile's ancestor seam.  The model keeps, of 400 seeded placements, those that put a
    new (side, pair | path) on one of the four rows around the staged range; a fully random
    permutation of every side is the last order"""
    case = Case.of_kinds(_keys(1400), [SEAM6_KINDS[x % 16] for x in range(1400)], lens=11)
    g = C.geometry(*case.k)
    rng = np.random.default_rng(6)
    orders, seen = [], set()
    for _ in range(400):
        cand = []
        for n, cuts in zip((k.size for k in case.k), (g.apart, g.i, g.j)):
            segs = []
            for b in np.unique(cuts[1:-1]).tolist():
                L = int(rng.choice(C.SEGMENTS))
                s = b - int(rng.integers(0, L + 2))
                if not segs or s > segs[-1][0] + segs[-1][1]:
                    segs.append((s, L))
            cand.append(C.displaced(n, segs))
        new = _halo_hits(case, cand) - seen
        if new:
            orders.append(cand)
            seen |= new
        if seen == HALO_ALL:
            break
    orders.append([rng.permutation(k.size) for k in case.k])
    return case, orders


SITES = {"ours_theirs": ("same", 2), "anc_ours": ("omod", 0), "anc_theirs": ("odel_tmod", 2)}  # victim kind, corrupted side
ROUTES = ("lds", "cap", "perm")
COLL_LENS = (1, 4, 5, 33, 63, 64, 65, 100)
VICTIM = 192  # the path that opens tile 1: 192 pairs lie before it


def collision_case(site, route, L):
    """seam 7: 400 paths (~800 rows), every path before the victim a pair, so the victim's entries are
    tile 1's first on ours and on theirs.  -> (Case, orders | None, side to corrupt, victim's index there)"""
    kinds = _pairs(400)
    kinds[VICTIM] = SITES[site][0]
    lens = np.full(400, 20, np.int64)
    lens[VICTIM] = L
    if route == "cap":
        lens[VICTIM + 1:VICTIM + 101] = 200  # ~100 long names in the victim's tile: over the cap
    case = Case.of_kinds(_keys(400), kinds, lens=lens, seed=7 + L)
    orders = None
    if route == "perm":  # the compared row of ours (else theirs) 9 before its sorted place
        moved = 1 if site == "anc_ours" else 2
        orders = [C.displaced(k.size, [(VICTIM - 9, 10)] if s == moved else []) for s, k in enumerate(case.k)]
    s = SITES[site][1]
    return case, orders, s, int(np.searchsorted(case.k[s], case.key[VICTIM]))


def corruptions(name):
    """{how: corrupted name}; a byte position that an earlier corruption already took is skipped"""
    L, out, taken = len(name), {}, set()
    for how, at in (("first", 0), ("byte3", 3), ("last_dword", 4 * ((L - 1) // 4)), ("last", L - 1)):
        if at < L and at not in taken:
            taken.add(at)
            b = bytearray(name)
            b[at] ^= 0x40
            out[how] = bytes(b)
    out["appended"] = name + b"x"
    out["dropped"] = name[:-1]
    return out


@functools.lru_cache(None)
def seam8_anc():
    """seam 8, the ancestor's order: 600 shared paths (4 tiles); the ancestor holds 50 keys before
    them, 400 deleted ones inside tile 2's key range (a range over 320, read from HBM) and 50 beyond"""
    kinds = ["bothdel"] * 50 + _pairs(600) + ["bothdel"] * 50
    key = _keys(700)
    g = C.geometry(key[50:650], key[50:650], key[50:650])
    lo = int(key[50 + int(g.i[2]) + 20])
    extra = lo + 1 + np.arange(400, dtype=np.uint64) % 15 + S * (np.arange(400, dtype=np.uint64) // 15)
    allk = np.concatenate([key, extra])
    o = np.argsort(allk)
    return Case.of_kinds(allk[o], [(kinds + ["bothdel"] * 400)[x] for x in o.tolist()])


def seam8_anc_positions():
    """{name: x}: the pair x - 1 | x of the ancestor to break, from the valid input's geometry"""
    case = seam8_anc()
    g = C.geometry(*case.k)
    nK = case.k[0].size
    big = int(np.argmax(g.nk))
    return g, {"first": 1, "before_all": 25, "staged": int(g.k0[1]) + 40, "seam": int(g.k0[1]),
               "over_acap": int(g.k0[big]) + 200, "last": nK - 1, "beyond_all": nK - 25}


SEAM3 = (["insert_first", "delete_first"] + ["rem%d_%s" % (r, o) for r in (1, 2, 3, 191, 193, 383) for o in ("tadd", "oadd")] +
         ["%s_%d" % (n, k) for n in ("anc", "ours", "theirs") for k in (0, 1)] + ["anc_only"])
SEAM4 = ["below", "above", "middle", "small_k", "ours_empty"]
NAMES = (["seam1", "seam2", "seam5_cap_sorted", "seam5_cap_perm", "seam5_mixed", "seam6", "seam8_anc"] +
         ["seam3_" + n for n in SEAM3] + ["seam4_" + n for n in SEAM4] +
         ["seam7_%s_%s" % (s, r) for s in SITES for r in ROUTES])


def case_of(name):
    """a positive crafted input by its name in NAMES"""
    if name.startswith("seam3_"):
        return seam3()[name[6:]]
    if name.startswith("seam4_"):
        return seam4()[name[6:]]
    if name.startswith("seam7_"):
        site, route = [(s, r) for s in SITES for r in ROUTES if name == "seam7_%s_%s" % (s, r)][0]
        return collision_case(site, route, 33)[0]
    return {"seam1": seam1, "seam2": seam2, "seam5_cap_sorted": lambda: seam5_cap(False),
            "seam5_cap_perm": lambda: seam5_cap(True), "seam5_mixed": seam5_mixed, "seam6": lambda: seam6()[0],
            "seam8_anc": seam8_anc}[name]()


@functools.lru_cache(None)
def oracle_of(name):
    return O.classify3(*case_of(name).flat())


# ---------------------------------------------------------------------------------------------
# CPU: constants, reach, oracle cross-check
# ---------------------------------------------------------------------------------------------
def test_constants_guard():
    """the constants the cases are built around are the kernel's defaults, and the default build
    overrides none of them: a retune fails here instead of moving every case off its seam"""
    want = dict(TILE=C.TILE, NT=C.NT, ACAP=C.ACAP, HALO=C.HALO, NAME_CH=C.NAME_CH, GROUP=C.GROUP,
                APART_STEP=C.APART_STEP, APART_PROBES=C.APART_PROBES)
    assert C.read_defaults() == want
    assert want == dict(TILE=384, NT=192, ACAP=320, HALO=8, NAME_CH=1000, GROUP=64, APART_STEP=256, APART_PROBES=8)
    flags = C.makefile_flags()
    assert "--offload-arch" in flags and "-DKD_J3B" not in flags and "-DKD_C2" not in flags and "-DC2_" not in flags


def test_model_splits_match_definition():
    """the model's vectorised splits are the merge-path splits by their definition (ties: ours first)"""
    for case in (seam2(), seam3()["insert_first"], seam4()["middle"], seam6()[0]):
        g = C.geometry(*case.k)
        for t in range(g.nt + 1):
            i, monotone = C.split_by_definition(case.k[1], case.k[2], int(g.d[t]))
            assert monotone and i == g.i[t] and g.j[t] == g.d[t] - i
        assert (case.k[0][g.apart[1:-1] - 1] < g.first[1:-1])[g.apart[1:-1] > 0].all()
        assert (case.k[0][np.minimum(g.apart[1:-1], case.k[0].size - 1)] >= g.first[1:-1])[g.apart[1:-1] < case.k[0].size].all()


def test_reach_seam1():
    """seam 1: the model's nk per tile takes every value 0..329, on both sides of the staged cap, with every
    lower-bound position, over more than five 64-tile groups"""
    case = seam1()
    g = C.geometry(*case.k)
    assert g.nt == 330 and case.k[2].size == 0 and case.k[1].size == 330 * TILE
    assert set(g.nk.tolist()) == set(range(330)), "the cases no longer reach every ancestor range width"
    assert {ACAP - 1, ACAP, ACAP + 1} <= set(g.nk.tolist()) and g.lk.any() and not g.lk.all(), \
        "the cases no longer reach both sides of the staged ancestor range's cap"
    assert g.nt > 5 * GROUP, "the cases no longer cross the placement's tile groups"
    # every key of ours is searched: its lower bound inside its tile's range takes every position 0..nk - 1
    # (the lookahead key is never passed), and nk where no lookahead key follows
    tile = np.arange(case.k[1].size) // TILE
    pos = np.searchsorted(case.k[0], case.k[1]) - g.k0[tile]
    hit = np.zeros((g.nt, 331), bool)
    hit[tile, pos] = True
    want = np.arange(331)[None, :] < (g.nk + (g.k1 == case.k[0].size))[:, None]
    assert np.array_equal(hit, want), "the cases no longer reach every lower-bound position of every width"
    assert set(case.v[0][case.v[1] >= 0].tolist()) == {-1, 0, 1}, "the outcomes no longer mix"  # clean, conflict, merge delta
    gh = C.case_geometry(case)
    assert gh.lnames.all()


def test_reach_seam2():
    """seam 2: the model's count of differing paths per tile is 0, 1, 191, 192, 193, 383 and 384, each block one tile"""
    case = seam2()
    p = C.paths(case)
    ndif = np.bincount(p.tile[p.differ], minlength=len(SEAM2_NDIF)).tolist()
    assert ndif == SEAM2_NDIF, "the cases no longer reach the compaction's pass boundaries"
    assert {0, 1, C.NT - 1, C.NT, C.NT + 1, 2 * C.NT - 1, 2 * C.NT} <= set(ndif)
    items = np.bincount(p.tile, weights=1 + p.matched, minlength=len(ndif)).tolist()
    assert items == [TILE] * len(ndif), "a block no longer fills one tile"
    only_ours = (p.io >= 0) & (p.it < 0) & (p.ia < 0)
    assert (np.bincount(p.tile[only_ours], minlength=len(ndif)) == TILE).any(), "no tile of 384 ours-only additions"
    c = O.classify3(*case.flat())[0]
    c = c[(c[:, 1] != C.NONE) & (c[:, 2] != C.NONE)]
    per_tile = np.bincount(p.tile[np.searchsorted(p.key, case.k[1][c[:, 1]])], minlength=len(ndif))
    pairs = np.bincount(p.tile[p.matched], minlength=len(ndif))
    assert ((per_tile == 192) & (pairs == 192)).any(), "no tile whose every matched pair conflicts"


def test_reach_seam3():
    """seam 3: every pair on items (2i + 1, 2i + 2) with the lookahead entry present; the ragged ends both ways
    round; an empty and a one-entry side in each role"""
    cases = seam3()
    for name in ("insert_first", "delete_first"):
        p = C.paths(cases[name])
        pos = np.searchsorted(cases[name].k[1], p.key) + np.searchsorted(cases[name].k[2], p.key)
        assert p.matched[1:].all() and not p.matched[0] and (pos[1:] % 2 == 1).all(), \
            "the cases no longer put every pair on items (2i + 1, 2i + 2)"
        assert {1, 127, 383} <= set((pos[p.matched] % TILE).tolist()), "no pair straddles the thread, wave and tile boundary"
        g = C.geometry(*cases[name].k)
        assert g.nt == 4 and (g.j1[:-1] < cases[name].k[2].size).all()  # the lookahead entry exists
    rems = {}
    for name, case in cases.items():
        if name.startswith("rem"):
            rems.setdefault((case.k[1].size + case.k[2].size) % TILE, set()).add(case.k[1].size > case.k[2].size)
    assert rems == {r: {True, False} for r in (1, 2, 3, 191, 193, 383)}, "the cases no longer reach the ragged ends"
    sizes = {name: tuple(k.size for k in case.k) for name, case in cases.items()}
    for role, name in enumerate(("anc", "ours", "theirs")):
        assert sizes[name + "_0"][role] == 0 and sizes[name + "_1"][role] == 1
        assert min(sizes[name + "_0"][:role] + sizes[name + "_0"][role + 1:]) > TILE
    assert sizes["anc_only"][1:] == (0, 0)


def test_reach_seam4():
    """seam 4: the true ancestor position lies more than 4 probes from k_apart3b's guess in both directions for
    some tile and within them for another; nK < 256; nO = 0"""
    cases = seam4()
    low = high = near = False
    for name, case in cases.items():
        g = C.geometry(*case.k)
        off = (g.apart - g.guess)[1:-1]
        low |= bool((off > C.APART_STEP * 4).any())
        high |= bool((off < -C.APART_STEP * 4).any())
        near |= bool((np.abs(off) <= C.APART_STEP * 4).any())
    assert low and high and near, "the cases no longer reach a guess that misses its bracket on either side"
    for name in ("below", "above", "middle"):
        assert cases[name].k[0].size == 6000 and all(600 < k.size < 800 for k in cases[name].k[1:])
    gs, gb = C.geometry(*cases["below"].k), C.geometry(*cases["above"].k)
    assert ((gs.apart - gs.guess)[1:-1] > C.APART_STEP * 4).any() and ((gb.apart - gb.guess)[1:-1] < -C.APART_STEP * 4).any()
    assert 0 < cases["small_k"].k[0].size < C.APART_STEP and C.geometry(*cases["small_k"].k).nt > 2
    assert cases["ours_empty"].k[1].size == 0 and C.geometry(*cases["ours_empty"].k).nt > 2


def test_reach_seam5():
    """seam 5: staged name chunks within 2 of the cap on both sides, for tiles of pairs and of ours-only rows, in
    sorted form and through walk orders; every length at every offset mod 4 at each compare site"""
    for perm in (False, True):
        case = seam5_cap(perm)
        g = C.case_geometry(case, perm, [np.arange(k.size) for k in case.k])
        ch = g.ch[:8].tolist()
        for tiles in (ch[:4], ch[4:]):  # matched pairs; ours-only rows
            assert {NAME_CH - 1, NAME_CH} & set(tiles) and {NAME_CH + 1, NAME_CH + 2} & set(tiles), \
                "the cases no longer reach the name cap from both sides"
        assert g.lnames[:8].any() and not g.lnames[:8].all()
        rows = (g.rA1 - g.rA0 + g.rB1 - g.rB0)[1:3].tolist()
        assert rows == [385 + (4 * HALO if perm else 0)] * 2
    case = seam5_mixed()
    p, sites = _sites(case)
    offs = case.offs()
    ln = [np.diff(o) for o in offs]
    idx = [p.ia, p.io, p.it]
    for name, (mask, second, first) in sites.items():
        for s in (first, second):
            x = idx[s][mask]
            got = set(zip(ln[s][x].tolist(), (offs[s][x] % 4).tolist()))
            assert got >= {(L, a) for L in LENS for a in range(4)}, "the cases no longer reach every length at every offset: " + name
    g = C.case_geometry(case)
    assert g.lnames.any() and not g.lnames.all()


def test_reach_seam6():
    """seam 6: some matched pair's and some differing path's walk row is exactly one before, the first of, the
    last of and one after the staged rows, on ours and on theirs"""
    case, orders = seam6()
    seen, moved = set(), set()
    for order in orders[:-1]:
        seen |= _halo_hits(case, order)
        moved |= {int(d) for o in order for d in np.abs(o - np.arange(o.size)).tolist()}
    assert {0} | {L - 1 for L in C.SEGMENTS} <= moved <= {0} | {L - 1 - 2 * x for L in C.SEGMENTS for x in range(L)}, \
        "the orders no longer displace rows by 7, 8, 9, 16 and 63"
    assert seen == HALO_ALL, "the cases no longer reach the rows around the staged names: %s" % sorted(HALO_ALL - seen)
    g = C.case_geometry(case, True, orders[0])
    assert g.nt >= 6 and g.lnames.all() and g.lk.all()


@pytest.mark.parametrize("site", list(SITES))
def test_reach_seam7(site):
    """seam 7: the victim is a path of its site in tile 1; its tile stages its names (lds), is over the cap (cap),
    or stages them with the compared row one row outside the halo (perm)"""
    for route in ROUTES:
        for L in COLL_LENS:
            case, orders, s, x = collision_case(site, route, L)
            perm = orders is not None
            g = C.case_geometry(case, perm, orders)
            p, sites = _sites(case)
            u = int(np.searchsorted(p.key, case.key[VICTIM]))
            assert sites[site][0][u] and p.tile[u] == 1 and len(case.names[s][x]) == L, "the victim is no longer at its site"
            if route == "cap":
                assert not g.lnames[1], "the cases no longer push the victim's tile over the name cap"
                continue
            assert g.lnames[1], "the victim's tile no longer stages its names"
            if perm:
                moved = 1 if site == "anc_ours" else 2
                row = int(orders[moved][[0, p.io[u], p.it[u]][moved]])
                r0 = int((g.rA0, g.rB0)[moved - 1][1])
                assert row == r0 - 1 == VICTIM - HALO - 1, "the victim's row is no longer just outside the halo"
    assert [len(corruptions(bytes(L))) for L in COLL_LENS] == [3, 4, 5, 5, 6, 6, 5, 6]  # impossible and repeated ones skipped


def test_reach_seam8():
    """seam 8: the ancestor positions lie where their names say in the valid input's geometry; tile 1 opens with
    entry 192 of ours and of theirs whatever the broken pair"""
    g, pos = seam8_anc_positions()
    case = seam8_anc()
    kK, first, last = case.k[0], min(case.k[1][0], case.k[2][0]), max(case.k[1][-1], case.k[2][-1])
    assert g.nt == 4 and pos["first"] == 1 and pos["last"] == kK.size - 1
    assert kK[pos["before_all"]] < first and kK[pos["beyond_all"] - 1] > last
    assert pos["seam"] in g.apart[1:-1].tolist() and 0 < pos["seam"] < kK.size, "the cases no longer reach a tile's ancestor seam"
    t = int(np.argmax(g.nk))
    assert g.nk[t] > ACAP and g.k0[t] < pos["over_acap"] - 1 and pos["over_acap"] < g.k1[t], \
        "the cases no longer reach an ancestor range read from HBM"
    assert g.lk[1] and g.k0[1] < pos["staged"] - 1 and pos["staged"] < g.k1[1]
    for in_theirs in (False, True):
        for x in SIDE_PAIRS:
            ka, kb = _broken_sides(x, "equal", in_theirs)
            i, monotone = C.split_by_definition(ka, kb, TILE)
            assert monotone and (i, TILE - i) == (192, 192), "tile 1 no longer opens with entry 192 of either side"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_python(name):
    """the oracle against the pure-Python classify3 on every crafted input: conflicts and merge
    deltas in path order, and the clean count"""
    case = case_of(name)
    oc, om, ocl = oracle_of(name)
    pc, pm, pcl = C.classify3(*case.flat())
    assert np.array_equal(oc.reshape(-1, 3), pc) and np.array_equal(om.reshape(-1, 2), pm) and ocl == pcl


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _options(engine, request, **opts):  # (as test_gpu_place2_updates._options: set, and restored at teardown)
    old = {k: engine.get_option(k) for k in opts}
    request.addfinalizer(lambda: [engine.set_option(k, v) for k, v in old.items()])
    for k, v in opts.items():
        engine.set_option(k, v)


def _same(r, want):
    oc, om, ocl = want
    assert np.array_equal(np.asarray(r.conflict).reshape(-1, 3), oc.reshape(-1, 3))
    assert np.array_equal(np.asarray(r.mdelta).reshape(-1, 2), om.reshape(-1, 2))
    assert r.n_clean == ocl


FULL_MATRIX = {(h, f, j) for h in (False, True) for f in ("sorted", "identity", "displaced") for j in (1, 0)}


KEYS = pytest.mark.parametrize("hashed", [False, True], ids=["int", "hash"])


def _matrix(engine, request, case, want, hashed, displaced=None):
    """engine.merge3 against the oracle with int or hash keys: sorted form | walk orders (identity,
    and the displaced orders) x merge3_join 1 | 0 (with both key modes: k_join3b's four
    instantiations, each against the two-step path); -> the combinations that ran"""
    ran = set()
    displaced = displaced or [[C.default_displaced(k.size, s) for s, k in enumerate(case.k)]]
    sides = case.sides(hashed)
    forms = [("sorted", sides), ("identity", [C.perm_side(engine, s, np.arange(s.n)) for s in sides])]
    forms += [("displaced", [C.perm_side(engine, s, o) for s, o in zip(sides, order)]) for order in displaced]
    for form, ss in forms:
        assert all(s.walk_rows for s in ss) == (form != "sorted")
        for join in (1, 0):
            _options(engine, request, merge3_join=join)
            assert engine.get_option("merge3_join") == join
            _same(engine.merge3(*ss), want)
            ran.add((hashed, form, join))
    assert ran == {c for c in FULL_MATRIX if c[0] == hashed}
    return ran


@gpu
@KEYS
def test_gpu_seam1_ancestor_search_every_width(engine, request, hashed):
    """seam 1: every lower-bound position of every ancestor range width 0..329 (LDS up to 320 keys,
    HBM beyond), over 330 tiles: the placement across the 64-tile groups"""
    _matrix(engine, request, seam1(), oracle_of("seam1"), hashed)


@gpu
@KEYS
def test_gpu_seam2_compaction_passes_and_clean_count(engine, request, hashed):
    """seam 2: tiles of 0, 1, 191, 192, 193, 383 and 384 differing paths; the clean count's ballot slices"""
    _matrix(engine, request, seam2(), oracle_of("seam2"), hashed)


@gpu
@KEYS
@pytest.mark.parametrize("name", SEAM3)
def test_gpu_seam3_straddles_and_ragged_ends(engine, request, name, hashed):
    """seam 3: pairs across the thread, wave and 384-item tile boundary; ragged last tiles; empty and
    one-entry sides in each role"""
    _matrix(engine, request, seam3()[name], oracle_of("seam3_" + name), hashed)


@gpu
@KEYS
@pytest.mark.parametrize("name", SEAM4)
def test_gpu_seam4_apart_guess(engine, request, name, hashed):
    """seam 4: k_apart3b's proportional guess too low, too high and near; nK < 256; nO = 0"""
    _matrix(engine, request, seam4()[name], oracle_of("seam4_" + name), hashed)


@gpu
@KEYS
@pytest.mark.parametrize("name", ["cap_sorted", "cap_perm", "mixed"])
def test_gpu_seam5_name_staging_cap(engine, request, name, hashed):
    """seam 5: tiles whose staged name chunks are 999, 1000, 1001 and 1002; names of every length in
    LENS at every offset mod 4, staged and over the cap"""
    _matrix(engine, request, case_of("seam5_" + name), oracle_of("seam5_" + name), hashed)


@gpu
@KEYS
def test_gpu_seam6_walk_rows_around_the_halo(engine, request, hashed):
    """seam 6: walk rows just inside and just outside the staged name rows, on ours and on theirs,
    for matched pairs and differing paths; displaced ancestor rows; one random permutation"""
    case, orders = seam6()
    _matrix(engine, request, case, oracle_of("seam6"), hashed, displaced=orders)


ROUTE = pytest.mark.parametrize("route", ROUTES)


def _collisions(engine, request, site, route):
    _options(engine, request, merge3_join=1)
    n = 0
    for L in COLL_LENS:
        case, orders, s, x = collision_case(site, route, L)
        build = lambda: [C.perm_side(engine, sd, o) for sd, o in zip(case.sides(True), orders)] if orders else case.sides(True)
        _same(engine.merge3(*build()), O.classify3(*case.flat()))  # the control
        good = case.names[s][x]
        for how, bad in corruptions(good).items():
            case.names[s][x] = bad
            with pytest.raises(N.Unsupported) as e:
                engine.merge3(*build())
            assert "hash key collision" in str(e.value), (route, L, how, str(e.value))  # (not the order bit)
            n += 1
        case.names[s][x] = good
    assert n == sum(len(corruptions(bytes(L))) for L in COLL_LENS) == 40
    _same(engine.merge3(*build()), O.classify3(*case.flat()))  # (the flag is consumed)


@gpu
@ROUTE
def test_gpu_seam7_collision_ours_theirs(engine, request, route):
    """seam 7, ours vs theirs on a matched pair: one corrupted byte or length is a collision, by the
    LDS compare, over the cap and for a walk row outside the halo"""
    _collisions(engine, request, "ours_theirs", route)


@gpu
@ROUTE
def test_gpu_seam7_collision_ancestor_ours(engine, request, route):
    """seam 7, the ancestor vs ours on a path ours modified, the ancestor's name alone corrupted"""
    _collisions(engine, request, "anc_ours", route)


@gpu
@ROUTE
def test_gpu_seam7_collision_ancestor_theirs(engine, request, route):
    """seam 7, the ancestor vs theirs where ours is absent"""
    _collisions(engine, request, "anc_theirs", route)


SIDE_PAIRS = (41, 192, 384, 1499)  # x of the broken pair x - 1 | x of ours / theirs


def _broken_sides(x, kind, in_theirs, n=1500):
    """test_gpu_walk_rejects_unsorted's layout for the 384-item tile: the other side holds 192 keys
    below and the rest above all of the faulty side's, so tile 0 is those 192 and the faulty side's
    first 192 whatever its pair 191 | 192 looks like"""
    other = np.concatenate([1 + np.arange(192), (1 << 40) + np.arange(n - 192)]).astype(np.uint64)
    bad = (1 << 20) + 10 * np.arange(n, dtype=np.uint64)
    bad[x] = bad[x - 1] - np.uint64(0 if kind == "equal" else 1)
    return (other, bad) if in_theirs else (bad, other)


def _rejected(engine, request, sides, valid, want):
    for join in (1, 0):
        _options(engine, request, merge3_join=join)
        with pytest.raises(N.Unsupported) as e:
            engine.merge3(*sides)
        assert "ascending" in str(e.value), str(e.value)
        _same(engine.merge3(*valid), want)  # the flag is consumed


@gpu
@pytest.mark.parametrize("kind", ["equal", "descending"])
def test_gpu_seam8_ancestor_order(engine, request, kind):
    """seam 8, the ancestor: an equal / a descending pair at 0 | 1, before every ours/theirs key, inside
    a staged range, at a tile's apart seam, inside a range over 320 keys, beyond every ours/theirs key
    and at nK - 2 | nK - 1 is rejected by both merge paths"""
    case = seam8_anc()
    valid, want = case.sides(False), oracle_of("seam8_anc")
    for x in seam8_anc_positions()[1].values():
        k = case.k[0].copy()
        k[x] = k[x - 1] - np.uint64(0 if kind == "equal" else 1)
        _rejected(engine, request, [C.int_side(k, case.oid[0])] + valid[1:], valid, want)


@gpu
@pytest.mark.parametrize("kind", ["equal", "descending"])
@pytest.mark.parametrize("in_theirs", [False, True], ids=["ours", "theirs"])
def test_gpu_seam8_side_order(engine, request, kind, in_theirs):
    """seam 8, ours and theirs: the pairs 40 | 41, 191 | 192 (tile 1's first entry against its
    lookbehind key), 383 | 384 and the last are rejected by both merge paths"""
    n = 1500
    good = (1 << 20) + 10 * np.arange(n, dtype=np.uint64)
    zero = np.zeros((n, 20), np.uint8)
    valid = [C.int_side(good, zero) for _ in range(3)]
    want = O.classify3(good, zero, good, zero, good, zero)
    for x in SIDE_PAIRS:
        ko, kt = _broken_sides(x, kind, in_theirs, n)
        sides = [valid[0], C.int_side(ko, zero), C.int_side(kt, zero)]
        _rejected(engine, request, sides, valid, want)
        if x == 192:  # and read through (identity) walk orders
            _rejected(engine, request, [C.perm_side(engine, s, np.arange(s.n)) for s in sides], valid, want)


@gpu
@pytest.mark.parametrize("hashed", [False, True], ids=["int", "hash"])
def test_gpu_device_resident_writes_nothing_beyond_counts(engine, request, hashed):
    """kd_merge3_device and kd_merge3_device_perm on canary-filled outputs: the lists equal the
    oracle's and no word past 3 * n_conflict / 2 * n_mdelta changed (seam 2's tiles)"""
    from kart_amd.device import DevBuf, DevSide

    case, want = seam2(), oracle_of("seam2")
    _options(engine, request, merge3_join=1)
    L, ctx = engine.L, engine.ctx
    n = sum(k.size for k in case.k)
    for perm in (False, True):
        conf, md, c = DevBuf(engine, 12 * (n + 1)), DevBuf(engine, 8 * (n + 1)), DevBuf(engine, 64)
        for b in (conf, md):
            N.check(L.kd_memset(ctx, b.ptr, CANARY, b.nbytes), "kd_memset")
        c.zero()
        if perm:
            ps = [C.perm_side(engine, s, C.default_displaced(s.n, x)) for x, s in enumerate(case.sides(hashed))]
            ks = [s.dperm.kd_side() for s in ps]
            N.check(L.kd_merge3_device_perm(ctx, *(ctypes.byref(k) for k in ks), *(s.dperm.order.ptr for s in ps), 0,
                                            conf.ptr, md.ptr, c.ptr, c.ptr + 32), "kd_merge3_device_perm")
        else:
            ds = [DevSide(engine, s) for s in case.sides(hashed)]
            ks = [d.kd_side() for d in ds]
            N.check(L.kd_merge3_device(ctx, *(ctypes.byref(k) for k in ks), 0, conf.ptr, md.ptr, c.ptr, c.ptr + 32),
                    "kd_merge3_device")
        engine.sync()
        cnt = c.download(np.uint64, 5)
        assert int(cnt[4]) & 0xFFFFFFFF == 0
        nc, nm = int(cnt[1]), int(cnt[2])
        rc, rm = conf.download(np.uint8, conf.nbytes), md.download(np.uint8, md.nbytes)
        assert np.array_equal(rc[:12 * nc].view(np.uint32).reshape(nc, 3), want[0].reshape(-1, 3))
        assert np.array_equal(rm[:8 * nm].view(np.uint32).reshape(nm, 2), want[1].reshape(-1, 2)) and int(cnt[0]) == want[2]
        assert (rc[12 * nc:] == CANARY).all() and (rm[8 * nm:] == CANARY).all(), "written beyond the counts"
