"""kd_treeparse.h on the CPU under AddressSanitizer and UBSan: the decoder's bounds rules and its
agreement with the Python reference, tree by tree (no GPU).

One stand-alone program (tests/treeparse_host_check.cpp) is built with the sanitizers and run once over
a corpus: every valid crafted tree, each of them cut at every byte position, every named invalid tree and
2,000 seeded mutations.  Each tree sits in a heap block of exactly its length, so any access outside it
ends the program.  tree_craft.parse decides what is right: the same status and the same entries, and
wherever the decoder says OK kart_amd.odb.parse_tree reads the same entries too (the device class is
never laxer than the host's parser).
"""
import os
import struct
import subprocess

import pytest

import tree_craft as C
from kart_amd import _native as N
from kart_amd import odb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("treeparse_host")
    exe = str(tmp / "treeparse_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kart_amd", "csrc"),
                    os.path.join(ROOT, "tests", "treeparse_host_check.cpp"), "-o", exe], check=True)
    return tmp, exe


@pytest.fixture(scope="module")
def results(program):
    tmp, exe = program
    valid = [t for _, t in C.valid_trees()]
    cut = C.truncations()
    invalid = [t for _, t, _ in C.crafted_invalid()]
    mut = C.mutations()
    items = valid + cut + invalid + mut
    corpus, out = str(tmp / "corpus.bin"), str(tmp / "out.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for t in items:
            f.write(struct.pack("<I", len(t)))
            f.write(t)
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True)
    assert r.returncode == 0, f"treeparse_host_check failed ({r.returncode}):\n{r.stderr[-4000:]}"
    raw = open(out, "rb").read()
    got, at = [], 0
    for t in items:
        st, n = struct.unpack_from("<BI", raw, at)
        at += 5
        ents = []
        for _ in range(n):
            mode, name, nlen, oid = struct.unpack_from("<IIII", raw, at)
            at += 16
            ents.append((mode, t[name:name + nlen], t[oid:oid + 20]))
        got.append((st, ents))
    big = raw[at]
    assert at + 1 == len(raw)
    bounds = (len(valid), len(valid) + len(cut), len(valid) + len(cut) + len(invalid), len(items))
    return items, got, bounds, big


def _check(items, got, lo, hi):
    n_ok = 0
    for k in range(lo, hi):
        want = C.parse(items[k])
        assert got[k] == want, f"item {k} ({items[k][:60]!r}...): {got[k][0]} / {len(got[k][1])} entries, expected {want[0]} / {len(want[1])}"
        if want[0] == C.OK:
            n_ok += 1
            try:
                host = odb.parse_tree(items[k])
            except UnicodeDecodeError:  # (parse_tree decodes names; the entries are compared where it can)
                continue
            assert [(m, nm.encode(), bytes.fromhex(o)) for m, _, o, nm in host] == want[1], f"item {k}: odb.parse_tree differs"
    return n_ok


def test_codes_are_the_header_s():
    assert (C.OK, C.EMODE, C.ENAME, C.EOID, C.ETREE, C.EORDER, C.EBIG, C.ECAP, C.ERANGE) == (
        N.KD_TJ_OK, N.KD_TJ_EMODE, N.KD_TJ_ENAME, N.KD_TJ_EOID, N.KD_TJ_ETREE, N.KD_TJ_EORDER, N.KD_TJ_EBIG, N.KD_TJ_ECAP,
        N.KD_TJ_ERANGE)
    assert C.MAX_BYTES == N.KD_TJ_MAX_BYTES and C.NONE == N.KD_NONE
    text = open(os.path.join(ROOT, "include", "kartdiff.h")).read()
    for name, code in list(C.CODES.items()) + [("ECAP", C.ECAP), ("ERANGE", C.ERANGE)]:
        assert f"#define KD_TJ_{name} {code}u" in text
    assert "#define KD_TJ_MAX_BYTES (1u << 30)" in text


def test_valid_trees_decode(results):
    items, got, (a, _, _, _), _ = results
    assert _check(items, got, 0, a) == a
    assert got[0] == (C.OK, [])  # the zero-length tree


def test_every_truncation(results):
    items, got, (a, b, _, _), _ = results
    n_ok = _check(items, got, a, b)
    # a prefix is valid exactly where it ends behind an entry
    assert n_ok == sum(len(C.parse(t)[1]) for _, t in C.valid_trees())


def test_crafted_invalid_trees_give_their_code(results):
    items, got, (_, b, c, _), big = results
    named = C.crafted_invalid()
    _check(items, got, b, c)
    for (name, _, code), (st, ents) in zip(named, got[b:c]):
        assert st == code and not ents, f"{name}: status {st}, expected {code}"
    assert big == C.EBIG
    assert {code for *_, code in named} | {big} == set(C.CODES.values())


def test_mutations_agree_with_the_reference(results):
    items, got, (_, _, c, d), _ = results
    n_ok = _check(items, got, c, d)
    assert d - c == 2000 and 0 < n_ok < 2000
    assert {got[k][0] for k in range(c, d)} >= {C.OK, C.EMODE, C.ENAME, C.EOID, C.EORDER}


def test_join_agrees_with_the_reference(program):
    """the K-way merge the kernels run (kd_tj::join) on the GPU test's task shapes and on refused trees:
    the same status and the same kept entries per root as the set-based reference, for every k and every
    pair of compared roots"""
    tmp, exe = program
    cases = []
    for k in (1, 2, 3):
        trees, tasks, _ = C.mixed(k)
        bad = [t for _, t, _ in C.crafted_invalid()]
        for cmp_ in C.compares(k):
            for task in tasks:
                cases.append((k, cmp_, [None if i == C.NONE else trees[i] for i in task]))
            for j, b in enumerate(bad):
                cases.append((k, cmp_, [b if r == j % k else trees[r] for r in range(k)]))
    corpus, out = str(tmp / "join.bin"), str(tmp / "join_out.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for k, cmp_, trees in cases:
            f.write(struct.pack("<Iii", k, *(cmp_ if cmp_ is not None else (-1, -1))))
            for t in trees:
                f.write(struct.pack("<II", t is not None, len(t or b"")) + (t or b""))
    r = subprocess.run([exe, "join", corpus, out], capture_output=True, text=True)
    assert r.returncode == 0, f"treeparse_host_check join failed ({r.returncode}):\n{r.stderr[-4000:]}"
    raw, at = open(out, "rb").read(), 0
    n_bad = 0
    for j, (k, cmp_, trees) in enumerate(cases):
        st, kept = C.join(trees, cmp_)
        assert raw[at] == st, f"case {j}: status {raw[at]}, expected {st}"
        at += 1
        if st:
            n_bad += 1
            continue
        for r in range(k):
            (n,) = struct.unpack_from("<I", raw, at)
            at += 4
            got = []
            for _ in range(n):
                mode, nlen = struct.unpack_from("<II", raw, at)
                got.append((raw[at + 8:at + 8 + nlen], mode, raw[at + 8 + nlen:at + 28 + nlen]))
                at += 28 + nlen
            assert got == kept[r], f"case {j} (k = {k}, compare {cmp_}) root {r}"
    assert at == len(raw) and n_bad == 11 * len(C.crafted_invalid())
