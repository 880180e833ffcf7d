"""kd_delta.h on the CPU under AddressSanitizer and UBSan: the decoder's bounds rules and its agreement
with a plain-Python applier, item by item (no GPU) — and that applier's agreement with git.

One stand-alone program (tests/delta_host_check.cpp) is built with the sanitizers and run once over a
corpus: every valid delta the GPU test uses, the crafted invalid ones, and 2,000 mutations (single bit
flips and truncations, fixed seed).  Base, delta and dst of each item sit in heap blocks of exactly
their lengths, so any access outside them ends the program.  tests/delta_craft.py's applier decides what
is right; git decides whether the applier is: a hand-made pack of crafted OFS_DELTA entries goes
through ``git index-pack`` and ``git cat-file --batch``.
"""
import os
import struct
import subprocess

import pytest

import delta_craft as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("delta_host")
    exe = str(tmp / "delta_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kart_amd", "csrc"),
                    os.path.join(ROOT, "tests", "delta_host_check.cpp"), "-o", exe], check=True)
    valid = C.all_valid()
    invalid = C.crafted_invalid()
    items = [(b, d, len(r)) for _, b, d, r in valid] + [(b, d, dl) for _, b, d, dl, _ in invalid] + C.mutations()
    corpus, out = str(tmp / "corpus.bin"), str(tmp / "out.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for b, d, dl in items:
            f.write(struct.pack("<III", len(b), len(d), dl))
            f.write(b)
            f.write(d)
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True)
    assert r.returncode == 0, f"delta_host_check failed ({r.returncode}):\n{r.stderr[-4000:]}"
    raw = open(out, "rb").read()
    got, at = [], 0
    for _, _, dl in items:
        st = raw[at]
        at += 1
        data = None
        if st == 0:
            data = raw[at:at + dl]
            at += dl
        got.append((st, data))
    assert at == len(raw)
    return valid, invalid, items, got


def test_valid_deltas_apply(results):
    valid, _, _, got = results
    for (name, base, delta, want), (st, data) in zip(valid, got):
        assert st == 0, f"{name}: status {st}"
        assert data == want, name


def test_crafted_invalid_deltas_give_their_code(results):
    valid, invalid, _, got = results
    assert {code for *_, code in invalid} == set(range(1, 9))
    for (name, _, _, _, code), (st, _) in zip(invalid, got[len(valid):]):
        assert st == code, f"{name}: status {st}, expected {code}"


def test_mutations_agree_with_the_applier(results):
    valid, invalid, items, got = results
    k0 = len(valid) + len(invalid)
    n_ok = 0
    for k in range(k0, len(items)):
        base, delta, dl = items[k]
        st, data = got[k]
        want = C.apply(base, delta, dl)
        if isinstance(want, int):
            assert st == want, f"mutation {k - k0}: the applier says {want}, status {st}"
        else:
            n_ok += 1
            assert st == 0 and data == want, f"mutation {k - k0}: the applier accepts it, status {st}"
    assert len(items) - k0 == 2000 and 0 < n_ok < 2000


def _git_objects(gitdir, oids):
    req = b"".join(o.hex().encode() + b"\n" for o in oids)
    raw = subprocess.run(["git", "--git-dir", gitdir, "cat-file", "--batch"], input=req, check=True, capture_output=True).stdout
    out, at = [], 0
    for _ in oids:
        nl = raw.index(b"\n", at)
        _, kind, size = raw[at:nl].split()
        out.append((kind.decode(), raw[nl + 1:nl + 1 + int(size)]))
        at = nl + 2 + int(size)
    return out


def test_the_applier_is_what_git_does(tmp_path):
    """a base per crafted delta and the delta as an OFS_DELTA entry behind it: git indexes the pack and
    reads back what the applier computed"""
    gitdir = C.init_bare(str(tmp_path / "pin.git"))
    picked = [v for v in C.all_valid() if len(v[1]) <= 500 or v[0] in ("copy16@3", "copy257@15", "copy65536@1", "copy255@7")]
    entries, want, seen = [], [], set()
    for name, base, delta, res in picked:
        # (git takes no delta below 4 bytes — an empty result's is 2 or 3 — though the format has them)
        if base in seen or res in seen or len(delta) < 4:
            continue
        seen |= {base, res}
        entries.append({"kind": "blob", "content": base})
        entries.append({"kind": "ofs", "base": len(entries) - 1, "delta": delta})
        want += [("blob", base), ("blob", res)]
    assert len(entries) // 2 >= 12
    _, _, oids = C.write_pack(gitdir, entries, index="git")
    assert _git_objects(gitdir, oids) == want


@pytest.mark.parametrize("name", ["copy-past-base", "opcode-0", "copy-over", "short"])
def test_git_refuses_what_the_applier_refuses(tmp_path, name):
    gitdir = C.init_bare(str(tmp_path / "bad.git"))
    (base, delta), = [(b, d) for n, b, d, _, _ in C.crafted_invalid() if n == name]
    assert isinstance(C.apply(base, delta), int)
    body, _, _ = C.build_pack([{"kind": "blob", "content": base}, {"kind": "ofs", "base": 0, "delta": delta}])
    path = str(tmp_path / "bad.pack")
    with open(path, "wb") as f:
        f.write(body)
    r = subprocess.run(["git", "--git-dir", gitdir, "index-pack", path], capture_output=True)
    assert r.returncode != 0, "git indexed a pack whose delta the applier refuses"
    # ... and the same pack with a delta the applier accepts is indexed: the refusal is about the delta
    good, _ = C.encode(base, [("c", 0, 50)])
    body, _, _ = C.build_pack([{"kind": "blob", "content": base}, {"kind": "ofs", "base": 0, "delta": good}])
    with open(path, "wb") as f:
        f.write(body)
    subprocess.run(["git", "--git-dir", gitdir, "index-pack", path], check=True, capture_output=True)
