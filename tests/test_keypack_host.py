"""kd_keypack.h on the CPU under AddressSanitizer and UBSan: the decoder the host packer and the device
kernel share, entry by entry (no GPU).

One stand-alone program (tests/keypack_host_check.cpp) is built with the sanitizers and run once over the
corpus of keypack_craft.py: the reference's int, hash and legacy path KATs, the 64 names of each of the
eight block classes, the pk extremes, every refusal the format rules name, each valid name cut at every
byte and 2,000 seeded mutations per structure.  Each entry sits in a heap block of exactly its length.
The expected keys and statuses come from base64 + msgpack + walkkey.py (keypack_craft.ref); the mutations
must equal kd_pack_int_keys / kd_pack_hash_keys on the same bytes, and so must everything else.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import keypack_craft as K
from kart_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"int": K.INT, "hash64": K.HASH64, "hashhex": K.HASHHEX}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("keypack_host")
    exe = str(tmp / "keypack_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kart_amd", "csrc"),
                    os.path.join(ROOT, "tests", "keypack_host_check.cpp"), "-o", exe], check=True)
    groups = {name: (K.group(cfg), K.mutations(cfg)) for name, cfg in CFGS.items()}
    corpus, out = str(tmp / "corpus.bin"), str(tmp / "out.bin")
    total = 0
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", sum(len(g) + len(m) for g, m in groups.values())))
        for name, (g, m) in groups.items():
            mode, levels, hex_ = CFGS[name]
            for e in [x[0] for x in g] + m:
                f.write(struct.pack("<IiiI", mode, levels, hex_, len(e)) + e)
                total += 1
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True)
    assert r.returncode == 0, f"keypack_host_check failed ({r.returncode}):\n{r.stderr[-4000:]}"
    raw = np.fromfile(out, np.uint8).reshape(total, 9)
    keys, status = raw[:, :8].copy().view(np.uint64).reshape(-1), raw[:, 8]
    res, at = {}, 0
    for name, (g, m) in groups.items():
        n = len(g) + len(m)
        res[name] = (g, m, keys[at:at + n], status[at:at + n])
        at += n
    return res


@pytest.mark.parametrize("name", list(CFGS))
def test_crafted_entries_give_the_reference_s_keys(results, name):
    g, _, keys, status = results[name]
    for j, (e, k, s) in enumerate(g):
        assert (int(keys[j]), int(status[j])) == (k, s), f"{name} item {j} {e!r}: key {int(keys[j]):#x} status {status[j]}, expected {k:#x} / {s}"
    assert {s for _, _, s in g} == ({0, 1, 2} if name == "int" else {0, 1})


def test_every_named_refusal(results):
    g = {e: (k, s) for e, k, s in results["int"][0]}
    for rule, e, st in K.int_refused():
        assert g[e] == (0, st), rule
    assert {st for _, _, st in K.int_refused()} == {1, 2}
    for name in ("hash64", "hashhex"):
        g = {e: (k, s) for e, k, s in results[name][0]}
        rules = K.hash_refused(CFGS[name])
        assert all(g[e] == (0, 1) for _, e, _ in rules)
        assert {"missing slash", "short path"} <= {r for r, _, _ in rules}
    assert "uppercase hex" in {r for r, _, _ in K.hash_refused(K.HASHHEX)}


def test_valid_names_cover_the_classes_and_extremes(results):
    from kart_amd import walkkey

    pks = {pk for _, pk in K.int_valid()}
    assert all(s + j in pks for s in walkkey.CLASS_BLOCK for j in range(64))
    assert {-(1 << 63), (1 << 63) - 1, 1 << 30, -(1 << 30)} <= pks and set(range(-64, 0)) <= pks
    ok = {e: k for e, k, s in results["int"][0] if s == 0}
    back = walkkey.int_keys_to_pks(np.array([ok[e] for e, _ in K.int_valid()], np.uint64))
    assert back.tolist() == [pk for _, pk in K.int_valid()]


@pytest.mark.parametrize("name", list(CFGS))
def test_program_equals_the_host_packer(results, name):
    """the crafted entries and the 2,000 mutations: the same keys and statuses as kd_pack_int_keys /
    kd_pack_hash_keys on the same bytes"""
    g, m, keys, status = results[name]
    assert len(m) == 2000
    hk, hs = K.host_pack([x[0] for x in g] + m, CFGS[name])
    assert np.array_equal(keys, hk) and np.array_equal(status, hs)
    ms = status[len(g):]
    assert 0 < np.count_nonzero(ms) < 2000  # (the mutations reach both outcomes)
    for e, k, s in zip(m, keys[len(g):], ms):  # ... and the reference agrees on them too
        assert K.ref(e, CFGS[name]) == (int(k), int(s)), e


def test_header_has_one_decoder():
    """the host packer calls the shared header: no second copy of the decoder in kd_ctx.hip"""
    text = open(os.path.join(ROOT, "kart_amd", "csrc", "kd_ctx.hip")).read()
    assert "kp::int_entry" in text and "kp::hash_entry" in text
    assert "decode_int_name" not in text and "fnv1a64" not in text and "b64v" not in text
    assert N.KD_KEY_INT == 0 and N.KD_KEY_HASH == 1
