"""kd_inflate.h on the CPU under AddressSanitizer and UBSan: the decoder's bounds rules and its
agreement with zlib, stream by stream (no GPU).

One stand-alone program (tests/inflate_host_check.cpp) is built with the sanitizers and run once over a
corpus: every valid stream the GPU test uses, the crafted streams, and 2,000 mutations (single bit
flips and truncations, fixed seed).  Each stream sits in heap blocks of exactly the bytes the decoder
may touch, so any access outside them ends the program.  Python's zlib decides what is right: where it
reaches the end of the stream with exactly the expected length the status is 0 and the bytes are equal,
everywhere else the status is nonzero, and every crafted invalid stream gives its named code.
"""
import os
import struct
import subprocess

import pytest

import inflate_craft as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inflate_host")
    exe = str(tmp / "inflate_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kart_amd", "csrc"),
                    os.path.join(ROOT, "tests", "inflate_host_check.cpp"), "-o", exe], check=True)
    valid = C.all_valid()
    invalid = C.crafted_invalid()
    items = [(s, len(e)) for _, s, e in valid] + [(s, dl) for _, s, dl, _ in invalid] + C.mutations()
    corpus, out = str(tmp / "corpus.bin"), str(tmp / "out.bin")
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for s, dl in items:
            f.write(struct.pack("<II", len(s), dl))
            f.write(s)
    r = subprocess.run([exe, corpus, out], capture_output=True, text=True)
    assert r.returncode == 0, f"inflate_host_check failed ({r.returncode}):\n{r.stderr[-4000:]}"
    raw = open(out, "rb").read()
    got, at = [], 0
    for _, dl in items:
        st = raw[at]
        at += 1
        data = None
        if st == 0:
            data = raw[at:at + dl]
            at += dl
        got.append((st, data))
    assert at == len(raw)
    return valid, invalid, items, got


def test_valid_streams_decode(results):
    valid, _, _, got = results
    for (name, stream, want), (st, data) in zip(valid, got):
        assert C.zlib_verdict(stream, len(want)) == want, f"{name}: the crafted stream is not what zlib reads"
        assert st == 0, f"{name}: status {st}"
        assert data == want, name


def test_crafted_invalid_streams_give_their_code(results):
    valid, invalid, _, got = results
    assert {code for *_, code in invalid} == set(range(1, 11))
    for (name, stream, dl, code), (st, _) in zip(invalid, got[len(valid):]):
        assert C.zlib_verdict(stream, dl) is None, f"{name}: zlib accepts it"
        assert st == code, f"{name}: status {st}, expected {code}"


def test_mutations_agree_with_zlib(results):
    valid, invalid, items, got = results
    k0 = len(valid) + len(invalid)
    n_ok = 0
    for k in range(k0, len(items)):
        stream, dl = items[k]
        st, data = got[k]
        want = C.zlib_verdict(stream, dl)
        if want is None:
            assert st != 0, f"mutation {k - k0}: zlib refuses it, status 0"
        else:
            n_ok += 1
            assert st == 0 and data == want, f"mutation {k - k0}: zlib accepts it, status {st}"
    assert len(items) - k0 == 2000 and n_ok < 2000
