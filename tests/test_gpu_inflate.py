"""kd_inflate_batch on the GPU against Python's zlib: block kinds, lengths, distances, the seams of
the one-lane-per-stream launch, alignment, raw items, invalid streams and determinism.

The streams come from tests/inflate_craft.py; the invalid ones (and every valid one) have already run
through the same decoder under the sanitizers on the CPU (tests/test_inflate_host.py).  Expected bytes
are zlib's.  The host form (Engine.inflate) is used where only results matter; the device form, with a
prefilled arena and 64 sentinel bytes behind it, where what is NOT written matters.
"""
import ctypes
import zlib

import numpy as np
import pytest

import inflate_craft as C
from kart_amd import _native as N
from kart_amd.device import DevBuf

pytestmark = pytest.mark.gpu

FILL = 0xEE
SENTINEL = bytes(range(101, 165))


@pytest.fixture(scope="module")
def valid():
    cases = C.all_valid()
    for name, stream, want in cases:
        assert zlib.decompress(stream) == want, name
    return cases


@pytest.fixture(scope="module")
def small(valid):
    return [(s, w) for _, s, w in valid if len(s) < 600 and len(w) < 2000]


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


def run_host(engine, items):
    """items [(src bytes, dst_len, kind)] -> ([bytes per item], status)"""
    src = np.frombuffer(b"".join(s for s, _, _ in items), np.uint8)
    so, do = _offsets([len(s) for s, _, _ in items]), _offsets([d for _, d, _ in items])
    kind = np.asarray([k for _, _, k in items], np.uint8)
    data, status = engine.inflate(src, so, do, kind if kind.any() else None)
    raw = data.tobytes()
    return [raw[int(do[i]):int(do[i + 1])] for i in range(len(items))], status


def run_device(engine, items, src_pre=0, dst_pre=0):
    """the device form: sources at byte src_pre of their buffer (8 bytes of padding behind them), the
    arena at byte dst_pre of a buffer prefilled with FILL and followed by SENTINEL.
    -> ([bytes per item], status, bytes before the arena, bytes behind it)"""
    n = len(items)
    blob = b"\x55" * src_pre + b"".join(s for s, _, _ in items) + b"\xA5" * 8
    so, do = _offsets([len(s) for s, _, _ in items]), _offsets([d for _, d, _ in items])
    total = int(do[-1])
    d_src = DevBuf.from_numpy(engine, np.frombuffer(blob, np.uint8))
    d_so, d_do = DevBuf.from_numpy(engine, so), DevBuf.from_numpy(engine, do)
    d_kind = DevBuf.from_numpy(engine, np.asarray([k for _, _, k in items], np.uint8))
    d_dst = DevBuf.from_numpy(engine, np.frombuffer(bytes([FILL]) * (dst_pre + total) + SENTINEL, np.uint8))
    d_st = DevBuf.from_numpy(engine, np.full(n, 0xFF, np.uint8))
    N.check(engine.L.kd_inflate_batch(engine.ctx, d_src.ptr + src_pre, d_so.ptr, d_kind.ptr, n, d_dst.ptr + dst_pre,
                                      d_do.ptr, d_st.ptr, N.KD_MEM_DEVICE), "kd_inflate_batch")
    engine.sync()
    raw = d_dst.download(np.uint8, dst_pre + total + 64).tobytes()
    status = d_st.download(np.uint8, n)
    arena = raw[dst_pre:dst_pre + total]
    return [arena[int(do[i]):int(do[i + 1])] for i in range(n)], status, raw[:dst_pre], raw[dst_pre + total:]


def test_block_kinds_lengths_distances(engine, valid):
    """every zlib-made and every crafted valid stream, one batch"""
    out, status = run_host(engine, [(s, len(w), 0) for _, s, w in valid])
    for (name, _, want), got, st in zip(valid, out, status):
        assert st == 0, f"{name}: status {st}"
        assert got == want, name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(engine, small, n):
    items = [small[(7 * k) % len(small)] for k in range(n)]
    out, status = run_host(engine, [(s, len(w), 0) for s, w in items])
    assert not status.any()
    assert out == [w for _, w in items]


def test_one_long_stream_among_tiny_ones(engine, small):
    rng = np.random.default_rng(5)
    long = (rng.integers(0, 256, 3000, dtype=np.uint8).tobytes() + b"field value, field value; " * 400) * 16
    long = long[:200 << 10]
    items = [small[k % len(small)] for k in range(63)]
    items.insert(17, (zlib.compress(long, 6), long))
    out, status = run_host(engine, [(s, len(w), 0) for s, w in items])
    assert not status.any()
    assert out == [w for _, w in items]


@pytest.mark.parametrize("where", ["first", "last", "all", "partial_last"])
def test_empty_streams(engine, small, where):
    empty = (zlib.compress(b""), b"")
    n = 70 if where == "partial_last" else 64
    items = [small[(3 * k) % len(small)] for k in range(n)]
    for k in {"first": [0], "last": [63], "all": range(64), "partial_last": [69]}[where]:
        items[k] = empty
    if where == "partial_last":
        items[68] = small[0]
    out, status, _, behind = run_device(engine, [(s, len(w), 0) for s, w in items])
    assert not status.any()
    assert out == [w for _, w in items]
    assert behind == SENTINEL


def test_alignment_of_sources_and_destinations(engine, small):
    """a stream at every (source offset mod 8, destination offset mod 8): fillers shift the two apart —
    a raw item moves both by its size, a 12-byte stream of one byte moves them by 12 and 1"""
    one = zlib.compress(b"x", 0)
    assert len(one) == 12
    items, probes = [], []
    at_s = at_d = 0
    for a in range(8):
        for b in range(8):
            j = (3 * (a - at_s % 8 - (b - at_d % 8))) % 8
            r = (b - at_d % 8 - j) % 8
            items += [(one, 1, 0)] * j + ([(bytes(range(r)), r, 1)] if r else [])
            at_s += 12 * j + r
            at_d += j + r
            assert at_s % 8 == a and at_d % 8 == b
            s, w = small[(a * 8 + b) % len(small)]
            probes.append((len(items), w))
            items.append((s, len(w), 0))
            at_s += len(s)
            at_d += len(w)
    for pre in (0, 3):
        out, status, before, behind = run_device(engine, items, src_pre=pre, dst_pre=(5 * pre) % 8)
        assert not status.any()
        for k, w in probes:
            assert out[k] == w
        assert before == bytes([FILL]) * len(before) and behind == SENTINEL


def test_raw_items_mixed_with_streams(engine, small):
    rng = np.random.default_rng(9)
    items, want = [], []
    for k in range(150):
        if k % 3 == 1:
            b = rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8).tobytes()
            items.append((b, len(b), 1))
            want.append(b)
        else:
            s, w = small[k % len(small)]
            items.append((s, len(w), 0))
            want.append(w)
    out, status = run_host(engine, items)
    assert not status.any()
    assert out == want
    # a raw item whose two ranges disagree is refused, not cut or padded
    out, status = run_host(engine, [(b"abcd", 3, 1), (b"abcd", 5, 1), (b"abcd", 4, 1)])
    assert status.tolist() == [N.KD_INF_EOVER, N.KD_INF_ESRC, 0] and out[2] == b"abcd"


@pytest.mark.parametrize("case", C.crafted_invalid(), ids=lambda c: f"{c[3]}_{c[0]}")
def test_invalid_stream_in_a_wave_of_valid_ones(engine, small, case):
    name, stream, dst_len, code = case
    assert C.zlib_verdict(stream, dst_len) is None
    items = [small[(5 * k) % len(small)] for k in range(64)]
    batch = [(s, len(w), 0) for s, w in items]
    batch[31] = (stream, dst_len, 0)
    out, status, _, behind = run_device(engine, batch)
    assert status[31] == code, f"{name}: status {status[31]}"
    assert not np.delete(status, 31).any()
    for k, (_, w) in enumerate(items):
        if k != 31:
            assert out[k] == w, f"neighbour {k} of {name}"
    assert behind == SENTINEL


def test_same_batch_twice_gives_equal_outputs(engine, valid):
    batch = [(s, len(w), 0) for _, s, w in valid] + [(s, d, 0) for _, s, d, _ in C.crafted_invalid()]
    a, sa = run_host(engine, batch)
    b, sb = run_host(engine, batch)
    assert np.array_equal(sa, sb)
    ok = [k for k in range(len(batch)) if sa[k] == 0]
    assert len(ok) == len(valid) and [a[k] for k in ok] == [b[k] for k in ok]


def test_host_offsets_are_checked(engine):
    s = np.frombuffer(zlib.compress(b"abc"), np.uint8)
    good = np.array([0, s.size], np.uint64)
    for so, do in ((np.array([s.size, 0], np.uint64), np.array([0, 3], np.uint64)),
                   (good, np.array([3, 0], np.uint64))):
        with pytest.raises(N.KdError):
            engine.inflate(s, so, do)
    data, status = engine.inflate(s, good, np.array([0, 3], np.uint64))
    assert status.tolist() == [0] and data.tobytes() == b"abc"
    data, status = engine.inflate(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    assert data.size == 0 and status.size == 0
