"""kd_delta_apply_batch on the GPU against a plain-Python applier: copy lengths around the 16-byte step
at every base and dst residue, inserts, long op streams, empty ranges, a far offset, shared bases, the
seams of the 16-lanes-per-item launch, invalid deltas and what is NOT written.

The deltas come from tests/delta_craft.py; every one of them has already run through the same decoder
under the sanitizers on the CPU (tests/test_delta_host.py).  The host form (Engine.apply_deltas) is used
where only results matter; the device form, with a prefilled arena, a guard range behind every item and
64 sentinel bytes behind the arena, where what is not written matters.
"""
import numpy as np
import pytest

import delta_craft as C
from kart_amd import _native as N
from kart_amd.device import DevBuf

pytestmark = pytest.mark.gpu

FILL = 0xEE
SENTINEL = bytes(range(101, 165))
GROUP, BLOCK = 4, 16  # items per wave and per workgroup of k_dl_apply (16 lanes per item, 256 per workgroup)


@pytest.fixture(scope="module")
def valid():
    return C.all_valid()


@pytest.fixture(scope="module")
def small(valid):
    return [v for v in valid if len(v[1]) < 4096]


def run_host(engine, bases, items):
    """items [(base index, delta, dst_len)] -> ([bytes per item], status)"""
    bo = C.offsets([len(b) for b in bases])
    do = C.offsets([len(d) for _, d, _ in items])
    po = C.offsets([dl for _, _, dl in items])
    data, status = engine.apply_deltas(np.frombuffer(b"".join(bases), np.uint8), bo, np.asarray([b for b, _, _ in items], np.uint32),
                                       np.frombuffer(b"".join(d for _, d, _ in items), np.uint8), do, po)
    raw = data.tobytes()
    return [raw[int(po[i]):int(po[i + 1])] for i in range(len(items))], status


def run_device(engine, bases, items, pre=(0, 0, 0)):
    """the device form: the three arenas at byte pre[k] of their buffers, dst prefilled with FILL and
    followed by SENTINEL.  -> ([bytes per item], status, bytes before the arena, bytes behind it)"""
    n = len(items)
    bp, dp, op = pre
    bo = C.offsets([len(b) for b in bases])
    do = C.offsets([len(d) for _, d, _ in items])
    po = C.offsets([dl for _, _, dl in items])
    total = int(po[-1])
    d_base = DevBuf.from_numpy(engine, np.frombuffer(b"\x55" * bp + b"".join(bases) + b"\x55" * 16, np.uint8))
    d_delta = DevBuf.from_numpy(engine, np.frombuffer(b"\x66" * dp + b"".join(d for _, d, _ in items) + b"\x66" * 16, np.uint8))
    d_bo, d_do, d_po = (DevBuf.from_numpy(engine, x) for x in (bo, do, po))
    d_idx = DevBuf.from_numpy(engine, np.asarray([b for b, _, _ in items], np.uint32))
    d_dst = DevBuf.from_numpy(engine, np.frombuffer(bytes([FILL]) * (op + total) + SENTINEL, np.uint8))
    d_st = DevBuf.from_numpy(engine, np.full(n, 0xFF, np.uint8))
    N.check(engine.L.kd_delta_apply_batch(engine.ctx, d_base.ptr + bp, d_bo.ptr, len(bases), d_idx.ptr, d_delta.ptr + dp, d_do.ptr, n,
                                          d_dst.ptr + op, d_po.ptr, d_st.ptr, N.KD_MEM_DEVICE), "kd_delta_apply_batch")
    engine.sync()
    raw = d_dst.download(np.uint8, op + total + 64).tobytes()
    status = d_st.download(np.uint8, n)
    arena = raw[op:op + total]
    return [arena[int(po[i]):int(po[i + 1])] for i in range(n)], status, raw[:op], raw[op + total:]


def test_every_valid_delta(engine, valid):
    """the whole corpus in one launch, a base per item: copies of 1, 15, 16, 17, 255, 256, 257 and 65,536
    bytes at every base and dst residue mod 16, inserts of 1 and 127, 300 one-byte ops, empty results, an
    empty base, every argument byte present, and an offset that needs its fourth byte"""
    names = {v[0] for v in valid}
    assert {"copy%d@%d" % (L, b) for L in (1, 15, 16, 17, 255, 256, 257, 0x10000) for b in range(16)} <= names
    assert {"insert1", "insert127", "ops300", "empty-result", "empty-both", "empty-base-inserts", "offset-4-bytes"} <= names
    got, status = run_host(engine, [b for _, b, _, _ in valid], [(k, d, len(r)) for k, (_, _, d, r) in enumerate(valid)])
    assert not status.any(), [valid[k][0] for k in np.flatnonzero(status)]
    for (name, _, _, want), g in zip(valid, got):
        assert g == want, name


@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, BLOCK - 1, BLOCK, BLOCK + 1, 1000])
def test_item_counts_around_the_wave_and_the_workgroup(engine, small, n):
    picks = [small[(7 * k) % len(small)] for k in range(n)]
    got, status, _, tail = run_device(engine, [b for _, b, _, _ in picks], [(k, d, len(r)) for k, (_, _, d, r) in enumerate(picks)])
    assert not status.any() and tail == SENTINEL
    assert got == [r for *_, r in picks]


def test_one_base_shared_by_70_items(engine):
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    other = rng.integers(0, 256, 100, dtype=np.uint8).tobytes()
    items, want = [], []
    for k in range(70):
        delta, res = C.encode(base, [("c", 13 * k, 100 + k), ("i", b"item %d" % k), ("c", 2999 - k, k + 1)])
        items.append((1, delta, len(res)))
        want.append(res)
    got, status = run_host(engine, [other, base], items)
    assert not status.any() and got == want


def test_invalid_items_between_valid_ones_write_nothing_outside(engine, small):
    """every crafted invalid item with valid neighbours, a guard range (an item that fails at once) behind
    every item: each code is the named one, the neighbours are right, the guards and the bytes around the
    arena are untouched"""
    invalid = C.crafted_invalid()
    bases, items, expect = [], [], []

    def add(base, delta, dst_len, want):
        bases.append(base)
        items.append((len(bases) - 1, delta, dst_len))
        expect.append(want)
        items.append((len(bases) - 1, C.header(len(base), 16) + b"\0", 16))  # the guard: opcode 0
        expect.append(C.EOP)

    for k, (name, base, delta, dst_len, code) in enumerate(invalid):
        _, vb, vd, vr = small[(5 * k) % len(small)]
        add(vb, vd, len(vr), vr)
        add(base, delta, dst_len, code)
    _, vb, vd, vr = small[3]
    add(vb, vd, len(vr), vr)
    items.append((len(bases), vd, len(vr)))  # base_idx = nb
    expect.append(C.ERANGE)
    got, status, head, tail = run_device(engine, bases, items, pre=(3, 5, 9))
    assert head == bytes([FILL]) * 9 and tail == SENTINEL
    for k, want in enumerate(expect):
        if isinstance(want, int):
            assert status[k] == want, (k, status[k], want)
            if want == C.EOP and items[k][2] == 16:
                assert got[k] == bytes([FILL]) * 16, "guard %d was written" % k
        else:
            assert status[k] == 0 and got[k] == want, k
    assert set(status.tolist()) >= set(range(0, 9)) | {C.ERANGE}


@pytest.mark.parametrize("pre", [(0, 0, 0), (1, 2, 3), (15, 9, 7)])
def test_host_and_device_forms_agree(engine, small, pre):
    invalid = C.crafted_invalid()
    bases = [b for _, b, _, _ in small] + [b for _, b, _, _, _ in invalid]
    items = [(k, d, len(r)) for k, (_, _, d, r) in enumerate(small)]
    items += [(len(small) + k, d, dl) for k, (_, _, d, dl, _) in enumerate(invalid)]
    hgot, hst = run_host(engine, bases, items)
    dgot, dst, _, tail = run_device(engine, bases, items, pre=pre)
    assert tail == SENTINEL
    assert np.array_equal(hst, dst)
    assert np.count_nonzero(hst) == len(invalid)
    for k in np.flatnonzero(hst == 0):
        assert hgot[k] == dgot[k] == small[k][3]


def test_offsets_are_checked(engine):
    base = np.frombuffer(b"0123456789", np.uint8)
    delta, res = C.encode(base.tobytes(), [("c", 2, 5)])
    d = np.frombuffer(delta, np.uint8)
    with pytest.raises(N.KdError):  # descending dst offsets (host form: refused before the launch)
        engine.apply_deltas(base, [0, 10], [0, 0], np.concatenate([d, d]), [0, len(d), 2 * len(d)], [0, 5, 3])
    data, status = engine.apply_deltas(base, [0, 10], [0, 1], np.concatenate([d, d]), [0, len(d), 2 * len(d)], [0, 5, 10])
    assert status.tolist() == [0, C.ERANGE] and data[:5].tobytes() == res
    data, status = engine.apply_deltas(base, [0, 10], np.zeros(0, np.uint32), np.zeros(0, np.uint8), [0], [0])
    assert data.size == 0 and status.size == 0
