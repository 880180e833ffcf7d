"""ObjectDB.read_batch_device against ObjectDB.read_batch: the same data, off and status for every
input, whatever the pack layout — plain streams inflated on the GPU, everything else read on the host
and placed by the same launch.
"""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from kart_amd import _native as N
from kart_amd.odb import ObjectDB

pytestmark = pytest.mark.gpu


def _blobs():
    """about 1,200 blobs of six kinds, the empty blob and one of KD_INF_MAX + 1 bytes"""
    rng = np.random.default_rng(11)
    out = [b"", bytes(rng.integers(0, 256, N.KD_INF_MAX + 1, dtype=np.uint8))]
    for k in range(300):  # point-like: a legend hash, a few numbers, a short name
        out.append(b"\x92\xc4\x14" + hashlib.sha1(b"legend").digest() + b"\x93" + rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
                   + b"name-%d" % k)
    for k in range(300):  # polygon-like: a header and 300 random bytes
        out.append(b"\x92\xc4\x14" + hashlib.sha1(b"legend").digest() + b"GP\x00\x03" + bytes(rng.integers(0, 256, 300, dtype=np.uint8))
                   + b"polygon %d" % k)
    for k in range(250):  # repeated text
        out.append((b"row %d of the survey; " % k) * int(rng.integers(2, 60)))
    for k in range(150):  # zero runs
        out.append(b"z%d" % k + bytes(int(rng.integers(1, 5000))) + b"end")
    for n in (1, 65_535, 65_536, 70_000):  # random blobs
        out.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))
    for k in range(200):  # a small alphabet
        out.append(b"%d:" % k + bytes(rng.integers(97, 101, int(rng.integers(10, 900)), dtype=np.uint8)))
    assert len(set(out)) == len(out)
    return out


def _oid(b):
    return hashlib.sha1(b"blob %d\0" % len(b) + b).digest()


def _import(gitdir, blobs, branch, depth0=True):
    """the blobs as files of one commit on ``branch``, written by one fast-import (one pack)"""
    lines = []
    for k, b in enumerate(blobs):
        lines.append(b"blob\nmark :%d\ndata %d\n" % (k + 1, len(b)) + b + b"\n")
    lines.append(b"commit refs/heads/%s\ncommitter t <t@t> 1600000000 +0000\ndata 1\nx\n" % branch.encode())
    for k in range(len(blobs)):
        lines.append(b"M 100644 :%d f/%d\n" % (k + 1, k))
    lines.append(b"\n")
    cmd = ["git", "-c", "fastimport.unpackLimit=0", "fast-import", "--quiet"] + (["--depth=0"] if depth0 else [])
    subprocess.run(cmd, input=b"".join(lines), env=dict(os.environ, GIT_DIR=gitdir), check=True)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    blobs = _blobs()
    oids = np.frombuffer(b"".join(_oid(b) for b in blobs), np.uint8).reshape(-1, 20)
    root = tmp_path_factory.mktemp("rbd")
    a = str(root / "a.git")
    subprocess.run(["git", "init", "-q", "--bare", a], check=True)
    _import(a, blobs, "main")
    return blobs, oids, root, a


def _same(engine, db, oids, blobs=None):
    data, off, status = db.read_batch(oids)
    dev, dstatus, stats = db.read_batch_device(engine, oids)
    ddata, doff = dev.download()
    assert np.array_equal(dstatus, status)
    assert np.array_equal(doff, off)
    assert np.array_equal(ddata, data)
    assert stats["device"] + stats["host"] + stats["fixups"] == len(oids)
    if blobs is not None:
        raw = ddata.tobytes()
        assert not status.any()
        assert [raw[int(off[i]):int(off[i + 1])] for i in range(len(blobs))] == blobs
    return stats


def test_fast_import_depth0_inflates_on_the_device(engine, corpus):
    """every blob but the oversized one is a plain stream: the host may read that one only"""
    blobs, oids, _, a = corpus
    db = ObjectDB(a)
    try:
        stats = _same(engine, db, oids, blobs)
        assert stats["host"] == 1 and stats["fixups"] == 0 and stats["device"] == len(blobs) - 1
        assert 0 < stats["compressed"] < sum(map(len, blobs))
    finally:
        db.close()


def test_repacked_with_deltas(engine, corpus):
    blobs, oids, root, a = corpus
    b = str(root / "b.git")
    shutil.copytree(a, b)
    subprocess.run(["git", "--git-dir", b, "repack", "-adfq", "--depth=50", "--window=50"], check=True)
    db = ObjectDB(b)
    try:
        stats = _same(engine, db, oids, blobs)
        assert stats["fixups"] == 0
    finally:
        db.close()


def test_two_packs_and_loose_objects(engine, corpus):
    blobs, oids, root, _ = corpus
    c = str(root / "c.git")
    subprocess.run(["git", "init", "-q", "--bare", c], check=True)
    _import(c, blobs[:500], "one")
    _import(c, blobs[500:-12], "two", depth0=False)
    for b in blobs[-12:]:
        subprocess.run(["git", "--git-dir", c, "hash-object", "-w", "--stdin"], input=b, check=True, capture_output=True)
    assert sum(f.endswith(".pack") for f in os.listdir(os.path.join(c, "objects", "pack"))) == 2
    db = ObjectDB(c)
    try:
        stats = _same(engine, db, oids, blobs)
        assert stats["host"] >= 12 and stats["device"] >= 400
    finally:
        db.close()


def test_input_order_duplicates_missing_and_non_blobs(engine, corpus):
    blobs, oids, _, a = corpus
    tree = subprocess.run(["git", "--git-dir", a, "rev-parse", "main^{tree}"], check=True, capture_output=True).stdout.decode().strip()
    db = ObjectDB(a)
    try:
        rng = np.random.default_rng(3)
        pick = rng.integers(0, len(blobs), 700)
        pick[10:20] = pick[0:10]  # duplicates
        ids = oids[pick].copy()
        ids[100] = np.frombuffer(hashlib.sha1(b"no such object").digest(), np.uint8)
        ids[200] = np.frombuffer(bytes.fromhex(tree), np.uint8)
        data, off, status = db.read_batch(ids)
        assert status[100] == 1 and status[200] == 2 and np.count_nonzero(status) == 2
        _same(engine, db, ids)
        _same(engine, db, ids[::-1].copy())
        # n = 0
        dev, st, stats = db.read_batch_device(engine, np.zeros((0, 20), np.uint8))
        assert dev.n == 0 and st.size == 0 and stats == {"device": 0, "host": 0, "compressed": 0, "fixups": 0}
        assert dev.download()[1].tolist() == [0]
    finally:
        db.close()


def _write_pack(gitdir, entries):
    """a pack of blob entries [(content, zlib stream)] written by hand, indexed by git"""
    body = b"PACK" + (2).to_bytes(4, "big") + len(entries).to_bytes(4, "big")
    for content, stream in entries:
        size = len(content)
        head = [(3 << 4) | (size & 15)]
        size >>= 4
        while size:
            head[-1] |= 0x80
            head.append(size & 0x7F)
            size >>= 7
        body += bytes(head) + stream
    body += hashlib.sha1(body).digest()
    path = os.path.join(gitdir, "objects", "pack", "pack-%s.pack" % hashlib.sha1(body).hexdigest())
    with open(path, "wb") as f:
        f.write(body)
    subprocess.run(["git", "--git-dir", gitdir, "index-pack", path], check=True, capture_output=True)
    return path


def test_stream_longer_than_the_bound_is_read_by_the_host(engine, tmp_path):
    """a valid stream git would never write — thirty empty stored blocks in it — is longer than the
    span the device gets: the device reports it, the host reads it, the result is the same"""
    import zlib

    import inflate_craft as C

    text = b"not much to say"
    d = C.Deflate().fixed(list(text))
    for _ in range(30):
        d.stored(b"")
    long_stream = d.fixed((), final=True).zlib()
    assert zlib.decompress(long_stream) == text and len(long_stream) > len(text) + 13 + 100
    blobs = [b"first blob " * 9, text, b"third blob " * 7, b""]
    gitdir = str(tmp_path / "h.git")
    subprocess.run(["git", "init", "-q", "--bare", gitdir], check=True)
    _write_pack(gitdir, [(b, long_stream if b is text else zlib.compress(b)) for b in blobs])
    oids = np.frombuffer(b"".join(_oid(b) for b in blobs), np.uint8).reshape(-1, 20)
    db = ObjectDB(gitdir)
    try:
        stats = _same(engine, db, oids, blobs)
        assert stats == {"device": 3, "host": 0, "compressed": stats["compressed"], "fixups": 1}
    finally:
        db.close()


def test_corrupt_stream_gets_the_host_status(engine, corpus, tmp_path):
    """a damaged packed blob fails on the device and on the host: status and length are the host route's,
    and every later blob still sits at the host route's offset"""
    blobs, oids, _, a = corpus
    c = str(tmp_path / "k.git")
    shutil.copytree(a, c)
    pack = next(os.path.join(c, "objects", "pack", f) for f in os.listdir(os.path.join(c, "objects", "pack"))
                if f.endswith(".pack"))
    os.chmod(pack, 0o644)
    victim = blobs.index(next(b for b in blobs if b.startswith(b"row 7 of the survey")))
    import zlib

    stream = zlib.compress(blobs[victim])  # git's stream of it: the same bytes at the default level
    raw = bytearray(open(pack, "rb").read())
    at = bytes(raw).find(stream)
    assert at > 0 and bytes(raw).find(stream, at + 1) < 0
    raw[at + len(stream) // 2] ^= 0x10
    with open(pack, "wb") as f:
        f.write(raw)
    db = ObjectDB(c)
    try:
        pick = np.arange(victim - 40, victim + 40)
        data, off, status = db.read_batch(oids[pick])
        assert status[40] == 2 and np.count_nonzero(status) == 1 and off[41] == off[40]
        stats = _same(engine, db, oids[pick])
        assert stats["host"] == 1 and stats["device"] == 79
    finally:
        db.close()
