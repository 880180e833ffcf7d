"""find_renames at the drop-in boundary: dataset_diff / diff_feature / get_dataset_diff fold a delete
and an insert of one blob into one update delta (WorkingCopy.find_renames' algebra at the TODO of
RichBaseDataset.diff_feature), field_diff names the pk column on the folded deltas, and the default
changes nothing.

Each test runs twice, as tests/test_dropin.py does: on the CPU against a stand-in engine whose
find_renames is the reference loop (tests/renames_ref.py) — that run checks the host logic — and,
marked gpu, against the HIP engine.
"""
import base64
import copy
import hashlib
import os

import msgpack
import numpy as np
import pytest

from checks import NONE
from fixtures import load
from kart_amd import dataset as D
from kart_amd import meta as M
from kart_amd import packing, synth
from kart_amd.adaptor import structs
from kart_amd.engine import Diff2Result
from renames_ref import renames_ref_arrays

K = 7  # features re-keyed with their blobs untouched


class RefEngine:
    """test-only stand-in with the Engine interface: the CPU oracle's diff2 / fielddiff, and the
    reference's two-dict loop for find_renames"""

    def diff2(self, A, B):
        from oracle import oracle as O

        delta, c = O.classify2(A.key, A.oid, B.key, B.oid)
        upd = delta[(delta[:, 0] != NONE) & (delta[:, 1] != NONE)]
        return Diff2Result(c["inserts"], c["updates"], c["deletes"], delta, upd)

    def fielddiff(self, od, oo, nd, no, pairs, maps):
        from oracle import oracle as O

        return O.fielddiff(od, oo, nd, no, pairs, maps)

    def find_renames(self, A, B, delta):
        return renames_ref_arrays(delta, A.oid, B.oid)


@pytest.fixture(params=["ref", pytest.param("gpu", marks=pytest.mark.gpu)])
def eng(request):
    if request.param == "ref":
        yield RefEngine()
    else:
        yield request.getfixturevalue("engine")


def git_oid(data):
    return np.frombuffer(hashlib.sha1(b"blob %d\x00" % len(data) + data).digest(), np.uint8)


def edited(blob, text):
    """the feature blob with its last value (the name) replaced"""
    legend, vals = msgpack.unpackb(blob, raw=False)
    vals[-1] = text
    return msgpack.packb([legend, vals], use_bin_type=True)


def make_version(fx, feats, meta=None):
    """a DatasetVersion of the points dataset holding ``feats`` {pk: blob bytes}"""
    pks = np.array(sorted(feats), np.int64)
    blobs = [feats[int(p)] for p in pks]
    names, off = synth.int_pk_paths(pks)
    oids = np.stack([git_oid(b) for b in blobs])
    if meta is None:
        meta = M.meta_items(fx.meta_files("head"), fx.attachments("head"))
    return D.DatasetVersion(fx.meta["ds_path"], fx.schema("head"), fx.legends, fx.encoding("head"), names, off, oids,
                            lambda i: blobs[int(i)], meta=meta)


class Case:
    """base and target versions of the points fixture's HEAD with crafted re-keyed features"""

    def __init__(self):
        fx = load("repo_points")
        self.fx = fx
        idx = fx.a["head_blob"]
        head = {}
        for name, bi in zip(fx.names("head"), idx):
            (pk,) = msgpack.unpackb(base64.urlsafe_b64decode(os.path.basename(name)))
            head[int(pk)] = fx.blob(int(bi))
        # the path encoder used for the new names gives the fixture's own names
        pk_sorted = sorted(head)
        arena, off = synth.int_pk_paths(np.array(pk_sorted, np.int64))
        made = {arena[int(off[i]):int(off[i + 1])].tobytes().decode() for i in range(len(pk_sorted))}
        assert made == set(fx.names("head"))
        P = pk_sorted
        fresh = max(P) + 100_000
        base, target = dict(head), dict(head)
        self.moved = {}  # old pk -> new pk, blob untouched
        for i in range(K):
            old, new = P[10 + i], fresh + 1 + i
            target[new] = target.pop(old)
            self.moved[old] = new
        # re-keyed AND edited: another blob, so a delete and an insert remain
        self.edit_old, self.edit_new = P[20], fresh + 100
        target[self.edit_new] = edited(target.pop(self.edit_old), "re-keyed and edited")
        # two deleted features share one blob with one inserted feature: one pair, the delete that
        # comes last in delta (= key) order; the other stays a delete
        a, b = P[30], P[31]
        base[b] = base[a]
        self.shared_new = fresh + 200
        target[self.shared_new] = base[a]
        del target[a], target[b]
        ka, kb = packing.pk_to_int_key(a), packing.pk_to_int_key(b)
        self.shared_win, self.shared_lose = (a, b) if ka > kb else (b, a)
        # ordinary updates, a delete and an insert in the same diff
        self.updated = [P[40], P[41]]
        for p in self.updated:
            target[p] = edited(target[p], f"edited {p}")
        self.deleted, self.inserted = P[50], fresh + 300
        del target[self.deleted]
        target[self.inserted] = edited(head[P[51]], "brand new")
        self.base_feats, self.target_feats = base, target
        self.pk_name = fx.schema("head").pk_columns[0].name

    def versions(self, target_meta=None):
        return make_version(self.fx, self.base_feats), make_version(self.fx, self.target_feats, target_meta)

    def expected(self):
        want = {("update", o, n) for o, n in self.moved.items()}
        want.add(("update", self.shared_win, self.shared_new))
        want.add(("delete", self.shared_lose, None))
        want |= {("delete", self.edit_old, None), ("insert", None, self.edit_new)}
        want |= {("update", p, p) for p in self.updated}
        want |= {("delete", self.deleted, None), ("insert", None, self.inserted)}
        return want

    def plain(self):
        """the diff without the pass: every re-keyed feature a delete and an insert"""
        want = {("delete", o, None) for o in self.moved} | {("insert", None, n) for n in self.moved.values()}
        want |= {("delete", self.shared_win, None), ("delete", self.shared_lose, None), ("insert", None, self.shared_new)}
        want |= {("delete", self.edit_old, None), ("insert", None, self.edit_new)}
        want |= {("update", p, p) for p in self.updated}
        want |= {("delete", self.deleted, None), ("insert", None, self.inserted)}
        return want


@pytest.fixture(scope="module")
def case():
    return Case()


def triples(fd):
    return {(d.type, d.old_key, d.new_key) for d in fd.values()}


def view(fd):
    """delta for delta: key order, type, keys, flags and the leaves the halves promise"""
    out = []
    for k, d in fd.items():
        halves = tuple(None if kv is None else (kv.key, kv.value.args[0]._i) for kv in (d.old, d.new))
        out.append((k, d.type, d.flags, halves))
    return out


def test_renames_fold_into_updates(eng, case):
    base, target = case.versions()
    fd = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    want = case.expected()
    assert triples(fd) == want
    assert fd.type_counts() == {"updates": K + 1 + 2, "deletes": 3, "inserts": 2}
    assert all(k == d.key for k, d in fd.items())
    keys = sorted(t[1] if t[1] is not None else t[2] for t in want)
    assert [k for k, _ in fd.sorted_items()] == keys
    # lazy values: a folded delta's two values differ in the pk alone
    for old, new in list(case.moved.items()) + [(case.shared_win, case.shared_new)]:
        d = fd[old]
        assert (d.old_key, d.new_key, d.flags) == (old, new, 0)
        ov, nv = d.old_value, d.new_value
        assert ov[case.pk_name] == old and nv[case.pk_name] == new
        assert {k: v for k, v in ov.items() if k != case.pk_name} == {k: v for k, v in nv.items() if k != case.pk_name}
    # get_dataset_diff passes the keyword on
    ds = D.get_dataset_diff(eng, base, target, find_renames=True)
    assert triples(ds["feature"]) == want


def test_field_diff_on_folded_deltas(eng, case):
    base, target = case.versions()
    parent = D.dataset_diff(eng, base, target)["feature"]
    assert D.field_diff(eng, parent, base, target) == 2
    fd = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    assert fd._kd_updates.n_total == len(fd) and D._live_batch(fd, base, target) is fd._kd_updates
    assert D.field_diff(eng, fd, base, target) == K + 1 + 2
    for old in list(case.moved) + [case.shared_win]:
        assert fd[old].changed_fields == [case.pk_name]
    for p in case.updated:
        assert fd[p].changed_fields == parent[p].changed_fields and fd[p].changed_fields
    # the by-hand path (a diff changed after dataset_diff): the same answers, the same count
    fd2 = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    del fd2[case.deleted]
    assert D._live_batch(fd2, base, target) is None
    assert D.field_diff(eng, fd2, base, target) == K + 1 + 2
    assert {k: d.changed_fields for k, d in fd2.items() if d.type == "update"} == \
        {k: d.changed_fields for k, d in fd.items() if d.type == "update"}


def test_reverse_gives_the_inverse(eng, case):
    base, target = case.versions()
    fwd = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    rev = D.dataset_diff(eng, base, target, reverse=True, find_renames=True)["feature"]
    assert triples(rev) == triples(~fwd)
    assert ("update", case.shared_new, case.shared_win) in triples(rev)
    for new, old in ((n, o) for o, n in case.moved.items()):
        assert (rev[new].old_key, rev[new].new_key) == (new, old)
        assert rev[new].old_value[case.pk_name] == new and rev[new].new_value[case.pk_name] == old


def test_default_is_unchanged(eng, case):
    base, target = case.versions()
    without = D.dataset_diff(eng, base, target)["feature"]
    off = D.dataset_diff(eng, base, target, find_renames=False)["feature"]
    assert triples(without) == case.plain()
    assert view(off) == view(without)
    assert off._kd_updates.n_total == without._kd_updates.n_total == len(without)
    gen = structs().DeltaDiff(D.diff_feature(eng, base, target, find_renames=False))
    assert view(gen) == view(structs().DeltaDiff(D.diff_feature(eng, base, target)))


def test_generator_and_python_builder_forms(eng, case, monkeypatch):
    """diff_feature as a generator yields the folded delta in the delete's place and drops the insert;
    the Python delta loop (no native builder) and a key filter give the reference's pairing too"""
    base, target = case.versions()
    want = case.expected()
    collected = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    deltas = list(D.diff_feature(eng, base, target, find_renames=True))
    assert {(d.type, d.old_key, d.new_key) for d in deltas} == want and len(deltas) == len(want)
    plain = [d.key for d in D.diff_feature(eng, base, target)]
    gone = set(case.moved.values()) | {case.shared_new}
    assert [d.key for d in deltas] == [k for k in plain if k not in gone]
    monkeypatch.setattr(D, "_pystr", None)
    assert triples(structs().DeltaDiff(D.diff_feature(eng, base, target, find_renames=True))) == want
    fd = D.dataset_diff(eng, base, target, find_renames=True)["feature"]
    assert view(fd) == view(collected) and fd._kd_updates.n_total == len(fd)

    class F(set):
        match_all = False

    (o1, n1), (o2, n2) = list(case.moved.items())[:2]
    # both halves of one pair pass the filter; of the other only the delete: nothing to pair it with
    got = structs().DeltaDiff(D.diff_feature(eng, base, target, F({str(o1), str(n1), str(o2)}), find_renames=True))
    assert triples(got) == {("update", o1, n1), ("delete", o2, None)}


def test_schema_change_disables_the_pass(eng, case):
    """can_find_renames: type updates alone keep the pass, any other schema change skips it; a diff
    with a side missing has nothing to pair"""
    meta = M.meta_items(case.fx.meta_files("head"), case.fx.attachments("head"))
    typed = copy.deepcopy(meta)
    col = next(c for c in typed["schema.json"] if c.get("primaryKeyIndex") is None and c.get("dataType") == "integer")
    col["size"] = 64 if col.get("size") != 64 else 32
    base, target = case.versions(typed)
    ds = D.dataset_diff(eng, base, target, find_renames=True)
    assert "schema.json" in ds["meta"] and D.can_find_renames(ds["meta"])
    assert triples(ds["feature"]) == case.expected()
    named = copy.deepcopy(meta)
    next(c for c in named["schema.json"] if c.get("primaryKeyIndex") is None)["name"] += "_2"
    base, target = case.versions(named)
    ds = D.dataset_diff(eng, base, target, find_renames=True)
    assert "schema.json" in ds["meta"] and not D.can_find_renames(ds["meta"])
    assert triples(ds["feature"]) == case.plain()
    assert D.can_find_renames({})
    base, _ = case.versions()
    assert D.get_dataset_diff(eng, None, base, find_renames=True)["feature"].type_counts() == {"inserts": base.n}
    assert D.get_dataset_diff(eng, base, None, find_renames=True)["feature"].type_counts() == {"deletes": base.n}
