"""The expected pairing of find_renames, restated from the reference's two-dict loop
(WorkingCopy.find_renames, kart/working_copy/base.py:829-854): inserts and deletes are keyed by their
hash in iteration order, later entries overwriting earlier ones; every hash present in both dicts
pairs its last delete with its last insert.  No product code is imported here.
"""
import numpy as np

NONE = 0xFFFFFFFF


def renames_ref(records):
    """records: (kind, oid bytes) per delta in delta order, kind "insert" / "delete" / anything else
    -> [(delta index of the delete, delta index of the insert)], ascending by the delete"""
    inserts, deletes = {}, {}
    for i, (kind, oid) in enumerate(records):
        if kind == "insert":
            inserts[oid] = i
        elif kind == "delete":
            deletes[oid] = i
    return sorted((d, inserts[h]) for h, d in deletes.items() if h in inserts)


def records_of(delta, oid_a, oid_b):
    """the (kind, oid bytes) records of a delta list [n, 2] over two sides' OID arrays [*, 20]"""
    out = []
    for a, b in np.asarray(delta, np.uint32).reshape(-1, 2).tolist():
        if a != NONE and b == NONE:
            out.append(("delete", oid_a[a].tobytes()))
        elif a == NONE and b != NONE:
            out.append(("insert", oid_b[b].tobytes()))
        else:
            out.append(("update", None))
    return out


def renames_ref_arrays(delta, oid_a, oid_b):
    """renames_ref over arrays, as the uint32 [k, 2] array the engine returns"""
    return np.asarray(renames_ref(records_of(delta, oid_a, oid_b)), np.uint32).reshape(-1, 2)
