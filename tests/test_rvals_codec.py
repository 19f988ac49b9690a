"""The checker of row column writes (rvalsref.py) against a yardstick that
shares nothing with it: the document model of modelgen.py and the reference's
own j2t (oracle.RefOracle, the port oracle where oracle/_ref was not built),
picked as test_vals_codec.py picks it. The descriptor is list<Cols>, Cols the
13 optional scalar, string and numeric-list fields test_vals_codec.py restricts
the "all" descriptor to; what rvalsref encodes from the columns taken out of
the elements of 300 documents must be the bytes j2t writes for the documents.
gen_doc draws at most 3 elements, so the last 30 documents are widened to 8 to
12. The same documents are encoded as set<Cols> too: j2t writes a set from a
JSON array as it writes a list, with the other wire type in the field header
around it and the same value bytes, so the root value's bytes are the same and
the plan's container only names the wire type. Bytes only; no tolerance. No
GPU."""
import random

import numpy as np
import pytest

import modelgen as M
import oracle
import rvalsref as RR
import valsgen as VG
import valsref as VR
from dynamicgo_amd import thrift as T
from test_vals_codec import STRUCT_FIELDS, as_input

N_DOCS = 300
N_WIDE = 30


@pytest.fixture(scope="module")
def chk():
    ref = oracle.RefOracle()
    print("\ntest_rvals_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return ref or oracle.PortOracle()


def row_columns():
    """(list<Cols>, set<Cols>, kinds, ids, documents, columns by row as valsgen builds them, row_off, present by column)"""
    whole = M.descriptors()["all"]
    fields = [whole.struct.field_by_id(i) for i in STRUCT_FIELDS]
    sub = T.struct_type("Cols", [T.FieldDescriptor(f.id, f.name, f.type, T.OPTIONAL) for f in fields])
    ltd, std = T.list_of(sub), T.set_of(sub)
    rng = random.Random("rvals/list<Cols>")
    docs = [M.gen_doc(rng, ltd) for _ in range(N_DOCS)]
    for d in docs[-N_WIDE:]:
        while len(d) < 8 or rng.random() < 0.5 and len(d) < 12:
            d.append(M.gen_doc(rng, sub))
    # j2t writes a struct's fields in the document's order: every element in column order
    docs = [[{f.alias: r[f.alias] for f in fields if f.alias in r} for r in d] for d in docs]
    rows = [r for d in docs for r in d]
    row_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    kinds, cols, present = [], [], []
    for f in fields:
        t = f.type
        kind = VR.STRING if t.type == M.STRING else (VR.SET if t.type == M.SET else VR.LIST) | t.elem.type \
            if t.type in (M.LIST, M.SET) else t.type
        pres = [f.alias in r for r in rows]
        vals = [as_input(t, r[f.alias]) if p else None for r, p in zip(rows, pres)]
        if kind == VR.STRING:
            col = VG.string_col([v or b"" for v in vals], phase=f.id)
        elif kind & (VR.LIST | VR.SET):
            col = VG.list_col([v or [] for v in vals])
        else:
            col = VG.scalar_col([v or 0 for v in vals])
        col["present"] = np.array(pres, dtype=np.uint8)
        kinds.append(kind), cols.append(col), present.append(pres)
    return ltd, std, kinds, [f.id for f in fields], docs, cols, row_off, present


def test_the_generator_meets_its_conditions():
    """From the model alone: every field is present in at least 15 % of the rows and absent in at least 15 %; the
    lists' lengths include 0, 1 and 2 or more, and the widened documents hold 8 to 12 elements."""
    _, _, kinds, ids, docs, cols, row_off, present = row_columns()
    n_rows = int(row_off[-1])
    assert len(docs) == N_DOCS and len(set(ids)) == len(ids) == 13
    for fid, pres in zip(ids, present):
        assert len(pres) == n_rows and 0.15 * n_rows <= sum(pres) <= 0.85 * n_rows, (fid, sum(pres), n_rows)
    lens = [len(d) for d in docs]
    assert {0, 1} <= set(lens) and max(lens[:-N_WIDE]) >= 2
    assert all(8 <= ln <= 12 for ln in lens[-N_WIDE:]) and len(set(lens[-N_WIDE:])) >= 3
    assert {VR.BOOL, VR.I08, VR.I16, VR.I32, VR.I64, VR.DOUBLE, VR.STRING, VR.SET | VR.I64} == set(kinds)
    inner = {int(b - a) for c, k in zip(cols, kinds) if k & (VR.LIST | VR.SET) for a, b in zip(c["elem_off"], c["elem_off"][1:])}
    assert {0, 1, 2} <= inner


def test_a_list_of_structs_is_j2t_of_the_documents(chk):
    ltd, _, kinds, ids, docs, cols, row_off, _ = row_columns()
    arena, off, status, cell_status = RR.encode_batch(kinds, ids, cols, row_off, N_DOCS, int(row_off[-1]))
    assert not any(status) and not any(cell_status)
    for i, d in enumerate(docs):
        assert arena[off[i]:off[i + 1]] == M.encode(chk, ltd, d), (i, d)


def test_a_set_of_structs_is_j2t_of_the_documents(chk):
    _, std, kinds, ids, docs, cols, row_off, _ = row_columns()
    arena, off, _, _ = RR.encode_batch(kinds, ids, cols, row_off, N_DOCS, int(row_off[-1]))
    for i, d in enumerate(docs):
        assert arena[off[i]:off[i + 1]] == M.encode(chk, std, d), (i, d)
