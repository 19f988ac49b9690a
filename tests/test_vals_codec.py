"""The checker of typed column writes (valsref.py) against a yardstick that
shares nothing with it: the document model of modelgen.py and the reference's
own j2t (oracle.RefOracle, the port oracle where oracle/_ref was not built),
picked as test_generic_codec.py picks it. What valsref encodes from a value, or
from the columns taken out of 300 documents, must be the bytes j2t writes for
the same value or for the documents restricted to those fields. Bytes only; no
tolerance.

JSON cannot carry a NaN, an infinity or an integer beyond its field's width, so
those inputs (and the 64-bit inputs narrower kinds cut down) are covered against
valsref alone, by test_vals_host.py and test_gpu_vals.py over valsgen's
matrix. No GPU."""
import base64
import random

import numpy as np
import pytest

import modelgen as M
import oracle
import valsgen as VG
import valsref as VR
from dynamicgo_amd import thrift as T

N_DOCS = 300
NUMERIC = {"bool": VR.BOOL, "byte": VR.I08, "i16": VR.I16, "i32": VR.I32, "i64": VR.I64, "double": VR.DOUBLE}
ROOTS = [(name, T.builtin(name), kind) for name, kind in NUMERIC.items()] + [("string", T.builtin("string"), VR.STRING)] + \
    [("list<%s>" % name, T.list_of(T.builtin(name)), VR.LIST | kind) for name, kind in NUMERIC.items()] + \
    [("set<%s>" % name, T.set_of(T.builtin(name)), VR.SET | kind) for name, kind in NUMERIC.items()]
# the "all" descriptor's scalar, string and numeric-list fields, in column order (not id order)
STRUCT_FIELDS = [4, 7, 1, 11, 6, 2, 8, 3, 5, 22, 23, 24, 32767]


@pytest.fixture(scope="module")
def chk():
    ref = oracle.RefOracle()
    print("\ntest_vals_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return ref or oracle.PortOracle()


def root_values(name, td):
    rng = random.Random("vals/" + name)
    return [M.gen_doc(rng, td) for _ in range(N_DOCS)]


def as_input(td, v):
    """a document value as valsref takes it"""
    if td.type == M.STRING:
        return base64.b64decode(v) if td.is_binary() else v.encode()
    if td.type in (M.LIST, M.SET):
        return [as_input(td.elem, e) for e in v]
    return int(v) if td.type != M.DOUBLE else float(v)


@pytest.mark.parametrize("name,td,kind", ROOTS, ids=[r[0] for r in ROOTS])
def test_one_value_is_what_j2t_writes(chk, name, td, kind):
    values = root_values(name, td)
    assert len(values) >= 50
    for v in values:
        assert VR.encode(kind, as_input(td, v)) == M.encode(chk, td, v), (name, v)
    assert VR.wire_type(kind) == td.type
    if td.type in (M.LIST, M.SET):
        assert {len(v) for v in values} >= {0, 1, 2}


def struct_columns():
    """(sub-descriptor, kinds, ids, docs restricted to the fields in column order, columns as valsgen builds them)"""
    whole = M.descriptors()["all"]
    fields = [whole.struct.field_by_id(i) for i in STRUCT_FIELDS]
    sub = T.struct_type("Cols", [T.FieldDescriptor(f.id, f.name, f.type, T.OPTIONAL) for f in fields])
    rng = random.Random(M.Corpus.SEEDS["all"])
    docs = [M.gen_doc(rng, whole) for _ in range(N_DOCS)]
    kinds, cols, present = [], [], []
    for f in fields:
        t = f.type
        kind = VR.STRING if t.type == M.STRING else (VR.SET if t.type == M.SET else VR.LIST) | t.elem.type \
            if t.type in (M.LIST, M.SET) else t.type
        pres = [f.alias in d for d in docs]
        vals = [as_input(t, d[f.alias]) if p else None for d, p in zip(docs, pres)]
        if kind == VR.STRING:
            col = VG.string_col([v or b"" for v in vals], phase=f.id)
        elif kind & (VR.LIST | VR.SET):
            col = VG.list_col([v or [] for v in vals])
        else:
            col = VG.scalar_col([v or 0 for v in vals])
        col["present"] = np.array(pres, dtype=np.uint8)
        kinds.append(kind), cols.append(col), present.append(pres)
    small = [{f.alias: d[f.alias] for f in fields if f.alias in d} for d in docs]
    return sub, kinds, [f.id for f in fields], small, cols, present


def test_the_generator_meets_its_conditions():
    """From the model alone: every kind has at least 50 encoded values, every struct field is absent from at least
    15 % and present in at least 15 % of the documents."""
    for name, td, kind in ROOTS:
        assert len(root_values(name, td)) >= 50, name
    _, kinds, ids, small, _, present = struct_columns()
    assert len(set(ids)) == len(ids) <= VR.MAX_COLS
    for fid, kind, pres in zip(ids, kinds, present):
        assert 0.15 * N_DOCS <= sum(pres) <= 0.85 * N_DOCS, (fid, sum(pres))
        assert sum(pres) >= 50, fid
    assert {VR.BOOL, VR.I08, VR.I16, VR.I32, VR.I64, VR.DOUBLE, VR.STRING, VR.SET | VR.I64} == set(kinds)
    assert len({len(d) for d in small}) >= 4  # messages of several field counts


def test_struct_mode_is_j2t_of_the_restricted_documents(chk):
    sub, kinds, ids, small, cols, _ = struct_columns()
    arena, off, status = VR.encode_batch(kinds, cols, N_DOCS, ids)
    K = len(kinds)
    assert not any(status)
    for i, d in enumerate(small):
        assert arena[off[i * K]:off[(i + 1) * K]] == M.encode(chk, sub, d), (i, d)
