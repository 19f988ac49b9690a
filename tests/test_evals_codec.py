"""The checker of entry column writes (evalsref.py) against a yardstick that
shares nothing with it: the document model of modelgen.py and the reference's
own j2t (oracle.RefOracle, the port oracle where oracle/_ref was not built),
picked as test_vals_codec.py picks it. What evalsref encodes from a container,
or from the columns taken out of 300 documents, must be the bytes j2t writes
for the same container or for the documents restricted to those fields. Bytes
only; no tolerance.

modelgen.gen_doc draws at most 4 list elements and at most 4 map entries (its
key vocabulary holds 4 keys a type), so the last 8 documents of every root are
widened here from gen_doc's own elements, keys and values to 8 to 12 entries.
Every root asked for is generated; none had to be left out. JSON cannot carry
duplicate keys, a NaN or an integer beyond its width: those inputs are covered
against evalsref alone, by test_evals_host.py and test_gpu_evals.py over
evalsgen's matrix. No GPU."""
import base64
import random

import numpy as np
import pytest

import evalsgen as EG
import evalsref as ER
import modelgen as M
import oracle
from dynamicgo_amd import thrift as T

N_DOCS, N_WIDE = 300, 8
VALUES = ["bool", "byte", "i16", "i32", "i64", "double", "string", "binary"]
KEYS = ["string", "byte", "i16", "i32", "i64"]
ROOTS = [("list<string>", T.list_of(T.builtin("string")), ER.LIST_STR), ("set<string>", T.set_of(T.builtin("string")), ER.SET_STR),
         ("list<binary>", T.list_of(T.builtin("binary")), ER.LIST_STR)] + \
    [("map<%s,%s>" % (k, v), T.map_of(T.builtin(k), T.builtin(v)), ER.map_kind(T.builtin(k).type, T.builtin(v).type))
     for k in KEYS for v in VALUES]
STRUCT_FIELDS = [19, 20, 13, 14]  # list<string>, map<string, i64>, map<byte, bool>, map<i16, binary>


@pytest.fixture(scope="module")
def chk():
    ref = oracle.RefOracle()
    print("\ntest_evals_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return ref or oracle.PortOracle()


def wide(rng, td):
    """a container of 8 to 12 entries from gen_doc's elements, keys and values"""
    want = rng.randint(8, 12)
    if td.type == M.MAP:
        out = {}
        while len(out) < want:
            out[M.gen_doc(rng, td.key)] = M.gen_doc(rng, td.elem)
        return out
    out = []
    while len(out) < want:
        v = M.gen_doc(rng, td.elem)
        if td.type == M.LIST or v not in out:
            out.append(v)
    return out


def root_values(name, td):
    rng = random.Random("evals/" + name)
    return [M.gen_doc(rng, td) for _ in range(N_DOCS - N_WIDE)] + [wide(rng, td) for _ in range(N_WIDE)]


def one(td, v):
    if td.type == M.STRING:
        return base64.b64decode(v) if td.is_binary() else v.encode()
    return float(v) if td.type == M.DOUBLE else int(v)


def as_input(td, v):
    """a document's container as evalsref takes it: elements, or (key, value) pairs in document order"""
    if td.type == M.MAP:
        return [(one(td.key, k), one(td.elem, x)) for k, x in v.items()]
    return [one(td.elem, e) for e in v]


@pytest.mark.parametrize("name,td,kind", ROOTS, ids=[r[0] for r in ROOTS])
def test_one_value_is_what_j2t_writes(chk, name, td, kind):
    values = root_values(name, td)
    assert len(values) >= 50
    assert {len(v) for v in values} >= {0, 1, 2} and max(len(v) for v in values) >= 8
    for v in values:
        assert ER.encode(kind, as_input(td, v)) == M.encode(chk, td, v), (name, v)
    assert ER.wire_type(kind) == td.type


def struct_columns():
    """(sub-descriptor, kinds, ids, docs restricted to the fields in column order, columns as evalsgen builds them,
    present)"""
    whole = M.descriptors()["all"]
    fields = [whole.struct.field_by_id(i) for i in STRUCT_FIELDS]
    sub = T.struct_type("Ents", [T.FieldDescriptor(f.id, f.name, f.type, T.OPTIONAL) for f in fields])
    rng = random.Random(M.Corpus.SEEDS["all"])
    docs = [M.gen_doc(rng, whole) for _ in range(N_DOCS)]
    kinds, cols, present = [], [], []
    for f in fields:
        t = f.type
        kind = ER.map_kind(t.key.type, t.elem.type) if t.type == M.MAP else (ER.SET if t.type == M.SET else ER.LIST) | ER.STRING
        pres = [f.alias in d for d in docs]
        rows = [as_input(t, d[f.alias]) if p else [] for d, p in zip(docs, pres)]
        col = EG.entry_col(kind, rows, phase=f.id)
        col["present"] = np.array(pres, dtype=np.uint8)
        kinds.append(kind), cols.append(col), present.append(pres)
    small = [{f.alias: d[f.alias] for f in fields if f.alias in d} for d in docs]
    return sub, kinds, [f.id for f in fields], small, cols, present


def test_the_generator_meets_its_conditions():
    """From the model alone: every root has at least 50 values, sizes 0, 1 and 2 and one container of 8 or more
    entries; every struct field is present in 15 % to 85 % of the documents."""
    for name, td, kind in ROOTS:
        values = root_values(name, td)
        assert len(values) >= 50, name
        assert {len(v) for v in values} >= {0, 1, 2} and max(len(v) for v in values) >= 8, name
    _, kinds, ids, small, _, present = struct_columns()
    assert ids == STRUCT_FIELDS
    for fid, pres in zip(ids, present):
        assert 0.15 * N_DOCS <= sum(pres) <= 0.85 * N_DOCS, (fid, sum(pres))
    assert kinds == [ER.LIST_STR, ER.map_kind(ER.STRING, ER.I64), ER.map_kind(ER.I08, ER.BOOL), ER.map_kind(ER.I16, ER.STRING)]
    assert len({len(d) for d in small}) >= 4  # messages of several field counts
    assert {} in small  # the all-absent message


def test_struct_mode_is_j2t_of_the_restricted_documents(chk):
    sub, kinds, ids, small, cols, _ = struct_columns()
    arena, off, status = ER.encode_batch(kinds, cols, N_DOCS, ids)
    K = len(kinds)
    assert not any(status)
    for i, d in enumerate(small):
        assert arena[off[i * K]:off[(i + 1) * K]] == M.encode(chk, sub, d), (i, d)
