"""The row-column checker (rowsref.py) against a second yardstick that shares
nothing with it: the document model (modelgen.py) and the reference's own j2t
(oracle.RefOracle, the port oracle where oracle/_ref was not built). On the
`nesting` descriptor's list of structs the rows of T = j2t(doc, D) must equal
[elem[field] for elem in doc[list]] in document order, and on its lists of
scalars the elements themselves. Bytes, integers and bit patterns only; no
tolerance.

No GPU: the kernels get the same expectations in test_gpu_rows_codec.py."""
import random

import pytest

import modelgen as M
import oracle
import rowsref as RR
import tgetref as R

N_DOCS = 300
F = R.FIELD
# Nesting: 2 list<Simple{1: byte, 2: i64, 3: double, 4: i32, 5: string, 6: binary}>, 5 list<i32>, 10 list<string>,
# 13 list<i64>. (parent path, [(sub-path, kind)])
PLANS = [
    ([(F, 2)], [([(F, 1)], M.COL_BYTE), ([(F, 2)], M.COL_INT), ([(F, 3)], M.COL_F64), ([(F, 4)], M.COL_INT),
                ([(F, 5)], M.COL_STR), ([(F, 6)], M.COL_STR), ([(F, 1)], M.COL_INT)]),
    ([(F, 5)], [([], M.COL_INT)]),
    ([(F, 10)], [([], M.COL_STR)]),
    ([(F, 13)], [([], M.COL_INT)]),
]


@pytest.fixture(scope="module")
def corpus():
    ref = oracle.RefOracle()
    print("\ntest_rows_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return M.Corpus(ref or oracle.PortOracle(), "nesting", N_DOCS)


def model_rows(doc, td, parent, columns):
    """("notfound", step) or ("ok", [[the model's cell of element j under column k]])"""
    r = M.sub(doc, td, parent)
    if isinstance(r, int):
        return "notfound", r
    elems, d = r
    return "ok", [[M.column(e, d.elem, p, k) for p, k in columns] for e in elems]


def same_message(head, cells, want, arena, what):
    """a message's head (status, step, count) and cells (anything with status / step / val / len, [row][column])
    against the model's; STR values are offsets into `arena`. Returns the OK cells seen."""
    if want[0] == "notfound":
        assert (head.status, head.step, head.count) == (R.NOT_FOUND, want[1], 0) and not cells, (what, head)
        return 0
    assert (head.status, head.count) == (R.OK, len(want[1])) and len(cells) == len(want[1]), (what, head)
    n_ok = 0
    for j, (row, wrow) in enumerate(zip(cells, want[1])):
        for k, (c, w) in enumerate(zip(row, wrow)):
            if w[0] == "notfound":
                assert (c.status, c.step) == (R.NOT_FOUND, w[1]), (what, j, k, c)
                continue
            assert c.status == R.OK, (what, j, k, c)
            n_ok += 1
            if w[4] is not None:  # bytes
                assert c.len == w[2] and bytes(arena[c.val:c.val + c.len]) == w[4], (what, j, k, c)
            else:
                assert c.val == w[1], (what, j, k, c, w)
    return n_ok


def test_the_corpus_meets_its_conditions():
    """From the model alone, with the seed of Corpus.SEEDS: every plan has at least 100 rows, lists of 0 and of 3
    elements and messages without the list; every column of the struct plan has cells that are there and cells that
    are not, but field 2: the model leaves fields with a value mapping out, so it is never there"""
    td = M.descriptors()["nesting"]
    rng = random.Random(M.Corpus.SEEDS["nesting"])
    docs = [M.gen_doc(rng, td) for _ in range(N_DOCS)]
    for parent, columns in PLANS:
        rows = [model_rows(d, td, parent, columns) for d in docs]
        sizes = [len(r[1]) for r in rows if r[0] == "ok"]
        assert sum(sizes) >= 100 and 0 in sizes and 3 in sizes and any(r[0] == "notfound" for r in rows), parent
    rows = [model_rows(d, td, *PLANS[0]) for d in docs]
    for k in range(len(PLANS[0][1])):
        cells = [row[k][0] for r in rows if r[0] == "ok" for row in r[1]]
        assert cells.count("notfound") >= 50 and (cells.count("ok") >= 50 if k != 1 else "ok" not in cells), k


def test_rows(corpus):
    n_ok = 0
    for parent, columns in PLANS:
        for doc, t in zip(corpus.docs, corpus.msgs):
            m = RR.message(t, parent, columns)
            n_ok += same_message(m.head, m.cells, model_rows(doc, corpus.td, parent, columns), t, parent)
    assert n_ok >= 1000
