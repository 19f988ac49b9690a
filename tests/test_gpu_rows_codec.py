"""GPU: the row-column kernels (dg_rows_* through the host entry and the device
entry) against the document model and the reference's j2t, as
test_rows_codec.py holds the checker to them."""
from collections import namedtuple

import pytest

import modelgen as M
import oracle
import rowsgen as RG
import test_gpu_rows as TR
import tgetref as R
from test_rows_codec import N_DOCS, PLANS, model_rows, same_message

pytestmark = pytest.mark.gpu

Head = namedtuple("Head", "status step count")
Cell = namedtuple("Cell", "status step val len")


@pytest.fixture(scope="module")
def corpus():
    ref = oracle.RefOracle()
    return M.Corpus(ref or oracle.PortOracle(), "nesting", N_DOCS)


@pytest.mark.parametrize("plan", range(len(PLANS)))
def test_rows(corpus, plan):
    parent, columns = PLANS[plan]
    arena = b"".join(corpus.msgs)
    s = RG.Set(corpus.msgs, parent, columns, R.STRUCT)
    n_ok = 0
    for what, run in (("host entry", TR.run_host), ("device entry", TR.run_device)):
        head, row_off, index, cols = run(s)
        off = row_off.tolist()
        cl = [[c[f].tolist() for f in ("status", "step", "val", "len")] for c in cols]
        for i, doc in enumerate(corpus.docs):
            cells = [[Cell(*(f[g] for f in c)) for c in cl] for g in range(off[i], off[i + 1])]
            h = Head(int(head["status"][i]), int(head["step"][i]), int(head["count"][i]))
            n_ok += same_message(h, cells, model_rows(doc, corpus.td, parent, columns), arena, (what, parent, i))
            for g in range(off[i], off[i + 1]):  # the index entry is the element's own bytes, inside its message
                assert int(index["msg"][g]) == i
    assert n_ok >= 2 * 100
