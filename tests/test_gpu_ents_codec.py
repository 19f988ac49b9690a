"""GPU: the entry-column kernels (dg_ents_* through the host entry and the
device entries) against the document model and the reference's j2t, as
test_ents_codec.py holds the checker to them."""
from collections import namedtuple

import pytest

import entsmodel as EM
import modelgen as M
import oracle
import test_gpu_ents as TE
from test_ents_codec import N_DOCS, same_cell

pytestmark = pytest.mark.gpu

Got = namedtuple("Got", "status step len keys klens vals vlens")


@pytest.fixture(scope="module")
def corpus():
    ref = oracle.RefOracle()
    return M.Corpus(ref or oracle.PortOracle(), "all", N_DOCS)


def cells_of(g, n):
    """column g of test_gpu_ents.run_host / run_device as one Got per message"""
    off = g["off"].tolist()
    zeros = [0] * off[-1]
    arr = {f: g[f].tolist() if f in g else zeros for f in ("keys", "klens", "vals", "vlens")}
    return [Got(int(g["status"][i]), int(g["step"][i]), int(g["len"][i]), *(arr[f][off[i]:off[i + 1]] for f in
                                                                         ("keys", "klens", "vals", "vlens")))
            for i in range(n)]


@pytest.mark.parametrize("stage", (0, 16))
def test_entries(knob, corpus, stage):
    knob("ents_stage", stage)
    n = len(corpus.msgs)
    arena = b"".join(corpus.msgs)
    n_ok = 0
    for what, run in (("host entry", TE.run_host), ("device entry", TE.run_device)):
        got = run(corpus.msgs, EM.COLUMNS)
        for k, (path, kind) in enumerate(EM.COLUMNS):
            for doc, c in zip(corpus.docs, cells_of(got[k], n)):
                # string keys and values are arena offsets: slice the arena itself
                n_ok += same_cell(c, EM.entries(doc, corpus.td, path, kind), arena, 0, (what, path, kind)) == "ok"
    assert n_ok >= 2 * 5 * 50
