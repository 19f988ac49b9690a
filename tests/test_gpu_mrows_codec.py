"""GPU: the map-row kernels (dg_rows_create_map and dg_rows_map_* through the
host entry and the device entry) against the document model and the
reference's j2t, as test_mrows_codec.py holds the checker to them. The
elements of a list column come through the public call (rows_batch, which runs
dg_rows_list_device over the map plan's cells)."""
from collections import namedtuple

import numpy as np
import pytest

import modelgen as M
import mrowsgen as MG
import oracle
import test_gpu_mrows as TM
import tgetref as R
from test_gpu_tget import to_paths
from test_mrows_codec import N_DOCS, PLANS, STR, model_rows, same_message

pytestmark = pytest.mark.gpu

Head = namedtuple("Head", "status step count")
Key = namedtuple("Key", "val len")
Cell = namedtuple("Cell", "status step val len elems")


@pytest.fixture(scope="module")
def corpora():
    ref = oracle.RefOracle()
    return {name: M.Corpus(ref or oracle.PortOracle(), name, N_DOCS) for name in ("nesting", "all")}


@pytest.mark.parametrize("plan", range(len(PLANS)))
def test_map_rows(corpora, plan):
    from dynamicgo_amd import generic as G
    name, parent, keys, columns = PLANS[plan]
    corpus = corpora[name]
    arena = b"".join(corpus.msgs)
    s = MG.Set(corpus.msgs, parent, columns, R.STRUCT, keys)
    # the list columns' elements by row, through the public call
    r = G.rows_batch(corpus.msgs, to_paths([parent])[0], [(to_paths([p])[0], k) for p, k in columns], keys=TM.KEY_NAMES[keys])
    elems = {k: (c.offsets.tolist(), c.values.view(np.uint64).tolist()) for k, c in enumerate(r.columns) if c.kind & G.COL_LIST}
    n_ok = 0
    for what, run in (("host entry", TM.run_host), ("device entry", TM.run_device)):
        head, row_off, index, cols, kd = run(s)
        off = row_off.tolist()
        kv, kl = kd["key"].tolist(), kd["key_len"].tolist()
        cl = [[c[f].tolist() for f in ("status", "step", "val", "len")] for c in cols]
        for i, doc in enumerate(corpus.docs):
            rows = range(off[i], off[i + 1])
            cells = [[Cell(*(f[g] for f in c), elems[k][1][elems[k][0][g]:elems[k][0][g + 1]] if k in elems else None)
                      for k, c in enumerate(cl)] for g in rows]
            h = Head(int(head["status"][i]), int(head["step"][i]), int(head["count"][i]))
            n_ok += same_message(h, [Key(kv[g], kl[g]) for g in rows], cells,
                                 model_rows(doc, corpus.td, parent, columns), arena, (what, name, parent, i))
            for g in rows:  # the index entry is the value's own bytes, inside its message, behind its key
                assert int(index["msg"][g]) == i
                assert keys != STR or int(index["off"][g]) == kv[g] + kl[g]
    assert n_ok >= 2 * 300
    assert r.offsets.tolist() == off and (r.keys.view(np.uint64).tolist() == kv if keys != STR else
                                          r.keys == [arena[o:o + ln] for o, ln in zip(kv, kl)])
