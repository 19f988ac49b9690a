"""GPU: the row-column kernels against the document model: the device entry
and the host entry over the batch of test_rvals_codec.py (list<Cols>, the 13
scalar, string and numeric-list fields of the "all" descriptor, out of the
elements of 300 documents) give the bytes modelgen.encode gives for the
documents, through the reference's own j2t where oracle/_ref was built. Bytes
only; no tolerance."""
import numpy as np
import pytest

import modelgen as M
import oracle
from test_rvals_codec import N_DOCS, row_columns

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("container", ("list", "set"))
def test_rows_on_the_device_are_j2t_of_the_documents(container):
    import torch
    from dynamicgo_amd import generic as G
    from test_gpu_rvals import Outs, dev_offsets, launch, to_dev, work_for, work_guards
    chk = oracle.RefOracle() or oracle.PortOracle()
    ltd, std, kinds, ids, docs, cols, row_off, _ = row_columns()
    td = ltd if container == "list" else std
    want = [M.encode(chk, td, d) for d in docs]
    K, need, n_rows = len(kinds), sum(map(len, want)), int(row_off[-1])
    with G.RowValuePlan(kinds, ids, container) as plan:
        assert plan.wire_type == td.type
        o = Outs(N_DOCS, n_rows * K, need)
        wt, work = work_for(plan, N_DOCS, n_rows)
        launch(plan, [to_dev(c) for c in cols], dev_offsets(row_off), N_DOCS, n_rows, o, work)
        torch.cuda.synchronize()
        out, off, st, cst = o.read("codec")
        work_guards(wt, "codec")
        arena, h_off, h_st, h_cst = G._row_values_host(plan, cols, row_off, N_DOCS, n_rows)
    assert not st.any() and not cst.any() and not h_st.any() and not h_cst.any() and int(off[-1]) == need == int(h_off[-1])
    assert (out[need:] == 0xAA).all()
    for i, w in enumerate(want):
        assert out[int(off[i]):int(off[i + 1])].tobytes() == w, (i, docs[i])
        assert arena[int(h_off[i]):int(h_off[i + 1])].tobytes() == w, (i, docs[i])
    assert np.array_equal(off, h_off)
