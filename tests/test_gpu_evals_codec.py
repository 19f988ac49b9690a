"""GPU: the entry-column kernels against the document model: the device entry
and the host entry over the struct-mode batch of test_evals_codec.py (fields
19, 20, 13 and 14 of the "all" descriptor out of 300 documents) give the bytes
modelgen.encode gives for the restricted documents, through the reference's own
j2t where oracle/_ref was built. Bytes only; no tolerance."""
import numpy as np
import pytest

import modelgen as M
import oracle
from test_evals_codec import N_DOCS, struct_columns

pytestmark = pytest.mark.gpu


def test_struct_mode_on_the_device_is_j2t_of_the_restricted_documents():
    import torch
    from dynamicgo_amd import generic as G
    from test_gpu_evals import Outs, launch, to_dev, work_for, work_guards
    chk = oracle.RefOracle() or oracle.PortOracle()
    sub, kinds, ids, small, cols, _ = struct_columns()
    want = [M.encode(chk, sub, d) for d in small]
    K, need = len(kinds), sum(map(len, want))
    with G.EntryValuePlan(kinds, ids) as plan:
        o = Outs(N_DOCS * K, need)
        wt, work = work_for(plan, N_DOCS, cols)
        launch(plan, [to_dev(c) for c in cols], N_DOCS, o, work)
        torch.cuda.synchronize()
        out, off, st = o.read("codec")
        work_guards(wt, "codec")
        arena, h_off, h_st = G._entry_values_host(plan, cols, N_DOCS)
    assert not st.any() and not h_st.any() and int(off[-1]) == need == int(h_off[-1])
    assert (out[need:] == 0xAA).all()
    for i, w in enumerate(want):
        assert out[int(off[i * K]):int(off[(i + 1) * K])].tobytes() == w, (i, small[i])
        assert arena[int(h_off[i * K]):int(h_off[(i + 1) * K])].tobytes() == w, (i, small[i])
    assert np.array_equal(off, h_off)
