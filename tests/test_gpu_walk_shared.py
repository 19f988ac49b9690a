"""GPU: what tget, cols, ents and rows share on the host (the pass state of
host_internal.h: queue, two alternating counter sets, deep frames, the event
that orders streams) and on the device (the pair pass of walk_kern.h), through
each component's device entry on ONE context: four calls in a row with no
synchronisation between them, alternating between two streams and between two
of the component's deep-chain batches (some messages nesting beyond the 8 LDS
frames and some not; the batches differ in size and in how many pairs they
queue, so a count that a deep pass failed to reset for the next call, or a
queue the next call reads too early, shows as another batch's pairs). Four calls
use each counter set twice; two streams use the ordering. Every run is compared
with the checker's answers, computed as the component's own deep test computes
them; every message is one the suite already runs.
Kids has test_counted_streams_and_back_to_back (test_gpu_kids.py)."""
import pytest

import colsgen as CG
import entsgen as EG
import rowsgen as RG
import tgetgen as TG
import tgetref as R
import test_gpu_cols as TC
import test_gpu_ents as TE
import test_gpu_rows as TR
import test_gpu_tget_deep as TD
from test_gpu_tget import expect as tget_expect, to_paths

pytestmark = pytest.mark.gpu

RUNS = 4  # run j: batch j % 2 on stream j % 2


def chain_batches():
    """colsgen's deep chains as test_deep_pass takes them (49 messages) and as rowsgen does (28)"""
    out = []
    for chains in (CG.deep_chains(), CG.deep_chains(per_depth=3)):
        frames = [TG.chain_frames(k, lf, [(R.FIELD, 2)]) for k, lf in chains]
        assert any(f > TG.LDS_FRAMES for f in frames) and any(f <= TG.LDS_FRAMES for f in frames)
        out.append([TG.chain_message(k, lf) for k, lf in chains])
    assert len(out[0]) != len(out[1])
    return out


def tget_runs(batches, streams):
    import torch
    from dynamicgo_amd import generic as G
    wants = [tget_expect(m, TG.CHAIN_PATHS) for m in batches]
    ups = [TD.Upload(m) for m in batches]
    outs = [TD.Outputs(ups[j % 2].n, len(TG.CHAIN_PATHS)) for j in range(RUNS)]
    with G.PathSet(to_paths(TG.CHAIN_PATHS)) as ps:
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            TD.launch(ps, ups[j % 2], o, stream=streams[j % 2])
        torch.cuda.synchronize()
    for j, o in enumerate(outs):
        o.verify(wants[j % 2], ups[j % 2].in_off, "tget, run %d" % (j + 1))


def cols_runs(batches, streams):
    import torch
    from dynamicgo_amd import generic as G
    wants = [CG.expect(m, CG.DEEP_COLUMNS) for m in batches]
    ups = [TC.upload(m) for m in batches]
    with G.ColumnPlan(TC.to_cols(CG.DEEP_COLUMNS)) as plan:
        outs = [TC.Outputs(len(batches[j % 2]), plan.count) for j in range(RUNS)]
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            arena, d_off, _ = ups[j % 2]
            G.columns_device(plan, arena, d_off, o.n, *o.args(), stream=streams[j % 2], max_len=max(map(len, batches[j % 2])))
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            what = "cols, run %d" % (j + 1)
            got = o.read(what)
            TC.emit_lists(plan, ups[j % 2][0], o, got, what, stream=streams[j % 2])  # the list launches use the same state
            TC.compare(got, wants[j % 2], what)


def ents_runs(streams):
    import torch
    from dynamicgo_amd import generic as G
    assert any(d + 1 > EG.LDS_FRAMES for d in EG.DEEP_DEPTHS) and any(d + 1 <= EG.LDS_FRAMES for d in EG.DEEP_DEPTHS)
    batches = [EG.deep_messages(), EG.deep_messages(per_depth=40)]  # test_deep_pass's, test_three_components_on_three_streams's
    wants = [EG.expect(m, EG.DEEP_COLUMNS) for m in batches]
    ups = [TE.upload(m) for m in batches]
    with G.EntryPlan(TE.to_cols(EG.DEEP_COLUMNS)) as plan:
        outs = [TE.Outputs(len(batches[j % 2]), plan.count) for j in range(RUNS)]
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            arena, d_off, _ = ups[j % 2]
            G.entries_device(plan, arena, d_off, o.n, *o.args(), stream=streams[j % 2], max_len=max(map(len, batches[j % 2])))
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            what = "ents, run %d" % (j + 1)
            got = o.read(what)
            TE.emit_all(plan, ups[j % 2][0], o, got, what, stream=streams[j % 2])
            TE.compare(got, wants[j % 2], what)


def rows_runs(streams):
    """rowsgen's two deep sets, a plan each; a call is three lane passes (head, index, cells), each with its deep
    pass on the counter set whose turn it is"""
    import torch
    sets = [(name, RG.deep_sets()[0][name]) for name in ("above", "inside")]
    wants = [TR.expect(name, s)[1] for name, s in sets]
    ups = [TR.upload(s.msgs) for _, s in sets]
    plans = [TR.plan_of(s) for _, s in sets]
    try:
        outs = []
        for j in range(RUNS):
            s, want = sets[j % 2][1], wants[j % 2]
            outs.append(TR.Outputs(len(s.msgs), len(s.columns), int(want[1][len(s.msgs)])))
        torch.cuda.synchronize()
        for j, o in enumerate(outs):  # the caller's index twice, then the context's own
            arena, d_off, _ = ups[j % 2]
            TR.launch(plans[j % 2], sets[j % 2][1], arena, d_off, o, own_index=j < 2, stream=streams[j % 2])
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            what = "rows %s, run %d" % (sets[j % 2][0], j + 1)
            RG.same(o.read(what, index=j < 2), wants[j % 2], what)
    finally:
        for p in plans:
            p.close()


def test_four_calls_on_two_streams_per_component():
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    batches = chain_batches()
    tget_runs(batches, streams)
    cols_runs(batches, streams)
    ents_runs(streams)
    rows_runs(streams)
