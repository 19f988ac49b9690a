"""GPU: batched SetByPath / UnsetByPath (dynamicgo_amd.generic over dg_edit_*)
against the pure-Python restatement of the reference in editref.py. Every case
runs on both routes of the splice (the edit_wave_min knob: 0 sends every
message to the wave route, a huge value every message to the lane route, which
runs with 1, 4 and 16 lanes a message: the edit_lanes knob), and
the bytes, out_len and ret of every message are compared exactly with the
checker's. Every device run also checks the memory contract: nothing stored in
front of the first slot or behind the last, nothing at or beyond out_len in a
slot that succeeded, nothing at all in the slot of a message that failed."""
import ctypes as C
import struct

import numpy as np
import pytest

import editgen as G
import editref as E
import slotguard as SG
import tgetref as R

pytestmark = pytest.mark.gpu

F, I, S, N, BK = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
LANE, WAVE = 1 << 40, 0  # edit_wave_min for the two routes
# (name, edit_wave_min, edit_lanes): the lane route with 1, 4 and 16 lanes a message, the wave route
ROUTES = (("lane", LANE, 1), ("lane x4", LANE, 4), ("lane x16", LANE, 16), ("wave", WAVE, 1))
FILL, GUARD = 0xEE, 64


def plan_of(case):
    from dynamicgo_amd import generic as X
    return X.EditPlan(G.paths_of(case.path), case.op)


def value_arena(case):
    """(val, val_off, val_len) as numpy arrays / None for dg_edit_batch_device"""
    if case.op != E.SET_OP:
        return None, None, 0
    if isinstance(case.values, bytes):
        return np.frombuffer(case.values + b"\0" * 16, dtype=np.uint8).copy(), None, len(case.values)
    off = np.zeros(len(case.msgs) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in case.values], out=off[1:])
    return np.frombuffer(b"".join(case.values) + b"\0" * 16, dtype=np.uint8).copy(), off, max(map(len, case.values), default=0)


def bound(case, i):
    return E.slot_bound(case.op, case.path, len(case.msgs[i]), len(case.value(i)) if case.op == E.SET_OP else 0)


def run_device(case, plan, caps=None, stream=None, hint=True):
    """dg_edit_batch_device over torch tensors -> [(ret, out)]. caps: the slot sizes, back to back behind a
    64-byte guard (so slot bases are unaligned); None: the exact bound rounded up to 16."""
    import torch
    from dynamicgo_amd import generic as X
    n = len(case.msgs)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in case.msgs], out=in_off[1:])
    if caps is None:
        caps = [(bound(case, i) + 15) & ~15 for i in range(n)]
    out_off = np.full(n + 1, GUARD, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    out_off[1:] += GUARD
    val, val_off, val_len = value_arena(case)
    arena = torch.from_numpy(np.frombuffer(b"".join(case.msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_in, d_oo = torch.from_numpy(in_off).cuda(), torch.from_numpy(out_off).cuda()
    d_val = None if val is None else torch.from_numpy(val).cuda()
    d_vo = None if val_off is None else torch.from_numpy(val_off).cuda()
    d_out = torch.full((int(out_off[n]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_ol = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    d_ret = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    ml = max((len(m) for m in case.msgs), default=0) if hint else 0
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # the uploads and fills above
    X.edit_device(plan, arena, d_in, n, case.val_type, d_val, d_vo, d_out, d_oo, d_ol, d_ret, root_type=case.root_type,
                  val_len=val_len if hint or val_off is None else 0, stream=stream, max_len=ml)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out, ol, ret = d_out.cpu().numpy(), d_ol.cpu().numpy().view(np.uint32), d_ret.cpu().numpy().view(np.uint64)
    assert (out[:GUARD] == FILL).all() and (out[int(out_off[n]):] == FILL).all(), "a store outside the slots"
    res = []
    for i in range(n):
        a, e = int(out_off[i]), int(out_off[i + 1])
        r = int(ret[i])
        used = int(ol[i]) if r & 0xFF == E.OK else 0
        assert used <= e - a, i
        assert (out[a + used:e] == FILL).all(), "message %d (ret %x): a store at or beyond out_len, or by a failed message" % (i, r)
        res.append((r, out[a:a + used].tobytes()))
        assert int(ol[i]) == E.out_len(r, res[-1][1]), (i, hex(r), int(ol[i]))
    return res


def same(got, want, case, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, %s, message %d (%r...): got %x / %d bytes, checker %x / %d bytes" % (
            case.what, what, i, case.msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))


def on_both_routes(knob, case, caps=None, plan=None):
    p = plan or plan_of(case)
    try:
        want = case.want(caps)
        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            same(run_device(case, p, caps), want, case, name + " route")
        return want
    finally:
        if plan is None:
            p.close()


@pytest.fixture(scope="module")
def fuzz():
    """the fuzz cases with the checker's answers, computed once"""
    cases = G.fuzz_cases()
    for c in cases:
        c.want()
    return cases


# -------------------------------------------------------------------- fuzz
def test_fuzz(knob, fuzz):
    sh = G.shares(fuzz)
    for k in ("replaced", "inserted", "deleted", "ErrNotFound", "ErrRead", "ErrDismatchType"):
        assert sh.get(k, 0) >= 0.05, (k, sh)
    assert {c.path[-1][0] for c in fuzz} == {F, I, S, N, BK} and {len(c.path) for c in fuzz} == {1, 2, 3}
    assert any(isinstance(c.values, list) for c in fuzz) and any(isinstance(c.values, bytes) and c.op == E.SET_OP for c in fuzz)
    for c in fuzz:
        on_both_routes(knob, c)


def test_default_route_and_hints(knob, fuzz):
    """the default knob, with and without the length hints, and a knob in the middle of the lengths"""
    from dynamicgo_amd.conv import default_context
    default = default_context().get_knob("edit_wave_min")
    for c in fuzz[::5]:
        with plan_of(c) as p:
            same(run_device(c, p), c.want(), c, "default knob")
            same(run_device(c, p, hint=False), c.want(), c, "default knob, no hints")
            knob("edit_wave_min", 300)
            knob("edit_lanes", 16)
            same(run_device(c, p), c.want(), c, "edit_wave_min 300, 16 lanes a message")
            knob("edit_wave_min", default)


# --------------------------------------------------------- alignment sweep
def test_alignment_sweep(knob):
    """prefix, old and new value lengths around the 16-byte units and the wave's 1024-byte stride; in exact-size
    slots back to back, so slot bases and message starts take every phase as the lengths vary"""
    c = G.sweep_case()
    want = on_both_routes(knob, c)
    assert all(r == E.word(E.OK, existed=True) for r, _ in want)
    on_both_routes(knob, c, [len(o) for _, o in want])


@pytest.mark.parametrize("kind", ("replace", "insert", "unset"))
def test_every_source_phase_meets_every_destination_phase(knob, kind):
    tested = G.sweep_message(5, 3, 20)
    val = G.wstr(b"0123456789abcdefghijk")
    op, path = {"replace": (E.SET_OP, [(F, 2)]), "insert": (E.SET_OP, [(F, 7)]), "unset": (E.UNSET_OP, [(F, 2)])}[kind]

    def case_of(msgs):
        return G.Case(op, path, msgs, R.STRING, val, what=kind + " at every phase")

    def cap(m):
        return E.slot_bound(op, path, len(m), len(val) if op == E.SET_OP else 0)

    c, caps = G.phase_layout(case_of, tested, cap)
    want = on_both_routes(knob, c, caps)
    assert all(r & 0xFF == E.OK for r, _ in want[1::2])


# -------------------------------------------------------------- count patch
def test_count_patch(knob):
    for c in G.count_cases():
        want = on_both_routes(knob, c)
        assert all(r & 0xFF in (E.OK, E.NOT_FOUND) for r, _ in want), c.what
    lst = G.count_cases()[0]
    assert lst.want()[-16][1][11:15] == b"\x80\x00\x00\x00"  # int32(0x7FFFFFFF + 1), the message with no filler


def test_smallest_messages(knob):
    for c in G.smallest_cases():
        on_both_routes(knob, c)
        on_both_routes(knob, c, [len(o) for _, o in c.want()])


def test_deep_values(knob):
    for c in G.deep_cases():
        want = on_both_routes(knob, c)
        assert all(r & 0xFF == E.OK for r, _ in want), c.what


# -------------------------------------------------------------------- slots
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("which", (0, 7, 8, 16, 21))
def test_slot_bounds_and_neighbours(knob, fuzz, route, which):
    """tight slots, guard bytes around every slot and unaligned slot bases (slotguard), the checker as the oracle"""
    from dynamicgo_amd import generic as X
    knob("edit_wave_min", route[1])
    knob("edit_lanes", route[2])
    c = fuzz[which]
    assert isinstance(c.values, bytes) or c.op == E.UNSET_OP or which == 0
    val = c.values if isinstance(c.values, bytes) else G.wstr(b"one value for all")
    by_msg = {m: E.edit(c.op, m, c.path, val, c.val_type) for m in c.msgs}
    pick = [m for m in c.msgs[:G.FUZZ_N] if by_msg[m][0] & 0xFF == E.OK][:20] + [m for m in c.msgs if by_msg[m][0] & 0xFF][:4]
    items = SG.items_for(pick, lambda m: by_msg[m], phases=(None, 5, 11))
    SG.assert_shares(items)
    d_val = None
    with plan_of(c) as plan:
        def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
            import torch
            nonlocal d_val
            if d_val is None and c.op == E.SET_OP:
                d_val = torch.from_numpy(np.frombuffer(val + b"\0" * 16, dtype=np.uint8).copy()).cuda()
            X.edit_device(plan, d_src, d_in, n, c.val_type, d_val, None, d_out, d_oo, d_ol, d_ret, val_len=len(val))

        spacer = b"\x00"
        sret, sout = E.edit(c.op, spacer, c.path, val, c.val_type)
        SG.check(launch, items, spacer, sout, "cuda", pending=False, spacer_ret=sret)


def test_one_byte_short(knob, fuzz):
    """DG_EDIT_E_OVERFLOW carries the size in aux and out_len and stores nothing; the neighbours, in exact-size
    slots on both sides, are whole"""
    for c in (fuzz[0], fuzz[8], fuzz[16], G.count_cases()[1]):
        ok = [i for i, (r, o) in enumerate(c.want()) if r & 0xFF == E.OK and o][:96]
        c = c.sub(ok)
        caps = [len(o) - (i % 3 == 1) for i, (_, o) in enumerate(c.want())]
        want = on_both_routes(knob, c, caps)
        assert [w[0] & 0xFF for w in want] == [E.E_OVERFLOW if i % 3 == 1 else E.OK for i in range(len(ok))]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_batch_sizes_agree_with_each_message_alone(knob, fuzz, n):
    """the checker's answer for a message does not depend on the batch, so neither may the device's"""
    for c in (fuzz[0], fuzz[11], fuzz[21]):
        idx = [(7 * k) % len(c.msgs) for k in range(n)]
        on_both_routes(knob, c.sub(idx))


# ------------------------------------------------- host entry and streams
def words(res):
    return [(r.status | (E.EXISTED if r.existed else 0) | r.aux << 32, r.raw) for r in res]


def test_host_entry(knob, fuzz):
    from dynamicgo_amd import generic as X
    names = {E.OK: None, E.NOT_FOUND: "ErrNotFound", E.E_READ: "ErrRead", E.E_TYPE: "ErrDismatchType"}
    for c in fuzz[::3]:
        for _, wm, lanes in ROUTES + (("between", 300, 4),):
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            if c.op == E.SET_OP:
                res = X.set_by_path_batch(c.msgs, G.paths_of(c.path), c.values, c.val_type)
            else:
                res = X.unset_by_path_batch(c.msgs, G.paths_of(c.path))
            same(words(res), c.want(), c, "host entry")
            assert [r.error for r in res] == [names[w & 0xFF] for w, _ in c.want()]
    assert X.set_by_path_batch([], [X.PathFieldId(1)], b"\0", R.BYTE) == []
    assert X.unset_by_path_batch([], [X.PathFieldId(1)]) == []
    for c in G.smallest_cases():
        with plan_of(c) as p:
            res = X.set_by_path_batch(c.msgs, p, c.values, c.val_type, root_type=c.root_type) if c.op == E.SET_OP else \
                X.unset_by_path_batch(c.msgs, p, root_type=c.root_type)
        same(words(res), c.want(), c, "host entry")


def test_host_entry_names_and_nomem(knob):
    """PathFieldName through the descriptor; a short output buffer is DG_E_NOMEM with *out_need, and the retry fits"""
    import t2jgen
    from dynamicgo_amd import _lib
    from dynamicgo_amd import generic as X
    td = t2jgen.all_types_desc()
    msgs = [G.field(R.STRING, 18, G.wstr(b"r")) + b"\x00"] * 5
    val = G.wstr(b"v" * 100)
    res = X.set_by_path_batch(msgs, [X.PathFieldName("str_f")], val, R.STRING, desc=td)
    want = [E.edit(E.SET_OP, m, [(F, 7)], val, R.STRING) for m in msgs]
    assert words(res) == want and all(len(o) == len(m) + 107 for m, (_, o) in zip(msgs, want))
    res = X.unset_by_path_batch(msgs, [X.PathFieldName("req_s")], desc=td)
    assert words(res) == [(E.word(E.OK, existed=True), b"\x00")] * 5
    with X.EditPlan([X.PathFieldId(7)], X.EDIT_SET) as p:
        L = _lib.lib()
        arena = np.frombuffer(b"".join(msgs), dtype=np.uint8)
        in_off = np.arange(6, dtype=np.uint64) * len(msgs[0])
        v = np.frombuffer(val, dtype=np.uint8)
        out_off, ret, need = np.zeros(6, dtype=np.uint64), np.zeros(5, dtype=np.uint64), C.c_uint64(0)
        total = sum(len(o) for _, o in want)
        for cap, rc_want in ((total - 1, -3), (total, 0)):
            out = np.zeros(total, dtype=np.uint8)
            rc = L.dg_edit_batch_host(p.ctx.h, p.h, R.STRUCT, arena.ctypes.data, in_off.ctypes.data, 5, R.STRING,
                                      v.ctypes.data, None, len(val), out.ctypes.data, cap, out_off.ctypes.data,
                                      ret.ctypes.data, C.byref(need))
            assert rc == rc_want and need.value == total
        assert out.tobytes() == b"".join(o for _, o in want) and list(ret) == [w for w, _ in want]


def test_side_stream_and_back_to_back(knob, fuzz):
    """edit_device on a side stream; then two edits back to back on one stream with no synchronisation between
    them, the second reading the first one's output: they share the context's record scratch in stream order"""
    import torch
    from dynamicgo_amd import generic as X
    side = torch.cuda.Stream()
    c = fuzz[0]
    for name, wm, lanes in ROUTES:
        knob("edit_wave_min", wm)
        knob("edit_lanes", lanes)
        with plan_of(c) as p:
            same(run_device(c, p, stream=side), c.want(), c, "side stream, " + name)
    # set field 7, then unset field 18 of the result
    msgs = [m for m, (r, _) in zip(c.msgs, c.want()) if r & 0xFF == E.OK][:128]
    val = G.wstr(b"first")
    first = [E.edit(E.SET_OP, m, [(F, 7)], val, R.STRING) for m in msgs]
    second = [E.edit(E.UNSET_OP, o, [(F, 18)]) for _, o in first]
    n = len(msgs)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(o) for _, o in first], out=slots[1:])  # exact: the second edit's input arena
    arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_in, d_mid_off = torch.from_numpy(in_off).cuda(), torch.from_numpy(slots).cuda()
    d_val = torch.from_numpy(np.frombuffer(val + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    with X.EditPlan([X.PathFieldId(7)], X.EDIT_SET) as p1, X.EditPlan([X.PathFieldId(18)], X.EDIT_UNSET) as p2:
        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            d_mid = torch.zeros(int(slots[n]) + 16, dtype=torch.uint8, device="cuda")
            d_out = torch.full((int(slots[n]) + 16,), FILL, dtype=torch.uint8, device="cuda")
            ol1, ol2 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            r1, r2 = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                X.edit_device(p1, arena, d_in, n, R.STRING, d_val, None, d_mid, d_mid_off, ol1, r1, val_len=len(val), stream=side)
                X.edit_device(p2, d_mid, d_mid_off, n, 0, None, None, d_out, d_mid_off, ol2, r2, stream=side)
            side.synchronize()
            assert r1.cpu().tolist() == [w for w, _ in first] and r2.cpu().tolist() == [w for w, _ in second]
            out, l2 = d_out.cpu().numpy(), ol2.cpu().numpy()
            for i in range(n):
                assert out[int(slots[i]):int(slots[i]) + int(l2[i])].tobytes() == second[i][1], (name, i)


# -------------------------------------------------------------- composition
def test_composition(knob, fuzz):
    from dynamicgo_amd import generic as X
    msgs = [m for m, (r, _) in zip(fuzz[0].msgs, fuzz[0].want()) if r & 0xFF == E.OK][:64]
    path, val = [X.PathFieldId(9), X.PathFieldId(2)], G.wstr(b"composed")
    once = X.set_by_path_batch(msgs, path, val, R.STRING)
    ok = [i for i, r in enumerate(once) if r.status == E.OK]
    assert len(ok) >= 16
    got = X.get_by_path_batch([once[i].raw for i in ok], [path])
    assert all(g[0].status == R.OK and g[0].raw == val for g in got)  # set then get
    twice = X.set_by_path_batch([once[i].raw for i in ok], path, val, R.STRING)
    assert [t.raw for t in twice] == [once[i].raw for i in ok] and all(t.existed for t in twice)  # set twice = set once
    gone = X.unset_by_path_batch([once[i].raw for i in ok], path)
    assert all(g.status == E.OK and g.existed for g in gone)
    back = X.set_by_path_batch([g.raw for g in gone], path, val, R.STRING)
    for b, g in zip(back, gone):  # unset then set: the front-insert form
        par = R.get_by_path(g.raw, [(F, 9)])
        assert not b.existed and b.raw == g.raw[:par.start] + G.field(R.STRING, 2, val) + g.raw[par.start:]


# ------------------------------------------------------ refusals and bounds
def test_create_refusals_and_slot_bound():
    from dynamicgo_amd import _lib
    from dynamicgo_amd import generic as X
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()
    for paths, text in (([[]], "empty path"), ([G.paths_of([(F, 1)]), G.paths_of([(F, 2)])], "2 paths")):
        h = C.c_void_p()
        blob = X.compile_paths(paths)
        assert L.dg_edit_create(ctx.h, blob, len(blob), X.EDIT_SET, C.byref(h)) == -6
        assert text in L.dg_last_error().decode()
    blob = bytearray(X.compile_paths([G.paths_of([(F, 1), (I, 2)])]))
    blob[0] ^= 1
    with pytest.raises(_lib.DGError):
        X.EditPlan(bytes(blob), X.EDIT_UNSET)
    for path in ([(F, 5)], [(F, 1), (I, 9)], [(S, b"abcde")], [(S, b"")], [(N, 3)], [(BK, b"12345678")]):
        for op in (E.SET_OP, E.UNSET_OP):
            with X.EditPlan(G.paths_of(path), op) as p:
                for ln, vl in ((0, 0), (100, 7), (1 << 20, 1 << 16)):
                    assert p.slot_bound(ln, vl) == E.slot_bound(op, path, ln, vl)
