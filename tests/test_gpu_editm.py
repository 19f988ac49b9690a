"""GPU: batched SetMany (dynamicgo_amd.generic over dg_editm_*) against the
pure-Python restatement of the reference in editmref.py. Every case runs on all
four routes of the splice (edit_wave_min 0: the wave route; a huge value: the
lane route with edit_lanes 1, 4 and 16), and the bytes, out_len and ret of every
message are compared exactly with the checker's. Every device run also checks
the memory contract: nothing stored in front of the first slot or behind the
last, nothing at or beyond out_len in a slot that succeeded, nothing at all in
the slot of a message that failed."""
import struct

import numpy as np
import pytest

import editgen as G
import editmgen as MG
import editmref as M
import editref as E
import slotguard as SG
import tgetref as R

pytestmark = pytest.mark.gpu

F, I, S, N, BK = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
LANE, WAVE = 1 << 40, 0
ROUTES = (("lane", LANE, 1), ("lane x4", LANE, 4), ("lane x16", LANE, 16), ("wave", WAVE, 1))
FILL, GUARD = 0xEE, 64


def plan_of(case):
    from dynamicgo_amd import generic as X
    return X.EditManyPlan(G.paths_of(case.parent), G.paths_of(case.steps), case.op)


def value_arena(case):
    """(val, val_off, val_lens) for dg_editm_batch_device: shared values back to back, or message-major"""
    k, n = case.k, len(case.msgs)
    if case.op != M.SET_OP:
        return None, None, [0] * k
    if case.shared:
        vs = [case.value(0, j) for j in range(k)]
        return np.frombuffer(b"".join(vs) + b"\0" * 16, dtype=np.uint8).copy(), None, [len(v) for v in vs]
    flat = [case.value(i, j) for i in range(n) for j in range(k)]
    off = np.zeros(n * k + 1, dtype=np.int64)
    np.cumsum([len(v) for v in flat], out=off[1:])
    lens = [max((len(case.value(i, j)) for i in range(n)), default=0) for j in range(k)]
    return np.frombuffer(b"".join(flat) + b"\0" * 16, dtype=np.uint8).copy(), off, lens


class Batch:
    """a case on the device: the uploads made once, launched and read back per route"""

    def __init__(self, case, caps=None, hint=True):
        import torch
        self.case, n = case, len(case.msgs)
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(m) for m in case.msgs], out=in_off[1:])
        if caps is None:
            caps = [(case.bound(i) + 15) & ~15 for i in range(n)]
        self.out_off = np.full(n + 1, GUARD, dtype=np.int64)
        np.cumsum(caps, out=self.out_off[1:])
        self.out_off[1:] += GUARD
        val, val_off, self.val_lens = value_arena(case)
        if not hint and val_off is not None:
            self.val_lens = [0] * case.k
        self.arena = torch.from_numpy(np.frombuffer(b"".join(case.msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        self.d_in, self.d_oo = torch.from_numpy(in_off).cuda(), torch.from_numpy(self.out_off).cuda()
        self.d_val = None if val is None else torch.from_numpy(val).cuda()
        self.d_vo = None if val_off is None else torch.from_numpy(val_off).cuda()
        self.ml = max((len(m) for m in case.msgs), default=0) if hint else 0
        self.n = n

    def fresh(self):
        import torch
        self.d_out = torch.full((int(self.out_off[self.n]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.d_ol = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device="cuda")
        self.d_ret = torch.full((max(self.n, 1),), -1, dtype=torch.int64, device="cuda")

    def launch(self, plan, stream=None):
        from dynamicgo_amd import generic as X
        c = self.case
        X.edit_many_device(plan, self.arena, self.d_in, self.n, c.val_types, self.d_val, self.d_vo, self.val_lens,
                           self.d_out, self.d_oo, self.d_ol, self.d_ret, root_type=c.root_type, stream=stream,
                           max_len=self.ml)

    def read(self):
        out, ol, ret = self.d_out.cpu().numpy(), self.d_ol.cpu().numpy().view(np.uint32), self.d_ret.cpu().numpy().view(np.uint64)
        n, out_off = self.n, self.out_off
        assert (out[:GUARD] == FILL).all() and (out[int(out_off[n]):] == FILL).all(), "a store outside the slots"
        res = []
        for i in range(n):
            a, e = int(out_off[i]), int(out_off[i + 1])
            r = int(ret[i])
            used = int(ol[i]) if r & 0xFF == M.OK else 0
            assert used <= e - a, i
            assert (out[a + used:e] == FILL).all(), "message %d (ret %x): a store at or beyond out_len, or by a failed message" % (i, r)
            res.append((r, out[a:a + used].tobytes()))
            assert int(ol[i]) == M.out_len(r, res[-1][1]), (i, hex(r), int(ol[i]))
        return res

    def run(self, plan, stream=None):
        import torch
        self.fresh()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        self.launch(plan, stream)
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        return self.read()


def same(got, want, case, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, %s, message %d (%r...): got %x / %d bytes, checker %x / %d bytes" % (
            case.what, what, i, case.msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))


def on_every_route(knob, case, caps=None, routes=ROUTES):
    want = case.want(caps)
    b = Batch(case, caps)
    with plan_of(case) as p:
        for name, wm, lanes in routes:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            same(b.run(p), want, case, name + " route")
    return want


@pytest.fixture(scope="module")
def fuzz():
    """the fuzz cases with the checker's answers, computed once"""
    cases = MG.fuzz_cases()
    for c in cases:
        c.want()
    return cases


# 1 ------------------------------------------------------------------- fuzz
def test_fuzz(knob, fuzz):
    sh = MG.shares(fuzz)
    for k in ("all replaced", "all inserted", "mixed", "dropped", "ErrNotFound", "ErrRead", "ErrDismatchType"):
        assert sh.get(k, 0) >= 0.05, (k, sh)
    assert {c.k for c in fuzz} >= {1, 2, 3, 5, 7}
    for c in fuzz:
        on_every_route(knob, c)


def test_fuzz_per_message_values_and_every_k(knob, fuzz):
    """the shared-value cases once more with every value given per message, and one list under K = 1..7"""
    for c in fuzz:
        if c.op == M.SET_OP and c.shared:
            on_every_route(knob, c.per_message())
    msgs = fuzz[0].msgs
    for k in range(1, 8):
        items = [((I, j if j % 2 else 1000 + j), G.wstr(b"k%d" % j * j), R.STRING) for j in range(k)]
        on_every_route(knob, MG.ManyCase(M.SET_OP, [(F, 19)], items, msgs, what="K = %d" % k))
        on_every_route(knob, MG.ManyCase(M.UNSET_OP, [], [((F, 18 + j),) for j in range(k)], msgs, what="K = %d" % k))


def test_default_route_and_hints(knob, fuzz):
    """the default knobs, with and without the length hints"""
    for c in fuzz[::4]:
        with plan_of(c) as p:
            same(Batch(c).run(p), c.want(), c, "default knobs")
            same(Batch(c, hint=False).run(p), c.want(), c, "default knobs, no hints")


# 2, 3, 4, 5 --------------------------------------------------------- sweeps
def test_adjacency(knob):
    for c in MG.adjacency_cases():
        want = on_every_route(knob, c)
        assert all(r & 0xFF == M.OK for r, _ in want), c.what
        on_every_route(knob, c, [len(o) for _, o in want])  # exact slots back to back: unaligned bases


def test_phase(knob):
    c = MG.phase_case()
    want = on_every_route(knob, c)
    assert all(r == M.word(M.OK, mask=7) for r, _ in want)
    assert {len(o) % 16 for _, o in want} == set(range(16)) and any(len(o) > 1024 for _, o in want)
    assert {R.get_by_path(m, [(F, 2)]).start % 16 for m in c.msgs} == set(range(16))
    on_every_route(knob, c, [len(o) for _, o in want])


def test_many_items_in_one_unit(knob):
    for c in MG.unit_cases():
        want = on_every_route(knob, c)
        on_every_route(knob, c, [len(o) for _, o in want])


def test_count_patch(knob):
    cases = MG.count_cases()
    for c in cases:
        want = on_every_route(knob, c)
        assert all(r & 0xFF == M.OK for r, _ in want), c.what
    two = cases[0]  # 0x7FFFFFFF + 2 wraps; the message with no filler: the count at 11
    wrap = [o for m, (_, o) in zip(two.msgs, two.want()) if m[11:15] == b"\x7f\xff\xff\xff"]
    assert wrap and wrap[0][11:15] == b"\x80\x00\x00\x01"


# 6 ------------------------------------------------------ failure atomicity
def test_failure_atomicity(knob):
    cases = MG.failure_cases()
    for bad in range(7):
        want = on_every_route(knob, cases[bad])
        assert all(w == (M.word(M.E_TYPE, R.I32, item=bad), b"") for w in want)
    names = {c.what: on_every_route(knob, c) for c in cases[7:]}
    assert names["STRKEY and BINKEY on one entry"][0][0] & 0xFF == M.E_SAME
    assert names["drop one entry twice"][0][0] & 0xFF == M.E_SAME
    assert names["an existing index twice"][0][0] == M.word(M.E_SAME, item=2)
    assert names["a missing index twice"][0][0] == M.word(M.OK)
    m = cases[0].msgs[0]
    assert names["unset below a missed parent"] == [(M.word(M.OK), m)]


# 7 ------------------------------------------------------------------ slots
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("which", (1, 2, 9, 17, 24))
def test_slot_bounds_and_neighbours(knob, fuzz, route, which):
    """tight slots, guard bytes around every slot and unaligned slot bases (slotguard), the checker as the oracle"""
    from dynamicgo_amd import generic as X
    knob("edit_wave_min", route[1])
    knob("edit_lanes", route[2])
    c = fuzz[which]
    items = [(st, v if isinstance(v, bytes) else G.wstr(b"one value for all"), t) for st, v, t in c.items]
    by_msg = {m: M.edit_many(c.op, m, c.parent, items, c.root_type) for m in c.msgs}
    pick = [m for m in c.msgs[:MG.FUZZ_N] if by_msg[m][0] & 0xFF == M.OK][:20] + [m for m in c.msgs if by_msg[m][0] & 0xFF][:4]
    sitems = SG.items_for(pick, lambda m: by_msg[m], phases=(None, 5, 11))
    SG.assert_shares(sitems)
    vals = [it[1] for it in items]
    d_val = None
    with plan_of(c) as plan:
        def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
            import torch
            nonlocal d_val
            if d_val is None and c.op == M.SET_OP:
                d_val = torch.from_numpy(np.frombuffer(b"".join(vals) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
            X.edit_many_device(plan, d_src, d_in, n, c.val_types, d_val, None, [len(v) for v in vals], d_out, d_oo, d_ol, d_ret)

        spacer = b"\x00"
        sret, sout = M.edit_many(c.op, spacer, c.parent, items, c.root_type)
        SG.check(launch, sitems, spacer, sout, "cuda", pending=False, spacer_ret=sret)


def test_exact_slots_and_one_byte_short(knob, fuzz):
    """exact-size slots pass; one byte short is DG_EDIT_E_OVERFLOW with the needed size in aux and out_len and no
    byte stored, the neighbours in exact-size slots on both sides whole"""
    for c in (fuzz[1], fuzz[2], fuzz[14], MG.count_cases()[1]):
        ok = [i for i, (r, o) in enumerate(c.want()) if r & 0xFF == M.OK and o][:96]
        c = c.sub(ok)
        same_caps = [len(o) for _, o in c.want()]
        assert on_every_route(knob, c, same_caps) == c.want()
        caps = [len(o) - (i % 3 == 1) for i, (_, o) in enumerate(c.want())]
        want = on_every_route(knob, c, caps)
        assert [w[0] & 0xFF for w in want] == [M.E_OVERFLOW if i % 3 == 1 else M.OK for i in range(len(ok))]
        assert all(w[0] == M.overflow(len(o)) for i, (w, (_, o)) in enumerate(zip(want, c.want())) if i % 3 == 1)


# 8 ------------------------------------------------------------ batch sizes
@pytest.mark.parametrize("n", (1, 3, 63, 64, 65, 255, 257))
def test_batch_sizes_agree_with_each_message_alone(knob, fuzz, n):
    for c in (fuzz[1], fuzz[14], fuzz[24]):
        idx = [(7 * k) % len(c.msgs) for k in range(n)]
        on_every_route(knob, c.sub(idx))


def test_wave_stride_loop_over_the_smallest_messages(knob):
    """2.5 grids of the wave route (8 blocks a CU, 4 messages a block) of one-byte and empty messages, and of
    every lane route: every wave takes its third message only where one is left"""
    import torch
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    n = n_cu * 8 * 4 * 5 // 2 + 3
    kinds = [b"\x00", b"", G.field(R.BOOL, 11, b"\x01") + b"\x00"]
    items = [((F, 10 + j), bytes([j & 1]), R.BOOL) for j in range(3)]
    one = [M.edit_many(M.SET_OP, m, [], items) for m in kinds]
    c = MG.ManyCase(M.SET_OP, [], items, [kinds[i % 3] for i in range(n)], what="the stride loop")
    c._want = [one[i % 3] for i in range(n)]
    on_every_route(knob, c)


def test_each_kernel_leaves_the_others_messages_alone(knob, fuzz):
    """edit_wave_min = 300 over a batch with outputs on both sides of it"""
    ph = MG.phase_case()
    drop = MG.ManyCase(M.UNSET_OP, [], [((F, 3),), ((F, 4),)], ph.msgs, what="drops on both sides of 300")
    for c in (ph, drop, MG.ManyCase(M.SET_OP, [], fuzz[4].items, fuzz[4].msgs + ph.msgs[:40], what="inserts on both sides of 300")):
        lens = [len(o) for r, o in c.want() if r & 0xFF == M.OK]
        assert min(lens) < 300 <= max(lens)
        on_every_route(knob, c, routes=(("both, 1 lane", 300, 1), ("both, 4 lanes", 300, 4), ("both, 16 lanes", 300, 16)))


# 9 ------------------------------------------------------- the single edit
def test_one_item_equals_the_single_edit_kernel(knob):
    """dg_edit_batch_device is dg_editm_batch_device with K = 1, so this compares one kernel reached through two
    entries: it pins the single edit's argument mapping (val_type, val_len, the value offsets, the path set of
    dg_edit_create) on every route, word for word, byte for byte. Both entries are judged by both independent
    restatements, the many-edit checker (editmref) and the single-edit checker (editref), not by each other."""
    import test_gpu_edit as TE
    for c in G.fuzz_cases()[::3]:
        mc = MG.ManyCase(c.op, c.path[:-1], [(c.path[-1], c.values, c.val_type)], c.msgs, c.root_type, c.what)
        with TE.plan_of(c) as p1, plan_of(mc) as pm:
            for name, wm, lanes in ROUTES:
                knob("edit_wave_min", wm)
                knob("edit_lanes", lanes)
                single = TE.run_device(c, p1)
                same(Batch(mc).run(pm), single, mc, "against dg_edit, " + name)
                same(single, mc.want(), mc, "dg_edit against the many-edit checker, " + name)
                same(single, c.want(), c, "dg_edit against the single-edit checker, " + name)


def test_four_items_equal_four_chained_single_edits(knob, fuzz):
    """K = 4 against four dg_edit calls, each on the previous one's output: the found items first (from the back
    of the message), then the missing ones in reverse item order"""
    from dynamicgo_amd import generic as X
    items = [((F, 18), G.wstr(b"replaced"), R.STRING), ((F, 901), struct.pack(">i", 1), R.I32),
             ((F, 22), struct.pack(">d", 2.0), R.DOUBLE), ((F, 902), G.wstr(b"inserted"), R.STRING)]
    msgs = [m for m in fuzz[0].msgs[:MG.FUZZ_N] if all(R.get_by_path(m, [(F, k)]).status == R.OK for k in (18, 20, 21, 22))][:64]
    assert len(msgs) >= 32
    c = MG.ManyCase(M.SET_OP, [], items, msgs)
    want = on_every_route(knob, c)
    assert all(r == M.word(M.OK, mask=5) for r, _ in want)
    found = sorted((items[0], items[2]), key=lambda it: -R.get_by_path(msgs[0], [it[0]]).start)
    cur = msgs
    for st, v, t in found + [items[3], items[1]]:
        res = X.set_by_path_batch(cur, G.paths_of([st]), v, t)
        assert all(r.status == E.OK for r in res)
        cur = [r.raw for r in res]
    # fields 18 and 22 stand in the same order in every message of this generator, so one order serves all
    assert cur == [o for _, o in want]
    drop = MG.ManyCase(M.UNSET_OP, [], [((F, k),) for k in (22, 18, 21, 20)], msgs)
    want = on_every_route(knob, drop)
    cur = msgs
    for k in sorted((22, 18, 21, 20), key=lambda k: -R.get_by_path(msgs[0], [(F, k)]).start):
        cur = [r.raw for r in X.unset_by_path_batch(cur, G.paths_of([(F, k)]))]
    assert cur == [o for _, o in want] and all(r == M.word(M.OK, mask=15) for r, _ in want)


# 10 ------------------------------------------------ host entry and streams
def words(res):
    return [(r.status | sum(1 << (8 + j) for j, x in enumerate(r.existed) if x) | r.item << 16 | r.aux << 32, r.raw) for r in res]


def test_host_entry(knob, fuzz):
    from dynamicgo_amd import generic as X
    names = {M.OK: None, M.NOT_FOUND: "ErrNotFound", M.E_READ: "ErrRead", M.E_TYPE: "ErrDismatchType", M.E_SAME: "ErrSame"}
    for c in fuzz[::3] + MG.failure_cases()[6:] + MG.unit_cases()[:4]:
        for _, wm, lanes in ROUTES + (("between", 300, 4),):
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            parent, steps = G.paths_of(c.parent), G.paths_of(c.steps)
            if c.op == M.SET_OP:
                res = X.set_many_batch(c.msgs, parent, [(s, v, t) for s, (_, v, t) in zip(steps, c.items)], root_type=c.root_type)
            else:
                res = X.unset_many_batch(c.msgs, parent, steps, root_type=c.root_type)
            same(words(res), c.want(), c, "host entry")
            assert [r.error for r in res] == [names[w & 0xFF] for w, _ in c.want()]
            assert [r.existed for r in res] == [M.existed_of(w, c.k) if w & 0xFF == M.OK else (False,) * c.k for w, _ in c.want()]
    assert X.set_many_batch([], [], [(X.PathFieldId(1), b"\0", R.BYTE)]) == []
    assert X.unset_many_batch([], [], [X.PathFieldId(1)]) == []


def test_host_entry_names_and_slot_bound():
    """PathFieldName through the descriptor, parent and last steps; dg_editm_slot_bound is the checker's"""
    import t2jgen
    from dynamicgo_amd import generic as X
    td = t2jgen.all_types_desc()
    msgs = [G.field(R.STRUCT, 21, G.field(R.I64, 1, b"\0" * 8) + b"\x00") + b"\x00"] * 3
    v = G.wstr(b"bee")
    res = X.set_many_batch(msgs, [X.PathFieldName("def_st")], [(X.PathFieldName("b"), v, R.STRING),
                                                               (X.PathFieldName("a"), b"\1" * 8, R.I64)], desc=td)
    want = [M.edit_many(M.SET_OP, m, [(F, 21)], [((F, 2), v, R.STRING), ((F, 1), b"\1" * 8, R.I64)]) for m in msgs]
    assert words(res) == want and res[0].existed == (False, True)
    for parent, steps in (([], [(F, 5), (F, 6)]), ([(F, 1)], [(I, 9)] * 7), ([], [(S, b"abcde"), (N, 3), (BK, b"12345678"), (S, b"")])):
        for op in (M.SET_OP, M.UNSET_OP):
            with X.EditManyPlan(G.paths_of(parent), G.paths_of(steps), op) as p:
                for ln, vl in ((0, 0), (100, 7), (1 << 20, 1 << 16)):
                    items = [(st, b"", 0) for st in steps]
                    assert p.slot_bound(ln, vl) == M.slot_bound(op, items, ln) + (vl if op == M.SET_OP else 0)


def test_streams(knob, fuzz):
    """a side stream; two unsynchronised many-edits back to back on one stream, the second reading the first
    one's output (they share the context's record scratch in stream order); a many-edit on one stream against a
    GetByPath on another (they share the lookup's workspace)"""
    import torch
    from dynamicgo_amd import generic as X
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    c = fuzz[1]
    b = Batch(c)
    with plan_of(c) as p:
        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            same(b.run(p, stream=side), c.want(), c, "side stream, " + name)
    # set fields 18 and 901, then unset fields 22 and 901 of the result
    msgs = [m for m in c.msgs[:MG.FUZZ_N] if R.get_by_path(m, [(F, 22)]).status == R.OK][:96]  # the unmutated ones
    assert len(msgs) >= 32
    it1 = [((F, 18), G.wstr(b"first"), R.STRING), ((F, 901), struct.pack(">i", 9), R.I32)]
    first = [M.edit_many(M.SET_OP, m, [], it1) for m in msgs]
    second = [M.edit_many(M.UNSET_OP, o, [], [((F, 22), b"", 0), ((F, 901), b"", 0)]) for _, o in first]
    assert all(r & 0xFF == M.OK for r, _ in first + second)
    n = len(msgs)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(o) for _, o in first], out=slots[1:])  # exact: the second edit's input arena
    arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_in, d_mid_off = torch.from_numpy(in_off).cuda(), torch.from_numpy(slots).cuda()
    vals = b"".join(v for _, v, _ in it1)
    d_val = torch.from_numpy(np.frombuffer(vals + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    paths = [G.paths_of([(F, 18)]), G.paths_of([(F, 22)])]
    got_want = [[R.get_by_path(m, [(F, 18)]), R.get_by_path(m, [(F, 22)])] for m in msgs]
    with X.EditManyPlan([], G.paths_of([(F, 18), (F, 901)]), X.EDIT_SET) as p1, \
            X.EditManyPlan([], G.paths_of([(F, 22), (F, 901)]), X.EDIT_UNSET) as p2, X.PathSet(paths) as ps:
        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            d_mid = torch.zeros(int(slots[n]) + 16, dtype=torch.uint8, device="cuda")
            d_out = torch.full((int(slots[n]) + 16,), FILL, dtype=torch.uint8, device="cuda")
            ol1, ol2 = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
            r1, r2 = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
            rec = torch.zeros((n, 2, 4), dtype=torch.int32, device="cuda")
            side.wait_stream(torch.cuda.current_stream())
            other.wait_stream(torch.cuda.current_stream())
            X.edit_many_device(p1, arena, d_in, n, [R.STRING, R.I32], d_val, None, [len(v) for _, v, _ in it1], d_mid,
                               d_mid_off, ol1, r1, stream=side)
            X.get_by_path_device(ps, arena, d_in, n, rec, stream=other)
            X.edit_many_device(p2, d_mid, d_mid_off, n, None, None, None, None, d_out, d_mid_off, ol2, r2, stream=side)
            side.synchronize()
            other.synchronize()
            assert r1.cpu().tolist() == [w for w, _ in first] and r2.cpu().tolist() == [w for w, _ in second]
            out, l2 = d_out.cpu().numpy(), ol2.cpu().numpy()
            for i in range(n):
                assert out[int(slots[i]):int(slots[i]) + int(l2[i])].tobytes() == second[i][1], (name, i)
            got = rec.cpu().numpy().view(X.REC_DTYPE).reshape(n, 2)
            for i in range(n):
                for k in range(2):
                    assert (int(got[i, k]["status"]), int(got[i, k]["start"]), int(got[i, k]["end"])) == \
                        (got_want[i][k].status, got_want[i][k].start, got_want[i][k].end), (name, i, k)
