"""GPU: what the batch size and the stream, not the message, decide in the cut
(batched MarshalTo) and the edit (batched SetByPath / UnsetByPath): the wave
kernels' stride loops over a queue or a batch longer than their grid
(cut_kern.hip, editm_kern.hip; the grids are set in cut_host.hip and, for
editm_host.hip, in host_internal.h), launches of one context with no synchronisation between them on
one stream and on several (the cut queue's two counters, the events that order
the streams), the queue and the record scratch growing while the launch before
may still use the old ones, single edits and a many-edit on two streams, which
share that record scratch, and an edit interleaved with a GetByPath, whose
scratch its lookup shares. Every message's ret, out_len and bytes are compared
with the checkers' (cutref.py, editref.py, editmref.py, tgetref.py); so are the guard bytes
around the slots and the fill behind every out_len.

The big batches cycle through a few dozen distinct short messages, a number
coprime to the grid, so that the messages a wave meets on its trips differ; the
checker runs once per distinct message."""
import math
import random
import struct

import numpy as np
import pytest

import cutgen as CG
import cutref as CR
import descgen
import editgen as EG
import editmgen as MG
import editmref as M
import editref as E
import slotguard as SG
import t2jgen
import tgetref as R
from test_gpu_tget import expect as tget_expect, to_paths
from test_gpu_tget_deep import Outputs, Upload, launch as tget_launch

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, SG.GUARD
F = R.FIELD
# the wave kernels' grids: min(ceil(n / WAVES), factor * CU) blocks of WAVES waves
CUT_GRID_FACTOR = 4   # cut_host.hip, cut_launch: `(uint64_t)c->n_cu * 4`
EDIT_GRID_FACTOR = 8  # host_internal.h, launch_splice_routes (edit_launch's): `(uint64_t)c->n_cu * 8`
DISTINCT = 61


def grid_waves(header, name, factor):
    """the waves of a full grid: the messages one trip of the stride loop takes"""
    import torch
    return descgen.kernel_const(header, name) * factor * torch.cuda.get_device_properties(0).multi_processor_count


class Batch:
    """n messages drawn from `items` by `order`, uploaded, with slots of caps[item] bytes back to back behind a
    guard, everything pre-filled. verify() compares the whole output with the image the checker's answers give."""

    def __init__(self, items, order, caps):
        import torch
        self.items, self.order, self.n = items, np.asarray(order, dtype=np.int64), len(order)
        self.caps = np.asarray(caps, dtype=np.int64)
        lens = np.array([len(m) for m in items], dtype=np.int64)
        self.in_off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(lens[self.order], out=self.in_off[1:])
        self.out_off = np.full(self.n + 1, GUARD, dtype=np.int64)
        np.cumsum(self.caps[self.order], out=self.out_off[1:])
        self.out_off[1:] += GUARD
        self.max_len = int(lens[self.order].max()) if self.n else 0
        arena = b"".join([items[k] for k in self.order]) + b"\xAA" * 16
        assert len(arena) < 2 << 20
        self.arena = torch.from_numpy(np.frombuffer(arena, dtype=np.uint8).copy()).cuda()
        self.d_in, self.d_oo = torch.from_numpy(self.in_off).cuda(), torch.from_numpy(self.out_off).cuda()
        self.d_out = torch.full((int(self.out_off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.d_ol = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.d_ret = torch.full((self.n,), -1, dtype=torch.int64, device="cuda")

    def verify(self, want, out_len, failed_slots_stay_empty, what):
        """want[item] = (ret, out); out_len(ret, out) -> the out_len the device stores. A failed cut may leave bytes
        in its own slot (the lane route's, before it declined); a failed edit stores nothing at all."""
        out, ol = self.d_out.cpu().numpy(), self.d_ol.cpu().numpy().view(np.uint32)
        ret = self.d_ret.cpu().numpy().view(np.uint64)
        exp_ret = np.array([w[0] for w in want], dtype=np.uint64)[self.order]
        exp_ol = np.array([out_len(*w) for w in want], dtype=np.uint32)[self.order]
        bad = np.flatnonzero((ret != exp_ret) | (ol != exp_ol))
        assert bad.size == 0, "%s: %d of %d messages differ, first %d (item %d, %r...): ret %x / out_len %d, checker %x / %d" % (
            what, bad.size, self.n, bad[0], self.order[bad[0]], self.items[self.order[bad[0]]][:24], ret[bad[0]],
            ol[bad[0]], exp_ret[bad[0]], exp_ol[bad[0]])
        imgs, checked = [], []
        for (r, o), cap in zip(want, self.caps):
            img = np.full(cap, FILL, dtype=np.uint8)
            if r & 0xFF == 0:
                img[:len(o)] = np.frombuffer(o, dtype=np.uint8)
            imgs.append(img)
            checked.append(np.full(cap, failed_slots_stay_empty or r & 0xFF == 0, dtype=bool))
        guard = np.full(GUARD, FILL, dtype=np.uint8)
        exp = np.concatenate([guard] + [imgs[k] for k in self.order] + [guard])
        chk = np.concatenate([guard != 0] + [checked[k] for k in self.order] + [guard != 0])
        bad = np.flatnonzero((out != exp) & chk)
        if bad.size:
            i = int(np.searchsorted(self.out_off, bad[0], side="right")) - 1
            assert False, "%s: byte %d of the output differs, %s" % (
                what, bad[0], "in a guard" if not 0 <= i < self.n else "%d bytes into the slot of message %d (item %d)" % (
                    bad[0] - self.out_off[i], i, self.order[i]))


def cut_launch(plan, b, opts=0, stream=None):
    from dynamicgo_amd import generic as X
    X.marshal_to_device(plan, b.arena, b.d_in, b.n, b.d_out, b.d_oo, b.d_ol, b.d_ret, opts, stream=stream, max_len=b.max_len)


def cut_out_len(ret, out):
    return ret >> 32 if ret & 0xFF == CR.E_OVERFLOW else len(out) if ret == 0 else 0


def cut_want(items, pair, opts, memo={}):
    """the checker, once per distinct message"""
    frm, to = pair
    for m in items:
        if (m, id(to), opts) not in memo:
            memo[m, id(to), opts] = CR.marshal_to(m, frm, to, opts)
    return [memo[m, id(to), opts] for m in items]


def cut_caps(items, want):
    """a slot that takes the checker's output of a flat-enough message: its length, the literals and a margin"""
    return [(max(len(m), len(o)) + 15 & ~15) + 16 for m, (_, o) in zip(items, want)]


# ------------------------------------------------------------ cut: messages
REQ_S = b"\x0b\x00\x0b\x00\x00\x00\x01r"


def wide_chain(kinds, val, tag=True, req=True):
    """A Wide message (cutgen.pair): node (field 15) = a chain of Nodes, one nested level per letter of `kinds`, the
    innermost with val and, with `tag`, a tag (dropped); then req_s. It opens 2 + the chain's containers."""
    head = b"".join(b"\x0c\x00\x02" if k == "S" else b"\x0f\x00\x03\x0c\x00\x00\x00\x01" for k in kinds)
    node = head + b"\x08\x00\x01" + struct.pack(">i", val) + (b"\x0b\x00\x04\x00\x00\x00\x02hi" if tag else b"") + \
        b"\x00" * (len(kinds) + 1)
    return b"\x0c\x00\x0f" + node + (REQ_S if req else b"") + b"\x00"


def cut_items(rng):
    """61 distinct messages of at most 64 bytes under cutgen.pair(): node chains of 1 to 9 containers, some cut
    short, one that loses nothing, and ones that fail with E_REQUIRED and E_TYPE"""
    items = [REQ_S + b"\x00",                                  # one container; cut to itself
             wide_chain("SS", 5, tag=False),                   # nothing dropped either
             b"", b"\x00", wide_chain("S", 1, req=False),      # E_READ, E_REQUIRED twice
             b"\x0b\x00\x01\x00\x00\x00\x00" + REQ_S + b"\x00",  # s_drop as a string: E_TYPE
             wide_chain("L", 2)[:-13] + b"\x0b\x00\x0f\x00\x00\x00\x00" + REQ_S + b"\x00"]  # node as a string behind a good one
    deep = wide_chain("SSSSSSS", 3)
    items += [deep[:k] for k in (5, 30, len(deep) - 1)]        # E_READ at three depths
    val = 100
    while len(items) < DISTINCT:
        for c in range(1, 9):                                   # containers of the chain itself: 2..9 with the root
            for kinds in CG.chains_of(c, rng, 2):
                items.append(wide_chain(kinds, val))
                val += 1
    items = items[:DISTINCT]
    assert len(set(items)) == DISTINCT and max(map(len, items)) <= 64
    return items


# ------------------------------------------------- cut: longer than the grid
def test_cut_queue_longer_than_the_grid(knob):
    """every message queued (cut_wave_min = 0): 2.5 grids of waves and 3, so the stride loop of cut_wave_kernel runs a
    third trip in part of the grid, each wave over the frames its earlier messages left in LDS"""
    from dynamicgo_amd import generic as X
    grid = grid_waves("cut_device.h", "CUT_WAVES", CUT_GRID_FACTOR)
    n = 2 * grid + grid // 2 + 3
    assert n > 2 * grid and math.gcd(DISTINCT, grid) == 1  # messages g and g + grid differ
    items = cut_items(random.Random(41))
    assert {n_frames(m) for m in items} >= set(range(1, 10))
    order = np.arange(n) % DISTINCT
    knob("cut_wave_min", 0)
    with X.CutPlan(*CG.pair()) as plan:
        for opts in (0, CR.WRITE_DEFAULT):
            want = cut_want(items, CG.pair(), opts)
            assert {r & 0xFF for r, _ in want} == {CR.OK, CR.E_READ, CR.E_TYPE, CR.E_REQUIRED}
            assert sum(r == 0 for r, _ in want) * 2 > DISTINCT
            b = Batch(items, order, cut_caps(items, want))
            cut_launch(plan, b, opts)
            b.verify(want, cut_out_len, False, "every message queued, opts %d" % opts)


def deep_and_shallow(rng):
    """(deep, shallow): distinct Wide messages that open 9 or 10 cut containers, which the lane route's 8 frames
    decline (one of them cut short behind its tenth: E_READ on the wave route), and ones of at most 8, some failing"""
    deep = [wide_chain(k, 1000 + j) for j, k in enumerate(CG.chains_of(8, rng, 8) + CG.chains_of(9, rng, 8))]
    deep.append(wide_chain("S" * 8, 7)[:40])
    shallow = [m for m in cut_items(rng) if n_frames(m) <= CG.LDS_FRAMES]
    assert max(map(len, deep)) <= 64
    return deep, shallow


def n_frames(msg):
    """the cut containers a Wide chain message opens before it ends, read off its bytes"""
    c, p = 1, 0
    if msg[:3] != b"\x0c\x00\x0f":
        return c
    c, p = 2, 3
    while True:
        if msg[p:p + 3] == b"\x0c\x00\x02" and len(msg) >= p + 3:
            c, p = c + 1, p + 3
        elif msg[p:p + 8] == b"\x0f\x00\x03\x0c\x00\x00\x00\x01":
            c, p = c + 2, p + 8
        else:
            return c


def test_cut_partly_queued_longer_than_the_grid(knob):
    """the default cut_wave_min: the lane route takes the shallow messages and queues those that open more than its
    8 frames, more than one grid of waves of them, in whatever order its atomics give"""
    from dynamicgo_amd import generic as X
    grid = grid_waves("cut_device.h", "CUT_WAVES", CUT_GRID_FACTOR)
    deep, shallow = deep_and_shallow(random.Random(42))
    assert all(n_frames(m) > CG.LDS_FRAMES for m in deep) and all(n_frames(m) <= CG.LDS_FRAMES for m in shallow)
    assert {n_frames(m) for m in deep[:-1]} == {9, 10} and len(set(deep)) == len(deep) and len(set(shallow)) == len(shallow)
    items = deep + shallow
    n = 3 * grid
    i = np.arange(n)
    is_deep = (i * 7) % 5 < 2  # two in five, spread among the shallow ones
    order = np.where(is_deep, i % len(deep), len(deep) + i % len(shallow))
    assert int(is_deep.sum()) > grid and math.gcd(len(deep), grid) == 1
    assert X.default_context().get_knob("cut_wave_min") > 64  # no message is queued for its length
    with X.CutPlan(*CG.pair()) as plan:
        for opts in (0, CR.WRITE_DEFAULT | CR.DISALLOW_UNKNOWN):
            want = cut_want(items, CG.pair(), opts)
            assert sum(r == 0 for r, _ in want[:len(deep)]) >= len(deep) - 1
            b = Batch(items, order, cut_caps(items, want))
            cut_launch(plan, b, opts)
            b.verify(want, cut_out_len, False, "two messages in five queued, opts %d" % opts)


# ---------------------------------------------------- edit: the wave route
def edit_items(rng):
    """61 distinct messages of at most 64 bytes for an edit of inner.b (field 9, field 2): b present, absent, inner
    absent, cut short, the smallest messages, and short messages of t2jgen.all_types_desc() with mutated copies"""
    f, w = EG.field, EG.wstr
    items = [b"", b"\x00"]
    for j in range(14):
        inner = f(R.I64, 1, struct.pack(">q", j)) + (f(R.STRING, 2, w(b"b" * j)) if j % 3 else b"") + b"\x00"
        m = (f(R.I32, 4, struct.pack(">i", j)) if j % 2 else b"") + f(R.STRUCT, 9, inner) + f(R.STRING, 18, w(b"r" * (j % 5))) + b"\x00"
        items.append(m)
        if j % 4 == 1:
            items.append(m[:len(m) - 9 - j % 5])  # ends inside inner
    items += [f(R.STRING, 18, w(b"no inner %d" % j)) + b"\x00" for j in range(3)]
    items.append(f(R.STRING, 9, w(b"inner is a string")) + b"\x00")
    td = t2jgen.all_types_desc()
    while len(items) < DISTINCT:
        m = t2jgen.gen_thrift(rng, td, keep_p=0.08)
        for m in (m, t2jgen.mutate(rng, m)):
            if len(m) <= 64 and m not in items and len(items) < DISTINCT:
                items.append(m)
    assert len(set(items)) == DISTINCT and max(map(len, items)) <= 64
    return items


EDIT_PATH = [(F, 9), (F, 2)]
EDIT_VALUES = [EG.wstr(b"v" * k) for k in (0, 1, 5, 12, 16, 33)] + [EG.wstr(b"long " * 64)]  # 7 values, one of 324 bytes


class EditBatch(Batch):
    """message i = items[i % 61] with value i % 7 (a SET; one value per message): 427 distinct (message, value) pairs"""

    def __init__(self, msgs, op, n):
        import torch
        self.op = op
        self.pairs = [(k % len(msgs), k % len(EDIT_VALUES)) for k in range(len(msgs) * len(EDIT_VALUES))]
        items = [msgs[a] for a, _ in self.pairs]
        self.vals = [EDIT_VALUES[v] if op == E.SET_OP else b"" for _, v in self.pairs]
        caps = [(E.slot_bound(op, EDIT_PATH, len(m), len(v)) + 15) & ~15 for m, v in zip(items, self.vals)]
        super().__init__(items, np.arange(n) % len(self.pairs), caps)
        self.d_val = self.d_vo = None
        self.val_len = 0
        if op == E.SET_OP:
            vlen = np.array([len(v) for v in self.vals], dtype=np.int64)
            vo = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(vlen[self.order], out=vo[1:])
            arena = b"".join([self.vals[k] for k in self.order]) + b"\0" * 16
            assert len(arena) + int(self.in_off[-1]) < 3 << 20
            self.d_val = torch.from_numpy(np.frombuffer(arena, dtype=np.uint8).copy()).cuda()
            self.d_vo = torch.from_numpy(vo).cuda()
            self.val_len = int(vlen.max())

    def want(self, memo={}):
        for key in zip(self.items, self.vals):
            if (self.op,) + key not in memo:
                memo[(self.op,) + key] = E.edit(self.op, key[0], EDIT_PATH, key[1], R.STRING)
        return [memo[(self.op,) + key] for key in zip(self.items, self.vals)]

    def launch(self, plan, stream=None):
        from dynamicgo_amd import generic as X
        X.edit_device(plan, self.arena, self.d_in, self.n, R.STRING, self.d_val, self.d_vo, self.d_out, self.d_oo, self.d_ol,
                      self.d_ret, val_len=self.val_len, stream=stream, max_len=self.max_len)


def edit_plan(op, ctx=None):
    from dynamicgo_amd import generic as X
    return X.EditPlan(EG.paths_of(EDIT_PATH), op, ctx=ctx)


def edit_outcomes(b):
    return {E.outcome(b.op, r) for r, _ in b.want()}


def test_edit_wave_route_over_a_batch_longer_than_the_grid(knob):
    """edit_wave_min = 0: the wave route alone, 2.5 grids of waves and 3 messages; then edit_wave_min = 300 over the
    same SET batch: the outputs of the 324-byte value go to the wave route, every other one to the lane route, and
    each kernel leaves the other's messages alone"""
    grid = grid_waves("edit_device.h", "ED_WAVES", EDIT_GRID_FACTOR)
    n = 2 * grid + grid // 2 + 3
    msgs = edit_items(random.Random(43))
    assert n > 2 * grid and math.gcd(DISTINCT * len(EDIT_VALUES), grid) == 1
    for op in (E.SET_OP, E.UNSET_OP):
        b = EditBatch(msgs, op, n)
        want = b.want()
        if op == E.SET_OP:
            assert edit_outcomes(b) >= {"replaced", "inserted", "ErrNotFound", "ErrRead"}
            long_ = sum(len(o) >= 300 for _, o in want)
            assert 0 < long_ < len(want) // 4
        else:
            assert edit_outcomes(b) >= {"deleted", "ErrRead"} and edit_outcomes(b) & {"ErrNotFound", "untouched"}
        with edit_plan(op) as plan:
            for wave_min in (0, 300) if op == E.SET_OP else (0,):
                knob("edit_wave_min", wave_min)
                knob("edit_lanes", 4)
                b.d_out.fill_(FILL)
                b.d_ol.fill_(-1)
                b.d_ret.fill_(-1)
                b.launch(plan)
                b.verify(want, E.out_len, True, "%s, edit_wave_min %d" % ("set" if op == E.SET_OP else "unset", wave_min))


# ------------------------------------------------ cut: launches back to back
def test_cut_back_to_back_launches(knob):
    """Three launches with nothing between them, on one side stream and then on three streams in issue order: A
    queues every message, B none, C some. A counts in one counter and zeroes the other, B counts in that one: the
    queue length B's wave kernel reads has to be B's own 0, and C's its own, whatever A left."""
    import torch
    from dynamicgo_amd import generic as X
    deep, shallow = deep_and_shallow(random.Random(44))
    items = deep + shallow
    nd, ns = len(deep), len(shallow)
    orders = {"A": np.arange(900) % nd, "B": nd + np.arange(300) % ns,
              "C": np.where(np.arange(500) % 3 == 0, np.arange(500) % nd, nd + np.arange(500) % ns)}
    assert X.default_context().get_knob("cut_wave_min") > 64
    want = cut_want(items, CG.pair(), CR.WRITE_DEFAULT)
    with X.CutPlan(*CG.pair()) as plan:
        one = torch.cuda.Stream()
        three = [torch.cuda.Stream() for _ in range(3)]
        for name, streams in (("one stream", [one] * 3), ("three streams", three)):
            batches = {k: Batch(items, o, cut_caps(items, want)) for k, o in orders.items()}
            torch.cuda.synchronize()  # the uploads and fills; nothing from here to the last launch
            for (k, b), s in zip(batches.items(), streams):
                cut_launch(plan, b, CR.WRITE_DEFAULT, stream=s)
            torch.cuda.synchronize()
            for k, b in batches.items():
                b.verify(want, cut_out_len, False, "%s, launch %s" % (name, k))


# -------------------------------------------- growth with a launch in flight
def test_queue_and_records_grow_while_a_launch_is_in_flight():
    """A context of its own, so the cut queue and the edit's record scratch start empty: a batch of 64, then with no
    synchronisation one of 5000 on another stream, which outgrows both (the host waits for the launch before, then
    reallocates), then the 64 again."""
    import torch
    from dynamicgo_amd import generic as X
    from dynamicgo_amd.conv import Context
    deep, shallow = deep_and_shallow(random.Random(45))
    items = deep + shallow
    want = cut_want(items, CG.pair(), 0)
    msgs = edit_items(random.Random(46))
    ctx = Context(0)  # fresh: cut_list and edit_rec have no capacity yet
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with X.CutPlan(*CG.pair(), ctx=ctx) as plan:
            bs = [Batch(items, np.arange(n) % len(items), cut_caps(items, want)) for n in (64, 5000, 64)]
            torch.cuda.synchronize()
            for b, s in zip(bs, (s1, s2, s1)):
                cut_launch(plan, b, 0, stream=s)
            torch.cuda.synchronize()
            for b in bs:
                b.verify(want, cut_out_len, False, "cut, fresh context, batch of %d" % b.n)
        for op in (E.SET_OP, E.UNSET_OP):
            with edit_plan(op, ctx) as plan:
                es = [EditBatch(msgs, op, n) for n in ((64, 5000, 64) if op == E.SET_OP else (64, 13000, 64))]
                torch.cuda.synchronize()
                for b, s in zip(es, (s1, s2, s1)):
                    b.launch(plan, stream=s)
                torch.cuda.synchronize()
                for b in es:
                    b.verify(b.want(), E.out_len, True, "edit %d, fresh context, batch of %d" % (op, b.n))
    finally:
        ctx.close()


# ------------------------- single edits and a many-edit on two streams
def test_single_and_many_edits_share_the_record_scratch_across_streams():
    """dg_edit and dg_editm keep their lookup's records in one scratch of the context. On a context of its own, 257
    fuzz messages (a block of the lane route and one lane more), with no synchronisation: a single SET on stream A
    (2 n records), a many-SET of 7 items on stream B, which outgrows the scratch (8 n) while A's splice may still
    read it, and a single UNSET on A, which has to wait for B's splice before its lookup writes over B's records;
    the second round starts on the grown scratch behind the first one's UNSET. Every slot has its exact bound,
    so the slot bases are unaligned and each neighbour's first byte is a guard."""
    import torch
    from dynamicgo_amd import generic as X
    from dynamicgo_amd.conv import Context
    n = 257
    msgs = EG.fuzz_cases()[0].msgs[:n]
    v1 = EG.wstr(b"x" * 33)
    seven = [((F, k), v, t) for k, v, t in ((1, b"\x01", R.BOOL), (2, b"\x7f", R.BYTE), (3, b"\x01\x02", R.I16),
                                           (4, struct.pack(">i", -1024), R.I32), (5, struct.pack(">q", 1 << 40), R.I64),
                                           (6, struct.pack(">d", 0.5), R.DOUBLE), (22, struct.pack(">d", 0.5), R.DOUBLE))]
    many = MG.ManyCase(M.SET_OP, [], seven, msgs)
    wants = [[E.edit(E.SET_OP, m, [(F, 18)], v1, R.STRING) for m in msgs], many.want(),
             [E.edit(E.UNSET_OP, m, [(F, 19)], b"", 0) for m in msgs]]
    assert {r & 0xFF for r, _ in wants[0]} >= {E.OK, E.E_READ} and {r & 0xFF for r, _ in wants[1]} >= {M.OK, M.E_READ}
    assert sum(r == E.word(E.OK, existed=True) for r, _ in wants[2]) > n // 4
    caps = [[E.slot_bound(E.SET_OP, [(F, 18)], len(m), len(v1)) for m in msgs], [many.bound(i) for i in range(n)],
            [len(m) for m in msgs]]
    vals = b"".join(v for _, v, _ in seven)

    def dev(b):
        return torch.from_numpy(np.frombuffer(b + b"\0" * 16, dtype=np.uint8).copy()).cuda()

    d_v1, d_v7 = dev(v1), dev(vals)
    ctx = Context(0)  # fresh: edit_rec has no capacity yet
    try:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        with X.EditPlan(EG.paths_of([(F, 18)]), E.SET_OP, ctx=ctx) as p_set, \
                X.EditPlan(EG.paths_of([(F, 19)]), E.UNSET_OP, ctx=ctx) as p_unset, \
                X.EditManyPlan([], EG.paths_of(many.steps), M.SET_OP, ctx=ctx) as p_many:
            rounds = [[Batch(msgs, np.arange(n), c) for c in caps] for _ in range(2)]
            torch.cuda.synchronize()  # the uploads and fills; nothing from here to the last launch
            for a, b, c in rounds:
                X.edit_device(p_set, a.arena, a.d_in, n, R.STRING, d_v1, None, a.d_out, a.d_oo, a.d_ol, a.d_ret,
                              val_len=len(v1), stream=sa, max_len=a.max_len)
                X.edit_many_device(p_many, b.arena, b.d_in, n, many.val_types, d_v7, None, [len(v) for _, v, _ in seven],
                                   b.d_out, b.d_oo, b.d_ol, b.d_ret, stream=sb, max_len=b.max_len)
                X.edit_device(p_unset, c.arena, c.d_in, n, 0, None, None, c.d_out, c.d_oo, c.d_ol, c.d_ret, stream=sa,
                              max_len=c.max_len)
            torch.cuda.synchronize()
            for r, bs in enumerate(rounds):
                for b, want, out_len, what in zip(bs, wants, (E.out_len, M.out_len, E.out_len),
                                                  ("single SET on A", "many-SET on B", "single UNSET on A")):
                    b.verify(want, out_len, True, "round %d, %s" % (r, what))
    finally:
        ctx.close()


# ------------------------------------- edit and GetByPath on two streams
def test_edit_interleaved_with_get_by_path(knob):
    """edit_device on one stream and get_by_path_device on another, in turn for 4 rounds with no synchronisation: the
    edit's lookup goes through the context's GetByPath workspace and its deep queue, which the other stream's
    launches use too. Each launch has outputs of its own."""
    import torch
    from dynamicgo_amd import generic as X
    import tgetgen as TG
    rng = random.Random(47)
    msgs = edit_items(rng)
    chains = [TG.random_chain(rng, rng.choice(range(10, 15))) for _ in range(300)] + \
        [TG.random_chain(rng, rng.choice(range(0, 6))) for _ in range(100)]
    get_msgs = [TG.chain_message(k, lf) for k, lf in chains]
    get_want = tget_expect(get_msgs, TG.CHAIN_PATHS)
    assert (get_want["status"] == R.OK).mean() > 0.5
    s_edit, s_get = torch.cuda.Stream(), torch.cuda.Stream()
    up = Upload(get_msgs)
    with edit_plan(E.SET_OP) as p_set, edit_plan(E.UNSET_OP) as p_unset, X.PathSet(to_paths(TG.CHAIN_PATHS)) as ps:
        edits = [EditBatch(msgs, E.SET_OP if r % 2 == 0 else E.UNSET_OP, 1500 + 427 * r) for r in range(4)]
        gets = [Outputs(len(get_msgs), len(TG.CHAIN_PATHS)) for _ in range(4)]
        torch.cuda.synchronize()
        for r in range(4):
            edits[r].launch(p_set if r % 2 == 0 else p_unset, stream=s_edit)
            tget_launch(ps, up, gets[r], stream=s_get)
        torch.cuda.synchronize()
        for r in range(4):
            edits[r].verify(edits[r].want(), E.out_len, True, "round %d, edit" % r)
            gets[r].verify(get_want, up.in_off, "round %d, GetByPath" % r)
