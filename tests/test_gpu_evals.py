"""GPU: entry column writes (dynamicgo_amd.generic over dg_evals_*) against the
checker of evalsref.py, which test_evals_codec.py holds against the reference's
j2t. Every case goes through the device entry and the host entry; every byte,
every offset and every status is compared, with guard bytes and guard entries
around every output. The inputs are evalsgen's, which test_evals_host.py runs
through the host build of the same encode."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import evalsgen as EG
import evalsref as ER
import faroff as FO

pytestmark = pytest.mark.gpu

GUARD = 64
FILL64 = 0x5A5A5A5A5A5A5A5A


def to_dev(col):
    """a column's arrays as device tensors (uint64 as int64, uint32 as int32); n_ent stays an int"""
    import torch
    views = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return {f: a if f == "n_ent" else torch.from_numpy(np.ascontiguousarray(a).view(views.get(a.dtype, a.dtype)).copy()).cuda()
            for f, a in col.items()}


class Outs:
    """d_out / d_out_off / d_status of one launch with their guards, and its d_work"""

    def __init__(self, pairs, room, sizing=False):
        import torch
        self.pairs, self.room = pairs, room
        self.off = torch.full((pairs + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.status = torch.full((pairs + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.out = None if sizing else torch.full((room + 16 + GUARD,), EG.GUARD, dtype=torch.uint8, device="cuda")

    def args(self):
        return self.out, self.off[GUARD:], self.status[GUARD:]

    def read(self, what):
        off, st = self.off.cpu().numpy().view(np.uint64), self.status.cpu().numpy()
        assert (off[:GUARD] == FILL64).all() and (off[GUARD + self.pairs + 1:] == FILL64).all(), "%s: a store around d_out_off" % what
        assert (st[:GUARD] == 0x5A).all() and (st[GUARD + self.pairs:] == 0x5A).all(), "%s: a store around d_status" % what
        return (None if self.out is None else self.out.cpu().numpy(), off[GUARD:GUARD + self.pairs + 1],
                st[GUARD:GUARD + self.pairs])


def work_for(plan, n, cols):
    """d_work of exactly the bytes asked for, between guards that verify() of the caller does not see: checked here"""
    import torch
    need = plan.work_bytes(n, [c["n_ent"] for c in cols])
    t = torch.full((need + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    return t, t[GUARD:GUARD + need]


def work_guards(t, what):
    h = t.cpu().numpy()
    assert (h[:GUARD] == 0x5A).all() and (h[-GUARD:] == 0x5A).all(), "%s: a store around d_work" % what


def launch(plan, dcols, n, o, work, base=0, cap=None, stream=None, status=True):
    from dynamicgo_amd import generic as G
    out, off, st = o.args()
    G.entry_values_device(plan, dcols, n, out, off, work, st if status else None, out_base=base,
                          cap=o.room if cap is None else cap, stream=stream)


def verify(got, want, base, cap, what):
    """out (with guards), off, status against the checker's (arena from base, off, status); cap: nothing at or beyond it"""
    out, off, st = got
    arena, woff, wst = want
    assert off.tolist() == woff, "%s: offsets" % what
    assert st.tolist() == wst, "%s: statuses" % what
    if out is None:
        return
    end = min(cap, woff[-1])
    assert (out[:base] == EG.GUARD).all(), "%s: a store before out_base" % what
    bad = np.nonzero(out[base:max(end, base)] != np.frombuffer(arena[:max(end - base, 0)], dtype=np.uint8))[0]
    assert bad.size == 0, "%s: byte %d of the arena" % (what, base + int(bad[0]))
    assert (out[max(end, base):] == EG.GUARD).all(), "%s: a store at cap or beyond" % what


def run_device(case, base=0, cap=None, sizing=False, want=None):
    import torch
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, n = case
    want = want or ER.encode_batch(kinds, cols, n, fids, base)
    need = want[1][-1]
    cap = need if cap is None else cap
    with G.EntryValuePlan(kinds, fids) as plan:
        o = Outs(n * len(kinds), max(cap, need), sizing)
        wt, work = work_for(plan, n, cols)
        launch(plan, [to_dev(c) for c in cols], n, o, work, base, cap)
        torch.cuda.synchronize()
        got = o.read(name)
        work_guards(wt, name)
    verify(got, want, base, cap, "%s, device entry" % name)
    return got, want


def run_host(case, want=None):
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, n = case
    want = want or ER.encode_batch(kinds, cols, n, fids)
    with G.EntryValuePlan(kinds, fids) as plan:
        arena, off, status = G._entry_values_host(plan, cols, n)
    assert off.tolist() == want[1] and status.tolist() == want[2], "%s, host entry" % name
    assert arena.tobytes() == want[0], "%s, host entry: bytes" % name


def check(case):
    want = ER.encode_batch(case[1], case[3], case[4], case[2])
    run_host(case, want)
    run_device(case, want=want)
    return want


# 1 ---------------------------------------------------------------- matrix
def test_kind_by_value_matrix():
    seen = set()
    for case in EG.matrix_cases():
        arena, off, st = check(case)
        kind = case[1][0]
        seen.add(kind)
        assert not any(st)
        if kind == ER.map_kind(ER.I08, ER.BOOL):  # message 4: 12 entries; 0xFF under I08 and the BOOL inputs 0, 1, 2, 2^63
            col = case[3][0]
            a, b = int(col["ent_off"][4]), int(col["ent_off"][5])
            item = arena[off[4]:off[5]]
            assert item[:6] == bytes([3, 2, 0, 0, 0, 12]) and b - a == 12
            assert item[6:] == b"".join(bytes([int(k) & 0xFF, int(v) != 0]) for k, v in zip(col["key"][a:b], col["val"][a:b]))
            assert 0xFF in col["key"][a:b].tolist() and {0, 1, 2, 2 ** 63} <= set(col["val"][:col["n_ent"]].tolist())
            assert set(item[7::2]) == {0, 1}
        if kind == ER.map_kind(ER.I64, ER.DOUBLE):
            item = arena[off[5]:off[6]]
            assert struct.unpack(">Q", item[14:22])[0] == EG.DOUBLES[5]  # a denormal, bit for bit
    assert seen == set(ER.ALL_KINDS)
    # duplicate keys and empty strings are in the inputs
    col = next(EG.matrix_cases())[3][0]
    assert 0 in col["val_len"][:col["n_ent"]].tolist()
    case = [c for c in EG.matrix_cases() if c[1][0] == ER.map_kind(ER.I08, ER.I64)][0]
    a, b = int(case[3][0]["ent_off"][5]), int(case[3][0]["ent_off"][6])
    assert len(set(case[3][0]["key"][a:b].tolist())) < b - a


# 2 ---------------------------------------------------------------- counts
@pytest.mark.parametrize("kind", EG.COUNT_KINDS, ids=["%#x" % k for k in EG.COUNT_KINDS])
def test_counts_around_the_wave_the_block_and_the_chunk(kind):
    cases = [c for c in EG.count_cases() if c[1] == [kind]]
    assert len(cases) == 2
    for case in cases:
        check(case)
        counts = np.diff(case[3][0]["ent_off"].astype(np.int64)).tolist()
        if case[0].startswith("counts"):
            assert sorted(counts) == EG.COUNTS
        else:
            k = counts.index(4097)
            assert counts[k - 1] == 0 and counts[k + 1] == 1


# 3 --------------------------------------------------------------- strings
@pytest.mark.parametrize("shift", range(16))
def test_strings_at_every_length_and_residue(shift):
    case = list(EG.string_cases())[shift]
    check(case)
    col = case[3][1]
    ne = col["n_ent"]
    assert {int(v) % 16 for v in col["val"][:ne]} == set(range(16))  # source residues
    assert int(col["val"][ne - 1]) + int(col["val_len"][ne - 1]) + 16 == len(col["val_src"])  # the last payload ends the arena
    if shift in (0, 5):
        assert sorted(col["val_len"][:ne].tolist()) == list(range(256)) + [16385]


# 4 ----------------------------------------------------- geometry and writes
@pytest.mark.parametrize("K", EG.GEOMETRY_K)
def test_geometry(K):
    for n in EG.GEOMETRY_N:
        case = EG.geometry_case(K, n)
        want = ER.encode_batch(case[1], case[3], n)
        run_device(case, want=want)
        if n == 64:
            run_host(case, want)
    kinds = EG.GEOMETRY_KINDS[:max(K, 2)]
    assert K == 1 or ({bool(ER.stride(k)) for k in kinds} == {True, False})  # fixed-stride and variable kinds in one plan


def test_one_message_changes_only_its_own_items():
    _, kinds, fids, cols, n = EG.geometry_case(7, 65)
    i, K = 30, len(kinds)
    rows = [[(7 * k, float(k)) for k in range(3)] for _ in range(n)]
    (out0, off0, _), _ = run_device(("base", kinds, fids, [EG.entry_col(kinds[0], rows)] + cols[1:], n))
    rows[i] = [(7 * k, float(k)) for k in range(11)]
    (out1, off1, _), _ = run_device(("changed", kinds, fids, [EG.entry_col(kinds[0], rows)] + cols[1:], n))
    a, e0, e1 = int(off0[i * K]), int(off0[(i + 1) * K]), int(off1[(i + 1) * K])
    d = e1 - e0
    assert d == 8 * 12
    assert (off1[:i * K + 1] == off0[:i * K + 1]).all() and (off1[(i + 1) * K:].astype(np.int64) - d == off0[(i + 1) * K:]).all()
    assert (out1[:a] == out0[:a]).all() and (out1[e1:int(off1[-1])] == out0[e0:int(off0[-1])]).all()
    assert out1[a:e1].tobytes() != out0[a:e0].tobytes()


# 5 -------------------------------------------------------- caps and sizing
def test_cap_below_the_need_and_out_base():
    """cap at the need, below it and 0, at several out_base; on the small batch every cap from 0 to the need, which
    cuts inside every header, key, length prefix and payload"""
    case = EG.geometry_case(7, 65)
    _, kinds, fids, cols, n = case
    for base in (0, 1, 13, 8191):
        want = ER.encode_batch(kinds, cols, n, fids, base)
        need = want[1][-1]
        for cap in (need, need - 1, base + (need - base) // 2, base + 1, base, 0):
            run_device(case, base=base, cap=cap, want=want)
    small = EG.geometry_case(7, 2, ids=True)
    want = ER.encode_batch(small[1], small[3], small[4], small[2], 5)
    import torch
    from dynamicgo_amd import generic as G
    need = want[1][-1]
    with G.EntryValuePlan(small[1], small[2]) as plan:
        dcols = [to_dev(c) for c in small[3]]
        wt, work = work_for(plan, 2, small[3])
        outs = [Outs(14, need) for _ in range(5, need + 1)]
        for cap, o in zip(range(5, need + 1), outs):
            launch(plan, dcols, 2, o, work, 5, cap)
        torch.cuda.synchronize()
        for cap, o in zip(range(5, need + 1), outs):
            verify(o.read("cap %d" % cap), want, 5, cap, "cap %d" % cap)
    # sizing: no d_out, offsets and statuses only; a NULL d_status is taken too
    run_device(case, base=5, sizing=True)
    with G.EntryValuePlan(kinds) as plan:
        o = Outs(n * len(kinds), 0, sizing=True)
        wt, work = work_for(plan, n, cols)
        launch(plan, [to_dev(c) for c in cols], n, o, work, status=False)
        torch.cuda.synchronize()
        _, off, st = o.read("no d_status")
        assert off.tolist() == ER.encode_batch(kinds, cols, n)[1] and (st == 0x5A).all()


# 6 ----------------------------------------------------------- error cells
def test_size_and_range_flags():
    """flagged cells are empty containers; the canary entries behind n_ent and the payloads of flagged cells (offset 0
    with lengths of 2^31 and 2^32 - 1) leave no trace in the output"""
    names = []
    for case in EG.flag_cases():
        want = ER.encode_batch(case[1], case[3], case[4], case[2])
        run_device(case, want=want, sizing=True)
        run_device(case, want=want)
        run_host(case, want)
        names.append(case[0])
        st = want[2]
        if case[0].startswith("ranges") and "struct" not in case[0]:
            assert st == [0, 2, 0, 2, 2, 0, 2, 0, 2, 2]
            kind = case[1][0]
            assert want[0][want[1][1]:want[1][2]] == ER.header(kind, 0)
        if case[0].startswith("sizes"):
            assert st == [1, 0, 0, 1, 0, 1]
    assert len(names) == 12
    # a count of 2^31 under n_ent = 2^32 - 1: a fixed-stride kind's sizing call reads d_ent_off alone
    for ids in (False, True):
        _, want = run_device(EG.count_flag_case(ids), sizing=True, base=7)
        assert want[2] == [ER.E_SIZE, ER.OK, ER.E_RANGE, ER.E_RANGE, ER.OK, ER.E_RANGE]


# 7 ------------------------------------------------------------ struct mode
def test_struct_mode():
    from dynamicgo_amd import generic as G
    for case in EG.struct_cases():
        arena, off, _ = check(case)
        if case[0] != "struct presence":
            continue
        K = 3
        msgs = [arena[off[i * K]:off[(i + 1) * K]] for i in range(8)]
        assert msgs[0] == b"\0" and all(m[-1] == 0 for m in msgs) and len(set(msgs)) == 8
        # read back: GetByPath and the entry casts give the inputs
        cols = G.entries_batch(msgs, [([G.PathFieldId(1)], "intmap[int]"), ([G.PathFieldId(255)], "list[str]"),
                                      ([G.PathFieldId(256)], "strmap[str]")])
        ins = case[3]
        for j, c in enumerate(cols):
            assert c.valid.tolist() == [bool(i >> j & 1) for i in range(8)]
        s32 = lambda v: ((int(v) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000  # noqa: E731 (written at 32 bits, read signed)
        s64 = lambda v: ((int(v) & ER.M64) ^ (1 << 63)) - (1 << 63)  # noqa: E731
        for i in range(8):
            a, b = int(ins[0]["ent_off"][i]), int(ins[0]["ent_off"][i + 1])
            if i & 1:
                assert cols[0].keys[i] == [s32(k) for k in ins[0]["key"][a:b]]
                assert cols[0].values[i] == [s64(v) for v in ins[0]["val"][a:b]]
            a, b = int(ins[1]["ent_off"][i]), int(ins[1]["ent_off"][i + 1])
            if i & 2:
                assert cols[1].values[i] == [ins[1]["val_src"][int(v):int(v) + int(ln)].tobytes()
                                             for v, ln in zip(ins[1]["val"][a:b], ins[1]["val_len"][a:b])]
            a, b = int(ins[2]["ent_off"][i]), int(ins[2]["ent_off"][i + 1])
            if i & 4:
                assert cols[2].keys[i] == [ins[2]["key_src"][int(v):int(v) + int(ln)].tobytes()
                                           for v, ln in zip(ins[2]["key"][a:b], ins[2]["key_len"][a:b])]


def test_public_host_wrappers():
    """entry_values_batch, build_entry_structs_batch and set_entry_columns_batch over Python sequences"""
    from dynamicgo_amd import generic as G
    tags = [["a", b"bc"], [], ["", "tag"]]
    counters = [{"x": 1, "yy": -2}, [("k", 5), ("k", 6)], {}]
    feats = [[(1, 1.5)], [], [(2, -0.0), (3, float("inf"))]]
    arena, off, st = G.entry_values_batch([tags, counters], [("list", "str"), ("map", "str", "i64")])
    want = b"".join(ER.encode(ER.LIST_STR, t) + ER.encode(ER.map_kind(ER.STRING, ER.I64),
                                                          list(c.items()) if isinstance(c, dict) else c)
                    for t, c in zip(tags, counters))
    assert arena.tobytes() == want and not st.any() and len(off) == 7
    msgs = G.build_entry_structs_batch([(19, ("list", "str"), tags), (20, ("map", "str", "i64"), counters, [1, 1, 0]),
                                        (5, ("map", "i32", "f64"), feats)])
    for i, m in enumerate(msgs):
        w = ER.field_begin(ER.LIST_STR, 19) + ER.encode(ER.LIST_STR, tags[i])
        if i < 2:
            c = counters[i]
            w += ER.field_begin(ER.MAP, 20) + ER.encode(ER.map_kind(ER.STRING, ER.I64), list(c.items()) if isinstance(c, dict) else c)
        w += ER.field_begin(ER.MAP, 5) + ER.encode(ER.map_kind(ER.I32, ER.DOUBLE), feats[i]) + b"\0"
        assert m == w, i
    res = G.set_entry_columns_batch(msgs, [], [(G.PathFieldId(19), ("list", "str"), [["z"]] * 3),
                                               (G.PathFieldId(7), ("map", "i64", "str"), [[(9, "nine")]] * 3)])
    assert all(r.status == G.EDIT_OK and r.existed == (True, False) for r in res)
    back = G.entries_batch([r.raw for r in res], [([G.PathFieldId(19)], "list[str]"), ([G.PathFieldId(7)], "intmap[str]")])
    assert back[0].values == [[b"z"]] * 3 and back[1].items(0) == [(9, b"nine")]
    assert G.eval_kind(("list", "str")) == 0x4B and G.eval_kind(("set", "binary")) == 0x8B
    assert G.eval_kind(("map", "str", "i64")) == 0x1BA and G.eval_kind(("map", "i32", "f64")) == 0x184
    assert G.eval_kind(np.uint16(0x4B)) == 0x4B and G.eval_kind(np.int64(0x184)) == 0x184  # numpy integers too
    for bad in (("list", "i64"), ("map", "bool", "i64"), ("map", "f64", "str"), 0x4A, 0x142, 5, 75.0, "0x4b"):
        with pytest.raises(ValueError):
            G.eval_kind(bad)
    with pytest.raises(ValueError):  # vals keeps refusing what evals takes
        G.val_kind(("list", "str"))


# 8 --------------------------------------------------- refusals, empty batches
def test_plan_create_rejects_and_empty_batches():
    import torch
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()

    def create(kinds, K=None, ids=None):
        h = C.c_void_p()
        kk = np.array(kinds, dtype=np.uint16)
        arr = None if ids is None else np.array(ids, dtype=np.int16)
        rc = L.dg_evals_create(ctx.h, kk.ctypes.data, len(kinds) if K is None else K, None if arr is None else arr.ctypes.data,
                               C.byref(h))
        if rc == 0:
            assert L.dg_evals_count(h) == len(kinds)
            assert [L.dg_evals_wire_type(h, k) for k in range(len(kinds))] == [ER.wire_type(k) for k in kinds]
            assert L.dg_evals_wire_type(h, len(kinds)) == 0
            L.dg_evals_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create(ER.ALL_KINDS[:16])[0] == 0 and create(ER.ALL_KINDS[16:32])[0] == 0 and create(ER.ALL_KINDS[32:])[0] == 0
    for kinds, text in (([0x4B, 0], "column 1: unknown kind 0"), ([12], "column 0: unknown kind 12"),
                        ([0x4B, 0x8B, 0x4A], "column 2: unknown kind 74"), ([0xCB], "column 0: unknown kind 203"),
                        ([0x100 | 2 << 4 | 8], "column 0: unknown kind 296"), ([0x100 | 4 << 4 | 8], "column 0: unknown kind 328"),
                        ([0x100 | 11 << 4 | 12], "column 0: unknown kind 444"), ([0x200 | 11 << 4 | 11], "column 0: unknown kind 699"),
                        ([8], "column 0: unknown kind 8"), ([0x42], "column 0: unknown kind 66")):
        rc, err = create(kinds)
        assert rc == -6 and text in err, (kinds, rc, err)  # DG_E_ARG
    for K in (0, 17):
        rc, err = create([0x4B] * 17, K=K)
        assert rc == -6 and "%d columns (1 to 16)" % K in err, (K, rc, err)
    # d_present without field ids, an n_ent beyond the limit, a d_work too small: refused at the call, nothing written
    rows = [[b"a"], [], [b"bc", b""]]
    col = EG.entry_col(ER.LIST_STR, rows)
    with G.EntryValuePlan([ER.LIST_STR]) as plan:
        o = Outs(3, 64)
        wt, work = work_for(plan, 3, [col])
        pres = dict(col, present=np.array([1, 0, 1], dtype=np.uint8))
        with pytest.raises(_lib.DGError, match="-6.*d_present in a plan without field ids"):
            launch(plan, [to_dev(pres)], 3, o, work)
        with pytest.raises(_lib.DGError, match="-6.*d_present in a plan without field ids"):
            G._entry_values_host(plan, [pres], 3)
        with pytest.raises(_lib.DGError, match="-6.*column 0: 4294967296 entries"):
            launch(plan, [dict(to_dev(col), n_ent=2 ** 32)], 3, o, work)
        assert L.dg_evals_work_bytes(plan.h, 3, np.array([2 ** 32], dtype=np.uint64).ctypes.data) == 0
        with pytest.raises(_lib.DGError, match="-3.*d_work"):  # DG_E_NOMEM
            launch(plan, [to_dev(col)], 3, o, work[:work.numel() - 8])
        torch.cuda.synchronize()
        out, _, _ = o.read("refused")
        assert (out == EG.GUARD).all()
        launch(plan, [to_dev(col)], 0, o, work)  # n = 0: DG_OK, nothing launched, nothing written
        torch.cuda.synchronize()
        assert (o.off.cpu().numpy().view(np.uint64) == FILL64).all()
        arena, off, st = G._entry_values_host(plan, [EG.entry_col(ER.LIST_STR, [])], 0)
        assert len(arena) == 0 and off.tolist() == [0] and len(st) == 0
        # a column with no entries at all: every array but ent_off may be NULL
        empty = {"ent_off": np.zeros(4, dtype=np.uint64), "n_ent": 0}
        run_device(("no entries", [ER.LIST_STR], None, [empty], 3))
        run_host(("no entries", [ER.LIST_STR], None, [empty], 3))


# 9 ------------------------------------------- round trip with the read side
def ents_to_evals(msgs, columns):
    """On the CPU, with entsref: per entry column, the evals kinds its OK cells name and, per kind, the cells whose
    container bytes in the message are what the kind writes from the entries read (a map of BOOL values only where
    its bool bytes are 0 or 1): [(column, kind, [message...])]."""
    import entsref as NR
    import tgetref as R
    out = []
    arena = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    for k, (path, ekind) in enumerate(columns):
        by_kind = {}
        base = 0
        for i, m in enumerate(msgs):
            c = NR.cell(m, path, ekind, R.STRUCT, base)
            base += len(m)
            if c.status != R.OK:
                continue
            kind = ER.LIST_STR if ekind == NR.LISTSTR else ER.map_kind(c.aux & 0xFF, c.aux >> 8)
            if not ER.kind_ok(kind):
                continue
            hdr = 5 if ekind == NR.LISTSTR else 6
            raw = m[c.val - (base - len(m)) - hdr:c.val - (base - len(m)) + c.span]
            kt, vt = ER.types(kind)
            col = {"ent_off": np.array([0, c.len], dtype=np.uint64), "n_ent": c.len,
                   "key": np.array(c.keys, dtype=np.uint64), "key_len": np.array(c.klens, dtype=np.uint32),
                   "val": np.array(c.vals, dtype=np.uint64), "val_len": np.array(c.vlens, dtype=np.uint32),
                   "key_src": arena, "val_src": arena}
            if ER.encode_cell(kind, col, 0)[0] == raw:
                by_kind.setdefault(kind, []).append(i)
        out += [(k, kind, rows) for kind, rows in sorted(by_kind.items())]
    return out


# the OK cells per evals kind that ents_to_evals finds, counted on the CPU with entsref (a set's item is a list's:
# 0x4b stands for both); "kinds" holds every kind, entsgen's own messages 33 and 13 of them
ROUND_TRIP = {
    "matrix": {0x4b: 8, 0x133: 1, 0x134: 1, 0x136: 1, 0x138: 6, 0x13a: 1, 0x13b: 1, 0x163: 1, 0x164: 1, 0x166: 1, 0x168: 6,
               0x16a: 1, 0x16b: 2, 0x182: 5, 0x183: 6, 0x184: 6, 0x186: 6, 0x188: 12, 0x18a: 6, 0x18b: 6, 0x1a3: 1, 0x1a4: 1,
               0x1a6: 1, 0x1a8: 6, 0x1aa: 1, 0x1ab: 1, 0x1b2: 8, 0x1b3: 10, 0x1b4: 8, 0x1b6: 10, 0x1b8: 18, 0x1ba: 12, 0x1bb: 8},
    "counts": {0x4b: 7, 0x132: 12, 0x133: 12, 0x13b: 10, 0x16a: 12, 0x184: 12, 0x18b: 10, 0x1a4: 12, 0x1a6: 12, 0x1b3: 9,
               0x1b4: 9, 0x1ba: 9, 0x1bb: 9},
    "kinds": {0x4b: 28, 0x132: 10, 0x133: 10, 0x134: 10, 0x136: 10, 0x138: 10, 0x13a: 10, 0x13b: 10, 0x162: 10, 0x163: 10,
              0x164: 10, 0x166: 10, 0x168: 10, 0x16a: 10, 0x16b: 10, 0x182: 10, 0x183: 10, 0x184: 10, 0x186: 10, 0x188: 10,
              0x18a: 10, 0x18b: 10, 0x1a2: 10, 0x1a3: 10, 0x1a4: 10, 0x1a6: 10, 0x1a8: 10, 0x1aa: 10, 0x1ab: 10, 0x1b2: 18,
              0x1b3: 18, 0x1b4: 12, 0x1b6: 18, 0x1b8: 18, 0x1ba: 18, 0x1bb: 12},
}


@pytest.mark.parametrize("which", ("matrix", "counts", "kinds"))
def test_round_trip_with_the_read_side(which):
    """entries_device + entry_emit_device, then entry_values_device on the tensors as they are, the thrift arena as
    both sources: every OK cell's item is the container's bytes in its message"""
    import torch
    import entsgen as NG
    from dynamicgo_amd import generic as G
    from test_gpu_ents import Outputs, to_cols, upload
    if which == "matrix":
        msgs, sets = NG.matrix_messages(), NG.MATRIX_SETS
    elif which == "counts":
        msgs, sets = NG.count_messages(), (NG.COUNT_COLUMNS,)
    else:
        msgs, sets = EG.kind_messages(), NG.MATRIX_SETS
    n = len(msgs)
    arena, d_off, in_off = upload(msgs)
    ent_cap = int(in_off[n]) // 2 + 64
    seen = {}
    for columns in sets:
        plan_rows = ents_to_evals(msgs, columns)
        with G.EntryPlan(to_cols(columns)) as plan:
            o = Outputs(n, plan.count)
            G.entries_device(plan, arena, d_off, n, *o.args(), max_len=max(map(len, msgs)))
            cells = None
            for k in sorted({k for k, _, _ in plan_rows}):
                ent_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                keys, vals = (torch.zeros(ent_cap, dtype=torch.int64, device="cuda") for _ in range(2))
                klens, vlens = (torch.zeros(ent_cap, dtype=torch.int32, device="cuda") for _ in range(2))
                G.entry_emit_device(plan, k, arena, n, *o.column(k), ent_off, keys, klens, vals, vlens, ent_cap=ent_cap)
                col = {"ent_off": ent_off, "key": keys, "key_len": klens, "val": vals, "val_len": vlens, "key_src": arena,
                       "val_src": arena, "n_ent": ent_cap}
                for kind, rows in [(kd, r) for kk, kd, r in plan_rows if kk == k]:
                    with G.EntryValuePlan([kind]) as ep:
                        out = torch.full((8 * int(in_off[n]) + 16 * n + 16,), EG.GUARD, dtype=torch.uint8, device="cuda")  # a wider kind fits
                        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
                        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
                        work = torch.zeros(ep.work_bytes(n, [ent_cap]), dtype=torch.uint8, device="cuda")
                        G.entry_values_device(ep, [col], n, out, off, work, st)
                        torch.cuda.synchronize()
                    cells = cells or o.read("round trip")
                    h_out, h_off = out.cpu().numpy(), off.cpu().numpy()
                    assert not st.cpu().numpy().any()
                    hdr = 6 if ER.is_map(kind) else 5
                    for i in rows:
                        v, span = int(cells[k]["val"][i]), int(cells[k]["span"][i])
                        assert cells[k]["status"][i] == 0
                        a = v - int(in_off[0])
                        want = b"".join(msgs)[a - hdr:a + span]
                        assert h_out[int(h_off[i]):int(h_off[i + 1])].tobytes() == want, (which, k, hex(kind), i)
                    seen[kind] = seen.get(kind, 0) + len(rows)
    assert seen == ROUND_TRIP[which], seen


# 10 ------------------------------------------------- the chain on the device
@pytest.fixture(scope="module")
def all_corpus():
    import modelgen as M
    import oracle
    return M.Corpus(oracle.RefOracle() or oracle.PortOracle(), "all", 300)


def test_ents_torch_evals_editm_on_one_stream(all_corpus):
    """entries_device + entry_emit_device, a torch + 1 on the values of the map<string, i64> field 20,
    entry_values_device and edit_many_device, all on one stream with no synchronisation between them, against the
    checker's many-edit over the checker's values"""
    import torch
    import editmref as EM
    import tgetref as R
    from dynamicgo_amd import generic as G
    msgs = all_corpus.msgs
    n = len(msgs)
    arena_np = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    total = int(in_off[n])
    arena, d_in = torch.from_numpy(arena_np).cuda(), torch.from_numpy(in_off).cuda()
    caps = np.array([(len(m) + 8 * 8 + 79) & ~15 for m in msgs])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    d_oo = torch.from_numpy(out_off).cuda()
    ent_cap = total // 2 + 64
    kind = ER.map_kind(ER.STRING, ER.I64)
    stream = torch.cuda.Stream()
    with G.EntryPlan([([G.PathFieldId(20)], "strmap[int]")]) as rp, G.EntryValuePlan([kind]) as ep, \
            G.EditManyPlan([], [G.PathFieldId(20)], G.EDIT_SET) as mp:
        val = torch.zeros((1, n), dtype=torch.int64, device="cuda")
        cell = torch.zeros((1, n, 2), dtype=torch.int32, device="cuda")
        lens, spans = (torch.zeros((1, n), dtype=torch.int32, device="cuda") for _ in range(2))
        ent_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        keys, vals = (torch.zeros(ent_cap, dtype=torch.int64, device="cuda") for _ in range(2))
        klens = torch.zeros(ent_cap, dtype=torch.int32, device="cuda")
        cap_v = 6 * n + total
        ev = torch.full((cap_v + 16,), EG.GUARD, dtype=torch.uint8, device="cuda")
        ev_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        work = torch.zeros(ep.work_bytes(n, [ent_cap]), dtype=torch.uint8, device="cuda")
        out = torch.full((int(out_off[n]) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        ol = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ret = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.entries_device(rp, arena, d_in, n, val, cell, lens, spans, stream=stream)
            G.entry_emit_device(rp, 0, arena, n, val[0], cell[0], lens[0], spans[0], ent_off, keys, klens, vals, None,
                                ent_cap=ent_cap, stream=stream)
            plus = vals + 1
            G.entry_values_device(ep, [{"ent_off": ent_off, "key": keys, "key_len": klens, "val": plus, "key_src": arena,
                                        "n_ent": ent_cap}], n, ev, ev_off, work, cap=cap_v, stream=stream)
            G.edit_many_device(mp, arena, d_in, n, ep.wire_types, ev, ev_off, [0], out, d_oo, ol, ret, stream=stream)
        torch.cuda.synchronize()
        h_eo = ent_off.cpu().numpy().view(np.uint64)
        cnt = int(h_eo[n])
        assert cnt >= 100
        col = {"ent_off": h_eo, "key": keys.cpu().numpy().view(np.uint64), "key_len": klens.cpu().numpy().view(np.uint32),
               "val": vals.cpu().numpy().view(np.uint64) + np.uint64(1), "key_src": arena_np, "n_ent": ent_cap}
        v_bytes, v_off, v_st = ER.encode_batch([kind], [col], n)
        assert ev_off.cpu().numpy().tolist() == v_off and not any(v_st)
        assert ev.cpu().numpy()[:v_off[-1]].tobytes() == v_bytes
        h_out, h_ol, h_ret = out.cpu().numpy(), ol.cpu().numpy(), ret.cpu().numpy().view(np.uint64)
        changed = 0
        for i, m in enumerate(msgs):
            items = [((R.FIELD, 20), v_bytes[v_off[i]:v_off[i + 1]], R.MAP)]
            w_ret, w_out = EM.edit_many(EM.SET_OP, m, [], items, cap=int(caps[i]))
            assert int(h_ret[i]) == w_ret, (i, hex(int(h_ret[i])), hex(w_ret))
            g_out = h_out[int(out_off[i]):int(out_off[i]) + (int(h_ol[i]) if w_ret & 0xFF == 0 else 0)].tobytes()
            assert g_out == w_out, i
            changed += g_out != m
        assert changed >= 50


# 11 -------------------------------------------------------------- streams
def test_two_streams_at_once():
    import torch
    from dynamicgo_amd import generic as G
    cases = [EG.geometry_case(7, 257), EG.geometry_case(16, 255)]
    wants = [ER.encode_batch(c[1], c[3], c[4]) for c in cases]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with G.EntryValuePlan(cases[0][1]) as pa, G.EntryValuePlan(cases[1][1]) as pb:
        da, db = [to_dev(c) for c in cases[0][3]], [to_dev(c) for c in cases[1][3]]
        rounds = [(Outs(257 * 7, wants[0][1][-1]), Outs(255 * 16, wants[1][1][-1]), work_for(pa, 257, cases[0][3]),
                   work_for(pb, 255, cases[1][3])) for _ in range(3)]
        torch.cuda.synchronize()
        for oa, ob, wa, wb in rounds:  # no synchronisation between the launches; a d_work per call in flight
            launch(pa, da, 257, oa, wa[1], stream=sa)
            launch(pb, db, 255, ob, wb[1], stream=sb)
        torch.cuda.synchronize()
        for r, (oa, ob, wa, wb) in enumerate(rounds):
            verify(oa.read("stream a"), wants[0], 0, wants[0][1][-1], "round %d, stream a" % r)
            verify(ob.read("stream b"), wants[1], 0, wants[1][1][-1], "round %d, stream b" % r)
            work_guards(wa[0], "stream a"), work_guards(wb[0], "stream b")


# 12 ----------------------------------------------------------- far offsets
@pytest.fixture(scope="module")
def far_arenas():
    import torch
    inp, out = FO.Arena(), FO.Arena()
    yield inp, out
    inp.free()
    out.free()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", FO.BOUNDS, ids=["2G", "4G"])
def test_far_offsets(far_arenas, B):
    """list<string> elements and map<string, i64> keys in a source arena at offsets below, across and beyond B,
    written to an output arena at an out_base that puts the pivot's item across B; the aliases of the source hold
    decoys, and everything outside the items in the output arena is still FILL. (The per-entry arrays themselves
    are small here; test_far_entry_arrays has them across the bounds.)"""
    import torch
    from dynamicgo_amd import generic as G
    inp, outa = far_arenas
    rng = random.Random(61)
    pay = [EG.payload(rng, rng.choice((1, 5, 8, 13, 24, 40, 300))) for _ in range(40)]
    pay.insert(20, EG.payload(rng, 100))
    n, pivot = len(pay), 20
    src_off = FO.place([len(p) for p in pay], B, pivot, -37)  # the pivot's payload straddles B
    FO.check_layout(src_off, B, guard=0, tail=FO.TAIL)
    inp.put_input(src_off, pay, B)
    for kind, per in ((ER.LIST_STR, 9), (ER.map_kind(ER.STRING, ER.I64), 18)):
        strs = {"key" if ER.is_map(kind) else "val": src_off[:-1].astype(np.uint64),
                "key_len" if ER.is_map(kind) else "val_len": np.array([len(p) for p in pay], dtype=np.uint32)}
        col = dict(strs, ent_off=np.arange(n + 1, dtype=np.uint64), n_ent=n)
        if ER.is_map(kind):
            col["val"] = np.arange(n, dtype=np.uint64) * np.uint64(0x0101010101010101)
        rel = [0]
        for p in pay:
            rel.append(rel[-1] + per + len(p))
        base = B - rel[pivot] - (per - 4 if not ER.is_map(kind) else 6) - 6
        woff = [base + r for r in rel]
        if ER.is_map(kind):
            arena = b"".join(ER.encode(kind, [(p, int(v))]) for p, v in zip(pay, col["val"]))
        else:
            arena = b"".join(ER.encode(kind, [p]) for p in pay)
        assert len(arena) == rel[-1]
        FO.check_layout(np.array(woff, dtype=np.int64), B)
        assert woff[pivot] < B < woff[pivot + 1]
        o_off = np.array(woff, dtype=np.int64)
        outa.prefill(o_off, B)
        with G.EntryValuePlan([kind]) as plan:
            off = torch.full((n + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
            st = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
            d = to_dev(col)
            d["key_src" if ER.is_map(kind) else "val_src"] = inp.base
            wt, work = work_for(plan, n, [col])
            G.entry_values_device(plan, [d], n, outa.base, off[GUARD:], work, st[GUARD:], out_base=base, cap=woff[-1])
            torch.cuda.synchronize()
            work_guards(wt, "far")
        h_off, h_st = off.cpu().numpy(), st.cpu().numpy()
        assert h_off[GUARD:GUARD + n + 1].tolist() == woff and (h_off[:GUARD].view(np.uint64) == FILL64).all()
        assert (h_off[GUARD + n + 1:].view(np.uint64) == FILL64).all()
        assert (h_st[GUARD:GUARD + n] == 0).all() and (h_st[:GUARD] == 0x5A).all() and (h_st[GUARD + n:] == 0x5A).all()
        got = outa.collect(o_off, B, what="d_out at %#x, kind %#x" % (B, kind))
        assert got.tobytes() == arena


FAR_ENTRIES = (2 ** 28, 2 ** 29, 2 ** 30)  # 8-byte arrays cross 2^31 and 2^32 bytes at the first two, 4-byte ones at the last two


@pytest.mark.parametrize("kind", (ER.map_kind(ER.I32, ER.DOUBLE), ER.map_kind(ER.STRING, ER.I64)), ids=("fixed", "variable"))
def test_far_entry_arrays(kind):
    """The per-entry arrays themselves across 2^31 and 2^32 bytes: n_ent = 2^30 + 8, so d_key and d_val (8 bytes an
    entry) are 8 GiB each, d_key_len and the entry sizes in d_work 4 GiB, the positions in d_work 8 GiB. Cell 0 owns
    entries 0 to 2; three cells own the 5 entries that straddle index 2^28, 2^29 and 2^30. The cells between them
    own the zeroed entries between and are absent (struct mode, d_present 0), so nothing of theirs is read. The fixed-stride kind indexes d_key / d_val there, the variable-stride kind
    also evals_entry_size_kernel, the scan's positions and the emit's pos[e0 + r]. The checker encodes the same
    entries from compact arrays: the bytes do not depend on where the entries lie."""
    import torch
    from dynamicgo_amd import generic as G
    rng = random.Random(71)
    kt, vt = ER.types(kind)
    n_ent = 2 ** 30 + 8
    spans = [(0, 3)] + [(b - 2, b + 3) for b in FAR_ENTRIES]
    rows = EG.rows_for(rng, kind, [b - a for a, b in spans])
    if kt == ER.STRING:  # distinct, non-empty keys: an entry read from a wrong index shows
        rows = [[(EG.payload(rng, 3 + (i + j) % 9), v) for j, (_, v) in enumerate(r)] for i, r in enumerate(rows)]
    compact = EG.entry_col(kind, [x for r in rows for x in (r, [])], tail=0)  # the absent cells own nothing here
    n = 2 * len(spans)
    compact["present"] = np.array([1, 0] * len(spans), dtype=np.uint8)
    want = ER.encode_batch([kind], [compact], n, [5])
    assert not any(want[2]) and [want[1][2 * i + 1] - want[1][2 * i] > 6 for i in range(len(spans))] == [True] * 4
    far = {"ent_off": torch.tensor([x for a, b in spans for x in (a, b)] + [n_ent], dtype=torch.int64, device="cuda"),
           "n_ent": n_ent, "present": torch.from_numpy(compact["present"].copy()).cuda()}
    at = 0
    names = [f for f in ("key", "key_len", "val", "val_len") if f in compact]
    for f in names:
        far[f] = torch.zeros(n_ent, dtype=torch.int64 if f in ("key", "val") else torch.int32, device="cuda")
        assert far[f].numel() * far[f].element_size() > 2 ** 32
    for a, b in spans:
        for f in names:
            src = compact[f][at:at + b - a]
            far[f][a:b] = torch.from_numpy(src.view(np.int64 if src.dtype == np.uint64 else np.int32).copy()).cuda()
        at += b - a
    for f in ("key_src", "val_src"):
        if f in compact:
            far[f] = torch.from_numpy(compact[f].copy()).cuda()
    need = want[1][-1]
    with G.EntryValuePlan([kind], [5]) as plan:
        o = Outs(n, need)
        wt, work = work_for(plan, n, [far])
        assert ER.stride(kind) or work.numel() > 12 * 2 ** 30
        launch(plan, [far], n, o, work)
        torch.cuda.synchronize()
        got = o.read("far entries")
        work_guards(wt, "far entries")
    verify(got, want, 0, need, "far entry arrays, kind %#x" % kind)
    del far, work, wt, o
    torch.cuda.empty_cache()
