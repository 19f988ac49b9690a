"""GPU: typed column writes (dynamicgo_amd.generic over dg_vals_*) against the
checker of valsref.py, which test_vals_codec.py holds against the reference's
j2t. Every case goes through the device entry with both emits (the head and
body passes, and knob vals_lane_emit = 1) and through the host entry; every
byte, every offset and every status is compared, with guard bytes and guard
entries around every output. The inputs are valsgen's, which test_vals_host.py
runs through the host build of the same encode."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import faroff as FO
import valsgen as VG
import valsref as VR

pytestmark = pytest.mark.gpu

GUARD = 64
FILL64 = 0x5A5A5A5A5A5A5A5A
LANES = (0, 1)


def to_dev(col):
    """a column's arrays as device tensors (uint64 as int64, uint32 as int32)"""
    import torch
    views = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return {f: torch.from_numpy(np.ascontiguousarray(a).view(views.get(a.dtype, a.dtype)).copy()).cuda()
            for f, a in col.items()}


class Outs:
    """d_out / d_out_off / d_status of one launch with their guards"""

    def __init__(self, pairs, room, sizing=False):
        import torch
        self.pairs, self.room = pairs, room
        self.off = torch.full((pairs + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.status = torch.full((pairs + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.out = None if sizing else torch.full((room + 16 + GUARD,), VG.GUARD, dtype=torch.uint8, device="cuda")

    def args(self):
        return self.out, self.off[GUARD:], self.status[GUARD:]

    def read(self, what):
        off, st = self.off.cpu().numpy().view(np.uint64), self.status.cpu().numpy()
        assert (off[:GUARD] == FILL64).all() and (off[GUARD + self.pairs + 1:] == FILL64).all(), "%s: a store around d_out_off" % what
        assert (st[:GUARD] == 0x5A).all() and (st[GUARD + self.pairs:] == 0x5A).all(), "%s: a store around d_status" % what
        return (None if self.out is None else self.out.cpu().numpy(), off[GUARD:GUARD + self.pairs + 1],
                st[GUARD:GUARD + self.pairs])


def launch(plan, dcols, n, o, base=0, cap=None, stream=None, status=True):
    from dynamicgo_amd import generic as G
    out, off, st = o.args()
    G.values_device(plan, dcols, n, out, off, st if status else None, out_base=base, cap=o.room if cap is None else cap,
                    stream=stream)


def verify(got, want, base, cap, what):
    """out (with guards), off, status against the checker's (arena from base, off, status); cap: nothing at or beyond it"""
    out, off, st = got
    arena, woff, wst = want
    assert off.tolist() == woff, "%s: offsets" % what
    assert st.tolist() == wst, "%s: statuses" % what
    if out is None:
        return
    end = min(cap, woff[-1])
    assert (out[:base] == VG.GUARD).all(), "%s: a store before out_base" % what
    bad = np.nonzero(out[base:max(end, base)] != np.frombuffer(arena[:max(end - base, 0)], dtype=np.uint8))[0]
    assert bad.size == 0, "%s: byte %d of the arena" % (what, base + int(bad[0]))
    assert (out[max(end, base):] == VG.GUARD).all(), "%s: a store at cap or beyond" % what


def run_device(case, knob, lane, base=0, cap=None, sizing=False, want=None):
    import torch
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, n = case
    want = want or VR.encode_batch(kinds, cols, n, fids, base)
    need = want[1][-1]
    cap = need if cap is None else cap
    knob("vals_lane_emit", lane)
    with G.ValuePlan(kinds, fids) as plan:
        o = Outs(n * len(kinds), max(cap, need), sizing)
        launch(plan, [to_dev(c) for c in cols], n, o, base, cap)
        torch.cuda.synchronize()
        got = o.read(name)
    verify(got, want, base, cap, "%s, device entry, lane_emit %d" % (name, lane))
    return got, want


def run_host(case, want=None):
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, n = case
    want = want or VR.encode_batch(kinds, cols, n, fids)
    with G.ValuePlan(kinds, fids) as plan:
        arena, off, status = G._values_host(plan, cols, n)
    assert off.tolist() == want[1] and status.tolist() == want[2], "%s, host entry" % name
    assert arena.tobytes() == want[0], "%s, host entry: bytes" % name


def check(case, knob):
    want = VR.encode_batch(case[1], case[3], case[4], case[2])
    run_host(case, want)
    for lane in LANES:
        run_device(case, knob, lane, want=want)
    return want


# 1 ---------------------------------------------------------------- matrix
def test_kind_by_value_matrix(knob):
    for case in VG.matrix_cases():
        arena, off, _ = check(case, knob)
        if case[0] == "matrix kind %d" % VR.I16:
            vals = [arena[a:b] for a, b in zip(off, off[1:])]
            assert vals[VG.INTS[VR.I16].index(0x10000)] == b"\0\0" and vals[VG.INTS[VR.I16].index(2 ** 15)] == b"\x80\0"
        if case[0] == "matrix kind %d" % VR.BOOL:
            assert arena == bytes([0, 1, 1, 1, 1, 1])
        if case[0] == "matrix kind %d" % VR.DOUBLE:
            assert [struct.unpack(">Q", arena[a:a + 8])[0] for a in off[:-1]] == VG.DOUBLES


# 2 --------------------------------------------------------------- strings
@pytest.mark.parametrize("shift", range(16))
def test_strings_at_every_length_and_residue(knob, shift):
    case = list(VG.string_cases())[shift]
    want = check(case, knob)
    col = case[3][-1]
    assert {int(v) % 16 for v in col["val"]} == set(range(16))  # source residues
    assert int(col["val"][-1]) + int(col["len"][-1]) + 16 == len(col["src"])  # the last payload ends the arena
    if shift in (0, 5):
        assert sorted(col["len"].tolist()) == VG.STRING_LENS
    K = len(case[1])
    assert all((want[1][i * K + K - 1] - want[1][i * K]) == shift for i in range(case[4]))  # the BOOL columns in front


def test_string_outputs_start_at_every_residue():
    """from the inputs alone: over the 16 shifts, every length is written at every output residue mod 16 it can be"""
    seen = set()
    for case in VG.string_cases():
        K, off = len(case[1]), VR.encode_batch(case[1], case[3], case[4])[1]
        seen |= {(off[i * K + K - 1] + 4) % 16 for i in range(case[4])}
    assert seen == set(range(16))


# 3 ------------------------------------------------------- lists and sets
def test_lists_and_sets(knob):
    seen = set()
    for case in VG.list_cases():
        check(case, knob)
        seen |= set(case[1])
        for col in case[3]:
            assert set(np.diff(col["elem_off"].astype(np.int64)).tolist()) <= set(VG.LIST_COUNTS)
    assert seen == {c | et for c in (VR.LIST, VR.SET) for et in VG.ELEM_TYPES}


# 4 ----------------------------------------------------- geometry and writes
@pytest.mark.parametrize("K", range(1, 17))
def test_geometry(knob, K):
    for n in VG.GEOMETRY_N:
        case = VG.geometry_case(K, n)
        want = VR.encode_batch(case[1], case[3], n)
        for lane in LANES if n in (1, 65, 257) else (0,):
            run_device(case, knob, lane, want=want)
        if n == 64:
            run_host(case, want)


def test_cap_below_the_need_and_out_base(knob):
    case = VG.geometry_case(7, 65)
    _, kinds, fids, cols, n = case
    for base in (0, 1, 13, 8191):
        want = VR.encode_batch(kinds, cols, n, fids, base)
        need = want[1][-1]
        for lane in LANES:
            for cap in (need, need - 1, base + (need - base) // 2, base + 1, base, 0):
                run_device(case, knob, lane, base=base, cap=cap, want=want)
    # sizing: no d_out, offsets and statuses only; a NULL d_status is taken too
    run_device(case, knob, 0, base=5, sizing=True)
    import torch
    from dynamicgo_amd import generic as G
    with G.ValuePlan(kinds) as plan:
        o = Outs(n * len(kinds), 0, sizing=True)
        launch(plan, [to_dev(c) for c in cols], n, o, status=False)
        torch.cuda.synchronize()
        _, off, st = o.read("no d_status")
        assert off.tolist() == VR.encode_batch(kinds, cols, n)[1] and (st == 0x5A).all()


def test_one_message_changes_only_its_own_bytes(knob):
    case = VG.geometry_case(7, 65)
    _, kinds, fids, cols, n = case
    (out0, off0, _), _ = run_device(case, knob, 0)
    i, K = 30, len(kinds)
    cols2 = [dict(c) for c in cols]
    cols2[0]["val"] = cols[0]["val"].copy()
    cols2[0]["val"][i] ^= 0xFFFF
    pay = [cols[1]["src"][int(v):int(v) + int(ln)].tobytes() for v, ln in zip(cols[1]["val"], cols[1]["len"])]
    pay[i] = b"another payload, longer than the one before it by a good deal"
    cols2[1] = VG.string_col(pay, phase=3)
    (out1, off1, _), _ = run_device(("changed", kinds, fids, cols2, n), knob, 0)
    a, e0, e1 = int(off0[i * K]), int(off0[(i + 1) * K]), int(off1[(i + 1) * K])
    d = e1 - e0
    assert d == len(pay[i]) - int(cols[1]["len"][i]) and d > 0
    assert (off1[:i * K + 1] == off0[:i * K + 1]).all() and (off1[(i + 1) * K:].astype(np.int64) - d == off0[(i + 1) * K:]).all()
    assert (out1[:a] == out0[:a]).all() and (out1[e1:int(off1[-1])] == out0[e0:int(off0[-1])]).all()
    assert out1[a:e1].tobytes() != out0[a:e0].tobytes()


# 5 ---------------------------------------------------------------- sizing
def test_closed_form_offsets_equal_the_scan(knob):
    """a plan of scalars takes the closed form; the same plan with a zero-length STRING column added goes through
    the scan, and its offsets, the added column's left out, are the same; out_base shifts every offset"""
    _, kinds, _, cols, n = next(VG.matrix_cases())
    empty = VG.string_col([b""] * n)
    for base in (0, 77):
        (_, off_c, _), _ = run_device(("closed", kinds, None, cols, n), knob, 0, base=base)
        (_, off_s, _), _ = run_device(("scanned", kinds + [VR.STRING], None, cols + [empty], n), knob, 0, base=base)
        K = len(kinds)
        scan = off_s[:-1].reshape(n, K + 1)
        assert (scan[:, K] - scan[:, K - 1] == 8).all()  # the DOUBLE before the empty string's 4 bytes
        shrunk = (scan[:, :K].astype(np.int64) - 4 * np.arange(n)[:, None]).reshape(-1)
        assert (shrunk == off_c[:-1].astype(np.int64)).all() and int(off_c[0]) == base
    run_device(("closed struct", [VR.I16, VR.BOOL], [7, -2], [cols[2], cols[0]], n), knob, 0, base=3)
    run_device(("closed sizing", kinds, None, cols, n), knob, 0, base=9, sizing=True)


# 6 ----------------------------------------------------------- error cells
def test_error_cells(knob):
    import torch
    from dynamicgo_amd import generic as G
    n = 6
    lens = np.array([3, 0x80000000, 5, 0xFFFFFFFF, 0x7FFFFFFF, 2], dtype=np.uint32)
    strs = {"val": np.zeros(n, dtype=np.uint64), "len": lens, "src": np.zeros(64, dtype=np.uint8)}
    counts = [2, 2 ** 31, 1, 2 ** 29, 2 ** 29 - 1, 0]
    lists = {"elem_off": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), "elems": np.zeros(8, dtype=np.uint64)}
    kinds = [VR.STRING, VR.LIST | VR.I64, VR.I32]
    cols = [strs, lists, VG.scalar_col([1], n)]
    want_len = [[VR.item_size(k, c) for k, c in zip(kinds, (int(lens[i]), counts[i], 0))] for i in range(n)]
    status = [z[1] for row in want_len for z in row]
    assert status == [0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    off = np.concatenate([[11], 11 + np.cumsum([z[0] for row in want_len for z in row])]).tolist()
    for lane in LANES:  # sizing calls only: no payload is read
        knob("vals_lane_emit", lane)
        with G.ValuePlan(kinds) as plan:
            o = Outs(n * 3, 0, sizing=True)
            launch(plan, [to_dev(c) for c in cols], n, o, base=11)
            torch.cuda.synchronize()
            verify(o.read("error cells"), (b"", off, status), 11, 0, "error cells, sizing")
    # one in-range emit: the flagged cells write the empty value of their kind and read nothing
    lens = np.array([3, 0x80000000, 5], dtype=np.uint32)
    strs = {"val": np.array([0, 9, 3], dtype=np.uint64), "len": lens,
            "src": np.frombuffer(b"abcdefgh" + bytes([VG.GUARD]) * 16, dtype=np.uint8)}
    lists = {"elem_off": np.array([0, 2, 3, 3 + 2 ** 29], dtype=np.uint64), "elems": np.array([1, 2, 3], dtype=np.uint64)}
    case = ("flagged emit", [VR.STRING, VR.SET | VR.I64], None, [strs, lists], 3)
    for lane in LANES:
        (out, off, st), want = run_device(case, knob, lane)
        assert st.tolist() == [0, 0, 1, 0, 0, 1]
        assert want[0][int(off[2]):int(off[3])] == b"\0\0\0\0" and want[0][int(off[5]):] == b"\x0a\0\0\0\0"


# 7 ------------------------------------------------------------ struct mode
def test_struct_mode(knob):
    from dynamicgo_amd import generic as G
    for case in VG.struct_cases():
        arena, off, _ = check(case, knob)
        if case[0] == "struct presence":
            K = 3
            msgs = [arena[off[i * K]:off[(i + 1) * K]] for i in range(8)]
            assert msgs[0] == b"\0" and all(m[-1] == 0 for m in msgs) and len(set(msgs)) == 8
            # read back: GetByPath and the casts give the inputs
            cols = G.columns_batch(msgs, [([G.PathFieldId(1)], "int"), ([G.PathFieldId(255)], "str"),
                                          ([G.PathFieldId(256)], "list[float64]")])
            ins = case[3]
            for j, c in enumerate(cols):
                assert c.valid.tolist() == [bool(i >> j & 1) for i in range(8)]
            s32 = lambda v: ((int(v) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000  # noqa: E731 (written at 32 bits, read signed)
            assert [int(v) for v, ok in zip(cols[0].values, cols[0].valid) if ok] == \
                [s32(v) for v, ok in zip(ins[0]["val"].tolist(), cols[0].valid) if ok]
            assert [v for v, ok in zip(cols[1].values, cols[1].valid) if ok] == \
                [ins[1]["src"][int(a):int(a) + int(ln)].tobytes()
                 for a, ln, ok in zip(ins[1]["val"], ins[1]["len"], cols[1].valid) if ok]
            eo = ins[2]["elem_off"]
            assert cols[2].values.view(np.uint64).tolist() == \
                [int(e) for i in range(8) if cols[2].valid[i] for e in ins[2]["elems"][int(eo[i]):int(eo[i + 1])]]
            got = G.get_by_path_batch(msgs, [[G.PathFieldId(255)]])
            assert [r[0].status == G.OK for r in got] == [bool(i >> 1 & 1) for i in range(8)]
        if case[0] == "struct field ids":
            assert case[2] == [1, 255, 256, 32767, -1]


def test_build_structs_and_set_columns_batch():
    """the public host wrappers over numpy arrays and Python sequences"""
    from dynamicgo_amd import generic as G
    ints = np.array([1, -2, 70000, 2 ** 31 - 1], dtype=np.int64)
    strs = [b"a", b"", "é", b"four"]
    dbl = [[1.5], [], [float("inf"), -0.0], [2.0, 3.0, 4.0]]
    msgs = G.build_structs_batch([(4, "i32", ints), (7, "str", strs, [1, 0, 1, 1]), (9, ("list", "f64"), dbl)])
    want = [struct.pack(">bhi", 8, 4, int(v)) + (struct.pack(">bhi", 11, 7, len(s)) + s if p else b"") +
            struct.pack(">bhbi", 15, 9, 4, len(d)) + b"".join(struct.pack(">d", x) for x in d) + b"\0"
            for v, s, p, d in zip(ints, [b"a", b"", "é".encode(), b"four"], [1, 0, 1, 1], dbl)]
    assert msgs == want
    arena, off, st = G.values_batch([ints, strs], ["i16", "binary"])
    assert arena.tobytes() == b"".join(struct.pack(">H", int(v) & 0xFFFF) + struct.pack(">i", len(s)) + s
                                       for v, s in zip(ints, [b"a", b"", "é".encode(), b"four"])) and not st.any()
    res = G.set_columns_batch(msgs, [], [(G.PathFieldId(4), "i32", ints + 1), (G.PathFieldId(5), "i64", ints)])
    cols = G.columns_batch([r.raw for r in res], [([G.PathFieldId(4)], "int"), ([G.PathFieldId(5)], "int")])
    assert all(r.status == G.EDIT_OK and r.existed == (True, False) for r in res)
    assert cols[0].values.tolist() == [2, -1, 70001, -2 ** 31] and cols[1].values.tolist() == ints.tolist()
    with pytest.raises(ValueError):
        G.set_columns_batch(msgs, [], [(G.PathFieldId(k), "i32", ints) for k in range(1, G.EDITM_MAX_ITEMS + 2)])
    assert G.val_kind("i32") == 8 and G.val_kind(("list", "f64")) == 0x44 and G.val_kind(("set", "bool")) == 0x82
    with pytest.raises(ValueError):
        G.val_kind(("list", "str"))


def test_plan_create_and_present_rejects():
    import torch
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()

    def create(kinds, K=None, ids=None):
        h = C.c_void_p()
        arr = None if ids is None else np.array(ids, dtype=np.int16)
        rc = L.dg_vals_create(ctx.h, bytes(kinds), len(kinds) if K is None else K, None if arr is None else arr.ctypes.data,
                              C.byref(h))
        if rc == 0:
            assert L.dg_vals_count(h) == len(kinds)
            assert [L.dg_vals_wire_type(h, k) for k in range(len(kinds))] == [VR.wire_type(k) for k in kinds]
            assert L.dg_vals_wire_type(h, len(kinds)) == 0
            L.dg_vals_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create([2, 3, 4, 6, 8, 10, 11, 0x42, 0x8A])[0] == 0 and create([8] * 16)[0] == 0
    for kinds, text in (([8, 0], "column 1: unknown kind 0"), ([12], "column 0: unknown kind 12"),
                        ([8, 8, 0x4B], "column 2: unknown kind 75"), ([0xC3], "column 0: unknown kind 195"),
                        ([0x40], "column 0: unknown kind 64"), ([5, 8], "column 0: unknown kind 5")):
        rc, err = create(kinds)
        assert rc == -6 and text in err, (kinds, rc, err)  # DG_E_ARG
    for K in (0, 17):
        rc, err = create([8] * 17, K=K)
        assert rc == -6 and "%d columns (1 to 16)" % K in err, (K, rc, err)
    # d_present in a plan without field ids: DG_E_ARG at the call, device and host entry
    col = VG.scalar_col([1, 2, 3])
    col["present"] = np.array([1, 0, 1], dtype=np.uint8)
    with G.ValuePlan([VR.I32]) as plan:
        o = Outs(3, 64)
        with pytest.raises(_lib.DGError, match="-6.*d_present in a plan without field ids"):
            launch(plan, [to_dev(col)], 3, o)
        with pytest.raises(_lib.DGError, match="-6.*d_present in a plan without field ids"):
            G._values_host(plan, [col], 3)
        torch.cuda.synchronize()
        out, _, _ = o.read("refused")
        assert (out == VG.GUARD).all()
        launch(plan, [to_dev(VG.scalar_col([1]))], 0, o)  # n = 0: DG_OK, nothing launched, nothing written
        torch.cuda.synchronize()
        assert (o.off.cpu().numpy().view(np.uint64) == FILL64).all()


# 8 ---------------------------------------------------- the chain on the device
@pytest.fixture(scope="module")
def all_corpus():
    import modelgen as M
    import oracle
    return M.Corpus(oracle.RefOracle() or oracle.PortOracle(), "all", 300)


@pytest.mark.parametrize("op", ("identity", "changed"))
def test_cols_torch_vals_editm_on_one_stream(knob, all_corpus, op):
    """columns_device + column_list_device, a torch op, values_device, edit_many_device, all on one stream with no
    synchronisation between them. The i32 field 4 and the string field 7 are set below the root, the list<double>
    inner.c below field 9 (one parent per many-edit, so two edits of the same batch). identity: where the read found
    all the items of an edit, its output is the input message byte for byte (a missing item is an insert, as SetMany
    has it, so there the checker's many-edit over the checker's values decides, as it does for `changed`: field 4
    + 1, field 7 from field 18's payloads in reversed message order, the elements doubled)."""
    import torch
    import editmref as EM
    import tgetref as R
    from dynamicgo_amd import generic as G
    msgs = all_corpus.msgs
    n = len(msgs)
    F = R.FIELD
    arena_np = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    total = int(in_off[n])
    arena, d_in = torch.from_numpy(arena_np).cuda(), torch.from_numpy(in_off).cuda()
    columns = [([G.PathFieldId(4)], "int"), ([G.PathFieldId(7)], "str"), ([G.PathFieldId(18)], "str"),
               ([G.PathFieldId(9), G.PathFieldId(3)], "list[float64]")]
    caps = np.array([(len(m) + max(map(len, msgs)) + 79) & ~15 for m in msgs])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    d_oo = torch.from_numpy(out_off).cuda()
    stream = torch.cuda.Stream()
    knob("vals_lane_emit", 0)
    with G.ColumnPlan(columns) as cp, G.ValuePlan(["i32", "str"]) as vp_a, G.ValuePlan([("list", "f64")]) as vp_b, \
            G.EditManyPlan([], [G.PathFieldId(4), G.PathFieldId(7)], G.EDIT_SET) as ep_a, \
            G.EditManyPlan([G.PathFieldId(9)], [G.PathFieldId(3)], G.EDIT_SET) as ep_b:
        val = torch.zeros((4, n), dtype=torch.int64, device="cuda")
        cell = torch.zeros((4, n, 2), dtype=torch.int32, device="cuda")
        lens = torch.zeros((4, n), dtype=torch.int32, device="cuda")
        elem_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        elems = torch.zeros(total // 8 + 1, dtype=torch.int64, device="cuda")
        cap_a, cap_b = 8 * n + 2 * total, 5 * n + total
        va = torch.full((cap_a + 16,), VG.GUARD, dtype=torch.uint8, device="cuda")
        vb = torch.full((cap_b + 16,), VG.GUARD, dtype=torch.uint8, device="cuda")
        va_off = torch.zeros(2 * n + 1, dtype=torch.int64, device="cuda")
        vb_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        outs = [torch.full((int(out_off[n]) + 64,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
        ols = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        rets = [torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.columns_device(cp, arena, d_in, n, val, cell, lens, stream=stream)
            G.column_list_device(cp, 3, arena, n, val[3], cell[3], lens[3], elem_off, elems, elems.numel(), stream=stream)
            if op == "identity":
                ints, s_val, s_len, els = val[0], val[1], lens[1], elems
            else:
                ints, s_val, s_len = val[0] + 1, val[2].flip(0).contiguous(), lens[2].flip(0).contiguous()
                els = (2 * elems.view(torch.float64)).view(torch.int64)
            G.values_device(vp_a, [{"val": ints}, {"val": s_val, "len": s_len, "src": arena}], n, va, va_off, cap=cap_a,
                            stream=stream)
            G.values_device(vp_b, [{"elem_off": elem_off, "elems": els}], n, vb, vb_off, cap=cap_b, stream=stream)
            G.edit_many_device(ep_a, arena, d_in, n, vp_a.wire_types, va, va_off, [0, 0], outs[0], d_oo, ols[0], rets[0],
                               stream=stream)
            G.edit_many_device(ep_b, arena, d_in, n, vp_b.wire_types, vb, vb_off, [0], outs[1], d_oo, ols[1], rets[1],
                               stream=stream)
        torch.cuda.synchronize()
        # the checker's values from the columns as read, with the same ops in numpy
        h_val, h_len = val.cpu().numpy().view(np.uint64), lens.cpu().numpy().view(np.uint32)
        h_eo, h_el = elem_off.cpu().numpy().view(np.uint64), elems.cpu().numpy().view(np.uint64)
        status = cell.cpu().numpy().reshape(4, n, 2).view(np.uint8).reshape(4, n, 8)[:, :, 0]
        if op == "identity":
            w_int, w_sv, w_sl, w_el = h_val[0], h_val[1], h_len[1], h_el
        else:
            w_int, w_sv, w_sl = h_val[0] + np.uint64(1), h_val[2][::-1].copy(), h_len[2][::-1].copy()
            w_el = (2 * h_el.view(np.float64)).view(np.uint64)
        a_bytes, a_off, _ = VR.encode_batch([VR.I32, VR.STRING], [{"val": w_int}, {"val": w_sv, "len": w_sl, "src": arena_np}], n)
        b_bytes, b_off, _ = VR.encode_batch([VR.LIST | VR.DOUBLE], [{"elem_off": h_eo, "elems": w_el}], n)
        assert va_off.cpu().numpy().tolist() == a_off and vb_off.cpu().numpy().tolist() == b_off
        assert va.cpu().numpy()[:a_off[-1]].tobytes() == a_bytes and vb.cpu().numpy()[:b_off[-1]].tobytes() == b_bytes
        same = [0, 0]
        for e, (out, ol, ret) in enumerate(zip(outs, ols, rets)):
            h_out, h_ol, h_ret = out.cpu().numpy(), ol.cpu().numpy(), ret.cpu().numpy().view(np.uint64)
            for i, m in enumerate(msgs):
                if e == 0:
                    items = [((F, 4), a_bytes[a_off[2 * i]:a_off[2 * i + 1]], R.I32),
                             ((F, 7), a_bytes[a_off[2 * i + 1]:a_off[2 * i + 2]], R.STRING)]
                    w_ret, w_out = EM.edit_many(EM.SET_OP, m, [], items, cap=int(caps[i]))
                    found = status[0, i] == 0 and status[1, i] == 0
                else:
                    items = [((F, 3), b_bytes[b_off[i]:b_off[i + 1]], R.LIST)]
                    w_ret, w_out = EM.edit_many(EM.SET_OP, m, [(F, 9)], items, cap=int(caps[i]))
                    found = status[3, i] == 0
                assert int(h_ret[i]) == w_ret, (op, e, i, hex(int(h_ret[i])), hex(w_ret))
                g_out = h_out[int(out_off[i]):int(out_off[i]) + (int(h_ol[i]) if w_ret & 0xFF == 0 else 0)].tobytes()
                assert g_out == w_out, (op, e, i)
                if op == "identity" and found:
                    assert g_out == m, (e, i)
                    same[e] += 1
        if op == "identity":
            assert same[0] >= 50 and same[1] >= 20, same


# 9 --------------------------------------------------------------- streams
def test_two_streams_and_a_column_read_beside(knob):
    import torch
    import colsgen as CG
    from dynamicgo_amd import generic as G
    from test_gpu_cols import Outputs, compare as cols_compare, to_cols, upload
    knob("vals_lane_emit", 0)
    cases = [VG.geometry_case(7, 257), VG.geometry_case(16, 1025)]
    wants = [VR.encode_batch(c[1], c[3], c[4]) for c in cases]
    msgs = CG.geometry_messages(257)
    cols_want = CG.expect(msgs, CG.GEOMETRY_COLUMNS)
    arena, d_off, _ = upload(msgs)
    sa, sb, sc = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    with G.ValuePlan(cases[0][1]) as pa, G.ValuePlan(cases[1][1]) as pb, G.ColumnPlan(to_cols(CG.GEOMETRY_COLUMNS)) as cp:
        da, db = [to_dev(c) for c in cases[0][3]], [to_dev(c) for c in cases[1][3]]
        rounds = [(Outs(257 * 7, wants[0][1][-1]), Outs(1025 * 16, wants[1][1][-1]), Outputs(len(msgs), cp.count))
                  for _ in range(3)]
        torch.cuda.synchronize()
        for oa, ob, oc in rounds:  # no synchronisation between the launches
            launch(pa, da, 257, oa, stream=sa)
            launch(pb, db, 1025, ob, stream=sb)
            G.columns_device(cp, arena, d_off, len(msgs), *oc.args(), stream=sc)
        torch.cuda.synchronize()
        for r, (oa, ob, oc) in enumerate(rounds):
            verify(oa.read("stream a"), wants[0], 0, wants[0][1][-1], "round %d, stream a" % r)
            verify(ob.read("stream b"), wants[1], 0, wants[1][1][-1], "round %d, stream b" % r)
            cols_compare(oc.read("round %d" % r), [{f: a for f, a in CG.arrays(col).items() if f in CG.CELL_FIELDS}
                                                   for col in cols_want], "round %d, columns beside" % r)


# 10 ----------------------------------------------------------- far offsets
@pytest.fixture(scope="module")
def far_arenas():
    import torch
    inp, out = FO.Arena(), FO.Arena()
    yield inp, out
    inp.free()
    out.free()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lane", LANES)
@pytest.mark.parametrize("B", FO.BOUNDS, ids=["2G", "4G"])
def test_far_offsets(knob, far_arenas, B, lane):
    """STRING payloads in a source arena at offsets below, across and beyond B, written to an output arena at an
    out_base that puts the pivot's value across B; the aliases of the source hold decoys, and everything outside the
    values in the output arena is still FILL"""
    import torch
    from dynamicgo_amd import generic as G
    inp, outa = far_arenas
    rng = random.Random(61)
    pay = [VG.payload(rng, rng.choice((1, 5, 8, 13, 24, 40, 300))) for _ in range(40)]
    pay.insert(20, VG.payload(rng, 100))
    n, pivot = len(pay), 20
    src_off = FO.place([len(p) for p in pay], B, pivot, -37)  # the pivot's payload straddles B
    FO.check_layout(src_off, B, guard=0, tail=FO.TAIL)
    inp.put_input(src_off, pay, B)
    col = {"val": src_off[:-1].astype(np.uint64), "len": np.array([len(p) for p in pay], dtype=np.uint32)}
    rel = [0]
    for p in pay:
        rel.append(rel[-1] + 4 + len(p))
    base = B - rel[pivot] - 6  # the pivot's item: its length ends 2 bytes below B, its payload lies across B
    woff = [base + r for r in rel]
    arena = b"".join(struct.pack(">i", len(p)) + p for p in pay)
    FO.check_layout(np.array(woff, dtype=np.int64), B)
    assert woff[pivot] + 4 < B < woff[pivot + 1] and any(int(v) >= B for v in col["val"]) and any(int(v) + 40 < B for v in col["val"])
    o_off = np.array(woff, dtype=np.int64)
    outa.prefill(o_off, B)
    knob("vals_lane_emit", lane)
    with G.ValuePlan([VR.STRING]) as plan:
        off = torch.full((n + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        st = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        d = to_dev(col)
        d["src"] = inp.base
        G.values_device(plan, [d], n, outa.base, off[GUARD:], st[GUARD:], out_base=base, cap=woff[-1])
        torch.cuda.synchronize()
    h_off, h_st = off.cpu().numpy(), st.cpu().numpy()
    assert h_off[GUARD:GUARD + n + 1].tolist() == woff and (h_off[:GUARD].view(np.uint64) == FILL64).all()
    assert (h_off[GUARD + n + 1:].view(np.uint64) == FILL64).all()
    assert (h_st[GUARD:GUARD + n] == 0).all() and (h_st[:GUARD] == 0x5A).all() and (h_st[GUARD + n:] == 0x5A).all()
    got = outa.collect(o_off, B, what="d_out at %#x, lane_emit %d" % (B, lane))
    assert got.tobytes() == arena
