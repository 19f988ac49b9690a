"""GPU: row column writes (dynamicgo_amd.generic over dg_rvals_*) against the
checker of rvalsref.py, which test_rvals_codec.py holds against the reference's
j2t. Every case goes through the device entry and the host entry; every byte,
every offset and every status is compared, with guard bytes and guard entries
around d_out, d_out_off, both status arrays and d_work. The inputs are
rvalsgen's, which test_rvals_host.py runs through the host build of the same
encode."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import faroff as FO
import rvalsgen as RG
import rvalsref as RR
import valsgen as VG
import valsref as VR

pytestmark = pytest.mark.gpu

GUARD = 64
FILL64 = 0x5A5A5A5A5A5A5A5A
CANARY = {"val": 0x7FFFFFFFFFFFFFF0, "len": 0xFFFFFFFF, "elem_off": 2 ** 62, "present": 1}


def to_dev(col, canaries=0):
    """a column's arrays as device tensors (uint64 as int64, uint32 as int32); with `canaries`, that many entries behind
    each per-row array that would show in the output if a row at or behind n_rows were read"""
    import torch
    views = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    out = {}
    for f, a in col.items():
        if canaries and f in CANARY:
            a = np.concatenate([a, np.full(canaries, CANARY[f], dtype=a.dtype)])
        out[f] = torch.from_numpy(np.ascontiguousarray(a).view(views.get(a.dtype, a.dtype)).copy()).cuda()
    return out


def dev_offsets(row_off):
    import torch
    return torch.from_numpy(np.ascontiguousarray(row_off).view(np.int64).copy()).cuda()


class Outs:
    """d_out / d_out_off / d_status / d_cell_status of one launch with their guards"""

    def __init__(self, n, cells, room, sizing=False):
        import torch
        self.n, self.cells, self.room = n, cells, room
        self.off = torch.full((n + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.status = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.cell_status = torch.full((cells + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.out = None if sizing else torch.full((room + 16 + GUARD,), RG.GUARD, dtype=torch.uint8, device="cuda")

    def read(self, what):
        off, st, cst = self.off.cpu().numpy().view(np.uint64), self.status.cpu().numpy(), self.cell_status.cpu().numpy()
        assert (off[:GUARD] == FILL64).all() and (off[GUARD + self.n + 1:] == FILL64).all(), "%s: a store around d_out_off" % what
        assert (st[:GUARD] == 0x5A).all() and (st[GUARD + self.n:] == 0x5A).all(), "%s: a store around d_status" % what
        assert (cst[:GUARD] == 0x5A).all() and (cst[GUARD + self.cells:] == 0x5A).all(), "%s: a store around d_cell_status" % what
        return (None if self.out is None else self.out.cpu().numpy(), off[GUARD:GUARD + self.n + 1], st[GUARD:GUARD + self.n],
                cst[GUARD:GUARD + self.cells])


def work_for(plan, n, n_rows):
    """d_work of exactly the bytes asked for, between guards"""
    import torch
    need = plan.work_bytes(n, n_rows)
    t = torch.full((need + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    return t, t[GUARD:GUARD + need]


def work_guards(t, what):
    h = t.cpu().numpy()
    assert (h[:GUARD] == 0x5A).all() and (h[-GUARD:] == 0x5A).all(), "%s: a store around d_work" % what


def launch(plan, dcols, d_row_off, n, n_rows, o, work, base=0, cap=None, stream=None, statuses=True):
    from dynamicgo_amd import generic as G
    G.row_values_device(plan, dcols, d_row_off, n, n_rows, o.out, o.off[GUARD:], work, o.status[GUARD:] if statuses else None,
                        o.cell_status[GUARD:] if statuses else None, out_base=base, cap=o.room if cap is None else cap,
                        stream=stream)


def rebase(want, base):
    return want[0], [x + base for x in want[1]], want[2], want[3]


def verify(got, want, base, cap, what, cells=True):
    """out (with guards), off, statuses against the checker's (arena from base, off, status, cell status)"""
    out, off, st, cst = got
    arena, woff, wst, wcst = want
    assert off.tolist() == woff, "%s: offsets" % what
    assert st.tolist() == wst, "%s: statuses" % what
    if cells:
        assert cst.tolist() == wcst, "%s: cell statuses" % what
    if out is None:
        return
    end = min(cap, woff[-1])
    assert (out[:base] == RG.GUARD).all(), "%s: a store before out_base" % what
    bad = np.nonzero(out[base:max(end, base)] != np.frombuffer(arena[:max(end - base, 0)], dtype=np.uint8))[0]
    assert bad.size == 0, "%s: byte %d of the arena" % (what, base + int(bad[0]))
    assert (out[max(end, base):] == RG.GUARD).all(), "%s: a store at cap or beyond" % what


def checker(case):
    return RR.encode_batch(*case[1:])


def run_device(case, want, base=0, cap=None, sizing=False, canaries=0):
    import torch
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, row_off, n, n_rows = case
    want = rebase(want, base)
    need = want[1][-1]
    cap = need if cap is None else cap
    with G.RowValuePlan(kinds, fids) as plan:
        o = Outs(n, n_rows * len(kinds), max(cap, need), sizing)
        wt, work = work_for(plan, n, n_rows)
        launch(plan, [to_dev(c, canaries) for c in cols], dev_offsets(row_off), n, n_rows, o, work, base, cap)
        torch.cuda.synchronize()
        got = o.read(name)
        work_guards(wt, name)
    verify(got, want, base, cap, "%s, device entry" % name)
    return got


def run_host(case, want):
    from dynamicgo_amd import generic as G
    name, kinds, fids, cols, row_off, n, n_rows = case
    with G.RowValuePlan(kinds, fids) as plan:
        arena, off, status, cst = G._row_values_host(plan, cols, row_off, n, n_rows)
    assert off.tolist() == want[1] and status.tolist() == want[2] and cst.tolist() == want[3], "%s, host entry" % name
    assert arena.tobytes() == want[0], "%s, host entry: bytes" % name


def check(case):
    want = checker(case)
    run_host(case, want)
    run_device(case, want)
    return want


# 1 --------------------------------------------------------- the generated cases
GROUPS = {"matrix": RG.matrix_cases, "counts": RG.count_cases, "present": RG.present_cases, "strings": RG.string_cases,
          "lists": RG.list_cases, "chunks": RG.chunk_cases, "overlap": RG.overlap_cases}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_generated_cases(group):
    kinds, statuses = set(), set()
    for case in GROUPS[group]():
        want = check(case)
        kinds |= set(case[1])
        statuses |= set(want[2])
    if group == "matrix":
        assert kinds == set(RR.ALL_KINDS)
    # rows are owned twice only across a message whose offsets fall
    assert statuses == ({RR.OK, RR.E_RANGE} if group == "overlap" else {RR.OK})


@pytest.mark.parametrize("K", (1, 2, 7, 16))
def test_geometry(K):
    """both emit routes at every K: the columns with d_present (scanned), and for K scalars the fixed stride"""
    for rows in (1, 64, 65, 257):
        case = RG.geometry_case(K, rows)
        want = checker(case)
        run_device(case, want)
        if rows == 65:
            run_host(case, want)
    check(RG.scalar_case())


@pytest.mark.parametrize("scalars", (True, False), ids=("fixed", "scanned"))
def test_n_and_cells_around_the_wave_the_block_and_the_scan_tile(scalars):
    """n messages of one row each and one message of n rows, K = 1 and 2, n around 64, 256 and 2048"""
    rng = random.Random(41)
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049):
        for K in (1, 2):
            kinds = ([VR.I16, VR.I64] if scalars else [VR.STRING, VR.I32])[:K]
            cols = [VG.column_for(rng, k, n) for k in kinds]
            if not scalars and K == 2:
                cols[1]["present"] = RG.present_col(rng, n)
            for row_off in (np.arange(n + 1), [0, n]):
                case = RG.case("n=%d K=%d" % (n, K), kinds, cols, row_off, n)
                run_device(case, checker(case))


# 2 -------------------------------------------------------- caps and sizing
def test_cap_below_the_need_and_out_base():
    """cap at the need, below it and 0, at several out_base; on a small batch every cap from out_base to the need,
    which cuts inside every list header, field header, length, payload and STOP"""
    import torch
    from dynamicgo_amd import generic as G
    case = RG.geometry_case(7, 65)
    want = checker(case)
    for base in (0, 1, 13, 8191):
        need = want[1][-1] + base
        for cap in (need, need - 1, base + (need - base) // 2, base + 1, base, 0):
            run_device(case, want, base=base, cap=cap)
    run_device(case, want, base=5, sizing=True)
    small = RG.geometry_case(7, 4, n=3, seed=5)
    _, kinds, fids, cols, row_off, n, n_rows = small
    swant = rebase(checker(small), 5)
    need = swant[1][-1]
    with G.RowValuePlan(kinds, fids) as plan:
        dcols, d_ro = [to_dev(c) for c in cols], dev_offsets(row_off)
        wt, work = work_for(plan, n, n_rows)
        outs = [Outs(n, n_rows * 7, need) for _ in range(5, need + 1)]
        for cap, o in zip(range(5, need + 1), outs):
            launch(plan, dcols, d_ro, n, n_rows, o, work, 5, cap)
        torch.cuda.synchronize()
        for cap, o in zip(range(5, need + 1), outs):
            verify(o.read("cap %d" % cap), swant, 5, cap, "cap %d" % cap)
        work_guards(wt, "caps")
        # both status arrays NULL
        o = Outs(n, n_rows * 7, need)
        launch(plan, dcols, d_ro, n, n_rows, o, work, 5, need, statuses=False)
        torch.cuda.synchronize()
        out, off, st, cst = o.read("no statuses")
        assert off.tolist() == swant[1] and (st == 0x5A).all() and (cst == 0x5A).all()
        assert out[5:need].tobytes() == swant[0]


# 3 ------------------------------------------------------------------ flags
def test_range_and_size_flags():
    """flagged messages are empty lists, flagged cells empty values; canary rows behind n_rows and the payloads of
    rows that no OK message owns (lengths of 2^31 - 64) leave no trace"""
    names = []
    for case in RG.flag_cases():
        want = checker(case)
        run_device(case, want, sizing=True, canaries=3)
        run_device(case, want, canaries=3)
        run_host(case, want)
        names.append(case[0])
        if case[0] == "range flags":
            assert want[2] == [0, 2, 2, 2, 0, 2, 2, 0]
            assert want[0][want[1][1]:want[1][2]] == b"\x0c\0\0\0\0"
        if case[0] == "size flags":
            assert want[2] == [0, 1, 0, 0, 0] and sum(want[3]) == 2
        if case[0].startswith("a list cell"):
            assert want[2] == [0, 0, 0] and want[3][4 * 2] == RR.E_SIZE and sum(want[3]) == 1
    assert len(names) == 3


def test_count_flags_in_a_sizing_call():
    """a count of 2^31 under n_rows = 2^31 + 8: the fixed-stride route's sizing call reads d_row_off alone"""
    import torch
    from dynamicgo_amd import generic as G
    (name, kinds, fids, cols, row_off, n, n_rows), (woff, wst) = RG.count_flag_case()
    with G.RowValuePlan(kinds, fids) as plan:
        o = Outs(n, 0, 0, sizing=True)
        t = torch.full((4096 + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        G.row_values_device(plan, [to_dev(c) for c in cols], dev_offsets(row_off), n, n_rows, None, o.off[GUARD:],
                            t[GUARD:GUARD + 4096], o.status[GUARD:], None, out_base=7)
        torch.cuda.synchronize()
        _, off, st, _ = o.read(name)
        work_guards(t, name)
    assert off.tolist() == [x + 7 for x in woff] and st.tolist() == wst


def test_messages_times_columns_beyond_2_32():
    """the cells are the rows', so n * K may pass 2^32 - 1 where n_rows * K does not: 2^28 messages of a plan of 16
    columns over 2 rows in a sizing call, the first and the last message owning a row each, the others empty"""
    import torch
    from dynamicgo_amd import generic as G
    n, K, n_rows = 2 ** 28, 16, 2
    kinds, fids = [VR.I64, VR.DOUBLE] * 5 + RG.SCALARS, RG.field_ids(16)
    stride = 1 + sum(3 + VR.WIDTH[k] for k in kinds)
    row_off = torch.ones(n + 1, dtype=torch.int64, device="cuda")
    row_off[0], row_off[n] = 0, 2
    cols = [to_dev(VG.scalar_col([j, j + 1])) for j in range(K)]
    with G.RowValuePlan(kinds, fids) as plan:
        off = torch.full((n + 1 + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        st = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        work = torch.empty(plan.work_bytes(n, n_rows), dtype=torch.uint8, device="cuda")
        G.row_values_device(plan, cols, row_off, n, n_rows, None, off, work, st, None)
        torch.cuda.synchronize()
        assert off[:3].tolist() == [0, 5 + stride, 10 + stride] and off[n - 1:n + 1].tolist() == [5 * n - 5 + stride, 5 * n + 2 * stride]
        assert (off[n + 1:] == FILL64).all().item() and not st[:n].any().item() and (st[n:] == 0x5A).all().item()
    del off, st, work, row_off
    torch.cuda.empty_cache()


# 4 ----------------------------------------------------------- independence
def test_one_row_changes_only_its_own_message():
    rng = random.Random(42)
    _, kinds, fids, cols, row_off, n, n_rows = RG.geometry_case(7, 257)
    g = n_rows // 2
    i = next(k for k in range(n) if int(row_off[k]) <= g < int(row_off[k + 1]))  # the message that owns row g
    assert 0 < i < n - 1
    pay = [VG.payload(rng, int(ln)) for ln in cols[1]["len"]]
    pay[g] = pay[g] + b"0123456789+"
    cols1 = list(cols)
    cols1[1] = dict(VG.string_col(pay, phase=5), present=np.ones(n_rows, dtype=np.uint8))
    cols0 = list(cols)
    pay0 = list(pay)
    pay0[g] = pay[g][:-11]
    cols0[1] = dict(VG.string_col(pay0, phase=5), present=np.ones(n_rows, dtype=np.uint8))
    c0, c1 = ("before", kinds, fids, cols0, row_off, n, n_rows), ("after", kinds, fids, cols1, row_off, n, n_rows)
    out0, off0, _, _ = run_device(c0, checker(c0))
    out1, off1, _, _ = run_device(c1, checker(c1))
    a, e0, e1 = int(off0[i]), int(off0[i + 1]), int(off1[i + 1])
    assert e1 - e0 == 11
    assert (off1[:i + 1] == off0[:i + 1]).all() and (off1[i + 1:].astype(np.int64) - 11 == off0[i + 1:]).all()
    assert (out1[:a] == out0[:a]).all() and (out1[e1:int(off1[-1])] == out0[e0:int(off0[-1])]).all()
    assert out1[a:e1].tobytes() != out0[a:e0].tobytes()


# 5 --------------------------------------------------- refusals, empty batches
def test_plan_create_rejects_refusals_and_empty_batches():
    import torch
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import Context, default_context
    L, ctx = _lib.lib(), default_context()

    def create(kinds, K=None, ids=True, container=15):
        h = C.c_void_p()
        kk = np.array(kinds, dtype=np.uint8)
        arr = np.arange(1, len(kinds) + 1, dtype=np.int16)
        rc = L.dg_rvals_create(ctx.h, kk.ctypes.data, len(kinds) if K is None else K, arr.ctypes.data if ids else None,
                               container, C.byref(h))
        if rc == 0:
            assert L.dg_rvals_count(h) == len(kinds) and L.dg_rvals_wire_type(h) == container
            L.dg_rvals_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create(RR.ALL_KINDS[:16])[0] == 0 and create(RR.ALL_KINDS[16:], container=14)[0] == 0
    assert L.dg_rvals_count(None) == 0 and L.dg_rvals_wire_type(None) == 0 and L.dg_rvals_work_bytes(None, 1, 1) == 0
    for kinds, text in (([8, 0], "column 1: unknown kind 0"), ([12], "column 0: unknown kind 12"), ([13], "column 0: unknown kind 13"),
                        ([8, 11, 0x4B], "column 2: unknown kind 75"), ([0xC8], "column 0: unknown kind 200"),
                        ([0x4C], "column 0: unknown kind 76")):
        rc, err = create(kinds)
        assert rc == -6 and text in err, (kinds, rc, err)  # DG_E_ARG
    for K in (0, 17):
        rc, err = create([8] * 17, K=K)
        assert rc == -6 and "%d columns (1 to 16)" % K in err, (K, rc, err)
    rc, err = create([8], ids=False)
    assert rc == -6 and "no field ids" in err
    for container in (0, 12, 13, 16):
        rc, err = create([8], container=container)
        assert rc == -6 and "container %d" % container in err
    with pytest.raises(ValueError):
        G.RowValuePlan([8], None)
    with pytest.raises(ValueError):
        G.RowValuePlan([("list", "str")], [1])
    case = RG.geometry_case(2, 64)
    _, kinds, fids, cols, row_off, n, n_rows = case
    with G.RowValuePlan(kinds, fids, "set") as plan:
        assert plan.wire_type == 14 and plan.count == 2
        o = Outs(n, n_rows * 2, 4096)
        wt, work = work_for(plan, n, n_rows)
        dcols, d_ro = [to_dev(c) for c in cols], dev_offsets(row_off)
        with pytest.raises(_lib.DGError, match="-3.*d_work"):  # DG_E_NOMEM
            launch(plan, dcols, d_ro, n, n_rows, o, work[:work.numel() - 8])
        with pytest.raises(_lib.DGError, match="-1.*d_work null or not 8-byte aligned"):
            launch(plan, dcols, d_ro, n, n_rows, o, work[4:])
        with pytest.raises(_lib.DGError, match="-1.*d_row_off null or not 8-byte aligned"):
            launch(plan, dcols, None, n, n_rows, o, work)
        with pytest.raises(_lib.DGError, match="-1.*d_out_off null or not 8-byte aligned"):
            G.row_values_device(plan, dcols, d_ro, n, n_rows, o.out, None, work)
        with pytest.raises(_lib.DGError, match="-1.*column 1: null buffer"):
            launch(plan, [dcols[0], dict(dcols[1], val=None)], d_ro, n, n_rows, o, work)
        with pytest.raises(_lib.DGError, match="-1.*column 0: values, offsets or elements not aligned"):
            launch(plan, [dict(dcols[0], val=dcols[0]["val"].view(torch.uint8)[4:]), dcols[1]], d_ro, n, n_rows, o, work)
        with pytest.raises(_lib.DGError, match="-1.*batch of 2147483648 rows x 2 columns"):
            launch(plan, dcols, d_ro, n, 2 ** 31, o, work)
        assert L.dg_rvals_work_bytes(plan.h, n, 2 ** 31) == 0 and L.dg_rvals_work_bytes(plan.h, 2 ** 32, 1) == 0
        with pytest.raises(_lib.DGError, match="-1.*null columns"):
            _lib.check(L.dg_rvals_batch_device(ctx.h, plan.h, None, d_ro.data_ptr(), n, n_rows, 0, None, 0, o.off.data_ptr(),
                                               None, None, work.data_ptr(), work.numel(), None))
        other = Context()
        with G.RowValuePlan(kinds, fids, ctx=other) as foreign:
            with pytest.raises(_lib.DGError, match="-1.*a plan of another context"):
                _lib.check(L.dg_rvals_batch_device(ctx.h, foreign.h, plan._cols(dcols), d_ro.data_ptr(), n, n_rows, 0, None, 0,
                                                   o.off.data_ptr(), None, None, work.data_ptr(), work.numel(), None))
            with pytest.raises(_lib.DGError, match="-1.*a plan of another context"):
                need = C.c_uint64()
                off = np.zeros(n + 1, dtype=np.uint64)
                _lib.check(L.dg_rvals_batch_host(ctx.h, foreign.h, plan._cols(cols), row_off.ctypes.data, n, n_rows, None, 0,
                                                 off.ctypes.data, None, None, C.byref(need)))
        other.close()
        torch.cuda.synchronize()
        out, _, _, _ = o.read("refused")
        assert (out == RG.GUARD).all()
        launch(plan, dcols, d_ro, 0, n_rows, o, work)  # n = 0: DG_OK, nothing launched, nothing written
        torch.cuda.synchronize()
        assert (o.off.cpu().numpy().view(np.uint64) == FILL64).all()
        work_guards(wt, "refusals")
        arena, off, st, cst = G._row_values_host(plan, cols, row_off[:1], 0, n_rows)
        assert len(arena) == 0 and off.tolist() == [0] and len(st) == 0
    # no rows at all: every per-row array may be NULL, every message is the empty list
    empty = ("no rows", [VR.STRING, VR.I32], [1, 2], [{}, {}], np.zeros(4, dtype=np.uint64), 3, 0)
    want = checker(empty)
    assert want[0] == b"\x0c\0\0\0\0" * 3
    run_device(empty, want)
    run_host(empty, want)


# 6 --------------------------------------------------------- host wrappers
def test_public_host_wrappers_and_read_back():
    """row_values_batch, build_row_lists_batch and set_rows_batch over Python rows; what they write, rows_batch reads
    back with root_type LIST and an empty parent"""
    from dynamicgo_amd import generic as G
    fields = [(1, "i32"), (2, "str"), (7, "f64"), (9, ("list", "i64")), (4, "bool")]
    rows = [[(5, b"ab", 1.5, [1, 2, 3], True), (None, b"", None, [], False)],
            [],
            [(-1, None, -0.0, None, None), (None, None, None, None, None), (2 ** 31 - 1, b"x" * 300, 2.5, list(range(70)), True)]]
    lists = G.build_row_lists_batch(fields, rows)
    kinds = [G.val_kind(k) for _, k in fields]
    for m, rs in zip(lists, rows):
        w = RR.list_header(len(rs))
        for r in rs:
            for (fid, _), kind, v in zip(fields, kinds, r):
                if v is not None:
                    w += VR.field_begin(kind, fid) + VR.encode(kind, v)
            w += b"\0"
        assert m == w
    arena, off, st, cst = G.row_values_batch(rows, fields)
    assert [arena[int(a):int(b)].tobytes() for a, b in zip(off, off[1:])] == lists and not st.any() and not cst.any()
    assert len(cst) == 5 * 5
    back = G.rows_batch(lists, (), [([G.PathFieldId(1)], "int"), ([G.PathFieldId(2)], "str"), ([G.PathFieldId(7)], "float64"),
                                    ([G.PathFieldId(9)], "list[int]"), ([G.PathFieldId(4)], "bool")], root_type=G.LIST)
    flat = [r for rs in rows for r in rs]
    assert back.offsets.tolist() == [0, 2, 2, 5] and not back.status.any()
    for j, c in enumerate(back.columns):
        assert c.valid.tolist() == [r[j] is not None for r in flat], j
    assert [int(v) for v, r in zip(back.columns[0].values, flat) if r[0] is not None] == [5, -1, 2 ** 31 - 1]
    assert [v for v, r in zip(back.columns[1].values, flat) if r[1] is not None] == [b"ab", b"", b"x" * 300]
    assert [struct.pack("<d", v) for v, r in zip(back.columns[2].values, flat) if r[2] is not None] == [
        struct.pack("<d", x) for x in (1.5, -0.0, 2.5)]
    eo = back.columns[3].offsets
    assert [back.columns[3].values[int(eo[g]):int(eo[g + 1])].tolist() for g, r in enumerate(flat) if r[3] is not None] == [
        [1, 2, 3], [], list(range(70))]
    # set_rows_batch: the list becomes field 3 of every message; a set's header names the other wire type
    import editmref as EM
    import tgetref as R
    msgs = [VR.field_begin(VR.I32, 1) + b"\0\0\0\x07\0"] * 3
    for container, wire in (("list", R.LIST), ("set", R.SET)):
        res = G.set_rows_batch(msgs, [G.PathFieldId(3)], fields, rows, container=container)
        assert all(r.status == G.EDIT_OK for r in res)
        for r, m, v in zip(res, msgs, lists):
            w_ret, w_out = EM.edit_many(EM.SET_OP, m, [], [((R.FIELD, 3), v, wire)], cap=len(m) + len(v) + 64)
            assert w_ret & 0xFF == 0 and r.raw == w_out and bytes([wire, 0, 3]) + v in r.raw
    with pytest.raises(ValueError):
        G.row_values_batch([[(1, 2)]], fields)
    assert G.row_values_batch([], fields)[1].tolist() == [0]


def test_batches_whose_lists_are_all_empty():
    """no message has a row (a list filtered to nothing): every wrapper gives 0C 00 00 00 00 per message"""
    import editmref as EM
    import tgetref as R
    from dynamicgo_amd import generic as G
    fields = [(1, "i32"), (2, "str"), (7, "f64"), (9, ("list", "i64")), (4, "bool")]
    empty = b"\x0c\0\0\0\0"
    for n in (1, 2, 5):
        rows = [[] for _ in range(n)]
        for plan in (fields, fields[:1], fields[3:4]):
            arena, off, st, cst = G.row_values_batch(rows, plan)
            assert arena.tobytes() == empty * n and off.tolist() == [5 * i for i in range(n + 1)]
            assert st.tolist() == [0] * n and len(cst) == 0
            assert G.build_row_lists_batch(plan, rows) == [empty] * n
            assert G.build_row_lists_batch(plan, rows, container="set") == [empty] * n
        msgs = [VR.field_begin(VR.I32, 1) + struct.pack(">i", i) + bytes([15, 0, 3]) + RR.list_header(1) + b"\0\0" for i in range(n)]
        res = G.set_rows_batch(msgs, [G.PathFieldId(3)], fields, rows)
        for r, m in zip(res, msgs):
            w_ret, w_out = EM.edit_many(EM.SET_OP, m, [], [((R.FIELD, 3), empty, R.LIST)], cap=len(m) + 64)
            assert r.status == G.EDIT_OK and w_ret & 0xFF == 0 and r.raw == w_out == m[:10] + empty + b"\0"
    # one message with rows among empty ones still takes the columns' route
    lists = G.build_row_lists_batch(fields[:1], [[], [(7,)], []])
    assert lists == [empty, RR.list_header(1) + bytes([8, 0, 1, 0, 0, 0, 7, 0]), empty]


def sext(v, bits):
    v = int(v) & ((1 << bits) - 1)
    return v - (1 << bits) if v >> (bits - 1) else v


def test_device_output_read_back_by_rows_batch():
    """what row_values_device writes for rvalsgen's cases with absent cells, read by rows_batch with root_type LIST and
    an empty parent: the rows' offsets, present for valid, and the input columns back for every OK cell"""
    from dynamicgo_amd import generic as G
    reads = {VR.BOOL: "bool", VR.DOUBLE: "float64", VR.STRING: "str", VR.LIST | VR.DOUBLE: "list[float64]"}
    cases = [c for c in RG.present_cases() if c[0] in ("presence", "last column absent")]
    assert len(cases) == 2
    cells = 0
    for case in cases:
        name, kinds, fids, cols, row_off, n, n_rows = case
        want = checker(case)
        assert not any(want[2]) and not any(want[3])
        out, off, _, _ = run_device(case, want)
        lists = [out[int(a):int(b)].tobytes() for a, b in zip(off, off[1:])]
        back = G.rows_batch(lists, (), [([G.PathFieldId(f)], reads.get(k, "list[int]" if k & VR.LIST else "int"))
                                        for f, k in zip(fids, kinds)], root_type=G.LIST)
        assert back.offsets.tolist() == row_off.tolist() and not back.status.any(), name
        absent = 0
        for j, (kind, col, c) in enumerate(zip(kinds, cols, back.columns)):
            pres = col.get("present", np.ones(n_rows, dtype=np.uint8))
            assert c.valid.tolist() == [bool(p) for p in pres], (name, j)
            absent += int((pres == 0).sum())
            for g in np.nonzero(pres)[0]:
                cells += 1
                if kind == VR.STRING:
                    a, ln = int(col["val"][g]), int(col["len"][g])
                    assert c.values[g] == col["src"][a:a + ln].tobytes(), (name, j, g)
                elif kind & VR.LIST:
                    a, b = int(col["elem_off"][g]), int(col["elem_off"][g + 1])
                    got = c.values[int(c.offsets[g]):int(c.offsets[g + 1])]
                    if kind & 0x3F == VR.DOUBLE:
                        assert got.view(np.uint64).tolist() == col["elems"][a:b].tolist(), (name, j, g)
                    else:
                        assert got.tolist() == [sext(e, 8 * VR.WIDTH[kind & 0x3F]) for e in col["elems"][a:b]], (name, j, g)
                else:
                    assert int(c.values[g]) == sext(col["val"][g], 8 * VR.WIDTH[kind]), (name, j, g)
        assert absent >= n_rows  # absent cells in every case
    assert cells >= 60


# 7 -------------------------------------------- round trip with the read side
ROUND_KINDS = [VR.I32, VR.STRING, VR.BOOL, VR.DOUBLE, VR.LIST | VR.I64, VR.I08, VR.I16, VR.I64]
ROUND_READS = ["int", "str", "bool", "float64", "list[int]", "int", "int", "int"]
ROUND_IDS = [1, 2, 3, 255, 256, 9, 32767, -1]


def round_trip_batch(n_rows=300, n=70, seed=43):
    """(messages whose field 5 is a list<struct> of exactly the plan's fields in column order, the case that writes
    the lists, its checker's answer)"""
    rng = random.Random(seed)
    cols = [VG.column_for(rng, k, n_rows, 150 if k == VR.STRING else None) for k in ROUND_KINDS]
    for j in (0, 1, 3, 4, 7):
        cols[j]["present"] = RG.present_col(rng, n_rows)
    case = RG.case("round trip", ROUND_KINDS, cols, RG.partition(rng, n_rows, n), n_rows, ROUND_IDS)
    want = checker(case)
    assert not any(want[2]) and not any(want[3])
    msgs = [VR.field_begin(VR.I64, 1) + struct.pack(">q", i) + bytes([15, 0, 5]) + want[0][want[1][i]:want[1][i + 1]] + b"\0"
            for i in range(n)]
    return msgs, case, want


class Read:
    """rows_device + row_list_device over `msgs` on `stream`: the tensors as they are written, and the columns
    row_values_device takes from them (present = the cell's status is OK)"""

    def __init__(self, msgs, n_rows, stream):
        import torch
        from dynamicgo_amd import generic as G
        n, P = len(msgs), len(ROUND_KINDS)
        self.arena_np = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(m) for m in msgs], out=in_off[1:])
        self.in_off = in_off
        self.arena, self.d_in = torch.from_numpy(self.arena_np).cuda(), torch.from_numpy(in_off).cuda()
        self.plan = G.RowPlan([G.PathFieldId(5)], [([G.PathFieldId(f)], k) for f, k in zip(ROUND_IDS, ROUND_READS)])
        self.head = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        self.row_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        self.val = torch.zeros((P, n_rows), dtype=torch.int64, device="cuda")
        self.cell = torch.zeros((P, n_rows, 2), dtype=torch.int32, device="cuda")
        self.lens = torch.zeros((P, n_rows), dtype=torch.int32, device="cuda")
        self.elem_cap = len(self.arena_np) // 8 + 8
        self.elem_off = torch.zeros(n_rows + 1, dtype=torch.int64, device="cuda")
        self.elems = torch.zeros(self.elem_cap, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            G.rows_device(self.plan, self.arena, self.d_in, n, self.head, self.row_off, None, self.val, self.cell, self.lens,
                          row_cap=n_rows, stream=stream, max_len=max(map(len, msgs)))
            G.row_list_device(self.plan, 4, self.arena, n_rows, self.val[4], self.cell[4], self.lens[4], self.elem_off,
                              self.elems, self.elem_cap, stream=stream)
            self.present = ((self.cell[:, :, 0] & 0xFF) == 0).to(torch.uint8)

    def cols(self, val=None):
        val = self.val if val is None else val
        out = []
        for j, kind in enumerate(ROUND_KINDS):
            c = {"present": self.present[j]}
            if kind & (VR.LIST | VR.SET):
                c.update(elem_off=self.elem_off, elems=self.elems)
            else:
                c.update(val=val[j])
            if kind == VR.STRING:
                c.update(len=self.lens[j], src=self.arena)
            out.append(c)
        return out


def test_round_trip_with_the_read_side():
    """rows_device + row_list_device, then row_values_device on the tensors as they are, the thrift arena as the
    strings' source: every message's item is the list's bytes in the message"""
    import torch
    from dynamicgo_amd import generic as G
    msgs, case, want = round_trip_batch()
    n, n_rows = case[5], case[6]
    stream = torch.cuda.Stream()
    r = Read(msgs, n_rows, stream)
    with G.RowValuePlan(ROUND_KINDS, ROUND_IDS) as plan:
        o = Outs(n, n_rows * len(ROUND_KINDS), want[1][-1])
        wt, work = work_for(plan, n, n_rows)
        with torch.cuda.stream(stream):
            launch(plan, r.cols(), r.row_off, n, n_rows, o, work, stream=stream)
        torch.cuda.synchronize()
        got = o.read("round trip")
        work_guards(wt, "round trip")
    assert r.row_off.cpu().numpy().tolist() == case[4].tolist()
    verify(got, want, 0, want[1][-1], "round trip")
    out, off = got[0], got[1]
    for i, m in enumerate(msgs):
        assert out[int(off[i]):int(off[i + 1])].tobytes() == m[14:-1], i


# 8 -------------------------------------------------- the chain on the device
def test_rows_torch_rvals_editm_on_one_stream():
    """rows_device + row_list_device, a torch + 1 on the I32 column, row_values_device and edit_many_device, all on
    one stream with no synchronisation between them, against the checker's many-edit over the checker's lists"""
    import torch
    import editmref as EM
    import tgetref as R
    from dynamicgo_amd import generic as G
    msgs, case, _ = round_trip_batch(seed=44)
    _, kinds, fids, cols, row_off, n, n_rows = case
    cols = [dict(c) for c in cols]
    cols[0]["val"] = cols[0]["val"] + np.uint64(1)
    want = checker(("chain", kinds, fids, cols, row_off, n, n_rows))
    caps = np.array([(len(m) + 64 + 79) & ~15 for m in msgs])
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    stream = torch.cuda.Stream()
    r = Read(msgs, n_rows, stream)
    with G.RowValuePlan(kinds, fids) as wp, G.EditManyPlan([], [G.PathFieldId(5)], G.EDIT_SET) as mp:
        cap_v = want[1][-1]
        ev = torch.full((cap_v + 16,), RG.GUARD, dtype=torch.uint8, device="cuda")
        ev_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        work = torch.zeros(wp.work_bytes(n, n_rows), dtype=torch.uint8, device="cuda")
        d_oo = torch.from_numpy(out_off).cuda()
        out = torch.full((int(out_off[n]) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        ol = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ret = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            plus = r.val.clone()
            plus[0] += 1
            G.row_values_device(wp, r.cols(plus), r.row_off, n, n_rows, ev, ev_off, work, cap=cap_v, stream=stream)
            G.edit_many_device(mp, r.arena, r.d_in, n, [wp.wire_type], ev, ev_off, [0], out, d_oo, ol, ret, stream=stream)
        torch.cuda.synchronize()
        assert ev_off.cpu().numpy().tolist() == want[1]
        h_ev = ev.cpu().numpy()
        assert h_ev[:cap_v].tobytes() == want[0] and (h_ev[cap_v:] == RG.GUARD).all()
        h_out, h_ol, h_ret = out.cpu().numpy(), ol.cpu().numpy(), ret.cpu().numpy().view(np.uint64)
        changed = 0
        for i, m in enumerate(msgs):
            items = [((R.FIELD, 5), want[0][want[1][i]:want[1][i + 1]], R.LIST)]
            w_ret, w_out = EM.edit_many(EM.SET_OP, m, [], items, cap=int(caps[i]))
            assert int(h_ret[i]) == w_ret, (i, hex(int(h_ret[i])), hex(w_ret))
            g_out = h_out[int(out_off[i]):int(out_off[i]) + (int(h_ol[i]) if w_ret & 0xFF == 0 else 0)].tobytes()
            assert g_out == w_out, i
            changed += g_out != m
        assert changed >= 30


# 9 ---------------------------------------------------------------- streams
def test_two_streams_at_once():
    import torch
    from dynamicgo_amd import generic as G
    cases = [RG.geometry_case(7, 257), RG.geometry_case(16, 257)]
    wants = [checker(c) for c in cases]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with G.RowValuePlan(cases[0][1], cases[0][2]) as pa, G.RowValuePlan(cases[1][1], cases[1][2]) as pb:
        da, db = [to_dev(c) for c in cases[0][3]], [to_dev(c) for c in cases[1][3]]
        ra, rb = dev_offsets(cases[0][4]), dev_offsets(cases[1][4])
        na, nb = cases[0][5], cases[1][5]
        rounds = [(Outs(na, 257 * 7, wants[0][1][-1]), Outs(nb, 257 * 16, wants[1][1][-1]), work_for(pa, na, 257),
                   work_for(pb, nb, 257)) for _ in range(3)]
        torch.cuda.synchronize()
        for oa, ob, wa, wb in rounds:  # no synchronisation between the launches; a d_work per call in flight
            launch(pa, da, ra, na, 257, oa, wa[1], stream=sa)
            launch(pb, db, rb, nb, 257, ob, wb[1], stream=sb)
        torch.cuda.synchronize()
        for k, (oa, ob, wa, wb) in enumerate(rounds):
            verify(oa.read("stream a"), wants[0], 0, wants[0][1][-1], "round %d, stream a" % k)
            verify(ob.read("stream b"), wants[1], 0, wants[1][1][-1], "round %d, stream b" % k)
            work_guards(wa[0], "stream a"), work_guards(wb[0], "stream b")


# 10 ----------------------------------------------------------- far offsets
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
    """a STRING column's payloads in a source arena at offsets below, across and beyond B, one row a message, written
    to an output arena at an out_base that puts the pivot's item across B; the aliases of the source hold decoys, and
    everything outside the items in the output arena is still FILL"""
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
    kinds, fids = [VR.STRING, VR.I16], [7, 8]
    near = [VG.string_col(pay), VG.scalar_col(list(range(n)))]
    row_off = np.arange(n + 1, dtype=np.uint64)
    arena, rel, wst, wcst = RR.encode_batch(kinds, fids, near, row_off, n, n)
    assert not any(wst) and not any(wcst)
    base = B - rel[pivot] - 40  # the pivot's item begins 40 bytes below B: its payload crosses it
    woff = [base + x for x in rel]
    o_off = np.array(woff, dtype=np.int64)
    FO.check_layout(o_off, B)
    assert woff[pivot] < B < woff[pivot + 1]
    outa.prefill(o_off, B)
    with G.RowValuePlan(kinds, fids) as plan:
        off = torch.full((n + 1 + 2 * GUARD,), FILL64, dtype=torch.int64, device="cuda")
        st = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        d = [to_dev(c) for c in near]
        d[0]["val"] = torch.from_numpy(src_off[:-1].copy()).cuda()
        d[0]["src"] = inp.base
        wt, work = work_for(plan, n, n)
        G.row_values_device(plan, d, dev_offsets(row_off), n, n, outa.base, off[GUARD:], work, st[GUARD:], None, out_base=base,
                            cap=woff[-1])
        torch.cuda.synchronize()
        work_guards(wt, "far")
    h_off, h_st = off.cpu().numpy(), st.cpu().numpy()
    assert h_off[GUARD:GUARD + n + 1].tolist() == woff and (h_off[:GUARD].view(np.uint64) == FILL64).all()
    assert (h_off[GUARD + n + 1:].view(np.uint64) == FILL64).all()
    assert (h_st[GUARD:GUARD + n] == 0).all() and (h_st[:GUARD] == 0x5A).all() and (h_st[GUARD + n:] == 0x5A).all()
    got = outa.collect(o_off, B, what="d_out at %#x" % B)
    assert got.tobytes() == arena
