"""GPU: typed column reads (dynamicgo_amd.generic over dg_cols_*) against the
checker of colsref.py: tgetref's GetByPath followed by the casts of cast.go.
Every case goes through the host entry and the device entry, and every field of
every cell, every value (doubles as u64) and every element is compared with
the checker's. The inputs are colsgen's, which test_cols_host.py runs through
the host build of the same decode."""
import random

import numpy as np
import pytest

import colsgen as CG
import colsref as CR
import faroff as FO
import t2jgen
import tgetgen as TG
import tgetref as R
from test_gpu_tget import expect as tget_expect, same as tget_same, to_paths

pytestmark = pytest.mark.gpu

GUARD = 64  # entries of fill on each side of every output
FILL = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A


def to_cols(columns):
    return [(to_paths([p])[0], k) for p, k in columns]


def upload(msgs, first=0):
    """(arena tensor with exactly 16 spare bytes, d_in_off, in_off): the messages back to back from offset `first`"""
    import torch
    in_off = np.full(len(msgs) + 1, first, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    in_off[1:] += first
    arena = torch.from_numpy(np.frombuffer(b"\xEE" * first + b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    return arena, torch.from_numpy(in_off).cuda(), in_off


class Outputs:
    """d_val / d_cell / d_len of one launch between GUARD entries of fill"""

    def __init__(self, n, P):
        import torch
        self.n, self.P, q = n, P, n * P
        self.val = torch.full((q + 2 * GUARD,), FILL, dtype=torch.int64, device="cuda")
        self.cell = torch.full((q + 2 * GUARD,), FILL, dtype=torch.int64, device="cuda")
        self.len = torch.full((q + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda")

    def args(self):
        return self.val[GUARD:], self.cell[GUARD:], self.len[GUARD:]

    def column(self, k):
        a = GUARD + k * self.n
        return self.val[a:a + self.n], self.cell[a:a + self.n], self.len[a:a + self.n]

    def read(self, what):
        """[column k as a dict of arrays]; the guards must be intact"""
        from dynamicgo_amd import generic as G
        q = self.n * self.P
        out = []
        hv, hc, hl = self.val.cpu().numpy().view(np.uint64), self.cell.cpu().numpy(), self.len.cpu().numpy().view(np.uint32)
        for name, h, fill in (("d_val", hv, FILL), ("d_cell", hc.view(np.uint64), FILL), ("d_len", hl, FILL32)):
            assert (h[:GUARD] == fill).all() and (h[GUARD + q:] == fill).all(), "%s: a store outside %s" % (what, name)
        cells = hc[GUARD:GUARD + q].view(G.COL_CELL_DTYPE)
        for k in range(self.P):
            s = slice(k * self.n, (k + 1) * self.n)
            out.append({"status": cells["status"][s], "type": cells["type"][s], "step": cells["step"][s],
                        "aux": cells["aux"][s], "val": hv[GUARD:][s], "len": hl[GUARD:][s]})
        return out


def emit_lists(plan, arena, o, got, what, stream=None):
    """the sizing call and the emit of every list column of `o`, into got[k]["off"] / ["elems"]"""
    import torch
    from dynamicgo_amd import generic as G
    n = o.n
    for k in plan.lists:
        v, c, ln = o.column(k)
        off = torch.full((n + 1 + GUARD,), FILL, dtype=torch.int64, device="cuda")
        G.column_list_device(plan, k, arena, n, v, c, ln, off, None, 0, stream=stream)  # sizing
        torch.cuda.synchronize()
        h_off = off.cpu().numpy().view(np.uint64)
        total = int(h_off[n])
        assert (h_off[n + 1:] == FILL).all(), "%s: a store behind d_elem_off" % what
        elems = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.int64, device="cuda")
        G.column_list_device(plan, k, arena, n, v, c, ln, off, elems[GUARD:], total, stream=stream)
        torch.cuda.synchronize()
        h = elems.cpu().numpy().view(np.uint64)
        assert (h[:GUARD] == FILL).all() and (h[GUARD + total:] == FILL).all(), "%s: a store outside d_elems" % what
        assert (off.cpu().numpy().view(np.uint64)[:n + 1] == h_off[:n + 1]).all()
        got[k]["off"], got[k]["elems"] = h_off[:n + 1], h[GUARD:GUARD + total]


def run_device(msgs, columns, root_type=R.STRUCT, lists=True):
    import torch
    from dynamicgo_amd import generic as G
    n = len(msgs)
    with G.ColumnPlan(to_cols(columns)) as plan:
        arena, d_off, _ = upload(msgs)
        o = Outputs(n, plan.count)
        G.columns_device(plan, arena, d_off, n, *o.args(), root_type=root_type, max_len=max(map(len, msgs), default=0))
        torch.cuda.synchronize()
        got = o.read("device entry")
        if lists and n:
            emit_lists(plan, arena, o, got, "device entry")
        return got


def run_host(msgs, columns, root_type=R.STRUCT):
    from dynamicgo_amd import generic as G
    with G.ColumnPlan(to_cols(columns)) as plan:
        val, cell, lens, elem_off, elems, _ = G.columns_records(msgs, plan, root_type)
        got = [{"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"], "aux": cell[k]["aux"],
                "val": val[k], "len": lens[k]} for k in range(plan.count)]
        for j, k in enumerate(plan.lists):
            eo = elem_off[j]
            got[k]["off"], got[k]["elems"] = eo - eo[0], elems[int(eo[0]):int(eo[-1])]
        if plan.lists:
            assert int(elem_off[0][0]) == 0 and int(elem_off[-1][-1]) == len(elems)
        return got


def compare(got, want, what):
    for k, col in enumerate(want):
        CG.same(got[k], CG.arrays(col) if isinstance(col, list) else col, "%s, column %d" % (what, k))


def check(msgs, columns, root_type=R.STRUCT, want=None):
    want = want or CG.expect(msgs, columns, root_type)
    compare(run_host(msgs, columns, root_type), want, "host entry")
    compare(run_device(msgs, columns, root_type), want, "device entry")
    return want


# ------------------------------------------------------------------- cases
def test_kind_by_wire_type_matrix():
    msgs = CG.matrix_messages()
    want = check(msgs, CG.MATRIX_COLUMNS)
    for st in (R.OK, R.NOT_FOUND, R.E_READ, CR.E_UNSUPPORTED):
        assert CG.share(want, st) > 0.01, st
    ints = {c.val for c in want[2] if c.status == R.OK}
    assert {0x80, 0xFF, 2 ** 64 - 2 ** 15, 2 ** 64 - 2 ** 31, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1} <= ints
    assert [c.val for c in want[0] if c.status == R.OK] == [0, 1, 0, 0]
    assert {c.val for c in want[3] if c.status == R.OK} == set(CG.DOUBLES)
    lens = [c.val for c in want[5] if c.status == R.OK]
    assert 0 in lens and 1 in lens and 2 ** 31 - 1 not in lens
    # the public columns: names of the errors, numpy values, bytes
    from dynamicgo_amd import generic as G
    cols = G.columns_batch(msgs, [(to_paths([[(R.FIELD, 1)]])[0], k) for k in ("int", "float64", "str", "list[int]", "bool")])
    names = {R.OK: None, R.NOT_FOUND: "ErrNotFound", R.E_READ: "ErrRead", R.E_TYPE: "ErrDismatchType",
             CR.E_UNSUPPORTED: "ErrUnsupportedType"}
    for c, w in zip(cols, (want[2], want[3], want[4], want[6], want[0])):
        assert [c.error(i) for i in range(len(msgs))] == [names[x.status] for x in w]
        assert c.valid.tolist() == [x.status == R.OK for x in w]
    assert cols[0].values.dtype == np.int64 and cols[0].values.view(np.uint64).tolist() == [c.val for c in want[2]]
    assert cols[1].values.dtype == np.float64 and cols[1].values.view(np.uint64).tolist() == [c.val for c in want[3]]
    assert cols[2].values == [m[c.val - b:c.val - b + c.len] if c.status == R.OK else b""
                              for m, c, b in zip(msgs, want[4], np.cumsum([0] + [len(m) for m in msgs]).tolist())]
    assert b"abc" in cols[2].values and bytes(range(40)) in cols[2].values
    assert cols[3].values.view(np.uint64).tolist() == [e for c in want[6] if c.elems for e in c.elems]
    assert cols[3].offsets.tolist() == CG.arrays(want[6])["off"].tolist()
    assert cols[4].values.dtype == np.bool_ and cols[4].values.tolist() == [bool(c.val) for c in want[0]]


@pytest.mark.parametrize("target", list(CG.TARGETS))
def test_alignment_and_the_arenas_end(target):
    """the target's value at every residue mod 16, the last one the last bytes before the 16 spare bytes"""
    msgs = CG.align_batch(target)
    want = check(msgs, CG.ALIGN_COLUMNS)
    assert sum(c.status == R.OK for col in want for c in col) >= 16
    starts = {R.get_by_path(m, [(R.FIELD, 2)]).start % 16 for m in msgs}
    assert len(starts) == 16


def test_geometry_and_guards():
    import torch
    from dynamicgo_amd import generic as G
    all_msgs = CG.geometry_messages(257)
    want_all = CG.expect(all_msgs, CG.GEOMETRY_COLUMNS)
    assert CG.share(want_all, R.OK) > 0.6
    for P in range(1, 9):
        cols = CG.GEOMETRY_COLUMNS[:P]
        with G.ColumnPlan(to_cols(cols)) as plan:
            o = Outputs(0, P)  # n = 0: nothing is launched, nothing stored
            G.columns_device(plan, None, None, 0, *o.args())
            torch.cuda.synchronize()
            o.read("n = 0")
            for n in (1, 63, 64, 65, 255, 256, 257):
                msgs = all_msgs[:n]
                want = [CG.arrays(col[:n]) for col in want_all[:P]]
                what = "P = %d, n = %d" % (P, n)
                arena, d_off, _ = upload(msgs)
                o = Outputs(n, P)
                G.columns_device(plan, arena, d_off, n, *o.args())
                torch.cuda.synchronize()
                got = o.read(what)
                emit_lists(plan, arena, o, got, what)
                compare(got, want, what)
                # message j changed (its first field header becomes the STOP byte): its cells change, no other
                j = n // 2
                changed = msgs[:j] + [b"\x00" + msgs[j][1:]] + msgs[j + 1:]
                arena2, _, _ = upload(changed)
                o2 = Outputs(n, P)
                G.columns_device(plan, arena2, d_off, n, *o2.args())
                torch.cuda.synchronize()
                got2 = o2.read(what + ", changed")
                for k in range(P):
                    assert got2[k]["status"][j] == R.NOT_FOUND, what
                    for f in CG.CELL_FIELDS:
                        keep = np.arange(n) != j
                        assert (got2[k][f][keep] == got[k][f][keep]).all(), (what, k, f)
    assert G.columns_batch([], to_cols(CG.GEOMETRY_COLUMNS))[2].values.shape == (0,)
    compare(run_host(all_msgs, CG.GEOMETRY_COLUMNS), want_all, "host entry")


# what the checker alone gives, counted on the CPU: the share of OK cells of each column of set A over the well-formed
# messages (the rest is NotFound), and of every status over each set
FUZZ_A_OK = [0.6005859375, 0.60595703125, 0.60400390625, 0.60107421875, 0.60595703125, 0.59423828125, 0.59423828125,
             0.62158203125]
# OK, NotFound, E_READ, E_TYPE, Unsupported over set A, set B, mutated set A, mutated set B
FUZZ_WANT = ([0.603455, 0.396545, 0.0, 0.0, 0.0], [0.158447, 0.617676, 0.0, 0.0, 0.223877],
             [0.402039, 0.148254, 0.449463, 0.0, 0.000244], [0.108398, 0.242981, 0.491577, 0.0, 0.157043])


@pytest.fixture(scope="module")
def corpus():
    rng, mrng = random.Random(1234), random.Random(4321)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(2048)]
    return msgs, [t2jgen.mutate(mrng, m) for m in msgs]


def shares(want):
    return [round(CG.share(want, st), 6) for st in (R.OK, R.NOT_FOUND, R.E_READ, R.E_TYPE, CR.E_UNSUPPORTED)]


def test_fuzz(corpus):
    msgs, bad = corpus
    a, b = check(msgs, CG.FUZZ_A), check(msgs, CG.FUZZ_B)
    ma, mb = check(bad, CG.FUZZ_A), check(bad, CG.FUZZ_B)
    print("set A OK per column:", [CG.share(col, R.OK) for col in a])
    print("shares A, B, mutated A, mutated B:", shares(a), shares(b), shares(ma), shares(mb))
    assert [CG.share(col, R.OK) for col in a] == FUZZ_A_OK
    assert all(0.59 <= s <= 0.63 for s in FUZZ_A_OK)  # the fields are set with p = 0.6
    assert all(CG.share(col, R.OK) + CG.share(col, R.NOT_FOUND) == 1.0 for col in a)
    assert (shares(a), shares(b), shares(ma), shares(mb)) == FUZZ_WANT
    assert CG.share(a, R.OK) >= 0.5
    for st in (R.OK, R.NOT_FOUND, CR.E_UNSUPPORTED):
        assert CG.share(b, st) >= 0.01, st
    assert CG.share(ma + mb, R.E_READ) >= 0.25
    assert all(sum(c.status != R.NOT_FOUND for c in col) == 662 for col in b[:5])  # f1000 is present in 662 messages
    f19 = b[7]  # list<string>: unsupported when not empty, OK and empty when empty
    assert any(c.status == CR.E_UNSUPPORTED and c.aux == R.STRING for c in f19)
    assert any(c.status == R.OK and c.len == 0 and c.type == R.STRING for c in f19)
    assert any(c.status == R.OK and c.len > 2 for c in a[7])


def test_deep_pass():
    chains = CG.deep_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want = check(msgs, CG.DEEP_COLUMNS)
    for path in ([(R.FIELD, 2)], [(R.FIELD, 1)]):
        frames = [TG.chain_frames(k, lf, path) for k, lf in chains]
        assert any(f > TG.LDS_FRAMES for f in frames) and any(f <= TG.LDS_FRAMES for f in frames)
    assert all(c.status == R.OK and c.val == 9 for c in want[0])
    hits = [c for col, d in zip(want[2:], CG.DEEP_LIST_DEPTHS) for c, ch in zip(col, chains) if ch == ("L" * d, "l")]
    assert len(hits) == 6 and all(c.status == R.OK and c.elems == [1, 2 ** 64 - 1] for c in hits)


def test_lists():
    import torch
    from dynamicgo_amd import generic as G
    msgs = CG.list_messages()
    want = check(msgs, CG.LIST_COLUMNS)
    for col in want[:2]:
        assert sorted({c.len for c in col if c.status == R.OK}) == sorted(CG.LIST_COUNTS)
        for st in (R.NOT_FOUND, R.E_READ, CR.E_UNSUPPORTED):
            assert any(c.status == st for c in col), st
    assert {c.type for c in want[0] if c.status == R.OK and c.len} == {R.BYTE, R.I16, R.I32, R.I64}
    # elem_cap below the need: nothing at or behind d_elems[elem_cap]; what is in front of it is right
    n = len(msgs)
    w = CG.arrays(want[0])
    total = int(w["off"][n])
    assert total > 4097 * 4
    with G.ColumnPlan(to_cols(CG.LIST_COLUMNS)) as plan:
        arena, d_off, _ = upload(msgs)
        o = Outputs(n, plan.count)
        G.columns_device(plan, arena, d_off, n, *o.args())
        v, c, ln = o.column(0)
        for cap in (0, 1, 255, 256, 257, total - 1):
            off = torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda")
            elems = torch.full((total + GUARD,), FILL, dtype=torch.int64, device="cuda")
            G.column_list_device(plan, 0, arena, n, v, c, ln, off, elems, cap)
            torch.cuda.synchronize()
            h = elems.cpu().numpy().view(np.uint64)
            assert (h[cap:] == FILL).all(), "cap %d: a store at or behind d_elems[elem_cap]" % cap
            assert (h[:cap] == w["elems"][:cap]).all(), cap
            assert off.cpu().numpy().view(np.uint64).tolist() == w["off"].tolist()  # [n] is still the need
        with pytest.raises(Exception, match="no list column"):
            G.column_list_device(plan, 2, arena, n, v, c, ln, off, None, 0)
        torch.cuda.synchronize()


def test_emit_search_variants(knob):
    """both ways a lane of the emit finds its message give the checker's elements"""
    msgs = CG.list_messages()
    want = CG.expect(msgs, CG.LIST_COLUMNS[:2])
    for full in (1, 0):
        knob("cols_full_search", full)
        compare(run_device(msgs, CG.LIST_COLUMNS[:2]), want, "cols_full_search %d" % full)


def test_plan_create_rejects():
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()
    blob = G.compile_paths(to_paths([[(R.FIELD, 1)], [(R.FIELD, 2)]]))

    def create(blob, kinds):
        h = C.c_void_p()
        rc = L.dg_cols_create(ctx.h, bytes(blob), len(blob), bytes(kinds), len(kinds), C.byref(h))
        if rc == 0:
            assert L.dg_cols_count(h) == len(kinds)
            L.dg_cols_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create(blob, [CR.INT, CR.LIST_F64])[0] == 0
    for kinds, text in (([CR.INT], "1 kinds for 2 paths"), ([CR.INT, 0], "unknown kind 0"), ([7, CR.INT], "unknown kind 7"),
                        ([CR.INT, CR.LIST | CR.STR], "unknown kind 21"), ([CR.INT, CR.LIST], "unknown kind 16")):
        rc, err = create(blob, kinds)
        assert rc == -6 and text in err, (kinds, rc, err)  # DG_E_ARG
    rc, err = create(blob[:16], [CR.INT, CR.INT])
    assert rc == -6 and "no header" in err
    with pytest.raises(ValueError):
        G.ColumnPlan([([G.PathFieldId(1)], "list[str]")])


def test_columns_and_get_by_path_on_two_streams():
    """columns_device on one stream and get_by_path_device on another, in turn for 4 rounds with no synchronisation,
    over chains that send both to their deep passes: each component has a deep queue, counters and frames of its own"""
    import torch
    from dynamicgo_amd import generic as G
    chains = CG.deep_chains(per_depth=40)
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    n = len(msgs)
    want = CG.expect(msgs, CG.DEEP_COLUMNS)
    get_want = tget_expect(msgs, TG.CHAIN_PATHS)
    assert sum(TG.chain_frames(k, lf, [(R.FIELD, 2)]) > TG.LDS_FRAMES for k, lf in chains) > n // 3
    s_cols, s_get = torch.cuda.Stream(), torch.cuda.Stream()
    arena, d_off, _ = upload(msgs)
    with G.ColumnPlan(to_cols(CG.DEEP_COLUMNS)) as plan, G.PathSet(to_paths(TG.CHAIN_PATHS)) as ps:
        outs = [Outputs(n, plan.count) for _ in range(4)]
        recs = [torch.full((n, ps.count, 4), FILL32, dtype=torch.int32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for r in range(4):
            G.columns_device(plan, arena, d_off, n, *outs[r].args(), stream=s_cols)
            G.get_by_path_device(ps, arena, d_off, n, recs[r], stream=s_get)
        torch.cuda.synchronize()
        for r in range(4):
            compare(outs[r].read("round %d" % r), [{f: a for f, a in CG.arrays(col).items() if f in CG.CELL_FIELDS}
                                                   for col in want], "round %d, columns" % r)
            tget_same(recs[r].cpu().numpy().view(G.REC_DTYPE).reshape(n, ps.count), get_want, "round %d, GetByPath" % r)


# -------------------------------------------------------------- far offsets
FAR_COLUMNS = [([(R.FIELD, 2)], CR.STR), ([(R.FIELD, 3)], CR.LIST_INT), ([(R.FIELD, 1)], CR.INT), ([(R.FIELD, 3)], CR.LEN)]
FAR_PIVOT = CG.fld(R.I32, 1, b"\x80\0\0\x03") + CG.fld(R.STRING, 2, CG.wstr(b"0123456789abcdef")) + \
    CG.fld(R.LIST, 3, CG.lst(R.I64, 3, CG.list_body(R.I64, 3, salt=9))) + b"\x00"
# where B falls in the pivot: in its first field header (the message straddles), in the string's payload (which
# starts at byte 14), in the list's first element (which starts at byte 38)
FAR_DELTAS = {"message": -1, "string payload": -(14 + 5), "first element": -(38 + 3)}


@pytest.fixture(scope="module")
def far_arenas():
    import torch
    inp, out = FO.Arena(), FO.Arena()
    yield inp, out
    inp.free()
    out.free()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("where", list(FAR_DELTAS))
@pytest.mark.parametrize("B", FO.BOUNDS, ids=["2G", "4G"])
def test_far_offsets(far_arenas, B, where):
    import torch
    from dynamicgo_amd import generic as G
    inp, outa = far_arenas
    rng = random.Random(51)
    small = [CG.geometry_message(rng) for _ in range(40)]
    msgs = small[:20] + [FAR_PIVOT] + small[20:]
    n, pivot = len(msgs), 20
    in_off = FO.place([len(m) for m in msgs], B, pivot, FAR_DELTAS[where])
    FO.check_layout(in_off, B, guard=0, tail=FO.TAIL)
    a = int(in_off[pivot])
    assert {"message": a < B < a + 3, "string payload": a + 14 < B < a + 30, "first element": a + 38 < B < a + 46}[where]
    inp.put_input(in_off, msgs, B)
    want = CG.expect(msgs, FAR_COLUMNS, first=int(in_off[0]))
    assert want[0][pivot].val == a + 14 and want[1][pivot].val == a + 38 and want[1][pivot].len == 3
    assert any(c.val >= B for c in want[0] if c.status == R.OK) and any(c.val < B for c in want[0] if c.status == R.OK)
    w1 = CG.arrays(want[1])
    total = int(w1["off"][n])
    # d_elems in the far output arena, its elements on both sides of B
    e_lo = B - 8  # element 1 starts exactly at B
    e_off = np.array([e_lo, e_lo + total * 8], dtype=np.int64)
    FO.check_layout(np.array([e_lo, B, e_lo + total * 8], dtype=np.int64), B)
    outa.prefill(e_off, B)
    with G.ColumnPlan(to_cols(FAR_COLUMNS)) as plan:
        d_off = torch.from_numpy(in_off).cuda()
        o = Outputs(n, plan.count)
        G.columns_device(plan, inp.base, d_off, n, *o.args())
        torch.cuda.synchronize()
        got = o.read("far input")
        v, c, ln = o.column(1)
        off = torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda")
        G.column_list_device(plan, 1, inp.base, n, v, c, ln, off, outa.base[e_lo:], total)
        torch.cuda.synchronize()
        got[1]["off"] = off.cpu().numpy().view(np.uint64)
        got[1]["elems"] = outa.collect(e_off, B, what="d_elems").view(np.uint64)
    compare(got, want, "input at %#x, %s" % (B, where))


# ------------------------------------------------- the entries' own contracts
def test_scalar_columns_without_d_len():
    """d_len may be NULL when no column is STR or a list; with one it is refused"""
    import torch
    from dynamicgo_amd import generic as G
    msgs = CG.geometry_messages(130)
    cols = [CG.GEOMETRY_COLUMNS[k] for k in (0, 3, 4, 5, 6)]
    want = CG.expect(msgs, cols)
    arena, d_off, _ = upload(msgs)
    with G.ColumnPlan(to_cols(cols)) as plan:
        o = Outputs(len(msgs), plan.count)
        v, c, _ = o.args()
        G.columns_device(plan, arena, d_off, len(msgs), v, c, None)
        torch.cuda.synchronize()
        got = o.read("no d_len")
    for k, col in enumerate(want):
        w = CG.arrays(col)
        CG.same({f: got[k][f] for f in CG.CELL_FIELDS if f != "len"}, {f: w[f] for f in CG.CELL_FIELDS if f != "len"},
                "no d_len, column %d" % k)
        assert (got[k]["len"] == FILL32).all()
    with G.ColumnPlan(to_cols(CG.GEOMETRY_COLUMNS[:2])) as plan:
        o = Outputs(len(msgs), plan.count)
        v, c, _ = o.args()
        with pytest.raises(Exception, match="needs d_len"):
            G.columns_device(plan, arena, d_off, len(msgs), v, c, None)


def test_host_entry_sizing_and_an_arena_not_at_zero():
    """dg_cols_batch_host as C callers see it: in_off[0] = 37 (STR and list values are offsets from `thrift`), two
    list columns whose elements follow one another, elems NULL and cap 0 for the need, DG_E_NOMEM below it"""
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    msgs = CG.list_messages()
    cols = [CG.LIST_COLUMNS[1], (CG.ONE, CR.STR), CG.LIST_COLUMNS[0]]
    first, n = 37, len(msgs)
    want = CG.expect(msgs + [CG.fld(R.STRING, 1, CG.wstr(b"payload")) + b"\x00"], cols, first=first)
    msgs = msgs + [CG.fld(R.STRING, 1, CG.wstr(b"payload")) + b"\x00"]
    n += 1
    arena = np.frombuffer(b"\xEE" * first + b"".join(msgs), dtype=np.uint8).copy()  # no spare bytes behind it
    in_off = np.full(n + 1, first, dtype=np.uint64)
    in_off[1:] += np.cumsum([len(m) for m in msgs]).astype(np.uint64)
    wa = [CG.arrays(col) for col in want]
    need_want = len(wa[0]["elems"]) + len(wa[2]["elems"])
    assert len(wa[0]["elems"]) > 4097 and len(wa[2]["elems"]) > 4 * 4097
    L = _lib.lib()
    with G.ColumnPlan(to_cols(cols)) as plan:
        def call(cap):
            val, cell = np.zeros((3, n), dtype=np.uint64), np.zeros((3, n), dtype=G.COL_CELL_DTYPE)
            lens, eo = np.zeros((3, n), dtype=np.uint32), np.zeros((2, n + 1), dtype=np.uint64)
            elems, need = np.full(cap + 8, FILL, dtype=np.uint64), C.c_uint64(0)
            rc = L.dg_cols_batch_host(plan.ctx.h, plan.h, R.STRUCT, arena.ctypes.data, in_off.ctypes.data, n,
                                      val.ctypes.data, cell.ctypes.data, lens.ctypes.data, eo.ctypes.data,
                                      elems.ctypes.data if cap else None, cap, C.byref(need))
            return rc, val, cell, lens, eo, elems, need.value

        for cap in (0, need_want - 1, need_want):
            rc, val, cell, lens, eo, elems, need = call(cap)
            assert rc == (0 if cap in (0, need_want) else -3) and need == need_want, (cap, rc, need)  # -3: DG_E_NOMEM
            for k in range(3):  # the cells and the offsets are filled at every cap
                CG.same({"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"],
                         "aux": cell[k]["aux"], "val": val[k], "len": lens[k]},
                        {f: wa[k][f] for f in CG.CELL_FIELDS}, "cap %d, column %d" % (cap, k))
            assert (eo[0] == wa[0]["off"]).all() and (eo[1] == wa[2]["off"] + wa[0]["off"][-1]).all()
            assert (elems[cap:] == FILL).all()
        assert (elems[:need_want] == np.concatenate([wa[0]["elems"], wa[2]["elems"]])).all()
    assert want[1][-1].status == R.OK and want[1][-1].len == 7
    assert bytes(arena[want[1][-1].val:want[1][-1].val + 7]) == b"payload"


def test_field_names_resolve_through_the_descriptor(corpus):
    from dynamicgo_amd import generic as G
    td = t2jgen.all_types_desc()
    name = next(nm for nm, f in td.struct.names.items() if f.id == 3)
    msgs = corpus[0][:200]
    by_name = G.columns_batch(msgs, [([G.PathFieldName(name)], "int")], desc=td)[0]
    want = CG.arrays(CR.column(msgs, [(R.FIELD, 3)], CR.INT))
    assert by_name.values.view(np.uint64).tolist() == want["val"].tolist()
    assert by_name.status.tolist() == want["status"].tolist() and 0 < by_name.valid.sum() < len(msgs)
