"""GPU: row columns (dynamicgo_amd.generic over dg_rows_*) against the checker
of rowsref.py, which composes kidsref (children, one level), tgetref's GetByPath
on every child's own bytes and colsref's casts. Every case goes through the
host entry and the device entry; every head field, row_off, every index entry,
every cell field and every value (doubles as u64) is compared with the
checker's. The inputs are rowsgen's, which test_rows_host.py runs through the
host build of the same walk."""
import random

import numpy as np
import pytest

import colsgen as CG
import colsref as CR
import faroff as FO
import kidsgen as KG
import rowsgen as RG
import rowsref as RR
import tgetgen as TG
import tgetref as R
from test_gpu_cols import FILL, FILL32, GUARD, upload
from test_gpu_tget import to_paths

pytestmark = pytest.mark.gpu

F, I = R.FIELD, R.INDEX


def plan_of(s):
    from dynamicgo_amd import generic as G
    return G.RowPlan(to_paths([s.parent])[0], [(to_paths([p])[0], k) for p, k in s.columns])


class Outputs:
    """every output of one launch between GUARD entries of fill: d_head, d_row_off, d_index and the cell arrays,
    column-major over cap"""

    def __init__(self, n, P, cap):
        import torch
        self.n, self.P, self.cap = n, P, cap

        def t(entries, words, dtype, fill):
            return torch.full((entries + 2 * GUARD, words) if words > 1 else (entries + 2 * GUARD,), fill, dtype=dtype,
                              device="cuda")

        self.head = t(n, 4, torch.int32, FILL32)
        self.row_off = t(n + 1, 1, torch.int64, FILL)
        self.index = t(cap, 4, torch.int32, FILL32)
        self.val = t(P * cap, 1, torch.int64, FILL)
        self.cell = t(P * cap, 1, torch.int64, FILL)
        self.len = t(P * cap, 1, torch.int32, FILL32)

    def column(self, k):
        a = GUARD + k * self.cap
        return self.val[a:a + self.cap], self.cell[a:a + self.cap], self.len[a:a + self.cap]

    def read(self, what, rows=None, cells=True, index=True, untouched=()):
        """(head, row_off, index, cols) as rowsgen.arrays gives them; the guards, and with `rows` given everything
        behind the first `rows` rows of the index and of every column, must be intact; untouched: cell arrays the
        launch was given another buffer for"""
        from dynamicgo_amd import generic as G
        n, P, cap = self.n, self.P, self.cap
        hh = self.head.cpu().numpy()
        ho = self.row_off.cpu().numpy().view(np.uint64)
        hi = self.index.cpu().numpy()
        hv, hc = self.val.cpu().numpy().view(np.uint64), self.cell.cpu().numpy().view(np.uint64)
        hl = self.len.cpu().numpy().view(np.uint32)
        for name, h, m, fill in (("d_head", hh.view(np.uint32), n, FILL32), ("d_row_off", ho, n + 1, FILL),
                                 ("d_index", hi.view(np.uint32), cap, FILL32), ("d_val", hv, P * cap, FILL),
                                 ("d_cell", hc, P * cap, FILL), ("d_len", hl, P * cap, FILL32)):
            assert (h[:GUARD] == fill).all() and (h[GUARD + m:] == fill).all(), "%s: a store outside %s" % (what, name)
        head = hh[GUARD:GUARD + n].copy().view(G.ROWS_HEAD_DTYPE).reshape(n)
        row_off = ho[GUARD:GUARD + n + 1]
        R_ = int(row_off[n]) if n else 0
        rows = min(R_, cap) if rows is None else rows
        ents = hi[GUARD:GUARD + cap].copy().view(G.ROW_ENT_DTYPE).reshape(cap)
        if not index:
            assert (hi.view(np.uint32) == FILL32).all(), "%s: d_index written though the cells were not asked for" % what
        else:
            assert (hi[GUARD + rows:].view(np.uint32) == FILL32).all(), "%s: an index entry at or behind row %d" % (what, rows)
        cols = []
        for k in range(P):
            a = GUARD + k * cap
            for name, h, fill in (("d_val", hv, FILL), ("d_cell", hc, FILL), ("d_len", hl, FILL32)):
                lo = a + (rows if cells and name not in untouched else 0)
                assert (h[lo:a + cap] == fill).all(), "%s: %s column %d written at or behind row %d" % (what, name, k, rows)
            c = hc[a:a + rows].copy().view(G.COL_CELL_DTYPE)
            cols.append({"status": c["status"], "type": c["type"], "step": c["step"], "aux": c["aux"], "val": hv[a:a + rows],
                         "len": hl[a:a + rows]})
        return ({f: head[f] for f in RG.HEAD_FIELDS}, row_off, {f: ents[f][:rows] for f in RG.ROW_FIELDS} if index else None,
                cols)


def cut(want, rows):
    """the checker's arrays with the index and the cells cut at `rows` rows"""
    head, row_off, index, cols = want
    return head, row_off, {f: a[:rows] for f, a in index.items()}, [{f: c[f][:rows] for f in CG.CELL_FIELDS} for c in cols]


def launch(plan, s, arena, d_off, o, own_index=True, cells=True, stream=None):
    from dynamicgo_amd import generic as G
    n = len(s.msgs)
    idx = o.index[GUARD:] if own_index and cells else None
    v, c, ln = (o.val[GUARD:], o.cell[GUARD:], o.len[GUARD:]) if cells else (None, None, None)
    G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], idx, v, c, ln, row_cap=o.cap if cells else 0,
                  root_type=s.root_type, stream=stream, max_len=max(map(len, s.msgs), default=0))


def run_device(s, first=0):
    """the sizing call, then the full call with row_cap = R"""
    import torch
    n, P = len(s.msgs), len(s.columns)
    with plan_of(s) as plan:
        arena, d_off, _ = upload(s.msgs, first)
        o = Outputs(n, P, 0)
        launch(plan, s, arena, d_off, o, cells=False)
        torch.cuda.synchronize()
        sized = o.read("sizing call", index=False)
        R_ = int(sized[1][n])
        o = Outputs(n, P, R_)
        launch(plan, s, arena, d_off, o)
        torch.cuda.synchronize()
        got = o.read("device entry")
        for f in RG.HEAD_FIELDS:
            assert (sized[0][f] == got[0][f]).all(), f
        assert (sized[1] == got[1]).all()
        return got


def run_host(s):
    from dynamicgo_amd import generic as G
    with plan_of(s) as plan:
        head, row_off, index, val, cell, lens, _ = G.rows_records(s.msgs, plan, s.root_type)
        cols = [{"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"], "aux": cell[k]["aux"],
                 "val": val[k], "len": lens[k]} for k in range(plan.count)]
        return {f: head[f] for f in RG.HEAD_FIELDS}, row_off, {f: index[f] for f in RG.ROW_FIELDS}, cols


_want = {}


def expect(name, s):
    """the checker's answer, computed once per set"""
    if name not in _want:
        w = RG.expect(s)
        _want[name] = (w, RG.arrays(w, len(s.columns)))
    return _want[name]


def check(name, s):
    want, arrays = expect(name, s)
    RG.same(run_host(s), arrays, name + ", host entry")
    RG.same(run_device(s), arrays, name + ", device entry")
    return want


# ------------------------------------------------------------------- cases
SETS = RG.all_sets()


@pytest.mark.parametrize("name", [k for k in SETS if k != "geometry"])
def test_built_sets(name):
    """the kind x element-type matrix over LIST and SET parents, the heads (a parent of every wire type, all 256
    element type bytes, negative counts, every prefix), the element bounds (the last element the arena's last bytes,
    elements at every residue mod 16) and both deep passes"""
    want = check(name, SETS[name])
    if name.startswith("arena's end"):
        s = SETS[name]
        starts = {m.rows[0].off % 16 for m in want}
        assert len(starts) == 16 and all(m.head.status == R.OK for m in want)
        last = want[-1].rows[-1]
        assert last.off + last.len == sum(map(len, s.msgs))  # the last element ends where the arena does
    if name == "lacks the next one's field":
        assert [row[1].status for row in want[0].cells] == [R.NOT_FOUND, R.OK, R.NOT_FOUND, CR.E_UNSUPPORTED, R.NOT_FOUND,
                                                            R.NOT_FOUND]
    if name == "element types":
        assert sum(m.head.status == R.OK for m in want) == 26 and sum(m.head.status == R.E_READ for m in want) == 490
    if name == "prefixes":
        assert [m.head.status for m in want].count(R.OK) == 9 and all(not m.rows for m in want if m.head.status != R.OK)
    if name in ("above", "inside"):
        chains = RG.deep_sets()[1]
        frames = [TG.chain_frames(k, lf, [(F, 2)]) for k, lf in chains]
        assert any(f > TG.LDS_FRAMES for f in frames) and any(f <= TG.LDS_FRAMES for f in frames)
        assert any(c.status == R.OK for m in want for row in m.cells for c in row)


def test_statuses_of_the_built_sets():
    seen_h, seen_c = set(), set()
    for name, s in SETS.items():
        h, c = RG.statuses(expect(name, s)[0])
        seen_h |= {st for st, _ in h}
        seen_c |= {st for st, _ in c}
    assert seen_h == seen_c == {R.OK, R.NOT_FOUND, R.E_READ, CR.E_UNSUPPORTED}


@pytest.fixture(scope="module")
def pool():
    return RG.geometry_elements(64)


def test_geometry_columns(pool):
    """P = 1..8 over lists of 0, 1, 2, 63..65 and 257 elements with empty and failed messages between them; a
    changed message changes only its own head, rows and cells"""
    import torch
    s8 = SETS["geometry"]
    want8 = expect("geometry", s8)[0]
    assert sum(m.head.status == R.OK for m in want8) == 7 and len({m.head.status for m in want8}) == 4
    assert len(want8[4].rows) == 63
    # message 4 (the list of 63) changed twice: its first element's first field gets another id (the rows stay, cells
    # of that row change), and its own field header becomes the STOP byte (not found: its rows go, the later messages'
    # rows move up). Nothing but its own head, rows and cells differs from the unchanged batch's answer.
    j = 4
    base = sum(map(len, s8.msgs[:j]))
    at = 3 + 5
    renamed = s8.msgs[j][:at + 1] + b"\x77\x77" + s8.msgs[j][at + 3:]
    gone = b"\x00" + s8.msgs[j][1:]
    for P in range(1, 9):
        s = RG.Set(s8.msgs, s8.parent, s8.columns[:P], s8.root_type)
        head, row_off, index, cols = expect("geometry", s8)[1]
        RG.same(run_device(s), (head, row_off, index, cols[:P]), "P = %d" % P)
        for what, m in (("renamed", renamed), ("gone", gone)):
            one = RR.message(m, s.parent, s.columns, s.root_type, base, j)
            want2 = [w if i != j else one for i, w in enumerate(want8)]
            want2 = [RR.Msg(w.head, w.rows, [row[:P] for row in w.cells]) for w in want2]
            RG.same(run_device(RG.Set(s8.msgs[:j] + [m] + s8.msgs[j + 1:], s.parent, s.columns, s.root_type)),
                    RG.arrays(want2, P), "P = %d, message %d %s" % (P, j, what))
            assert one.head.status == (R.OK if what == "renamed" else R.NOT_FOUND) and one.cells != want8[j].cells
    RG.same(run_host(s8), expect("geometry", s8)[1], "host entry")
    torch.cuda.synchronize()


@pytest.mark.parametrize("total", (63, 64, 65, 255, 256, 257))
def test_pairs_around_the_block(pool, total):
    """R * P at 63 .. 257 with P = 1, and R at the same values with P = 3: one block's rows span several messages"""
    msgs = RG.geometry_batch(RG.sizes_for(total), pool)
    for P in (1, 3):
        s = RG.Set(msgs, RG.ONE, CG.GEOMETRY_COLUMNS[:P], R.STRUCT)
        want = RG.expect(s)
        assert sum(len(m.rows) for m in want) == total
        RG.same(run_device(s), RG.arrays(want, P), "R = %d, P = %d" % (total, P))


@pytest.mark.parametrize("n", (1, 255, 257, 2049))
def test_batch_sizes(pool, n):
    """n at 1, 255, 257 and 2 049, one past a scan tile; n = 0 launches nothing"""
    import torch
    from dynamicgo_amd import generic as G
    rng = random.Random(n)
    msgs = RG.geometry_batch([rng.randrange(4) for _ in range(n)], pool, fails=False)[:n]
    msgs = [m if i % 7 != 3 else b"\x00" for i, m in enumerate(msgs)]
    s = RG.Set(msgs, RG.ONE, CG.GEOMETRY_COLUMNS[:2], R.STRUCT)
    RG.same(run_device(s), RG.arrays(RG.expect(s), 2), "n = %d" % n)
    if n == 1:
        with plan_of(s) as plan:
            o = Outputs(0, 2, 0)
            G.rows_device(plan, None, None, 0, o.head[GUARD:], o.row_off[GUARD:])
            torch.cuda.synchronize()
            assert o.read("n = 0", index=False)[1].tolist() == [0]
            r = G.rows_batch([], plan)
            assert len(r.status) == 0 and r.offsets.tolist() == [0] and r.columns[0].values.shape == (0,)


def test_long_lists(pool):
    """a list of 2 049 struct elements between short ones, and lists of 0..2 049 fixed-size elements, whose index
    entries are arithmetic"""
    s = RG.Set(RG.geometry_batch((1, 2049, 2), pool, fails=False), RG.ONE, CG.GEOMETRY_COLUMNS[:3], R.STRUCT)
    check("long struct list", s)
    msgs = [RG.rows_field([CG.list_body(et, 1, salt=j) for j in range(c)], et) + b"\x00"
            for et in (R.I64, R.I16, R.BYTE, R.DOUBLE) for c in RG.LIST_SIZES]
    check("long fixed lists", RG.Set(msgs, RG.ONE, [([], CR.INT), ([], CR.F64)], R.STRUCT))


@pytest.mark.parametrize("own_index", (True, False), ids=["index given", "index NULL"])
def test_row_cap(own_index):
    """row_cap = R, R - 1, 0 and R + 70 with guards: no row at an index >= row_cap is stored, d_row_off[n] still
    tells the need; one call with room to spare needs no sizing call"""
    import torch
    from dynamicgo_amd import generic as G
    s = SETS["geometry"]
    want = expect("geometry", s)[1]
    n, P = len(s.msgs), len(s.columns)
    total = int(want[1][n])
    arena, d_off, _ = upload(s.msgs)
    with plan_of(s) as plan:
        for cap in (total, total - 1, 257, 0, total + 70):
            o = Outputs(n, P, cap)
            launch(plan, s, arena, d_off, o, own_index=own_index)
            torch.cuda.synchronize()
            rows = min(cap, total)
            got = o.read("row_cap %d" % cap, rows=rows, index=own_index)
            RG.same(got, cut(want, rows), "row_cap %d" % cap)
            assert int(got[1][n]) == total
        # the index alone: cells NULL with d_index given
        o = Outputs(n, P, total)
        G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], o.index[GUARD:], row_cap=total)
        torch.cuda.synchronize()
        got = o.read("index alone", cells=False)
        CG.same(got[2], want[2], "index alone")
        v, c, _ = Outputs(n, P, total).column(0)
        with pytest.raises(Exception, match="needs d_len"):
            G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], None, v, c, None, row_cap=total)
        with pytest.raises(Exception, match="2\\^32 pairs"):
            G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], None, v, c, o.len, row_cap=2 ** 30)
        torch.cuda.synchronize()


def test_chains_around_max_skip_depth():
    """test_gpu_kids.py's two cases on the head: below field 1 the node's own skip takes one level of the 1 023,
    as the root it does not, so the last depth that is OK lies one apart. A row's lookup starts a fresh budget on
    the element's bytes: the cell of a chain one level deeper than its head allows is still OK."""
    chains = [c for c in KG.limit_chains() if c[0][0] in "LE"]
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    cols = [([], CR.LEN), ([(I, 0)], CR.LEN)]
    last_ok = {}
    for what, ms, path in (("f1", msgs, RG.ONE), ("as root", [m[3:-8] for m in msgs], [])):
        for kind in "LE":
            sel = [i for i, (k, _) in enumerate(chains) if k[0] == kind]
            s = RG.Set([ms[i] for i in sel], path, cols, msgs[sel[0]][0] if what == "as root" else R.STRUCT)
            name = "limit %s %s" % (what, kind)
            _want[name] = TG.deep_checker(lambda: (lambda w: (w, RG.arrays(w, 2)))(RG.expect(s)))
            want = check(name, s)
            ok = [m.head.status == R.OK for m in want]
            assert any(ok) and not all(ok) and all(m.head.status in (R.OK, R.E_READ) for m in want)
            assert all(m.cells[0][0].status == R.OK for m in want if m.head.status == R.OK)
            last_ok[what, kind] = 1018 + sum(ok) - 1
    for kind in "LE":
        assert last_ok["as root", kind] == last_ok["f1", kind] + 1
    # the parents that are no list, at the same depths: E_READ where the skip gives up, unsupported before
    others = [c for c in KG.limit_chains() if c[0][0] in "SMK"]
    s = RG.Set([TG.chain_message(k, lf) for k, lf in others], RG.ONE, cols, R.STRUCT)
    _want["limit others"] = TG.deep_checker(lambda: (lambda w: (w, RG.arrays(w, 2)))(RG.expect(s)))
    want = check("limit others", s)
    assert {m.head.status for m in want} == {R.E_READ, CR.E_UNSUPPORTED}


def test_fixed_lists_against_columns_batch():
    """list<i64> (and the other widths) through the empty sub-path under INT: the elements themselves, the values
    columns_batch gives for the same field as a list column"""
    from dynamicgo_amd import generic as G
    msgs = [m for m in CG.list_messages() if len(m) < 40000]
    parent = to_paths([RG.ONE])[0]
    r = G.rows_batch(msgs, parent, [([], "int"), ([], "float64")])
    ci, cf = G.columns_batch(msgs, [(parent, "list[int]"), (parent, "list[float64]")])
    ok_i, ok_f = ci.valid & (ci.lengths > 0), cf.valid & (cf.lengths > 0)
    assert ok_i.sum() > 20 and ok_f.sum() > 5
    for col, c, ok in ((r.columns[0], ci, ok_i), (r.columns[1], cf, ok_f)):
        for i in np.nonzero(ok)[0]:
            a, b = int(r.offsets[i]), int(r.offsets[i + 1])
            assert r.status[i] == R.OK and b - a == int(c.lengths[i])
            assert col.valid[a:b].all()
            assert (col.values[a:b].view(np.uint64) == c.values[int(c.offsets[i]):int(c.offsets[i + 1])].view(np.uint64)).all()
    # a list the cast rejects is still a list of rows: the rows' cells say so one by one
    bools = [i for i in range(len(msgs)) if r.head["elem_type"][i] == R.BOOL and r.head["count"][i]]
    assert bools and all(r.columns[0].status[int(r.offsets[i])] == CR.E_UNSUPPORTED for i in bools)
    assert (r.status == R.OK).sum() > 40 and {r.error(i) for i in range(len(msgs))} == {
        None, "ErrNotFound", "ErrRead", "ErrUnsupportedType"}


def test_row_list_device():
    """dg_rows_list_device over a list<i64> field of the elements, rows of 0..257 elements: items[*].tags as a ragged
    tensor over rows"""
    import torch
    from dynamicgo_amd import generic as G
    counts = [0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 3]
    elems = [CG.fld(R.I32, 1, b"\0\0\0\1") + CG.fld(R.LIST, 2, CG.lst(R.I64, c, CG.list_body(R.I64, c, salt=c))) + b"\x00"
             for c in counts]
    elems.append(CG.fld(R.LIST, 2, CG.lst(R.STRING, 1, CG.wstr(b"x"))) + b"\x00")  # unsupported: no elements
    elems.append(b"\x00")                                                          # not found
    msgs = [RG.rows_field(elems[:5]) + b"\x00", b"\x00", RG.rows_field(elems[5:]) + b"\x00", RG.rows_field([]) + b"\x00"]
    s = RG.Set(msgs, RG.ONE, [([(F, 2)], CR.LIST_INT), ([(F, 1)], CR.INT), ([(F, 2)], CR.LEN)], R.STRUCT)
    want = RG.expect(s)
    cells = [row[0] for m in want for row in m.cells]
    w_off = np.concatenate([[0], np.cumsum([len(c.elems or []) for c in cells])]).astype(np.uint64)
    w_el = np.array([e for c in cells for e in (c.elems or [])], dtype=np.uint64)
    n, rows, total = len(msgs), len(cells), len(w_el)
    assert rows == len(elems) and total == sum(counts)
    arena, d_off, _ = upload(msgs)
    with plan_of(s) as plan:
        o = Outputs(n, 3, rows)
        launch(plan, s, arena, d_off, o)
        v, c, ln = o.column(0)
        for cap in (total, total - 1, 0):
            off = torch.full((rows + 1 + GUARD,), FILL, dtype=torch.int64, device="cuda")
            el = torch.full((total + GUARD,), FILL, dtype=torch.int64, device="cuda")
            G.row_list_device(plan, 0, arena, rows, v, c, ln, off, el if cap else None, cap)
            torch.cuda.synchronize()
            h_off, h = off.cpu().numpy().view(np.uint64), el.cpu().numpy().view(np.uint64)
            assert (h_off[:rows + 1] == w_off).all() and (h_off[rows + 1:] == FILL).all()
            assert (h[:cap] == w_el[:cap]).all() and (h[cap:] == FILL).all(), cap
        with pytest.raises(Exception, match="no list column"):
            G.row_list_device(plan, 1, arena, rows, v, c, ln, off, None, 0)
        RG.same(o.read("list rows"), RG.arrays(want, 3), "list rows")
        # the public call gives the same ragged column
        r = G.rows_batch(msgs, plan)
        assert r.columns[0].offsets.astype(np.uint64).tolist() == w_off.tolist()
        assert r.columns[0].values.view(np.uint64).tolist() == w_el.tolist()
        assert r.offsets.tolist() == [0, 5, 5, rows, rows] and r.index["msg"].tolist() == [0] * 5 + [2] * (rows - 5)


def test_streams():
    """rows on one stream against columns_device and children_device on two others, and two unsynchronised rows
    launches on two streams: each component has a queue, counters and frames of its own, and rows orders its own"""
    import torch
    from dynamicgo_amd import generic as G
    sets, _ = RG.deep_sets()
    s = sets["inside"]
    msgs, n, P = s.msgs, len(s.msgs), len(s.columns)
    want = expect("inside", s)[1]
    total = int(want[1][n])
    col_want = CG.expect(msgs, [(RG.ONE, CR.LEN)])
    kid_want = KG.expect(msgs, RG.ONE, False)
    arena, d_off, _ = upload(msgs)
    st = [torch.cuda.Stream() for _ in range(4)]
    with plan_of(s) as plan, G.ColumnPlan([(to_paths([RG.ONE])[0], CR.LEN)]) as cp, G.PathSet(to_paths([RG.ONE])) as ps:
        outs = [[Outputs(n, P, total) for _ in range(4)] for _ in range(2)]
        cv = [torch.full((n,), FILL, dtype=torch.int64, device="cuda") for _ in range(8)]
        kh = [torch.full((n, 4), FILL32, dtype=torch.int32, device="cuda") for _ in range(4)]
        ko = [torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda") for _ in range(4)]
        kr = [torch.full((int(kid_want[1][n]), 8), FILL32, dtype=torch.int32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for r in range(4):
            launch(plan, s, arena, d_off, outs[0][r], stream=st[0])
            G.columns_device(cp, arena, d_off, n, cv[2 * r], cv[2 * r + 1], None, stream=st[1])
            G.children_device(ps, arena, d_off, n, kh[r], ko[r], kr[r], kr[r].shape[0], stream=st[2])
            launch(plan, s, arena, d_off, outs[1][r], own_index=False, stream=st[3])
        torch.cuda.synchronize()
        for r in range(4):
            RG.same(outs[0][r].read("round %d" % r), want, "round %d, stream 0" % r)
            RG.same(outs[1][r].read("round %d" % r, index=False), want, "round %d, stream 3" % r)
            assert cv[2 * r].cpu().numpy().view(np.uint64).tolist() == [c.val for c in col_want[0]]
            KG.same((kh[r].cpu().numpy().view(G.KIDS_HEAD_DTYPE).reshape(n), ko[r].cpu().numpy().view(np.uint64),
                     kr[r].cpu().numpy().view(G.KIDS_REC_DTYPE).reshape(-1)), kid_want, "round %d, children" % r)


# -------------------------------------------------------------- far offsets
FAR_ELEMS = [CG.fld(R.I32, 1, b"\x80\0\0\x03") + CG.fld(R.STRING, 2, CG.wstr(b"0123456789abcdef")) + b"\x00",
             CG.fld(R.STRING, 2, CG.wstr(b"second")) + b"\x00", CG.fld(R.I32, 1, b"\0\0\0\7") + b"\x00"]
FAR_PIVOT = RG.rows_field(FAR_ELEMS) + b"\x00"
FAR_COLUMNS = [([(F, 2)], CR.STR), ([(F, 1)], CR.INT)]
# where B falls in the pivot: in its field header (the message straddles), inside element 0's string payload (which
# starts at byte 8 + 14), at the first byte of element 1 (8 + 31)
FAR_DELTAS = {"message": -1, "string payload": -(8 + 14 + 5), "element 1": -(8 + 31)}


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
def test_far_offsets(far_arenas, pool, B, where):
    """inputs, element and STR offsets and the output arrays across 2^31 and 2^32: the index lies in the far output
    arena with B inside it, d_val behind it, wholly above B"""
    import torch
    from dynamicgo_amd import generic as G
    inp, outa = far_arenas
    small = RG.geometry_batch([1, 2, 0, 3] * 5, pool, fails=False)
    msgs = small[:10] + [FAR_PIVOT] + small[10:]
    n, pivot = len(msgs), 10
    in_off = FO.place([len(m) for m in msgs], B, pivot, FAR_DELTAS[where])
    FO.check_layout(in_off, B, guard=0, tail=FO.TAIL)
    inp.put_input(in_off, msgs, B)
    s = RG.Set(msgs, RG.ONE, FAR_COLUMNS, R.STRUCT)
    want = RG.expect(s, first=int(in_off[0]))
    wa = RG.arrays(want, 2)
    a = int(in_off[pivot])
    assert want[pivot].rows[0].off == a + 8 and want[pivot].cells[0][0].val == a + 8 + 14
    assert {"message": a < B < a + 3, "string payload": a + 22 < B < a + 38, "element 1": want[pivot].rows[1].off == B}[where]
    offs = [c.val for m in want for row in m.cells for c in row[:1] if c.status == R.OK]
    assert any(o >= B for o in offs) and any(o < B for o in offs)
    total = int(wa[1][n])
    # d_index (16 bytes a row, B at its middle) and behind it d_val (8 bytes a cell) in the far output arena
    i_lo = B - 16 * (total // 2)
    i_off = np.array([i_lo, B, i_lo + 16 * total], dtype=np.int64)
    v_lo = i_lo + 16 * total + 4096
    v_off = np.array([v_lo, v_lo + 16 * total], dtype=np.int64)
    FO.check_layout(i_off, B, others=[(v_lo - FO.GUARD, v_lo + 16 * total + FO.GUARD)])
    outa.prefill(i_off, B)
    outa.prefill(v_off, B)
    with plan_of(s) as plan:
        d_off = torch.from_numpy(in_off).cuda()
        o = Outputs(n, 2, total)
        G.rows_device(plan, inp.base, d_off, n, o.head[GUARD:], o.row_off[GUARD:], outa.base[i_lo:], outa.base[v_lo:],
                      o.cell[GUARD:], o.len[GUARD:], row_cap=total)
        torch.cuda.synchronize()
        got = o.read("far", index=False, untouched=("d_val",))
        ents = outa.collect(i_off, B, what="d_index").view(G.ROW_ENT_DTYPE)
        vals = outa.collect(v_off, B, what="d_val").view(np.uint64)
    CG.same(got[0], wa[0], "far head")
    assert (got[1] == wa[1]).all()
    CG.same({f: ents[f] for f in RG.ROW_FIELDS}, wa[2], "far index")
    for k in range(2):
        assert (vals[k * total:(k + 1) * total] == wa[3][k]["val"]).all(), k
        CG.same({f: got[3][k][f] for f in CG.CELL_FIELDS if f != "val"}, {f: wa[3][k][f] for f in CG.CELL_FIELDS if f != "val"},
                "far column %d" % k)


# -------------------------------------------------------------------- fuzz
@pytest.mark.parametrize("plan", list(RG.FUZZ_PLANS))
@pytest.mark.parametrize("corpus", ("fuzz", "mutated"))
def test_fuzz(corpus, plan):
    msgs = KG.fuzz_messages(2048)[corpus == "mutated"]
    parent, cols = RG.FUZZ_PLANS[plan]
    want = check("%s %s" % (corpus, plan), RG.Set(msgs, parent, cols, R.STRUCT))
    heads, cells = RG.statuses(want)
    print(corpus, plan, heads, cells, sum(len(m.rows) for m in want))
    assert (heads, cells, sum(len(m.rows) for m in want)) == RG.FUZZ_WANT[corpus, plan]


def test_fuzz_counts_cover_the_statuses():
    """from the counts alone: every status occurs among the heads or the cells, the lookup's E_TYPE included, and
    under the list-of-structs plan the messages with rows are the majority"""
    seen = {st for h, c, _ in RG.FUZZ_WANT.values() for st, _ in h + c}
    assert seen == {R.OK, R.NOT_FOUND, R.E_READ, R.E_TYPE, CR.E_UNSUPPORTED}
    heads = dict(RG.FUZZ_WANT["fuzz", "f10"][0])
    assert heads[R.OK] > sum(heads.values()) / 2


# ------------------------------------------------- the entries' own contracts
def test_host_entry_sizing_and_an_arena_not_at_zero():
    """dg_rows_batch_host as C callers see it: in_off[0] = 37 (offsets are from `thrift`), all outputs NULL and cap 0
    for the need, DG_E_NOMEM below it, columns row_cap apart with the slack untouched, index NULL"""
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    s = SETS["geometry"]
    first, n, P = 37, len(s.msgs), 3
    s = RG.Set(s.msgs, s.parent, s.columns[:P], s.root_type)
    wa = RG.arrays(RG.expect(s, first=first), P)
    total = int(wa[1][n])
    arena = np.frombuffer(b"\xEE" * first + b"".join(s.msgs), dtype=np.uint8).copy()  # no spare bytes behind it
    in_off = np.full(n + 1, first, dtype=np.uint64)
    in_off[1:] += np.cumsum([len(m) for m in s.msgs]).astype(np.uint64)
    L = _lib.lib()
    with plan_of(s) as plan:
        def call(cap, index=True, sizing=False):
            head, row_off = np.zeros(n, dtype=G.ROWS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
            idx = np.full(cap + 1, 0x5A, dtype=G.ROW_ENT_DTYPE)
            val, cell = np.full((P, cap + 1), FILL, dtype=np.uint64), np.full((P, cap + 1), FILL, dtype=np.uint64)
            lens, need = np.full((P, cap + 1), FILL32, dtype=np.uint32), C.c_uint64(0)
            ptr = (lambda a: None) if sizing else (lambda a: a.ctypes.data)
            rc = L.dg_rows_batch_host(plan.ctx.h, plan.h, s.root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                      head.ctypes.data, row_off.ctypes.data, ptr(idx) if index else None, ptr(val), ptr(cell),
                                      ptr(lens), 0 if sizing else cap + 1, C.byref(need))
            return rc, head, row_off, idx, val, cell, lens, need.value

        for cap, index, sizing in ((0, True, True), (total, True, False), (total + 5, False, False)):
            rc, head, row_off, idx, val, cell, lens, need = call(cap, index, sizing)
            assert rc == 0 and need == total
            CG.same({f: head[f] for f in RG.HEAD_FIELDS}, wa[0], "host head")
            assert (row_off == wa[1]).all()
            if sizing:
                continue
            for k in range(P):
                c = cell[k, :total].copy().view(G.COL_CELL_DTYPE)
                CG.same({"status": c["status"], "type": c["type"], "step": c["step"], "aux": c["aux"], "val": val[k, :total],
                         "len": lens[k, :total]}, wa[3][k], "host column %d" % k)
            assert (val[:, total:] == FILL).all() and (cell[:, total:] == FILL).all() and (lens[:, total:] == FILL32).all()
            if index:
                CG.same({f: idx[f][:total] for f in RG.ROW_FIELDS}, wa[2], "host index")
            assert (idx["len"][total if index else 0:] == 0x5A).all()
        head, row_off = np.zeros(n, dtype=G.ROWS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        small = np.zeros((P, total - 1), dtype=np.uint64)
        need = C.c_uint64(0)
        rc = L.dg_rows_batch_host(plan.ctx.h, plan.h, s.root_type, arena.ctypes.data, in_off.ctypes.data, n, head.ctypes.data,
                                  row_off.ctypes.data, None, small.ctypes.data, small.ctypes.data, small.ctypes.data,
                                  total - 1, C.byref(need))
        assert rc == -3 and need.value == total and (small == 0).all()  # DG_E_NOMEM


def test_plan_create_rejects_and_names_resolve():
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    from dynamicgo_amd.http import ConvError
    import t2jgen
    L, ctx = _lib.lib(), default_context()
    one = G.compile_paths(to_paths([RG.ONE]))
    two = G.compile_paths(to_paths([RG.ONE, [(F, 2)]]))

    def create(parent, sub, kinds):
        h = C.c_void_p()
        rc = L.dg_rows_create(ctx.h, bytes(parent), len(parent), bytes(sub), len(sub), bytes(kinds), len(kinds), C.byref(h))
        if rc == 0:
            assert L.dg_rows_count(h) == len(kinds)
            L.dg_rows_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create(one, two, [CR.INT, CR.LIST_F64])[0] == 0
    for parent, sub, kinds, text in ((two, two, [CR.INT, CR.INT], "2 parent paths"), (one, two, [CR.INT], "1 kinds for 2"),
                                     (one, two, [CR.INT, 7], "unknown kind 7"), (one[:16], two, [CR.INT, CR.INT], "no header")):
        rc, err = create(parent, sub, kinds)
        assert rc == -6 and text in err, (kinds, rc, err)  # DG_E_ARG
    # names: the parent's through the descriptor, a sub-path's through the descriptor of the list's elements
    td = t2jgen.all_types_desc()
    msgs = KG.fuzz_messages(200)[0]
    f10 = td.struct.field_by_id(10)
    inners = next(nm for nm, f in td.struct.names.items() if f.id == 10)
    a, b = (next(nm for nm, f in f10.type.elem.struct.names.items() if f.id == k) for k in (1, 2))
    by_name = G.rows_batch(msgs, [G.PathFieldName(inners)], [([G.PathFieldName(a)], "int"), ([G.PathFieldName(b)], "str")],
                           desc=td)
    by_id = G.rows_batch(msgs, to_paths([[(F, 10)]])[0], [(to_paths([[(F, 1)]])[0], "int"), (to_paths([[(F, 2)]])[0], "str")])
    assert len(by_id.index) > 100 and by_id.columns[0].valid.sum() > 100
    assert by_name.columns[0].values.tolist() == by_id.columns[0].values.tolist()
    assert by_name.columns[1].values == by_id.columns[1].values and by_name.offsets.tolist() == by_id.offsets.tolist()
    with pytest.raises(ConvError):
        G.RowPlan([G.PathFieldId(10)], [([G.PathFieldName("a")], "int")])
    with pytest.raises(ConvError):
        G.RowPlan([G.PathFieldName(inners)], [([G.PathFieldName("nope")], "int")], desc=td)
