"""GPU: map rows (dynamicgo_amd.generic over dg_rows_create_map and
dg_rows_map_*) against the checker of mrowsref.py, which composes kidsref
(children of the MAP node, one level: the keys and the value spans), tgetref's
GetByPath on every value's own bytes and colsref's casts. Every case goes
through the host entry and the device entry; every head field, row_off, every
index entry, every key, every key length, every cell field and every value is
compared with the checker's. The inputs are mrowsgen's, which test_mrows_host.py
runs through the host build of the same head and index."""
import random
import struct

import numpy as np
import pytest

import colsgen as CG
import colsref as CR
import faroff as FO
import kidsgen as KG
import mrowsgen as MG
import mrowsref as MR
import rowsgen as RG
import test_gpu_rows as TR
import tgetgen as TG
import tgetref as R
from test_gpu_cols import FILL, FILL32, GUARD, upload
from test_gpu_tget import to_paths

pytestmark = pytest.mark.gpu

F, I = R.FIELD, R.INDEX
KEY_NAMES = {MG.STR: "str", MG.INT: "int"}


def plan_of(s):
    from dynamicgo_amd import generic as G
    return G.RowPlan(to_paths([s.parent])[0], [(to_paths([p])[0], k) for p, k in s.columns], keys=KEY_NAMES[s.keys])


class Outputs(TR.Outputs):
    """test_gpu_rows' outputs and d_key, d_key_len (cap entries each) between GUARD entries of fill"""

    def __init__(self, n, P, cap):
        import torch
        super().__init__(n, P, cap)
        self.key = torch.full((cap + 2 * GUARD,), FILL, dtype=torch.int64, device="cuda")
        self.key_len = torch.full((cap + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda")

    def read(self, what, rows=None, cells=True, index=True, untouched=(), keys=True, lens=True):
        """(head, row_off, index, cols, keys) as mrowsgen.arrays gives them; everything behind the first `rows` keys and
        key lengths, and all of an array the launch did not get (keys / lens False), must be intact"""
        head, row_off, ents, cols = super().read(what, rows, cells, index, untouched)
        n, cap = self.n, self.cap
        R_ = int(row_off[n]) if n else 0
        rows = min(R_, cap) if rows is None else rows
        hk, hl = self.key.cpu().numpy().view(np.uint64), self.key_len.cpu().numpy().view(np.uint32)
        out = {}
        for name, h, fill, given in (("key", hk, FILL, keys), ("key_len", hl, FILL32, lens)):
            lo = GUARD + (rows if given else 0)
            assert (h[:GUARD] == fill).all() and (h[lo:] == fill).all(), "%s: d_%s written at or behind row %d" % (what, name, rows)
            if given:
                out[name] = h[GUARD:GUARD + rows]
        return head, row_off, ents, cols, out


def cut(want, rows):
    head, row_off, index, cols = TR.cut(want[:4], rows)
    return head, row_off, index, cols, {f: a[:rows] for f, a in want[4].items()}


def launch(plan, s, arena, d_off, o, own_index=True, cells=True, keys=True, lens=True, stream=None):
    from dynamicgo_amd import generic as G
    n = len(s.msgs)
    idx = o.index[GUARD:] if own_index and cells else None
    v, c, ln = (o.val[GUARD:], o.cell[GUARD:], o.len[GUARD:]) if cells else (None, None, None)
    G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], idx, v, c, ln, row_cap=o.cap if cells else 0,
                  root_type=s.root_type, stream=stream, max_len=max(map(len, s.msgs), default=0),
                  keys=o.key[GUARD:] if keys and cells else None, key_lens=o.key_len[GUARD:] if lens and cells else None)


def run_device(s, first=0):
    """the sizing call, then the full call with row_cap = R"""
    import torch
    n, P = len(s.msgs), len(s.columns)
    with plan_of(s) as plan:
        arena, d_off, _ = upload(s.msgs, first)
        o = Outputs(n, P, 0)
        launch(plan, s, arena, d_off, o, cells=False)
        torch.cuda.synchronize()
        sized = o.read("sizing call", index=False, keys=False, lens=False)
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
        head, row_off, index, val, cell, lens, _, key, key_len = G.rows_records(s.msgs, plan, s.root_type)
        cols = [{"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"], "aux": cell[k]["aux"],
                 "val": val[k], "len": lens[k]} for k in range(plan.count)]
        return ({f: head[f] for f in RG.HEAD_FIELDS}, row_off, {f: index[f] for f in RG.ROW_FIELDS}, cols,
                {"key": key, "key_len": key_len})


_want = {}


def expect(name, s):
    """the checker's answer, computed once per set"""
    if name not in _want:
        w = MG.expect(s)
        _want[name] = (w, MG.arrays(w, len(s.columns)))
    return _want[name]


def check(name, s):
    want, arrays = expect(name, s)
    MG.same(run_host(s), arrays, name + ", host entry")
    MG.same(run_device(s), arrays, name + ", device entry")
    return want


# ------------------------------------------------------------------- cases
SETS = MG.all_sets()


@pytest.mark.parametrize("name", list(SETS))
def test_built_sets(name):
    """key type x value type under both key kinds, all 256 key and value type bytes at size 0 and 1, negative counts,
    a parent of every wire type, maps and others as the root, every prefix, the keys at the width edges, duplicate
    keys, entries at every residue mod 16 with the last one the arena's last bytes, a key that ends the arena, both
    deep passes, maps of 0..257 entries between empty and failed messages, and fixed maps beside their walked form"""
    s = SETS[name]
    want = check(name, s)
    heads = [m.head for m in want]
    if name.startswith("matrix"):
        ok = [h.status == R.OK for h in heads]
        assert sum(ok) == (7 if s.keys == MG.STR else 28) and all(h.status == MR.E_UNSUPPORTED for h in heads if h.status)
        assert {h.elem_type for h in heads if h.status} == ({R.STRING} if s.keys == MG.INT else set(MR.K.INTS))
    if name.startswith("type bytes"):
        unsupported = [h for h in heads if h.status == MR.E_UNSUPPORTED]
        assert unsupported and all(h.type == R.MAP and h.count == 0 for h in unsupported)
        assert sum(h.status == R.OK and h.count == 0 for h in heads) >= 10  # size 0 is still a map of the key kind
    if name.startswith("arena's end"):
        assert len({m.head.first % 16 for m in want}) == 16 and all(h.status == R.OK for h in heads)
        last = want[-1].rows[-1]
        assert last.off + last.len == sum(map(len, s.msgs))  # the last value ends where the arena does
    if name == "a key ends the arena":
        assert [h.status for h in heads] == [R.OK, R.E_READ, R.OK, R.E_READ]
    if name == "prefixes":
        assert [h.status for h in heads].count(R.OK) == 9 and all(not m.rows for m in want if m.head.status != R.OK)
    if name == "string keys":
        assert [k.len for k in want[0].keys] == [0, 1, 1, 0] and want[1].keys[0].len == 3
    if name.startswith("deep values"):
        assert any(c.status == R.OK and c.val == 9 for m in want for row in m.cells for c in row[:1])
    if name.startswith("root type %d" % R.MAP):
        assert {h.status for h in heads} == {R.OK, R.E_READ, MR.E_UNSUPPORTED}


def test_statuses_of_the_built_sets():
    seen_h, seen_c = set(), set()
    for name, s in SETS.items():
        h, c = MG.statuses(expect(name, s)[0])
        seen_h |= {st for st, _ in h}
        seen_c |= {st for st, _ in c}
    assert seen_h == {R.OK, R.NOT_FOUND, R.E_READ, MR.E_UNSUPPORTED} and seen_h <= seen_c


@pytest.fixture(scope="module")
def pool():
    return RG.geometry_elements(64)


@pytest.mark.parametrize("P", (1, 8))
def test_columns_and_a_changed_message(P):
    """P = 1 and 8 over the geometry maps; a changed message changes only its own head, rows, keys and cells"""
    s8 = SETS["geometry, str keys"]
    want8, (head, row_off, index, cols, keys) = expect("geometry, str keys", s8)
    assert sum(m.head.status == R.OK for m in want8) == 7 and len({m.head.status for m in want8}) == 4
    j = 4
    assert len(want8[j].rows) == 63
    s = MG.Set(s8.msgs, s8.parent, s8.columns[:P], s8.root_type, s8.keys)
    MG.same(run_device(s), (head, row_off, index, cols[:P], keys), "P = %d" % P)
    base = sum(map(len, s8.msgs[:j]))
    m = s8.msgs[j]
    at = 3 + 6 + 4  # entry 0's key payload "-100": another key of the same length; then the field header as STOP
    rekeyed = m[:at] + b"+" + m[at + 1:]
    gone = b"\x00" + m[1:]
    for what, m2 in (("rekeyed", rekeyed), ("gone", gone)):
        one = MR.message(m2, s.parent, s.columns, s.keys, s.root_type, base, j)
        want2 = [w if i != j else one for i, w in enumerate(want8)]
        want2 = [MR.Msg(w.head, w.rows, w.keys, [row[:P] for row in w.cells]) for w in want2]
        MG.same(run_device(MG.Set(s8.msgs[:j] + [m2] + s8.msgs[j + 1:], s.parent, s.columns, s.root_type, s.keys)),
                MG.arrays(want2, P), "P = %d, message %d %s" % (P, j, what))
        assert one.head.status == (R.OK if what == "rekeyed" else R.NOT_FOUND)
    arena = b"".join(s8.msgs[:j] + [rekeyed])
    k0 = MR.message(rekeyed, s.parent, s.columns, s.keys, s.root_type, base, j).keys[0]
    assert arena[k0.val:k0.val + k0.len] == b"+100"


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_batch_sizes(pool, n):
    """n at 1 and around the wave and the block; n = 0 launches nothing"""
    import torch
    from dynamicgo_amd import generic as G
    rng = random.Random(n)
    for kt, kind in ((R.STRING, MG.STR), (R.I16, MG.INT)):
        msgs = MG.geometry_batch([rng.randrange(4) for _ in range(n)], pool, kt, fails=False)[:n]
        msgs = [m if i % 7 != 3 else b"\x00" for i, m in enumerate(msgs)]
        s = MG.Set(msgs, MG.ONE, CG.GEOMETRY_COLUMNS[:2], R.STRUCT, kind)
        MG.same(run_device(s), MG.arrays(MG.expect(s), 2), "n = %d" % n)
    if n == 1:
        with plan_of(s) as plan:
            o = Outputs(0, 2, 0)
            G.rows_device(plan, None, None, 0, o.head[GUARD:], o.row_off[GUARD:])
            torch.cuda.synchronize()
            assert o.read("n = 0", index=False, keys=False, lens=False)[1].tolist() == [0]
            r = G.rows_batch([], plan)
            assert len(r.status) == 0 and r.offsets.tolist() == [0] and len(r.keys) == 0 and len(r.key_lengths) == 0


def test_long_maps(pool):
    """a map of 2 049 struct values between short ones under both key kinds (the walk), and map<i32, i64> of 0..2 049
    entries (arithmetic) beside the same data under string keys (the walk)"""
    for kt, kind in ((R.STRING, MG.STR), (R.I64, MG.INT)):
        s = MG.Set(MG.geometry_batch((1, 2049, 2), pool, kt, fails=False), MG.ONE, CG.GEOMETRY_COLUMNS[:3], R.STRUCT, kind)
        check("long struct map %d" % kind, s)
    a = check("long fixed maps", MG.Set(MG.fixed_batch(MG.MAP_SIZES, False), MG.ONE, [([], CR.INT)], R.STRUCT, MG.INT))
    b = check("long walked maps", MG.Set(MG.fixed_batch(MG.MAP_SIZES, True), MG.ONE, [([], CR.INT)], R.STRUCT, MG.STR))
    assert [m.head.count for m in a] == [m.head.count for m in b] and max(m.head.count for m in a) == 2049
    assert [[c[0].val for c in m.cells] for m in a] == [[c[0].val for c in m.cells] for m in b]


@pytest.mark.parametrize("name", ("geometry, str keys", "fixed maps"))
def test_row_cap_and_null_keys(name):
    """row_cap = R, R - 1, 0 and R + 70 with guards, with d_index given and NULL, and d_key NULL, d_key_len NULL and both
    NULL: no index entry, key, key length or cell of a row >= row_cap is stored and d_row_off[n] still tells the need;
    the index alone with its keys; the list entries' texts"""
    import torch
    from dynamicgo_amd import generic as G
    s = SETS[name]
    want = expect(name, s)[1]
    n, P = len(s.msgs), len(s.columns)
    total = int(want[1][n])
    arena, d_off, _ = upload(s.msgs)
    with plan_of(s) as plan:
        for cap in (total, total - 1, 0, total + 70):
            for own_index, keys, lens in ((True, True, True), (False, True, True), (True, False, True), (True, True, False),
                                          (False, False, False)):
                o = Outputs(n, P, cap)
                launch(plan, s, arena, d_off, o, own_index=own_index, keys=keys, lens=lens)
                torch.cuda.synchronize()
                rows = min(cap, total)
                what = "row_cap %d, index %s, keys %s, lens %s" % (cap, own_index, keys, lens)
                got = o.read(what, rows=rows, index=own_index, keys=keys and cap > 0, lens=lens and cap > 0)
                w = cut(want, rows)
                MG.same(got, w[:4] + ({f: w[4][f] for f in got[4]},), what)
                assert int(got[1][n]) == total
        # the index alone: cells NULL with d_index, d_key and d_key_len given
        o = Outputs(n, P, total)
        G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], o.index[GUARD:], row_cap=total,
                      keys=o.key[GUARD:], key_lens=o.key_len[GUARD:])
        torch.cuda.synchronize()
        got = o.read("index alone", cells=False)
        CG.same(got[2], want[2], "index alone")
        CG.same(got[4], want[4], "index alone, keys")
        v, c, _ = Outputs(n, P, total).column(0)
        with pytest.raises(Exception, match="2\\^32 pairs"):
            G.rows_device(plan, arena, d_off, n, o.head[GUARD:], o.row_off[GUARD:], None, v, c, o.len, row_cap=2 ** 32 // P)
        torch.cuda.synchronize()


def test_chains_around_max_skip_depth():
    """kidsgen's chains around MaxSkipDepth on the head: below field 1 the node's own skip takes one level of the
    1 023, as the root it does not, so the last depth that is OK lies one apart. The M chains are maps of string keys;
    the K chains have a map as the key (unsupported where the skip still succeeds), the others are no maps."""
    chains = KG.limit_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    cols = [([], CR.LEN)]
    last_ok = {}
    sel = [i for i, (k, _) in enumerate(chains) if k[0] == "M"]
    for what, ms, path, rt in (("f1", [msgs[i] for i in sel], MG.ONE, R.STRUCT), ("as root", [msgs[i][3:-8] for i in sel], [], R.MAP)):
        s = MG.Set(ms, path, cols, rt, MG.STR)
        name = "limit %s" % what
        _want[name] = TG.deep_checker(lambda: (lambda w: (w, MG.arrays(w, 1)))(MG.expect(s)))
        want = check(name, s)
        ok = [m.head.status == R.OK for m in want]
        assert any(ok) and not all(ok) and all(m.head.status in (R.OK, R.E_READ) for m in want)
        last_ok[what] = sum(ok)
    assert last_ok["as root"] == last_ok["f1"] + 1
    for kind in (MG.STR, MG.INT):
        s = MG.Set(msgs, MG.ONE, cols, R.STRUCT, kind)
        name = "limit all %d" % kind
        _want[name] = TG.deep_checker(lambda: (lambda w: (w, MG.arrays(w, 1)))(MG.expect(s)))
        want = check(name, s)
        assert {m.head.status for m in want} == ({R.OK, R.E_READ, MR.E_UNSUPPORTED} if kind == MG.STR else
                                                {R.E_READ, MR.E_UNSUPPORTED})


def test_row_list_device_over_map_rows():
    """dg_rows_list_device takes a map plan unchanged: map<string, list<i64>> rows of 0..257 elements as a ragged
    tensor over rows"""
    import torch
    from dynamicgo_amd import generic as G
    counts = [0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 3]
    vals = [CG.lst(R.I64, c, CG.list_body(R.I64, c, salt=c)) for c in counts]
    key = lambda j: CG.wstr(b"key%d" % j)  # noqa: E731
    msgs = [MG.map_field(R.STRING, R.LIST, [(key(j), v) for j, v in enumerate(vals[:5])]) + b"\x00", b"\x00",
            MG.map_field(R.STRING, R.LIST, [(key(j), v) for j, v in enumerate(vals[5:])]) + b"\x00",
            MG.map_field(R.STRING, R.LIST, []) + b"\x00"]
    s = MG.Set(msgs, MG.ONE, [([], CR.LIST_INT), ([], CR.LEN)], R.STRUCT, MG.STR)
    want = MG.expect(s)
    cells = [row[0] for m in want for row in m.cells]
    w_off = np.concatenate([[0], np.cumsum([len(c.elems or []) for c in cells])]).astype(np.uint64)
    w_el = np.array([e for c in cells for e in (c.elems or [])], dtype=np.uint64)
    n, rows, total = len(msgs), len(cells), len(w_el)
    assert rows == len(vals) and total == sum(counts)
    arena, d_off, _ = upload(msgs)
    with plan_of(s) as plan:
        o = Outputs(n, 2, rows)
        launch(plan, s, arena, d_off, o)
        v, c, ln = o.column(0)
        off = torch.full((rows + 1 + GUARD,), FILL, dtype=torch.int64, device="cuda")
        el = torch.full((total + GUARD,), FILL, dtype=torch.int64, device="cuda")
        G.row_list_device(plan, 0, arena, rows, v, c, ln, off, el, total)
        torch.cuda.synchronize()
        h_off, h = off.cpu().numpy().view(np.uint64), el.cpu().numpy().view(np.uint64)
        assert (h_off[:rows + 1] == w_off).all() and (h_off[rows + 1:] == FILL).all()
        assert (h[:total] == w_el).all() and (h[total:] == FILL).all()
        MG.same(o.read("list rows"), MG.arrays(want, 2), "list rows")
        r = G.rows_batch(msgs, plan)  # the public call gives the same ragged column, and the keys as bytes
        assert r.columns[0].offsets.astype(np.uint64).tolist() == w_off.tolist()
        assert r.columns[0].values.view(np.uint64).tolist() == w_el.tolist()
        assert r.keys == [b"key%d" % j for j in range(5)] + [b"key%d" % j for j in range(len(vals) - 5)]
        assert r.key_lengths.tolist() == [len(k) for k in r.keys] and r.offsets.tolist() == [0, 5, 5, rows, rows]


def test_public_keys_of_an_int_plan():
    from dynamicgo_amd import generic as G
    s = SETS["int key edges"]
    r = G.rows_batch(s.msgs, to_paths([s.parent])[0], [([], "int")], keys="int")
    want = expect("int key edges", s)[0]
    assert r.keys.dtype == np.int64 and r.keys.tolist() == [struct.unpack("<q", struct.pack("<Q", k.val))[0]
                                                            for m in want for k in m.keys]
    assert r.keys[:4].tolist() == [0, 127, 128, 255] and r.keys[4] == -1 and r.key_lengths[:5].tolist() == [1, 1, 1, 1, 2]
    lp = G.rows_batch(s.msgs, to_paths([s.parent])[0], [([], "int")])  # a list plan: a MAP parent is still unsupported
    assert lp.keys is None and lp.key_lengths is None and (lp.status == MR.E_UNSUPPORTED).all() and (lp.head["type"] == R.MAP).all()


def test_plan_kinds():
    """a map plan at the list entries and a list plan at the map entries are DG_E_ARG with a text, an unknown key kind
    too; dg_rows_create_map keeps dg_rows_create's limits and texts; names resolve against the map's value descriptor"""
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    import t2jgen
    L, ctx = _lib.lib(), default_context()
    one = G.compile_paths(to_paths([MG.ONE]))
    two = G.compile_paths(to_paths([MG.ONE, [(F, 2)]]))

    def create(parent, sub, kinds, key_kind):
        h = C.c_void_p()
        rc = L.dg_rows_create_map(ctx.h, bytes(parent), len(parent), bytes(sub), len(sub), bytes(kinds), len(kinds), key_kind,
                                  C.byref(h))
        if rc == 0:
            assert L.dg_rows_count(h) == len(kinds) and L.dg_rows_key_kind(h) == key_kind
            L.dg_rows_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    assert create(one, two, [CR.INT, CR.LIST_F64], 1)[0] == 0 and create(one, two, [CR.INT, CR.LIST_F64], 2)[0] == 0
    for parent, sub, kinds, kk, text in ((two, two, [CR.INT, CR.INT], 1, "2 parent paths"), (one, two, [CR.INT], 2, "1 kinds for 2"),
                                         (one, two, [CR.INT, 7], 1, "unknown kind 7"), (one, two, [CR.INT, CR.INT], 0, "unknown key kind 0"),
                                         (one, two, [CR.INT, CR.INT], 3, "unknown key kind 3")):
        rc, err = create(parent, sub, kinds, kk)
        assert rc == -6 and text in err, (kinds, kk, rc, err)  # DG_E_ARG
    with pytest.raises(ValueError):
        G.RowPlan([], [([], "int")], keys="bytes")
    s = SETS["string keys"]
    arena, d_off, _ = upload(s.msgs)
    n = len(s.msgs)
    o = Outputs(n, 2, 8)
    need = C.c_uint64(0)
    with plan_of(s) as mp, TR.plan_of(s) as lp:
        assert L.dg_rows_key_kind(mp.h) == 1 and L.dg_rows_key_kind(lp.h) == 0 and L.dg_rows_key_kind(None) == 0
        args = (C.c_uint8(R.STRUCT), arena.data_ptr(), d_off.data_ptr(), n, o.head[GUARD:].data_ptr(), o.row_off[GUARD:].data_ptr())
        for plan, entry, extra, text in ((mp, L.dg_rows_batch_device, (), "a map plan at a list entry"),
                                         (lp, L.dg_rows_map_batch_device, (None, None), "a list plan at a map entry")):
            rc = entry(ctx.h, plan.h, *args, None, *extra, None, None, None, 0, None, 0)
            assert rc == -6 and text in (L.dg_last_error() or b"").decode()
        h_arena, h_off = np.frombuffer(b"".join(s.msgs), dtype=np.uint8).copy(), np.zeros(n + 1, dtype=np.uint64)
        h_off[1:] = np.cumsum([len(m) for m in s.msgs])
        head, row_off = np.zeros(n, dtype=G.ROWS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        hargs = (C.c_uint8(R.STRUCT), h_arena.ctypes.data, h_off.ctypes.data, n, head.ctypes.data, row_off.ctypes.data)
        for plan, entry, extra, text in ((mp, L.dg_rows_batch_host, (), "a map plan at a list entry"),
                                         (lp, L.dg_rows_map_batch_host, (None, None), "a list plan at a map entry")):
            rc = entry(ctx.h, plan.h, *hargs, None, *extra, None, None, None, 0, C.byref(need))
            assert rc == -6 and text in (L.dg_last_error() or b"").decode()
    o.read("refused calls", rows=0, index=False, cells=False, keys=False, lens=False)
    # names: the parent's through the descriptor, a sub-path's through the descriptor of the map's values
    td = t2jgen.all_types_desc()
    msgs = KG.fuzz_messages(200)[0]
    by_name = G.rows_batch(msgs, [G.PathFieldName("m_i32")], [([G.PathFieldName("a")], "int"), ([G.PathFieldName("b")], "str")],
                           desc=td, keys="int")
    by_id = G.rows_batch(msgs, to_paths([[(F, 15)]])[0], [(to_paths([[(F, 1)]])[0], "int"), (to_paths([[(F, 2)]])[0], "str")],
                         keys="int")
    assert len(by_id.index) > 100 and by_id.columns[0].valid.sum() > 100 and (by_id.key_lengths == 4).all()
    assert by_name.columns[0].values.tolist() == by_id.columns[0].values.tolist() and by_name.keys.tolist() == by_id.keys.tolist()
    assert by_name.columns[1].values == by_id.columns[1].values and by_name.offsets.tolist() == by_id.offsets.tolist()


def test_host_entry_sizing_and_an_arena_not_at_zero():
    """dg_rows_map_batch_host as C callers see it: in_off[0] = 37 (offsets, string keys' too, are from `thrift`), all
    outputs NULL and cap 0 for the need, DG_E_NOMEM below it, key and key_len NULL"""
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    s = SETS["geometry, str keys"]
    first, n, P = 37, len(s.msgs), 3
    s = MG.Set(s.msgs, s.parent, s.columns[:P], s.root_type, s.keys)
    wa = MG.arrays(MG.expect(s, first=first), P)
    total = int(wa[1][n])
    arena = np.frombuffer(b"\xEE" * first + b"".join(s.msgs), dtype=np.uint8).copy()  # no spare bytes behind it
    in_off = np.full(n + 1, first, dtype=np.uint64)
    in_off[1:] += np.cumsum([len(m) for m in s.msgs]).astype(np.uint64)
    L = _lib.lib()
    with plan_of(s) as plan:
        def call(cap, keys=True, sizing=False):
            head, row_off = np.zeros(n, dtype=G.ROWS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
            idx = np.full(cap + 1, 0x5A, dtype=G.ROW_ENT_DTYPE)
            key, klen = np.full(cap + 1, FILL, dtype=np.uint64), np.full(cap + 1, FILL32, dtype=np.uint32)
            val, cell = np.full((P, cap + 1), FILL, dtype=np.uint64), np.full((P, cap + 1), FILL, dtype=np.uint64)
            lens, need = np.full((P, cap + 1), FILL32, dtype=np.uint32), C.c_uint64(0)
            ptr = (lambda a: None) if sizing else (lambda a: a.ctypes.data)
            rc = L.dg_rows_map_batch_host(plan.ctx.h, plan.h, s.root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                          head.ctypes.data, row_off.ctypes.data, ptr(idx), ptr(key) if keys else None,
                                          ptr(klen) if keys else None, ptr(val), ptr(cell), ptr(lens), 0 if sizing else cap + 1,
                                          C.byref(need))
            return rc, head, row_off, idx, key, klen, val, need.value

        for cap, keys, sizing in ((0, True, True), (total, True, False), (total + 5, False, False)):
            rc, head, row_off, idx, key, klen, val, need = call(cap, keys, sizing)
            assert rc == 0 and need == total
            CG.same({f: head[f] for f in RG.HEAD_FIELDS}, wa[0], "host head")
            assert (row_off == wa[1]).all()
            if sizing:
                continue
            CG.same({f: idx[f][:total] for f in RG.ROW_FIELDS}, wa[2], "host index")
            assert (val[0, :total] == wa[3][0]["val"]).all() and (val[:, total:] == FILL).all()
            if keys:
                CG.same({"key": key[:total], "key_len": klen[:total]}, wa[4], "host keys")
            assert (key[total if keys else 0:] == FILL).all() and (klen[total if keys else 0:] == FILL32).all()
        head, row_off = np.zeros(n, dtype=G.ROWS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        small = np.zeros((P, total - 1), dtype=np.uint64)
        need = C.c_uint64(0)
        rc = L.dg_rows_map_batch_host(plan.ctx.h, plan.h, s.root_type, arena.ctypes.data, in_off.ctypes.data, n, head.ctypes.data,
                                      row_off.ctypes.data, None, small.ctypes.data, small.ctypes.data, small.ctypes.data,
                                      small.ctypes.data, small.ctypes.data, total - 1, C.byref(need))
        assert rc == -3 and need.value == total and (small == 0).all()  # DG_E_NOMEM


# -------------------------------------------------------------- far offsets
FAR_VALUES = [CG.fld(R.I32, 1, b"\x80\0\0\x03") + CG.fld(R.STRING, 2, CG.wstr(b"0123456789abcdef")) + b"\x00",
              CG.fld(R.STRING, 2, CG.wstr(b"second")) + b"\x00", CG.fld(R.I32, 1, b"\0\0\0\7") + b"\x00"]
FAR_KEYS = [CG.wstr(b"a far key of 20 bytes"[:20]), CG.wstr(b""), CG.wstr(b"k")]
FAR_PIVOT = MG.map_field(R.STRING, R.STRUCT, list(zip(FAR_KEYS, FAR_VALUES))) + b"\x00"
FAR_COLUMNS = [([(F, 2)], CR.STR), ([(F, 1)], CR.INT)]


def test_far_offsets(pool):
    """inputs, key, value and STR offsets and the output arrays across 2^32: the bound lies inside the pivot's first key
    payload; d_key lies in the far output arena with the bound inside it, d_index behind it, wholly above"""
    import torch
    from dynamicgo_amd import generic as G
    B = FO.BOUNDS[1]
    inp, outa = FO.Arena(), FO.Arena()
    try:
        small = MG.geometry_batch([1, 2, 0, 3] * 5, pool, R.STRING, fails=False)
        msgs = small[:10] + [FAR_PIVOT] + small[10:]
        n, pivot = len(msgs), 10
        in_off = FO.place([len(m) for m in msgs], B, pivot, -(3 + 6 + 4 + 7))
        FO.check_layout(in_off, B, guard=0, tail=FO.TAIL)
        inp.put_input(in_off, msgs, B)
        s = MG.Set(msgs, MG.ONE, FAR_COLUMNS, R.STRUCT, MG.STR)
        want = MG.expect(s, first=int(in_off[0]))
        wa = MG.arrays(want, 2)
        a = int(in_off[pivot])
        assert want[pivot].keys[0] == MR.Key(a + 13, 20) and a + 13 < B < a + 33 and want[pivot].rows[0].off == a + 33 > B
        koffs = [k.val for m in want for k in m.keys]
        assert any(o >= B for o in koffs) and any(o < B for o in koffs)
        total = int(wa[1][n])
        k_lo = B - 8 * (total // 2)
        k_off = np.array([k_lo, B, k_lo + 8 * total], dtype=np.int64)
        i_lo = (k_lo + 8 * total + 4096 + 15) & ~15  # the index takes 16-byte stores
        i_off = np.array([i_lo, i_lo + 16 * total], dtype=np.int64)
        FO.check_layout(k_off, B, others=[(i_lo - FO.GUARD, i_lo + 16 * total + FO.GUARD)])
        outa.prefill(k_off, B)
        outa.prefill(i_off, B)
        with plan_of(s) as plan:
            d_off = torch.from_numpy(in_off).cuda()
            o = Outputs(n, 2, total)
            G.rows_device(plan, inp.base, d_off, n, o.head[GUARD:], o.row_off[GUARD:], outa.base[i_lo:], o.val[GUARD:],
                          o.cell[GUARD:], o.len[GUARD:], row_cap=total, keys=outa.base[k_lo:], key_lens=o.key_len[GUARD:])
            torch.cuda.synchronize()
            got = o.read("far", index=False, keys=False)
            keys = outa.collect(k_off, B, what="d_key").view(np.uint64)
            ents = outa.collect(i_off, B, what="d_index").view(G.ROW_ENT_DTYPE)
        MG.same((got[0], got[1], {f: ents[f] for f in RG.ROW_FIELDS}, got[3], {"key": keys, "key_len": got[4]["key_len"]}), wa, "far")
    finally:
        inp.free()
        outa.free()
        torch.cuda.empty_cache()


# -------------------------------------------------------------------- fuzz
@pytest.mark.parametrize("plan", list(MG.FUZZ_PLANS))
@pytest.mark.parametrize("corpus", ("fuzz", "mutated"))
def test_fuzz(corpus, plan):
    msgs = KG.fuzz_messages(2048)[corpus == "mutated"]
    parent, cols, kind = MG.FUZZ_PLANS[plan]
    want = check("%s %s" % (corpus, plan), MG.Set(msgs, parent, cols, R.STRUCT, kind))
    heads, cells = MG.statuses(want)
    print(corpus, plan, heads, cells, sum(len(m.rows) for m in want))
    assert (heads, cells, sum(len(m.rows) for m in want)) == MG.FUZZ_WANT[corpus, plan]


def test_fuzz_counts_cover_the_statuses():
    """from the counts alone: every status a head can have occurs, and under the two descriptor plans the messages with
    rows are the majority"""
    seen = {st for h, _, _ in MG.FUZZ_WANT.values() for st, _ in h}
    assert seen == {R.OK, R.NOT_FOUND, R.E_READ, MR.E_UNSUPPORTED}
    for plan in ("str f12", "int f15"):
        heads = dict(MG.FUZZ_WANT["fuzz", plan][0])
        assert heads[R.OK] > sum(heads.values()) / 2
