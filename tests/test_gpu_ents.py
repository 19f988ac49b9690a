"""GPU: entry columns (dynamicgo_amd.generic over dg_ents_*) against the checker
of entsref.py: tgetref's GetByPath followed by Node.List of strings, Node.StrMap
and Node.IntMap of cast.go. Every case goes through the host entry and the
device entries, and every field of every cell, every offset, key, value and
length is compared with the checker's. The inputs are entsgen's, which
test_ents_host.py runs through the host build of the same decode."""
import random

import numpy as np
import pytest

import entsgen as EG
import entsref as ER
import faroff as FO
import t2jgen
import tgetref as R
from test_gpu_tget import expect as tget_expect, same as tget_same, to_paths

pytestmark = pytest.mark.gpu

GUARD = 64  # entries of fill on each side of every output
FILL = 0x5A5A5A5A5A5A5A5A
FILL32 = 0x5A5A5A5A
STAGES = (0, 4, 8, 16)  # knob ents_stage: every lane stores its entries, or R of them staged a round
ENTRY_ARRAYS = (("keys", 8), ("klens", 4), ("vals", 8), ("vlens", 4))


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


def filled(count, width):
    """count + 2 GUARD entries of `width` bytes, all fill"""
    import torch
    if width == 8:
        return torch.full((count + 2 * GUARD,), FILL, dtype=torch.int64, device="cuda")
    return torch.full((count + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda")


def unguard(t, count, what):
    """the `count` entries between the guards, which must be intact"""
    h = t.cpu().numpy()
    h = h.view(np.uint64) if h.dtype == np.int64 else h.view(np.uint32)
    fill = FILL if h.dtype == np.uint64 else FILL32
    assert (h[:GUARD] == fill).all() and (h[GUARD + count:] == fill).all(), "a store outside %s" % what
    return h[GUARD:GUARD + count]


class Outputs:
    """d_val / d_cell / d_len / d_span of one launch between GUARD entries of fill"""

    def __init__(self, n, P):
        self.n, self.P = n, P
        self.t = [filled(n * P, w) for w in (8, 8, 4, 4)]

    def args(self):
        return [t[GUARD:] for t in self.t]

    def column(self, k):
        a = GUARD + k * self.n
        return [t[a:a + self.n] for t in self.t]

    def read(self, what):
        """[column k as a dict of arrays]; the guards must be intact"""
        from dynamicgo_amd import generic as G
        q = self.n * self.P
        hv, hc, hl, hs = (unguard(t, q, "%s: %s" % (what, nm)) for t, nm in zip(self.t, ("d_val", "d_cell", "d_len", "d_span")))
        cells = hc.view(G.COL_CELL_DTYPE)
        out = []
        for k in range(self.P):
            s = slice(k * self.n, (k + 1) * self.n)
            out.append({"status": cells["status"][s], "type": cells["type"][s], "step": cells["step"][s],
                        "aux": cells["aux"][s], "val": hv[s], "len": hl[s], "span": hs[s]})
        return out


def emit_column(plan, k, arena, o, what, stream=None, cap=None):
    """the sizing call and the emit of column k of `o`: (off, {array: entries}); an array the kind does not write
    must come back untouched. cap: ent_cap instead of the need (nothing at or behind it is stored)."""
    import torch
    from dynamicgo_amd import generic as G
    n = o.n
    col = o.column(k)
    off = torch.full((n + 1 + GUARD,), FILL, dtype=torch.int64, device="cuda")
    G.entry_emit_device(plan, k, arena, n, *col, off, stream=stream)  # sizing
    torch.cuda.synchronize()
    h_off = off.cpu().numpy().view(np.uint64)
    total = int(h_off[n])
    assert (h_off[n + 1:] == FILL).all(), "%s: a store behind d_ent_off" % what
    outs = {f: filled(total, w) for f, w in ENTRY_ARRAYS}
    G.entry_emit_device(plan, k, arena, n, *col, off, *(outs[f][GUARD:] for f, _ in ENTRY_ARRAYS),
                        ent_cap=total if cap is None else cap, stream=stream)
    torch.cuda.synchronize()
    assert (off.cpu().numpy().view(np.uint64)[:n + 1] == h_off[:n + 1]).all()
    got = {f: unguard(outs[f], total, "%s: column %d's %s" % (what, k, f)) for f, _ in ENTRY_ARRAYS}
    for f, w in ENTRY_ARRAYS:
        if f not in EG.written(plan.kinds[k]):
            assert (got[f] == (FILL if w == 8 else FILL32)).all(), "%s: column %d stored %s" % (what, k, f)
    return h_off[:n + 1], got


def emit_all(plan, arena, o, got, what, stream=None):
    for k in range(plan.count):
        got[k]["off"], ents = emit_column(plan, k, arena, o, what, stream)
        got[k].update({f: ents[f] for f in EG.written(plan.kinds[k])})


def run_device(msgs, columns, root_type=R.STRUCT):
    import torch
    from dynamicgo_amd import generic as G
    n = len(msgs)
    with G.EntryPlan(to_cols(columns)) as plan:
        arena, d_off, _ = upload(msgs)
        o = Outputs(n, plan.count)
        G.entries_device(plan, arena, d_off, n, *o.args(), root_type=root_type, max_len=max(map(len, msgs), default=0))
        torch.cuda.synchronize()
        got = o.read("device entry")
        if n:
            emit_all(plan, arena, o, got, "device entry")
        return got


def run_host(msgs, columns, root_type=R.STRUCT):
    from dynamicgo_amd import generic as G
    with G.EntryPlan(to_cols(columns)) as plan:
        val, cell, lens, ent_off, keys, klens, vals, vlens, _ = G.entries_records(msgs, plan, root_type)
        got = []
        for k in range(plan.count):
            eo = ent_off[k]
            a, b = int(eo[0]), int(eo[-1])
            g = {"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"], "aux": cell[k]["aux"],
                 "val": val[k], "len": lens[k], "off": eo - eo[0]}
            ents = {"keys": keys[a:b], "klens": klens[a:b], "vals": vals[a:b], "vlens": vlens[a:b]}
            for f in ents:  # what the kind does not write is zero
                if f in EG.written(plan.kinds[k]):
                    g[f] = ents[f]
                else:
                    assert not ents[f].any(), (k, f)
            got.append(g)
        assert int(ent_off[0][0]) == 0 and int(ent_off[-1][-1]) == len(vals)
        return got


def compare(got, want, what):
    for k, col in enumerate(want):
        EG.same(got[k], EG.arrays(col) if isinstance(col, list) else col, "%s, column %d" % (what, k))


def check(msgs, columns, root_type=R.STRUCT, want=None):
    want = want or EG.expect(msgs, columns, root_type)
    compare(run_host(msgs, columns, root_type), want, "host entry")
    compare(run_device(msgs, columns, root_type), want, "device entry")
    return want


# ------------------------------------------------------------------- cases
def test_kind_by_type_matrix():
    from test_ents_host import matrix_properties
    msgs = EG.matrix_messages()
    sets = [check(msgs, cols) for cols in EG.MATRIX_SETS]
    matrix_properties(sets)
    # the public columns: names of the errors, Python ints, floats, bools and bytes in wire order
    from dynamicgo_amd import generic as G
    kinds = ("list[str]", "strmap[int]", "intmap[str]", "intmap[float64]", "intmap[bool]", "strmap[str]")
    by = dict(zip(ER.KINDS, sets[0] + sets[1][:1]))
    want = [by[G.ent_kind(k)] for k in kinds]
    cols = G.entries_batch(msgs, [(to_paths([EG.ONE])[0], k) for k in kinds])
    names = {R.OK: None, R.NOT_FOUND: "ErrNotFound", R.E_READ: "ErrRead", R.E_TYPE: "ErrDismatchType",
             ER.E_UNSUPPORTED: "ErrUnsupportedType"}
    base = np.cumsum([0] + [len(m) for m in msgs]).tolist()
    for c, w, kind in zip(cols, want, kinds):
        assert [c.error(i) for i in range(len(msgs))] == [names[x.status] for x in w]
        assert c.valid.tolist() == [x.status == R.OK for x in w]
        assert c.offsets.tolist() == EG.arrays(w)["off"].tolist()
        for i, x in enumerate(w):
            if x.status != R.OK:
                assert c.values[i] == [] and (c.keys is None or c.keys[i] == [])
                continue
            m, b = msgs[i], base[i]
            if kind in ("list[str]", "intmap[str]", "strmap[str]"):
                assert c.values[i] == [m[o - b:o - b + ln] for o, ln in zip(x.vals, x.vlens)]
            elif kind == "intmap[float64]":
                assert np.array(c.values[i], dtype=np.float64).view(np.uint64).tolist() == x.vals
            elif kind == "intmap[bool]":
                assert c.values[i] == [bool(v) for v in x.vals]
            else:
                assert [v & (2 ** 64 - 1) for v in c.values[i]] == x.vals
            if kind == "list[str]":
                assert c.keys is None and c.items(i) == c.values[i]
            elif kind.startswith("strmap"):
                assert c.keys[i] == [m[o - b:o - b + ln] for o, ln in zip(x.keys, x.klens)]
                assert c.items(i) == list(zip(c.keys[i], c.values[i]))
            else:
                assert [v & (2 ** 64 - 1) for v in c.keys[i]] == x.keys
    assert any(ks == [b"a", b"b", b"a"] for ks in cols[1].keys)  # the duplicate key stays, in wire order
    assert any(ks == [0x00, 0x7F, 0x80, 0xFF] for ks in cols[4].keys)  # I08 keys are unsigned
    with pytest.raises(ValueError):
        G.ent_kind("list[int]")
    with pytest.raises(ValueError):
        G.ent_kind("strmap[byte]")


@pytest.mark.parametrize("target", list(EG.TARGETS))
def test_alignment_and_the_arenas_end(target):
    """the target at every residue mod 16, the last one the last bytes before the 16 spare bytes"""
    msgs = EG.align_batch(target)
    want = check(msgs, EG.ALIGN_COLUMNS) + check(msgs, EG.ALIGN_COLUMNS_B)
    assert sum(c.status == R.OK for col in want for c in col) >= 16
    assert len({R.get_by_path(m, [(R.FIELD, 2)]).start % 16 for m in msgs}) == 16


def test_geometry_and_guards():
    import torch
    from dynamicgo_amd import generic as G
    all_msgs = EG.geometry_messages(257)
    want_all = EG.expect(all_msgs, EG.GEOMETRY_COLUMNS)
    assert EG.by_status(want_all)[R.OK] > 0.6 * 257 * 8
    for P in range(1, 9):
        cols = EG.GEOMETRY_COLUMNS[:P]
        with G.EntryPlan(to_cols(cols)) as plan:
            o = Outputs(0, P)  # n = 0: nothing is launched, nothing stored
            G.entries_device(plan, None, None, 0, *o.args())
            torch.cuda.synchronize()
            o.read("n = 0")
            for n in (1, 63, 64, 65, 255, 256, 257):
                msgs = all_msgs[:n]
                want = [EG.arrays(col[:n]) for col in want_all[:P]]
                what = "P = %d, n = %d" % (P, n)
                arena, d_off, _ = upload(msgs)
                o = Outputs(n, P)
                G.entries_device(plan, arena, d_off, n, *o.args())
                torch.cuda.synchronize()
                got = o.read(what)
                emit_all(plan, arena, o, got, what)
                compare(got, want, what)
                if n not in (1, 65, 257):
                    continue
                # message j changed (its first field header becomes the STOP byte): its cells and slots change, no other
                j = n // 2
                changed = msgs[:j] + [b"\x00" + msgs[j][1:]] + msgs[j + 1:]
                arena2, _, _ = upload(changed)
                o2 = Outputs(n, P)
                G.entries_device(plan, arena2, d_off, n, *o2.args())
                torch.cuda.synchronize()
                got2 = o2.read(what + ", changed")
                emit_all(plan, arena2, o2, got2, what + ", changed")
                for k in range(P):
                    assert got2[k]["status"][j] == R.NOT_FOUND and got2[k]["len"][j] == 0, what
                    keep = np.arange(n) != j
                    for f in EG.CELL_FIELDS:
                        assert (got2[k][f][keep] == got[k][f][keep]).all(), (what, k, f)
                    a, b = int(got[k]["off"][j]), int(got[k]["off"][j + 1])
                    assert (np.diff(got2[k]["off"].astype(np.int64))[keep] == np.diff(got[k]["off"].astype(np.int64))[keep]).all()
                    for f in EG.written(plan.kinds[k]):
                        assert (got2[k][f] == np.concatenate([got[k][f][:a], got[k][f][b:]])).all(), (what, k, f)
    assert G.entries_batch([], to_cols(EG.GEOMETRY_COLUMNS))[2].values == []
    compare(run_host(all_msgs, EG.GEOMETRY_COLUMNS), want_all, "host entry")


def test_counts_and_ent_cap():
    import torch
    from dynamicgo_amd import generic as G
    msgs = EG.count_messages()
    want = check(msgs, EG.COUNT_COLUMNS)
    for col, (_, kind) in zip(want, EG.COUNT_COLUMNS):
        fixed = kind & ER.INTMAP and kind & 15 != ER.STR
        assert {c.len for c in col if c.status == R.OK} >= set(EG.FIXED_COUNTS if fixed else EG.VAR_COUNTS), kind
        for st in (R.NOT_FOUND, ER.E_UNSUPPORTED):
            assert any(c.status == st for c in col), (kind, st)
    # ent_cap below the need: nothing at or behind slot ent_cap of any array; what is in front of it is right
    n = len(msgs)
    with G.EntryPlan(to_cols(EG.COUNT_COLUMNS)) as plan:
        arena, d_off, _ = upload(msgs)
        o = Outputs(n, plan.count)
        G.entries_device(plan, arena, d_off, n, *o.args())
        for k in (1, 3, 4):  # a string-keyed, an int-keyed variable and a fixed-stride column
            w = EG.arrays(want[k])
            total = int(w["off"][n])
            assert total > 257
            for cap in (total - 1, 257, 1, 0):
                off, got = emit_column(plan, k, arena, o, "cap %d" % cap, cap=cap)
                assert off.tolist() == w["off"].tolist()  # [n] is still the need
                for f, wd in ENTRY_ARRAYS:
                    if f in EG.written(plan.kinds[k]):
                        assert (got[f][cap:] == (FILL if wd == 8 else FILL32)).all(), "cap %d: a store at or behind %s[ent_cap]" % (cap, f)
                        assert (got[f][:cap] == w[f][:cap]).all(), (cap, f)
        with pytest.raises(Exception, match="column 8 of a plan of 8"):
            G.entry_emit_device(plan, 8, arena, n, *o.column(0), torch.zeros(n + 1, dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()


@pytest.mark.parametrize("stage", STAGES)
def test_both_shapes_of_the_variable_stride_emit(knob, stage):
    """every lane storing its own entries (0) and R entries staged in LDS a round (4, 8, 16): counts of R - 1, R,
    R + 1 and 2 R + 1 with unequal neighbours in a wave, and the counts around the wave and the block"""
    knob("ents_stage", stage)
    msgs, counts = EG.stage_messages()
    want = EG.expect(msgs, EG.STAGE_COLUMNS)
    assert {c.len for c in want[0]} == set(counts) >= {3, 4, 5, 9, 7, 8, 17, 15, 16, 33}
    compare(run_device(msgs, EG.STAGE_COLUMNS), want, "ents_stage %d" % stage)
    msgs = EG.count_messages()
    cols = EG.COUNT_COLUMNS[:4]
    compare(run_device(msgs, cols), EG.expect(msgs, cols), "ents_stage %d, counts" % stage)


def test_deep_pass():
    msgs = EG.deep_messages()
    want = check(msgs, EG.DEEP_COLUMNS)
    depth = [d for d in EG.DEEP_DEPTHS for _ in range(3)]
    assert any(d + 1 > EG.LDS_FRAMES for d in depth) and any(d + 1 <= EG.LDS_FRAMES for d in depth)
    assert all(c.status == R.OK and c.len == 2 for c in want[0])
    for col, d in zip(want[1:], EG.DEEP_DEPTHS):
        assert [c.status == R.OK and c.vlens == [2, 0, 4] for c in col] == [md == d for md in depth]


def test_three_components_on_three_streams():
    """entries_device, columns_device and get_by_path_device on a stream each, in turn for 4 rounds with no
    synchronisation, over messages that send all three to their deep passes: each has a deep queue, counters and
    frames of its own"""
    import torch
    import colsgen as CG
    import colsref as CR
    from dynamicgo_amd import generic as G
    msgs = EG.deep_messages(per_depth=40)
    n = len(msgs)
    ccols = [([(R.FIELD, 2)], CR.LEN), ([(R.FIELD, 1)], CR.LEN)]
    paths = [[(R.FIELD, 2)], [(R.FIELD, 1), (R.INDEX, 0)]]
    want, cwant, gwant = EG.expect(msgs, EG.DEEP_COLUMNS), CG.expect(msgs, ccols), tget_expect(msgs, paths)
    s_ent, s_col, s_get = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    arena, d_off, _ = upload(msgs)
    with G.EntryPlan(to_cols(EG.DEEP_COLUMNS)) as plan, G.ColumnPlan(to_cols(ccols)) as cplan, G.PathSet(to_paths(paths)) as ps:
        outs = [Outputs(n, plan.count) for _ in range(4)]
        couts = [[torch.full((n * 2,), FILL, dtype=torch.int64, device="cuda") for _ in range(2)] +
                 [torch.full((n * 2,), FILL32, dtype=torch.int32, device="cuda")] for _ in range(4)]
        recs = [torch.full((n, ps.count, 4), FILL32, dtype=torch.int32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for r in range(4):
            G.entries_device(plan, arena, d_off, n, *outs[r].args(), stream=s_ent)
            G.columns_device(cplan, arena, d_off, n, *couts[r], stream=s_col)
            G.get_by_path_device(ps, arena, d_off, n, recs[r], stream=s_get)
        torch.cuda.synchronize()
        for r in range(4):
            compare(outs[r].read("round %d" % r), [{f: a for f, a in EG.arrays(col).items() if f in EG.CELL_FIELDS}
                                                   for col in want], "round %d, entries" % r)
            cells = couts[r][1].cpu().numpy().view(G.COL_CELL_DTYPE)
            for k in range(2):
                assert cells["status"][k * n:(k + 1) * n].tolist() == [c.status for c in cwant[k]]
                assert couts[r][0].cpu().numpy()[k * n:(k + 1) * n].tolist() == [c.val for c in cwant[k]]
            tget_same(recs[r].cpu().numpy().view(G.REC_DTYPE).reshape(n, ps.count), gwant, "round %d, GetByPath" % r)


# -------------------------------------------------------------- far offsets
FAR_COLUMNS = [([(R.FIELD, 5)], ER.STRMAP | ER.STR), ([(R.FIELD, 3)], ER.INTMAP | ER.F64), ([(R.FIELD, 1)], ER.LISTSTR)]
FAR_PIVOT = EG.fld(R.LIST, 1, EG.lst(R.STRING, 2, EG.wstr(b"first") + EG.wstr(b"second"))) + \
    EG.fld(R.MAP, 5, EG.mp(R.STRING, R.STRING, 2, EG.wstr(b"0123456789abcdef") + EG.wstr(b"value") + EG.wstr(b"k") + EG.wstr(b"v"))) + \
    EG.fld(R.MAP, 3, EG.mp(R.I32, R.DOUBLE, 3, EG.entries(R.I32, R.DOUBLE, 3))) + b"\x00"
# where B falls in the pivot: in its first field header (the message straddles), in the first key's payload (which
# starts at byte 40), in the fixed-stride map's first entry (which starts at byte 84)
FAR_DELTAS = {"message": -1, "key payload": -(40 + 5), "first entry": -(84 + 3)}


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
    """the arena, the string offsets in d_key / d_val and the slots d_ent_off points at on both sides of 2^31 and 2^32"""
    import torch
    from dynamicgo_amd import generic as G
    inp, outa = far_arenas
    rng = random.Random(51)
    small = [EG.geometry_message(rng) for _ in range(40)]
    msgs = small[:20] + [FAR_PIVOT] + small[20:]
    n, pivot = len(msgs), 20
    in_off = FO.place([len(m) for m in msgs], B, pivot, FAR_DELTAS[where])
    FO.check_layout(in_off, B, guard=0, tail=FO.TAIL)
    a = int(in_off[pivot])
    assert {"message": a < B < a + 3, "key payload": a + 40 < B < a + 56, "first entry": a + 84 < B < a + 96}[where]
    inp.put_input(in_off, msgs, B)
    want = EG.expect(msgs, FAR_COLUMNS, first=int(in_off[0]))
    assert want[0][pivot].keys[0] == a + 40 and want[1][pivot].val == a + 84 and want[1][pivot].len == 3
    assert want[0][pivot].klens == [16, 1] and want[2][pivot].vlens == [5, 6]
    assert any(c.val >= B for c in want[2] if c.status == R.OK) and any(c.val < B for c in want[2] if c.status == R.OK)
    with G.EntryPlan(to_cols(FAR_COLUMNS)) as plan:
        d_off = torch.from_numpy(in_off).cuda()
        o = Outputs(n, plan.count)
        G.entries_device(plan, inp.base, d_off, n, *o.args())
        torch.cuda.synchronize()
        got = o.read("far input")
        for k in range(plan.count):
            w = EG.arrays(want[k])
            total = int(w["off"][n])
            assert total > 8
            # the four arrays one behind the other in the far output arena, slot 1 of the first exactly at B
            fs = EG.written(plan.kinds[k])
            widths = dict(ENTRY_ARRAYS)
            lo, at, wins = B - widths[fs[0]], {}, []
            for f in fs:
                at[f] = np.array([lo, lo + total * widths[f]], dtype=np.int64)
                wins.append(at[f])
                lo += total * widths[f] + 4 * FO.GUARD
                lo += -lo % 8
            FO.check_layout(np.array([at[fs[0]][0], B, at[fs[0]][1]], dtype=np.int64), B,
                            others=[(int(x[0]) - FO.GUARD, int(x[1]) + FO.GUARD) for x in wins[1:]])
            for x in wins:
                outa.prefill(x, B)
            off = torch.full((n + 1,), FILL, dtype=torch.int64, device="cuda")
            ptr = {f: outa.base[int(at[f][0]):] if f in at else None for f, _ in ENTRY_ARRAYS}
            G.entry_emit_device(plan, k, inp.base, n, *o.column(k), off, ptr["keys"], ptr["klens"], ptr["vals"], ptr["vlens"],
                                ent_cap=total)
            torch.cuda.synchronize()
            got[k]["off"] = off.cpu().numpy().view(np.uint64)
            for f in fs:
                raw = outa.collect(at[f], B, what="column %d's %s" % (k, f))
                got[k][f] = raw.view(np.uint64 if widths[f] == 8 else np.uint32)
    compare(got, want, "input at %#x, %s" % (B, where))


# --------------------------------------------------------------------- fuzz
def test_fuzz():
    """the mutated fuzz corpus under two column sets: the per-status counts are the checker's, and every status
    occurs under each set (test_ents_host.py judges the seeds on the CPU)"""
    msgs = EG.fuzz_corpus()
    for cols in (EG.FUZZ_A, EG.FUZZ_B):
        want = check(msgs, cols)
        counts = EG.by_status(want)
        print("statuses:", counts)
        for got in (run_host(msgs, cols), run_device(msgs, cols)):
            assert [int(sum((g["status"] == st).sum() for g in got)) for st in range(5)] == counts
        assert counts[R.OK] and counts[R.NOT_FOUND] and counts[R.E_READ] and counts[ER.E_UNSUPPORTED], counts
    f19 = EG.expect(msgs, EG.FUZZ_A[:2])
    assert sum(c.status == R.OK and c.len > 0 for c in f19[0]) > 50 and sum(c.status == R.OK and c.len > 0 for c in f19[1]) > 50


# ------------------------------------------------- the entries' own contracts
def test_plan_create_rejects():
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()
    blob = G.compile_paths(to_paths([[(R.FIELD, 1)], [(R.FIELD, 2)]]))

    def create(blob, kinds):
        h = C.c_void_p()
        rc = L.dg_ents_create(ctx.h, bytes(blob), len(blob), bytes(kinds), len(kinds), C.byref(h))
        if rc == 0:
            assert L.dg_ents_count(h) == len(kinds)
            L.dg_ents_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    for kind in ER.KINDS:
        assert create(blob, [ER.LISTSTR, kind])[0] == 0, kind
    bad = [0, 5, 0x10, 0x20, 0x40, 0x60 | ER.INT, ER.STRMAP | 2, ER.INTMAP | 6, 0x10 | ER.INT, 0x80 | ER.STRMAP | ER.INT]
    for kind in bad:
        rc, err = create(blob, [ER.LISTSTR, kind])
        assert rc == -6 and "column 1: unknown entry kind %d" % kind in err, (kind, rc, err)  # DG_E_ARG
    rc, err = create(blob, [ER.LISTSTR])
    assert rc == -6 and "1 kinds for 2 paths" in err
    rc, err = create(blob[:16], [ER.LISTSTR, ER.LISTSTR])
    assert rc == -6 and "no header" in err
    with pytest.raises(ValueError):
        G.EntryPlan([([G.PathFieldId(1)], "int")])


def test_host_entry_sizing_and_an_arena_not_at_zero():
    """dg_ents_batch_host as C callers see it: in_off[0] = 37 (values, string keys and string values are offsets
    from `thrift`), three columns whose entries follow one another, the arrays NULL and cap 0 for the need,
    DG_E_NOMEM below it, an array left NULL"""
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    cols = [EG.COUNT_COLUMNS[1], EG.COUNT_COLUMNS[4], EG.COUNT_COLUMNS[0]]
    msgs = EG.count_messages()
    first, n = 37, len(msgs)
    want = EG.expect(msgs, cols, first=first)
    arena = np.frombuffer(b"\xEE" * first + b"".join(msgs), dtype=np.uint8).copy()  # no spare bytes behind it
    in_off = np.full(n + 1, first, dtype=np.uint64)
    in_off[1:] += np.cumsum([len(m) for m in msgs]).astype(np.uint64)
    wa = [EG.arrays(col) for col in want]
    need_want = sum(len(w["vals"]) for w in wa)
    assert len(wa[1]["vals"]) > 4097
    L = _lib.lib()
    with G.EntryPlan(to_cols(cols)) as plan:
        def call(cap, with_klens=True):
            val, cell = np.zeros((3, n), dtype=np.uint64), np.zeros((3, n), dtype=G.COL_CELL_DTYPE)
            lens, eo = np.zeros((3, n), dtype=np.uint32), np.zeros((3, n + 1), dtype=np.uint64)
            outs = [np.full(cap + 8, FILL, dtype=np.uint64), np.full(cap + 8, FILL32, dtype=np.uint32),
                    np.full(cap + 8, FILL, dtype=np.uint64), np.full(cap + 8, FILL32, dtype=np.uint32)]
            need = C.c_uint64(0)
            ptrs = [x.ctypes.data if cap else None for x in outs]
            if not with_klens:
                ptrs[1] = None
            rc = L.dg_ents_batch_host(plan.ctx.h, plan.h, R.STRUCT, arena.ctypes.data, in_off.ctypes.data, n,
                                      val.ctypes.data, cell.ctypes.data, lens.ctypes.data, eo.ctypes.data, *ptrs, cap,
                                      C.byref(need))
            return rc, val, cell, lens, eo, outs, need.value

        for cap in (0, need_want - 1, need_want):
            rc, val, cell, lens, eo, outs, need = call(cap)
            assert rc == (0 if cap in (0, need_want) else -3) and need == need_want, (cap, rc, need)  # -3: DG_E_NOMEM
            base = 0
            for k in range(3):  # the cells and the offsets are filled at every cap
                EG.same({"status": cell[k]["status"], "type": cell[k]["type"], "step": cell[k]["step"],
                         "aux": cell[k]["aux"], "val": val[k], "len": lens[k]},
                        {f: wa[k][f] for f in EG.CELL_FIELDS if f != "span"}, "cap %d, column %d" % (cap, k))
                assert (eo[k] == wa[k]["off"] + base).all()
                base += int(wa[k]["off"][-1])
            for x in outs:
                assert (x[cap:] == (FILL if x.dtype == np.uint64 else FILL32)).all()
        zeros = [np.zeros(len(w["vals"]), dtype=np.uint64) for w in wa]
        for x, f, blank in zip(outs, EG.ENTRY_FIELDS, ((2,), (1, 2), (), (0, 1))):
            assert (x[:need_want] == np.concatenate([zeros[k] if k in blank else wa[k][f] for k in range(3)])).all(), f
        rc, _, _, _, _, outs, _ = call(need_want, with_klens=False)
        assert rc == 0 and (outs[1] == FILL32).all() and (outs[0][:len(wa[0]["keys"])] == wa[0]["keys"]).all()


def test_field_names_resolve_through_the_descriptor():
    from dynamicgo_amd import generic as G
    td = t2jgen.all_types_desc()
    name = next(nm for nm, f in td.struct.names.items() if f.id == 20)
    rng = random.Random(1234)
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(200)]
    by_name = G.entries_batch(msgs, [([G.PathFieldName(name)], "strmap[int]")], desc=td)[0]
    want = ER.column(msgs, [(R.FIELD, 20)], ER.STRMAP | ER.INT)
    assert [[v & (2 ** 64 - 1) for v in vs] for vs in by_name.values] == [c.vals or [] for c in want]
    assert sum(len(vs) for vs in by_name.values) > 100
