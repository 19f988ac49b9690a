"""GPU: the six thrift/generic operations against the document model of
modelgen.py and the reference's own j2t (oracle.RefOracle, the port oracle
where oracle/_ref does not exist): what test_generic_codec.py asks of the
Python restatements, asked of the kernels. No expected value comes from a
*ref.py; the launch helpers of the other GPU tests are borrowed for the uploads,
the guard bytes and the slot contract. Every operation runs through its host
entry and its device entry, on every route its routing knobs select, over two
batches per descriptor: 600 ordinary documents (the 256-lane block edge is
crossed twice) and 40 of which every other one carries strings long enough for
messages of 4 to 20 KB. Bytes, integers and bit patterns only."""
import random

import pytest

import editgen as EG
import editmgen as EMG
import modelgen as M
import oracle
import test_gpu_cols as TCO
import test_gpu_cut as TC
import test_gpu_edit as TE
import test_gpu_editm as TM
import test_gpu_kids as TK
import test_gpu_tget as TT

pytestmark = pytest.mark.gpu

OK, NOT_FOUND = 0, 1
BATCHES = {"ordinary": dict(n=600, seed=7), "long": dict(n=40, seed=8, long_p=(0.3, 0.0))}
CASES = [(name, b) for name in M.Corpus.SEEDS for b in BATCHES]
_corpora = {}


@pytest.fixture(scope="module")
def chk():
    ref = oracle.RefOracle()
    print("\ntest_gpu_generic_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return ref or oracle.PortOracle()


@pytest.fixture(params=CASES, ids=["%s-%s" % c for c in CASES])
def corpus(request, chk):
    """the batch's documents and messages, made once per module; its memo keeps every encoding asked for"""
    if request.param not in _corpora:
        name, b = request.param
        _corpora[request.param] = M.Corpus(chk, name, **BATCHES[b])
    return _corpora[request.param]


def test_the_batches(chk):
    for name, b in CASES:
        if (name, b) not in _corpora:
            _corpora[name, b] = M.Corpus(chk, name, **BATCHES[b])
        lens = [len(m) for m in _corpora[name, b].msgs]
        if b == "long":
            assert sum(n > 4096 for n in lens) >= 8 and sum(n < 1024 for n in lens) >= 8, lens
        else:
            assert len(lens) > 2 * 256 and min(lens) < 150 and max(lens) > 500, (min(lens), max(lens))


# ---------------------------------------------------------------- GetByPath
def test_get_by_path(corpus):
    from dynamicgo_amd import generic as G
    name, td, msgs = corpus.name, corpus.td, corpus.msgs
    paths = M.PATHS[name]["exist"] + M.PATHS[name]["never"] + [[]]
    assert {k for p in paths for k, _ in p} == {M.FIELD, M.INDEX, M.STRKEY, M.INTKEY, M.BINKEY}
    n_ok = 0
    for a in range(0, len(paths), 8):  # 8 to a PathSet
        chunk = paths[a:a + 8]
        want = [[M.sub(d, td, p) for p in chunk] for d in corpus.docs]
        with G.PathSet(TT.to_paths(chunk)) as ps:
            host = G.get_by_path_records(msgs, ps)
        for what, got in (("host entry", host), ("device entry", TT.run_device(msgs, chunk))):
            assert got.shape == (len(msgs), len(chunk))
            for i, row in enumerate(want):
                for k, w in enumerate(row):
                    g = got[i, k]
                    if isinstance(w, int):
                        assert (int(g["status"]), int(g["step"])) == (NOT_FOUND, w), (what, i, chunk[k], g)
                    else:
                        assert (int(g["status"]), int(g["type"]), int(g["step"])) == (OK, w[1].type, len(chunk[k])), (
                            what, i, chunk[k], g)
                        assert msgs[i][int(g["start"]):int(g["end"])] == corpus.enc(w[1], w[0]), (what, i, chunk[k])
                        n_ok += 1
    assert n_ok >= 4 * len(msgs)


# ---------------------------------------------------------------- MarshalTo
def _cut(knob, corpus, plan, want, opts=0):
    from dynamicgo_amd import generic as X
    msgs = corpus.msgs
    TC.on_both_routes(knob, plan, msgs, want, opts)
    res = X.marshal_to_batch(msgs, plan, opts=opts)
    TC.same([(r.status | (r.aux & 0xFFFFFFFF) << 32, r.raw) for r in res], want, msgs, "host entry, opts %d" % opts)


def test_marshal_to(knob, corpus):
    from dynamicgo_amd import generic as X
    rng = random.Random(M.Corpus.SEEDS[corpus.name] + 11)
    for _ in range(20):
        to = M.narrow(rng, corpus.td)
        with X.CutPlan(corpus.td, to) as plan:
            _cut(knob, corpus, plan, [(0, corpus.enc(to, d)) for d in corpus.docs])


def test_marshal_to_error_classes(knob, corpus):
    """E_REQUIRED with the field id against j2t's code 10 and value, E_UNKNOWN under DISALLOW_UNKNOWN against
    j2t without flag 0x1: the two classes that held for the restatement"""
    from dynamicgo_amd import generic as X
    rng = random.Random(M.Corpus.SEEDS[corpus.name] + 12)
    seen = {}
    for _ in range(6):
        to = M.narrow(rng, corpus.td, keep=0.5, require=0.08)
        want = [M.cut_want(corpus.chk, d, to) for d in corpus.docs]
        with X.CutPlan(corpus.td, to) as plan:
            _cut(knob, corpus, plan, want)
        frm = M.narrow(rng, corpus.td, keep=0.97)
        want2 = [M.cut_unknown_want(corpus.chk, d, frm, corpus.td) for d in corpus.docs]
        with X.CutPlan(frm, M.narrow(rng, frm, keep=1.0)) as plan:
            _cut(knob, corpus, plan, want2, M.CUT_DISALLOW_UNKNOWN)
        for r, _ in want + want2:
            seen[r & 0xFF] = seen.get(r & 0xFF, 0) + 1
    assert min(seen.get(c, 0) for c in (0, M.CUT_E_REQUIRED, M.CUT_E_UNKNOWN)) >= 10, seen


# ------------------------------------------- SetByPath / UnsetByPath, SetMany
_WORD = {"replaced": 0x100, "inserted": 0, "deleted": 0x100, "untouched": 0, "notfound": NOT_FOUND}  # status | EXISTED


def _low(res, bits):
    return [(r & bits, out) for r, out in res]


def test_edit(knob, corpus):
    from dynamicgo_amd import generic as X
    td, msgs = corpus.td, corpus.msgs
    for form, op, path in M.EDITS[corpus.name]:
        vtd = M.desc_at(td, path)
        vals = corpus.values(form, vtd) if op == M.SET_OP else [None] * len(msgs)
        raw = [corpus.enc(vtd, v) for v in vals] if op == M.SET_OP else b""
        want = []
        for d, v in zip(corpus.docs, vals):
            cls, new = M.edit(d, td, op, path, v)
            want.append((_WORD[cls], corpus.enc(td, new) if new is not None else b""))
        case = EG.Case(op, path, msgs, vtd.type if op == M.SET_OP else 0, raw, what=form)
        with TE.plan_of(case) as plan:
            for route, wm, lanes in TE.ROUTES:
                knob("edit_wave_min", wm)
                knob("edit_lanes", lanes)
                TE.same(_low(TE.run_device(case, plan), 0x1FF), want, case, route + " route")
            res = X.set_by_path_batch(msgs, plan, raw, vtd.type) if op == M.SET_OP else X.unset_by_path_batch(msgs, plan)
        TE.same([(r.status | r.existed << 8, r.raw) for r in res], want, case, "host entry")


def test_edit_many(knob, corpus):
    from dynamicgo_amd import generic as X
    td, msgs = corpus.td, corpus.msgs
    assert {len(s) for _, _, _, s in M.MANY[corpus.name]} >= {2, 3, 7}
    for form, op, parent, steps in M.MANY[corpus.name]:
        ptd = M.desc_at(td, parent)
        vtds = [M.desc_at(ptd, [s]) for s in steps]
        vals = [corpus.values("%s/%d" % (form, j), d) for j, d in enumerate(vtds)]
        want = []
        for i, d in enumerate(corpus.docs):
            cls, mask, item, new = M.many(d, td, op, parent, [(s, vals[j][i]) for j, s in enumerate(steps)])
            st = NOT_FOUND if cls == "notfound" else OK
            want.append((st | mask << 8 | item << 16, corpus.enc(td, new) if new is not None else b""))
        if op == M.SET_OP:
            items = [(s, [corpus.enc(vtds[j], v) for v in vals[j]], vtds[j].type) for j, s in enumerate(steps)]
        else:
            items = [(s,) for s in steps]
        case = EMG.ManyCase(op, parent, items, msgs, what=form)
        b = TM.Batch(case)
        with TM.plan_of(case) as plan:
            for route, wm, lanes in TM.ROUTES:
                knob("edit_wave_min", wm)
                knob("edit_lanes", lanes)
                TM.same(_low(b.run(plan), 0x7FFFF), want, case, route + " route")
            if op == M.SET_OP:
                res = X.set_many_batch(msgs, plan, [(None, v, t) for _, v, t in items])
            else:
                res = X.unset_many_batch(msgs, plan)
        got = [(r.status | sum(e << 8 + j for j, e in enumerate(r.existed)) | r.item << 16, r.raw) for r in res]
        TM.same(got, want, case, "host entry")


# ------------------------------------------------------------------ Children
def _same_kids(corpus, got, want, what):
    head, rec_off, recs = got
    msgs = corpus.msgs
    assert len(head) == len(msgs) and int(rec_off[0]) == 0
    at = 0
    for i, (w, t) in enumerate(zip(want, msgs)):
        h = head[i]
        assert int(rec_off[i]) == at, (what, i)
        if isinstance(w, int):
            assert (int(h["status"]), int(h["direct"]), int(h["count"])) == (NOT_FOUND, w, 0), (what, i, h)
            continue
        (typ, kt, et, direct), kids = w
        assert (int(h["status"]), int(h["type"]), int(h["key_type"]), int(h["elem_type"]), int(h["direct"]),
                int(h["count"])) == (OK, typ, kt, et, direct, len(kids)), (what, i, h)
        for g, k in zip(recs[at:at + len(kids)], kids):
            assert (int(g["kind"]), int(g["key"]), int(g["type"]), int(g["depth"]), int(g["parent"]), int(g["n_desc"])) == (
                k.kind, k.key, k.type, k.depth, k.parent, k.n_desc), (what, i, g)
            assert t[int(g["start"]):int(g["end"])] == corpus.enc(k.td, k.value), (what, i, g)
            if k.kind == M.STRKEY:
                assert t[int(g["key_start"]) + 4:int(g["key_start"]) + 4 + k.key] == k.key_bytes, (what, i, g)
        at += len(kids)
    assert int(rec_off[len(msgs)]) == at == len(recs), what


@pytest.mark.parametrize("recurse", (False, True), ids=("one-level", "recursive"))
def test_children(knob, corpus, recurse):
    from dynamicgo_amd import generic as G
    for path in M.KID_PATHS[corpus.name]:
        want = [M.children(d, corpus.td, path, recurse) for d in corpus.docs]
        _same_kids(corpus, G.children_records(corpus.msgs, TT.to_paths([path])[0], recurse), want, "host entry")
        dev = TK.Dev(corpus.msgs, path)
        try:
            for wide in (1, 0):
                knob("kids_wide_min", wide)
                _same_kids(corpus, dev.run(recurse), want, "device entry, kids_wide_min %d" % wide)
        finally:
            dev.close()


# ------------------------------------------------------------------- Columns
def _same_cols(corpus, columns, got, what):
    arena = b"".join(corpus.msgs)
    for k, (path, kind) in enumerate(columns):
        g = got[k]
        at = 0
        for i, d in enumerate(corpus.docs):
            w = M.column(d, corpus.td, path, kind)
            where = (what, k, i)
            if kind & 16:
                assert int(g["off"][i]) == at, where
            if w[0] == "notfound":
                assert (int(g["status"][i]), int(g["step"][i])) == (NOT_FOUND, w[1]), where
                continue
            _, val, ln, elems, text = w
            assert int(g["status"][i]) == OK, where
            if text is not None:
                v = int(g["val"][i])
                assert (int(g["len"][i]), arena[v:v + ln]) == (ln, text), where
            elif elems is not None:
                assert int(g["len"][i]) == ln and g["elems"][at:at + ln].tolist() == elems, where
                at += ln
            else:
                assert int(g["val"][i]) == val, where
        if kind & 16:
            assert int(g["off"][len(corpus.docs)]) == at == len(g["elems"]), (what, k)


def test_columns(knob, corpus):
    for columns in (M.COLUMNS[corpus.name], M.COLUMNS_2[corpus.name]):
        _same_cols(corpus, columns, TCO.run_host(corpus.msgs, columns), "host entry")
        for full in (1, 0):
            knob("cols_full_search", full)
            _same_cols(corpus, columns, TCO.run_device(corpus.msgs, columns), "device entry, cols_full_search %d" % full)
    if corpus.name == "all":
        assert {k for _, k in M.COLUMNS["all"]} == set(M.COL_KINDS)  # all eight kinds in one plan
