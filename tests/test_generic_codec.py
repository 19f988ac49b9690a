"""The six thrift/generic restatements (tgetref, cutref, editref, editmref,
kidsref, colsref) against a second yardstick that shares nothing with them: the
document model of modelgen.py and the reference's own j2t (oracle.RefOracle,
the port oracle where oracle/_ref was not built). Every operation on
T = j2t(doc, D) must give what the same operation on the document gives once it
is encoded again. Bytes, integers and bit patterns only; no tolerance.

No GPU: the kernels get the same expectations in test_gpu_generic_codec.py."""
import random

import pytest

import colsref as C
import cutref as CR
import editmref as EM
import editref as E
import kidsref as K
import modelgen as M
import oracle
import tgetref as R

N_DOCS = 300
SEEDS = M.Corpus.SEEDS
NAMES = list(SEEDS)


@pytest.fixture(scope="module")
def chk():
    ref = oracle.RefOracle()
    print("\ntest_generic_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return ref or oracle.PortOracle()


_corpora = {}


def corpus_of(chk, name):
    if name not in _corpora:
        _corpora[name] = M.Corpus(chk, name, N_DOCS)
    return _corpora[name]


@pytest.fixture(params=NAMES)
def corpus(request, chk):
    return corpus_of(chk, request.param)


# ------------------------------------------------ what keeps the rest from being vacuous
@pytest.mark.parametrize("name", NAMES)
def test_the_generator_meets_its_conditions(name):
    """From the model alone: every schema path that can exist is found in at least 15 % of the documents and
    missed in at least 15 %, the others never; every edit class has at least 50 OK cases; every column kind at
    least 50 OK cells (bool and list<double> in "all" alone: "nesting" has neither)."""
    td = M.descriptors()[name]
    rng = random.Random(SEEDS[name])
    docs = [M.gen_doc(rng, td) for _ in range(N_DOCS)]
    for p in M.PATHS[name]["exist"]:
        found = sum(not isinstance(M.sub(d, td, p), int) for d in docs)
        assert 0.15 * N_DOCS <= found <= 0.85 * N_DOCS, (p, found)
    for p in M.PATHS[name]["never"]:
        assert all(isinstance(M.sub(d, td, p), int) for d in docs), p
    steps = {(len(p), M.sub(d, td, p)) for p in M.PATHS[name]["exist"] + M.PATHS[name]["never"] for d in docs
             if isinstance(M.sub(d, td, p), int)}
    assert {s for _, s in steps} >= {0, 1, 2} and any(s < n - 1 for n, s in steps)
    classes = {}
    for form, op, path in M.EDITS[name]:
        for d in docs:
            c = M.edit(d, td, op, path, 0)[0]
            classes[c] = classes.get(c, 0) + 1
            classes[form, c] = classes.get((form, c), 0) + 1
    for c in ("replaced", "inserted", "deleted"):
        assert classes.get(c, 0) >= 50, classes
    for c in ("notfound", "untouched"):
        assert classes.get(c, 0) >= 10, classes
    for form in ("insert at a list's front", "unset list element 0", "unset field", "set nested string"):
        ok = sum(v for (f, c), v in ((k, v) for k, v in classes.items() if isinstance(k, tuple))
                 if f == form and c in ("replaced", "inserted", "deleted"))
        assert ok >= 50, (form, ok)
    many = {}
    for form, op, parent, steps_ in M.MANY[name]:
        for d in docs:
            c, mask, _, _ = M.many(d, td, op, parent, [(s, 0) for s in steps_])
            c = c if c != "set" else "replaces" if mask == (1 << len(steps_)) - 1 else "inserts" if not mask else "mixed"
            many[c] = many.get(c, 0) + 1
    for c in ("replaces", "inserts", "mixed", "dropped"):
        assert many.get(c, 0) >= 50, many
    for c in ("notfound", "untouched"):
        assert many.get(c, 0) >= 10, many
    assert {len(s) for _, _, _, s in M.MANY[name]} >= {2, 3, 7}
    cells = {}
    for path, kind in M.COLUMNS[name] + M.COLUMNS_2[name]:
        cells[kind] = cells.get(kind, 0) + sum(M.column(d, td, path, kind)[0] == "ok" for d in docs)
    kinds = set(M.COL_KINDS) - ({M.COL_BOOL, M.COL_LIST_F64} if name == "nesting" else set())
    assert all(cells.get(k, 0) >= 50 for k in kinds), cells
    if name == "all":
        assert {k for _, k in M.COLUMNS[name]} == set(M.COL_KINDS)


def test_the_documents_carry_what_the_issue_lists():
    td = M.descriptors()["all"]
    rng = random.Random(SEEDS["all"])
    text = b"".join(M.dump(M.gen_doc(rng, td)) for _ in range(N_DOCS)).decode()
    for piece in ("5e-324", "1e+300", "0.0", "-9223372036854775808", "9223372036854775807", "-128", "32767", "\\n", "é",
                  "中", "😀", '\\"', '"-1":', '"-32768":', '"-2":'):
        assert piece in text, piece
    assert "null" not in text


# ---------------------------------------------------------------- GetByPath
def test_get_by_path(corpus):
    td = corpus.td
    ok = miss = 0
    for doc, t in zip(corpus.docs, corpus.msgs):
        for p in M.PATHS[corpus.name]["exist"] + M.PATHS[corpus.name]["never"] + [[]]:
            want, got = M.sub(doc, td, p), R.get_by_path(t, p)
            if isinstance(want, int):
                assert (got.status, got.step) == (R.NOT_FOUND, want), (p, got)
                miss += 1
            else:
                assert (got.status, got.type, got.step) == (R.OK, want[1].type, len(p)), (p, got)
                assert t[got.start:got.end] == corpus.enc(want[1], want[0]), p
                ok += 1
    assert ok >= 1000 and miss >= 1000


def test_get_by_path_every_node_three_steps_down(corpus):
    """every node of the first 60 documents down to 3 steps, by the path the model gives it"""
    n = 0

    def walk(doc, t, v, d, path):
        nonlocal n
        got = R.get_by_path(t, path)
        assert (got.status, got.type) == (R.OK, d.type) and t[got.start:got.end] == corpus.enc(d, v), path
        n += 1
        if len(path) == 3 or d.type not in M.COMPLEX:
            return
        for k in M.children(v, d)[1]:
            val = k.key_bytes if k.kind == M.STRKEY else k.key
            walk(doc, t, k.value, k.td, path + [(k.kind, val)])

    for doc, t in list(zip(corpus.docs, corpus.msgs))[:60]:
        walk(doc, t, doc, corpus.td, [])
    assert n >= 1000  # 60 documents of well over 17 nodes each


# ---------------------------------------------------------------- MarshalTo
def test_marshal_to(corpus):
    rng = random.Random(SEEDS[corpus.name] + 1)
    dropped = 0
    for j in range(100):
        to = M.narrow(rng, corpus.td)
        for i in range(3 * j, 3 * j + 3):
            ret, out = CR.marshal_to(corpus.msgs[i], corpus.td, to, 0)
            assert ret == 0 and out == corpus.enc(to, corpus.docs[i]), (j, i, hex(ret))
            dropped += len(out) < len(corpus.msgs[i])
    assert dropped >= 250


def test_marshal_to_required(corpus):
    """`to` marks REQUIRED a field the document lacks: j2t's code 10 with the id in the value against the
    cut's E_REQUIRED with the id in aux, and the model's id for both (modelgen.cut_want)"""
    rng = random.Random(SEEDS[corpus.name] + 2)
    n_err = n_ok = 0
    for j in range(60):
        to = M.narrow(rng, corpus.td, keep=0.5, require=0.04)
        for i in range(5 * j, 5 * j + 5):
            want = M.cut_want(corpus.chk, corpus.docs[i], to)
            assert CR.marshal_to(corpus.msgs[i], corpus.td, to, 0) == want, (j, i, hex(want[0]))
            n_err += want[0] & 0xFF == CR.E_REQUIRED
            n_ok += want[0] == 0
    assert n_err >= 10 and n_ok >= 10, (n_err, n_ok)


def test_marshal_to_disallow_unknown(corpus):
    """DISALLOW_UNKNOWN against j2t without flag 0x1 (modelgen.cut_unknown_want): `from` is a narrowing that
    lacks some of the message's fields, `to` a field-for-field copy of it, so the cut walks every struct j2t
    walks"""
    rng = random.Random(SEEDS[corpus.name] + 3)
    n_err = n_ok = 0
    for j in range(60):
        frm = M.narrow(rng, corpus.td, keep=0.97)
        to = M.narrow(rng, frm, keep=1.0)
        for i in range(5 * j, 5 * j + 5):
            want = M.cut_unknown_want(corpus.chk, corpus.docs[i], frm, corpus.td)
            assert CR.marshal_to(corpus.msgs[i], frm, to, CR.DISALLOW_UNKNOWN) == want, (j, i, hex(want[0]))
            assert want[0] or want[1] == corpus.msgs[i]
            n_err += want[0] & 0xFF == CR.E_UNKNOWN
            n_ok += want[0] == 0
    assert n_err >= 10 and n_ok >= 10, (n_err, n_ok)


# --------------------------------------------------- SetByPath / UnsetByPath
_CLASS = {"replaced": (E.OK, True), "inserted": (E.OK, False), "deleted": (E.OK, True), "untouched": (E.OK, False),
          "notfound": (E.NOT_FOUND, False)}


@pytest.mark.parametrize("name,k", [(n, k) for n in NAMES for k in range(len(M.EDITS[n]))])
def test_edit(chk, name, k):
    corpus = corpus_of(chk, name)
    form, op, path = M.EDITS[name][k]
    vtd = M.desc_at(corpus.td, path)
    values = corpus.values(form, vtd) if op == M.SET_OP else [None] * len(corpus.docs)
    for doc, t, v in zip(corpus.docs, corpus.msgs, values):
        cls, new = M.edit(doc, corpus.td, op, path, v)
        if op == M.SET_OP:
            ret, out = E.edit(E.SET_OP, t, path, corpus.enc(vtd, v), vtd.type)
        else:
            ret, out = E.edit(E.UNSET_OP, t, path)
        assert (ret & 0xFF, bool(ret & E.EXISTED)) == _CLASS[cls], (form, cls, hex(ret))
        assert out == (corpus.enc(corpus.td, new) if new is not None else b""), (form, cls)


# --------------------------------------------------------- SetMany / UnsetMany
@pytest.mark.parametrize("name,k", [(n, k) for n in NAMES for k in range(len(M.MANY[n]))])
def test_edit_many(chk, name, k):
    corpus = corpus_of(chk, name)
    form, op, parent, steps = M.MANY[name][k]
    ptd = M.desc_at(corpus.td, parent)
    vtds = [M.desc_at(ptd, [s]) for s in steps]
    vals = [corpus.values("%s/%d" % (form, j), d) for j, d in enumerate(vtds)]
    for i, (doc, t) in enumerate(zip(corpus.docs, corpus.msgs)):
        items = [(s, vals[j][i]) for j, s in enumerate(steps)]
        cls, mask, item, new = M.many(doc, corpus.td, op, parent, items)
        ret, out = EM.edit_many(op, t, parent, [(s, corpus.enc(vtds[j], v) if op == M.SET_OP else b"", vtds[j].type)
                                                for j, (s, v) in enumerate(items)])
        st = EM.NOT_FOUND if cls == "notfound" else EM.OK
        assert (EM.status_of(ret), ret >> 8 & 0xFF, EM.item_of(ret)) == (st, mask, item), (form, cls, hex(ret))
        assert out == (corpus.enc(corpus.td, new) if new is not None else b""), (form, cls)


# ------------------------------------------------------------------ Children
@pytest.mark.parametrize("recurse", (False, True))
def test_children(corpus, recurse):
    n_ok = n_miss = n_kids = 0
    for path in M.KID_PATHS[corpus.name]:
        for doc, t in zip(corpus.docs, corpus.msgs):
            want = M.children(doc, corpus.td, path, recurse)
            head, kids = K.children(t, path, recurse)
            if isinstance(want, int):
                assert (head.status, head.direct, kids) == (R.NOT_FOUND, want, []), path
                n_miss += 1
                continue
            (typ, kt, et, direct), recs = want
            assert (head.status, head.type, head.key_type, head.elem_type, head.direct, head.count) == (
                R.OK, typ, kt, et, direct, len(recs)), (path, head)
            assert len(kids) == len(recs)
            for g, w in zip(kids, recs):
                assert (g.kind, g.key, g.type, g.depth, g.parent, g.n_desc) == (w.kind, w.key, w.type, w.depth, w.parent,
                                                                              w.n_desc), (path, g)
                assert t[g.start:g.end] == corpus.enc(w.td, w.value)
                if w.kind == M.STRKEY:
                    assert K.key_bytes(t, g) == w.key_bytes
                n_kids += 1
            n_ok += 1
    assert n_ok >= 400 and n_miss >= 100 and n_kids >= 3000, (n_ok, n_miss, n_kids)


# ------------------------------------------------------------------- Columns
def test_columns(corpus):
    n_ok = n_miss = 0
    for path, kind in M.COLUMNS[corpus.name] + M.COLUMNS_2[corpus.name]:
        for doc, t in zip(corpus.docs, corpus.msgs):
            want = M.column(doc, corpus.td, path, kind)
            got = C.cell(t, path, kind)
            if want[0] == "notfound":
                assert (got.status, got.step) == (R.NOT_FOUND, want[1]), (path, got)
                n_miss += 1
                continue
            _, val, ln, elems, text = want
            assert got.status == R.OK, (path, kind, got)
            if text is not None:
                assert (got.len, t[got.val:got.val + got.len]) == (ln, text), path
            elif elems is not None:
                assert (got.len, got.elems) == (ln, elems), path
            else:
                assert got.val == val, (path, kind, got.val, val)
            n_ok += 1
    assert n_ok >= 1000 and n_miss >= 500
