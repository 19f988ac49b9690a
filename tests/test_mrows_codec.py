"""The map-row checker (mrowsref.py) against a second yardstick that shares
nothing with it: the document model (modelgen.py) and the reference's own j2t
(oracle.RefOracle, the port oracle where oracle/_ref was not built). On the
`nesting` and `all` descriptors' maps the rows of T = j2t(doc, D) must equal
modelgen.children(doc, D, parent) in document order: every key, and every cell
as modelgen.column of the kid's value. Bytes, integers and bit patterns only; no
tolerance.

No GPU: the kernels get the same expectations in test_gpu_mrows_codec.py."""
import random

import pytest

import modelgen as M
import mrowsref as MR
import oracle
import tgetref as R

N_DOCS = 300
F = R.FIELD
STR, INT = MR.KEY_STR, MR.KEY_INT
# (descriptor, parent path, key kind, [(sub-path, kind)])
PLANS = [
    # map<string, Simple{1: byte, 2: i64 with a value mapping, 3: double, 4: i32, 5: string, 6: binary}>
    ("nesting", [(F, 15)], STR, [([(F, 1)], M.COL_BYTE), ([(F, 3)], M.COL_F64), ([(F, 4)], M.COL_INT), ([(F, 5)], M.COL_STR),
                                 ([(F, 6)], M.COL_STR), ([(F, 2)], M.COL_INT)]),
    ("nesting", [(F, 7)], STR, [([], M.COL_STR)]),    # map<string, string>
    ("nesting", [(F, 9)], INT, [([], M.COL_INT)]),    # map<i32, i64>
    ("nesting", [(F, 12)], INT, [([], M.COL_STR)]),   # map<i64, string>
    # map<i32, Inner{1: i64 required, 2: string, 3: list<double>}>
    ("all", [(F, 15)], INT, [([(F, 1)], M.COL_INT), ([(F, 2)], M.COL_STR), ([(F, 3)], M.COL_LIST_F64)]),
    ("all", [(F, 12)], STR, [([], M.COL_LIST_INT)]),  # map<string, list<i32>>
    ("all", [(F, 14)], INT, [([], M.COL_STR)]),       # map<i16, binary>
    ("all", [(F, 13)], INT, [([], M.COL_BOOL)]),      # map<byte, bool>
]
NEVER_THERE = ("nesting", 5)  # plan 0's last column, field 2: the model leaves fields with a value mapping out
ALWAYS_THERE = ("all", 0)     # Inner's required field


@pytest.fixture(scope="module")
def corpora():
    ref = oracle.RefOracle()
    print("\ntest_mrows_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return {name: M.Corpus(ref or oracle.PortOracle(), name, N_DOCS) for name in ("nesting", "all")}


def model_rows(doc, td, parent, columns):
    """("notfound", step) or ("ok", key type, [(the kid, [the model's cell of its value under column k])])"""
    r = M.children(doc, td, parent)
    if isinstance(r, int):
        return "notfound", r
    (t, kt, _, direct), kids = r
    assert t == M.MAP and direct == len(kids)
    return "ok", kt, [(kid, [M.column(kid.value, kid.td, p, k) for p, k in columns]) for kid in kids]


def same_message(head, keys, cells, want, arena, what):
    """a message's head (status, step, count), keys (val, len) and cells (anything with status / step / val / len,
    and elems or None, [row][column]) against the model's; string keys and STR values are offsets into `arena`.
    Returns the OK cells seen."""
    if want[0] == "notfound":
        assert (head.status, head.step, head.count) == (R.NOT_FOUND, want[1], 0) and not cells and not keys, (what, head)
        return 0
    _, kt, rows = want
    assert (head.status, head.count) == (R.OK, len(rows)) and len(cells) == len(keys) == len(rows), (what, head)
    n_ok = 0
    for j, (key, row, (kid, wrow)) in enumerate(zip(keys, cells, rows)):
        if kid.kind == M.STRKEY:
            assert key.len == kid.key and bytes(arena[key.val:key.val + key.len]) == kid.key_bytes, (what, j, key)
        else:
            assert kid.kind == M.INTKEY and (key.val, key.len) == (kid.key % 2 ** 64, M.INT_BITS[kt] // 8), (what, j, key, kid.key)
        for k, (c, w) in enumerate(zip(row, wrow)):
            if w[0] == "notfound":
                assert (c.status, c.step) == (R.NOT_FOUND, w[1]), (what, j, k, c)
                continue
            assert c.status == R.OK, (what, j, k, c)
            n_ok += 1
            if w[4] is not None:  # bytes
                assert c.len == w[2] and bytes(arena[c.val:c.val + c.len]) == w[4], (what, j, k, c)
            elif w[3] is not None:  # a list: its length and, where the caller has them, its elements
                assert c.len == w[2] and (c.elems is None or list(c.elems) == w[3]), (what, j, k, c, w)
            else:
                assert c.val == w[1], (what, j, k, c, w)
    return n_ok


def test_the_corpus_meets_its_conditions():
    """From the model alone, with the seeds of Corpus.SEEDS and 300 documents: every plan has at least 300 rows, maps of
    0 and of 3 entries and at least 100 messages without the map; every struct sub-column has at least 100 cells that
    are there and at least 100 that are not, but `nesting` field 2 (never there) and `all` 15 field 1 (always there)"""
    tds = M.descriptors()
    docs = {}
    for name in ("nesting", "all"):
        rng = random.Random(M.Corpus.SEEDS[name])
        docs[name] = [M.gen_doc(rng, tds[name]) for _ in range(N_DOCS)]
    for name, parent, _, columns in PLANS:
        rows = [model_rows(d, tds[name], parent, columns) for d in docs[name]]
        sizes = [len(r[2]) for r in rows if r[0] == "ok"]
        assert sum(sizes) >= 300 and 0 in sizes and 3 in sizes, (name, parent)
        assert sum(r[0] == "notfound" for r in rows) >= 100, (name, parent)
        if not columns[0][0]:
            continue  # the values themselves: always there
        for k in range(len(columns)):
            cells = [wrow[k][0] for r in rows if r[0] == "ok" for _, wrow in r[2]]
            if (name, k) == NEVER_THERE:
                assert "ok" not in cells
            elif (name, k) == ALWAYS_THERE:
                assert "notfound" not in cells and len(cells) >= 300
            else:
                assert cells.count("ok") >= 100 and cells.count("notfound") >= 100, (name, parent, k)


def test_map_rows(corpora):
    n_ok = n_rows = 0
    for name, parent, keys, columns in PLANS:
        c = corpora[name]
        for doc, t in zip(c.docs, c.msgs):
            m = MR.message(t, parent, columns, keys)
            n_ok += same_message(m.head, m.keys, m.cells, model_rows(doc, c.td, parent, columns), t, (name, parent))
            n_rows += len(m.rows)
            for r, key in zip(m.rows, m.keys):  # the index entry is the value's span: it starts where the key ends
                assert r.off == (key.val + key.len if keys == STR else r.off) and r.off + r.len <= len(t)
    assert n_rows >= 8 * 300 and n_ok >= 3000
