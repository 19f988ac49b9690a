"""The entry-column checker (entsref.py) against a second yardstick that shares
nothing with it: the document model (modelgen.py, entsmodel.py) and the
reference's own j2t (oracle.RefOracle, the port oracle where oracle/_ref was
not built). The entries of T = j2t(doc, D) must be list(doc.items()) in
document order. Bytes, integers and bit patterns only; no tolerance.

No GPU: the kernels get the same expectations in test_gpu_ents_codec.py."""
import random

import pytest

import entsmodel as EM
import entsref as ER
import modelgen as M
import oracle
import tgetref as R

N_DOCS = 300


@pytest.fixture(scope="module")
def corpus():
    ref = oracle.RefOracle()
    print("\ntest_ents_codec: the oracle is %s" % ("RefOracle (oracle/_ref)" if ref else "PortOracle (oracle/_build)"))
    return M.Corpus(ref or oracle.PortOracle(), "all", N_DOCS)


def same_cell(got, want, t, base, what):
    """a checker cell (or anything with its fields) against the model's"""
    if want[0] == "notfound":
        assert (got.status, got.step) == (R.NOT_FOUND, want[1]), (what, got)
        return "miss"
    if want[0] == "unsupported":
        assert got.status == ER.E_UNSUPPORTED, (what, got)
        return "unsupported"
    ents = want[1]
    assert (got.status, got.len) == (R.OK, len(ents)), (what, got)
    for j, (k, v) in enumerate(ents):
        if isinstance(k, bytes):
            assert t[got.keys[j] - base:got.keys[j] - base + got.klens[j]] == k, (what, j)
        elif k is not None:
            assert got.keys[j] == k, (what, j, got.keys[j], k)
        if isinstance(v, bytes):
            assert t[got.vals[j] - base:got.vals[j] - base + got.vlens[j]] == v, (what, j)
        else:
            assert got.vals[j] == v, (what, j, got.vals[j], v)
    return "ok" if ents else "empty"


def test_the_corpus_meets_its_conditions():
    """From the model alone, with the seed of Corpus.SEEDS: every positive column has at least 50 OK cells that
    are not empty, and the two fields no kind takes are unsupported whenever they are not empty"""
    td = M.descriptors()["all"]
    rng = random.Random(M.Corpus.SEEDS["all"])
    docs = [M.gen_doc(rng, td) for _ in range(N_DOCS)]
    for path, kind in EM.POSITIVE:
        cells = [EM.entries(d, td, path, kind) for d in docs]
        assert sum(c[0] == "ok" and len(c[1]) > 0 for c in cells) >= 50, (path, kind)
        assert all(c[0] in ("ok", "notfound") for c in cells)
    for path, kind in EM.NEGATIVE:
        cells = [EM.entries(d, td, path, kind) for d in docs]
        assert sum(c[0] == "unsupported" for c in cells) >= 50 and all(c[0] != "ok" or c[1] == [] for c in cells)
    cells = [EM.entries(d, td, *EM.POSITIVE[2]) for d in docs]
    keys = [k for c in cells if c[0] == "ok" for k, _ in c[1]]
    assert 255 in keys and 128 in keys and all(0 <= k <= 255 for k in keys)  # I08 keys -1 and -128, masked


def test_entries(corpus):
    seen = {}
    for path, kind in EM.COLUMNS:
        for doc, t in zip(corpus.docs, corpus.msgs):
            r = same_cell(ER.cell(t, path, kind), EM.entries(doc, corpus.td, path, kind), t, 0, (path, kind))
            seen[kind, r] = seen.get((kind, r), 0) + 1
    for _, kind in EM.POSITIVE:
        assert seen.get((kind, "ok"), 0) >= 50, seen
    assert sum(v for (_, r), v in seen.items() if r == "unsupported") >= 150 and \
        sum(v for (_, r), v in seen.items() if r == "miss") >= 300, seen
