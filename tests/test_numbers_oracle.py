"""CPU: the number corpora of numgen.py against three references at once --
the compiled reference (oracle/_ref), its C restatement (PortOracle) and
Python's own correctly rounded float() / repr(). The corpus is only useful on
the GPU if its expected values are beyond doubt, so here every finite,
well-formed token must parse to float(token) bit for bit in the reference, the
restatement must equal the reference in every field type, and the reference's
f64toa must give repr()'s shortest digits and round-trip."""
import re
import struct
from collections import Counter

import pytest

import numgen
import oracle
from dynamicgo_amd import thrift as T
from test_gpu_flat import flat_desc

JSON_NUMBER = re.compile(r"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?\Z")
NUM_FIELDS = ("y", "s16", "s32", "s64", "d", "vm64", "vm16", "far")

# finite, well-formed tokens on which the reference does not give float(token);
# the reference wins on the GPU. At most 8, each with what the reference does.
REF_NOT_PYTHON = [
]


def double_desc():
    return T.struct_type("D", [T.FieldDescriptor(1, "d", T.builtin("double"), T.OPTIONAL)])


def parse_all(chk, tokens):
    """[(status, 8 bytes or None)] of {"d":TOKEN} for every token."""
    fl = T.flatten(double_desc())
    rets, outs = chk.j2t_batch(fl, [b'{"d":' + t.encode() + b"}" for t in tokens], 1, nthreads=8)
    res = []
    for r, o in zip(rets, outs):
        if int(r) == 0:
            assert o[:3] == b"\x04\x00\x01" and len(o) == 12 and o[11] == 0, o
        res.append((int(r), o[3:11] if int(r) == 0 else None))
    return res


def check_against_python(chk):
    assert len(REF_NOT_PYTHON) <= 8
    toks = numgen.j2t_tokens()
    res = parse_all(chk, [t for _, t in toks])
    bad = []
    for (c, t), (r, o) in zip(toks, res):
        if not JSON_NUMBER.match(t):
            if r == 0:
                bad.append((c, t[:60], "malformed but accepted"))
            continue
        want = float(t)
        if r != 0:
            if want not in (float("inf"), float("-inf")):
                bad.append((c, t[:60], hex(r)))
        elif o != struct.pack(">d", want) and t not in REF_NOT_PYTHON:
            bad.append((c, t[:60], o.hex(), struct.pack(">d", want).hex()))
    assert not bad, (len(bad), bad[:6])


def test_corpus_classes_are_populated():
    n = Counter(c for c, _ in numgen.j2t_tokens())
    assert set(n) == {"mid", "seam", "exact", "elfail", "shape", "zeros", "cvt", "rand"}
    d = Counter(c for c, _ in numgen.t2j_doubles())
    assert set(d) == {"pow2", "pow10", "fmt", "digits"}
    for c, k in list(n.items()) + list(d.items()):
        assert k >= (16 if c in ("fmt", "cvt") else 32), (c, k)
    assert n["rand"] == 5000 and len(numgen.mids()) >= 60
    assert len(set(numgen.t2j_ints())) >= 32
    # deterministic: a second build gives the same corpus
    numgen._J2T = numgen._T2J = None
    again = Counter(c for c, _ in numgen.j2t_tokens())
    assert again == n


def test_midpoints_are_exact_halves():
    """The construction itself: each midpoint is exactly between its two
    doubles, so it has no nearest double and only round-half-even decides."""
    from fractions import Fraction
    for b, d, k in numgen.mids():
        mid = Fraction(int(d), 10 ** k)
        lo = Fraction(numgen.b2f(b))
        hi = Fraction(2) ** 1024 if (b + 1) >> 52 == 2047 else Fraction(numgen.b2f(b + 1))
        assert mid - lo == hi - mid and hi > lo, hex(b)
        even = b if b % 2 == 0 else b + 1
        if even >> 52 != 2047:
            assert numgen.f2b(float(numgen.render(d, k))) == even, hex(b)


def test_port_parse_equals_python():
    check_against_python(oracle.PortOracle())


def test_reference_parse_equals_python():
    ref = oracle.RefOracle()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    check_against_python(ref)


def test_port_equals_reference_in_every_field():
    ref = oracle.RefOracle()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    port = oracle.PortOracle()
    fl = T.flatten(flat_desc())
    toks = numgen.j2t_tokens()
    for f in NUM_FIELDS:
        msgs = [('{"req":1,"%s":%s}' % (f, t)).encode() for _, t in toks]
        for flags in (0x1, 0x41):
            r1, o1 = ref.j2t_batch(fl, msgs, flags, nthreads=8)
            r2, o2 = port.j2t_batch(fl, msgs, flags, nthreads=8)
            bad = [(f, toks[i][0], msgs[i][:60], hex(int(r1[i])), hex(int(r2[i])))
                   for i in range(len(msgs)) if int(r1[i]) != int(r2[i]) or o1[i] != o2[i]]
            assert not bad, (len(bad), bad[:5])


def ref_f64_texts(chk, values):
    """The reference's f64toa text of every value (lists of 40 doubles)."""
    td = T.struct_type("L", [T.FieldDescriptor(1, "d", T.list_of(T.builtin("double")), T.OPTIONAL)])
    fl = T.flatten(td)
    side = T.flatten_t2j(fl)
    texts = []
    for a in range(0, len(values), 40):
        part = values[a:a + 40]
        m = b"\x0f\x00\x01\x04" + struct.pack(">i", len(part)) + b"".join(struct.pack(">d", v) for v in part) + b"\x00"
        r, j = chk.t2j(fl, side, m, 0)
        assert r == 0 and j.startswith(b'{"d":[') and j.endswith(b"]}"), (r, j[:60])
        got = j[6:-2].decode().split(",")
        assert len(got) == len(part)
        texts += got
    return texts


def ref_i64_texts(chk, values):
    td = T.struct_type("L", [T.FieldDescriptor(1, "i", T.list_of(T.builtin("i64")), T.OPTIONAL)])
    fl = T.flatten(td)
    m = b"\x0f\x00\x01\x0a" + struct.pack(">i", len(values)) + b"".join(struct.pack(">q", v) for v in values) + b"\x00"
    r, j = chk.t2j(fl, T.flatten_t2j(fl), m, 0)
    assert r == 0
    return j[6:-2].decode().split(",")


def test_reference_f64toa_equals_repr():
    chk = oracle.RefT2JOracle()
    if chk is None:
        pytest.skip("oracle/_ref not built")
    vals = [v for _, v in numgen.t2j_doubles()]
    texts = ref_f64_texts(chk, vals)
    bad = []
    for v, t in zip(vals, texts):
        if numgen.f2b(float(t)) != numgen.f2b(v) or numgen.sig_digits(t) != numgen.sig_digits(repr(v)):
            bad.append((v.hex(), t, repr(v)))
    assert not bad, (len(bad), bad[:6])
    ints = numgen.t2j_ints()
    assert ref_i64_texts(chk, ints) == [str(v) for v in ints]
