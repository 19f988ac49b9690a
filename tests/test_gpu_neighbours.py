"""GPU: a message's result does not depend on the bytes behind it.

The kernels read 16-byte windows past a message's end, and every other test
lays its messages out so that zero bytes follow (the arena's padding), or a
next message that starts afresh. Here a number, a string, a literal or a
Thrift scalar that ends exactly at a message's end is followed by the bytes
that would COMPLETE it: every document is cut at every position k, and s[:k]
and s[k:] sit next to each other as two messages; and each prefix ends a batch
whose arena goes on with zeros, 0xFF, the completing bytes, or quotes and
backslashes. Every message must get what the oracle gives it alone."""
import random
import struct

import numpy as np
import pytest

import oracle
import slotguard as SG
import t2jgen
from dynamicgo_amd import thrift as T, workloads as W
from test_gpu_slots import FLAT, NO_FLAT, NO_WAVE, j2t_launch, t2j_launch

pytestmark = pytest.mark.gpu

if oracle.ref_lib_path() is None:
    pytest.skip("oracle/_ref not built", allow_module_level=True)

DEV = "cuda:0"
QB = b'"\\' * 8  # alternating quote and backslash


def convert(launch, msgs, slot, tail=None):
    """One launch over generous 8-aligned slots -> [(ret, out)]."""
    off = np.cumsum([SG.GUARD] + [slot(len(m)) for m in msgs])
    r = SG.launch_twice(launch, msgs, off, int(off[-1]) + SG.GUARD, DEV, tail=tail, fills=SG.FILLS[:1])[0]
    res = []
    for i in range(len(msgs)):
        ret, n = int(r.ret[i]), int(r.out_len[i])
        assert n <= off[i + 1] - off[i], (msgs[i], n)
        res.append((ret, r.out[off[i]:off[i] + n].tobytes()))
    return res


def open_string_tail(m):
    """Bytes after the opening quote of a string the message ends inside, or
    None."""
    i, start = 0, None
    while i < len(m):
        c = m[i]
        if start is None:
            if c == 0x22:
                start = i + 1
        elif c == 0x5C:
            i += 1
        elif c == 0x22:
            start = None
        i += 1
    return None if start is None else len(m) - start


def j2t_expect(fl, flags):
    """The compiled reference, except for its one undefined verdict (DESIGN
    §4): an unterminated string whose bytes after the opening quote end on a
    SIMD block boundary -- there the port oracle, as test_oracle.py does."""
    ref, port = oracle.RefOracle(), oracle.PortOracle()

    def f(m):
        t = open_string_tail(m)
        return (port if t is not None and t % 16 == 0 else ref).j2t(fl, m, flags)
    return f


J2T_DOCS = [
    ("Simple", W.simple_desc, b'{"ByteField":-7,"I64Field":123456789012,"DoubleField":-1.25e-3,"I32Field":77,'
                              b'"StringField":"str","BinaryField":"aGVsbG8="}'),
    ("Nesting", W.nesting_desc, b'{"String":"s","ListI32":[1,-22,333],"MapStringString":{"k":"v"},"Double":2.5,'
                                b'"SimpleStruct":{"ByteField":1,"I64Field":10},"ListString":["a",""],"I64":-9,"Byte":null}'),
    ("i64", lambda: T.builtin("i64"), b"12345"),
    ("double", lambda: T.builtin("double"), b"1.5e3"),
    ("Simple", W.simple_desc, b'{"I32Field":1,"StringField":"ends in an escape\\n"}'),
    ("string", lambda: T.builtin("string"), b'"root \\u00e9 string"'),
]
J2T_ROUTES = {"flat": (1 | FLAT, {}), "small": (1 | NO_FLAT, {"wave_min": 1 << 20}), "wave": (1, {"wave_min": 0}),
              "lane": (1 | NO_WAVE, {"small_mpw": 0})}


def cuts(s):
    return [(s[:k], s[k:]) for k in range(len(s) + 1)]


def _mismatches(msgs, got, want):
    return [(m, hex(g[0]), g[1][:40], hex(w[0]), w[1][:40]) for m, g, w in zip(msgs, got, want)
            if (g[0], g[1] if g[0] == 0 else b"") != (w[0], w[1])]


@pytest.mark.parametrize("route", list(J2T_ROUTES))
def test_j2t_completing_neighbours(route, knob):
    flags, knobs = J2T_ROUTES[route]
    for k, v in knobs.items():
        knob(k, v)
    for name, mk, doc in J2T_DOCS:
        fl = T.flatten(mk())
        msgs = [part for pair in cuts(doc) for part in pair]
        expect = j2t_expect(fl, 1)
        got = convert(j2t_launch(fl, flags), msgs, lambda n: (4 * n + 64 + 7) // 8 * 8)
        bad = _mismatches(msgs, got, [expect(m) for m in msgs])
        assert not bad, (name, len(bad), bad[:3])


@pytest.mark.parametrize("route", ["default", "wave"])
def test_j2t_arena_tail(route, knob):
    """Each prefix as the batch's last message; the 16 bytes behind the arena
    are zeros, 0xFF, the completing bytes, quotes and backslashes."""
    if route == "wave":
        knob("wave_min", 0)
    for name, mk, doc in J2T_DOCS:
        fl = T.flatten(mk())
        expect = j2t_expect(fl, 1)
        launch = j2t_launch(fl, 1)
        for k in range(len(doc) + 1):
            msgs = [doc, doc[:k]]
            want = [expect(m) for m in msgs]
            for tail in (bytes(16), b"\xff" * 16, (doc[k:k + 16] + bytes(16))[:16], QB):
                got = convert(launch, msgs, lambda n: (4 * n + 64 + 7) // 8 * 8, tail=tail)
                bad = _mismatches(msgs, got, want)
                assert not bad, (name, k, tail, bad)


# ---------------------------------------------------------------- t2j
def _str(b):
    return struct.pack(">i", len(b)) + b


def t2j_docs():
    td = t2jgen.all_types_desc()
    rng = random.Random(3)
    while True:
        m = t2jgen.gen_thrift(rng, td)
        if 60 <= len(m) <= 160 and oracle.RefT2JOracle().t2j(T.flatten(td), T.flatten_t2j(T.flatten(td)), m, 0)[0] == 0:
            break
    i64, string = T.builtin("i64"), T.builtin("string")
    # a struct ends in its STOP byte: the roots here are containers, whose last element ends the message
    return [("all-types", td, m),
            ("ends in an i64", T.list_of(i64), b"\x0a" + struct.pack(">iqq", 2, -5, 0x0102030405060708)),
            ("ends in a string", T.list_of(string), b"\x0b" + struct.pack(">i", 2) + _str(b"first") + _str(b"tail string\x01")),
            ("ends in a map of strings", T.map_of(string, string),
             b"\x0b\x0b" + struct.pack(">i", 2) + _str(b"k1") + _str(b"value one") + _str(b"k2") + _str(b"v2"))]


def _t2j_route(route, knob):
    if route == "wave":
        knob("t2j_wave_min", 1)
    else:
        knob("t2j_wave_min", 0)
        knob("t2j_spread", int(route[-1]))


@pytest.mark.parametrize("route", ["lane-spread1", "lane-spread4", "wave"])
def test_t2j_completing_neighbours(route, knob):
    _t2j_route(route, knob)
    chk = oracle.RefT2JOracle()
    for name, td, doc in t2j_docs():
        fl = T.flatten(td)
        side = T.flatten_t2j(fl)
        msgs = [part for pair in cuts(doc) for part in pair]
        got = convert(t2j_launch(fl, 0), msgs, lambda n: (8 * n + 64 + 7) // 8 * 8)
        bad = _mismatches(msgs, got, [chk.t2j(fl, side, m, 0) for m in msgs])
        assert not bad, (name, len(bad), bad[:3])


@pytest.mark.parametrize("route", ["lane-spread1", "wave"])
def test_t2j_arena_tail(route, knob):
    _t2j_route(route, knob)
    chk = oracle.RefT2JOracle()
    for name, td, doc in t2j_docs():
        fl = T.flatten(td)
        side = T.flatten_t2j(fl)
        launch = t2j_launch(fl, 0)
        for k in range(len(doc) + 1):
            msgs = [doc, doc[:k]]
            want = [chk.t2j(fl, side, m, 0) for m in msgs]
            for tail in (bytes(16), b"\xff" * 16, (doc[k:k + 16] + bytes(16))[:16], QB):
                got = convert(launch, msgs, lambda n: (8 * n + 64 + 7) // 8 * 8, tail=tail)
                bad = _mismatches(msgs, got, want)
                assert not bad, (name, k, tail, bad)
