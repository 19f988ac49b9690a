"""GPU: number conversion both ways on the branch-targeted corpora of
numgen.py (validated on the CPU by test_numbers_oracle.py and
test_num_host.py), byte for byte and status word for status word against the
compiled reference (the C restatement when oracle/_ref is absent).

j2t: every token in every numeric field of test_gpu_flat.flat_desc(), before a
',' and before a '}', on each route -- flat, small, wave (both instances),
lane, exact and the default routing -- with the bail counters saying that the
tokens the fast path must decline went to the exact machine and the rest did
not; then as map keys, map values and list elements, and as a root scalar.

t2j: every double and integer of the corpus in lists and alone in a struct, on
the lane and the wave kernel."""
import os
import struct
import subprocess
import tempfile
from collections import Counter

import numpy as np
import pytest

import numgen
import oracle
from dynamicgo_amd import conv, thrift as T
from test_gpu_flat import flat_desc
from test_gpu_parity import _raw_batch
from test_gpu_t2j import compare

pytestmark = pytest.mark.gpu

NO_FAST, NO_WAVE, FLAT, NO_FLAT = 1 << 17, 1 << 18, 1 << 19, 1 << 21
I64S, NULLNAN = 2, 4
FIELDS = ("y", "s16", "s32", "s64", "d", "vm64", "vm16", "far")
FLAGS = (0x1, 0x41)
NEVER_THIN = ("mid", "seam", "exact", "elfail", "zeros", "cvt")
FAR = 1 << 30  # wave_min: no message is long enough for the wave kernel


def _chk():
    return oracle.RefOracle() or oracle.PortOracle()


class Corpus:
    """The messages of one route's batch, what the reference makes of them
    (once per flag word), and how many of them the fast path must decline."""

    def __init__(self):
        toks = numgen.thin(numgen.j2t_tokens(), NEVER_THIN, {"rand": 10, "shape": 3})
        assert Counter(c for c, _ in toks)["rand"] == 500
        self.fl = T.flatten(flat_desc())
        self.msgs, self.tok = [], []
        for c, t in toks:
            for f in (("d",) if c == "mid" else FIELDS):
                self.msgs.append(('{"req":1,"%s":%s}' % (f, t)).encode())
                self.msgs.append(('{"%s":%s,"req":2}' % (f, t)).encode())
                self.tok += [(c, f, t)] * 2
        assert 30000 < len(self.msgs) < 60000, len(self.msgs)
        self.want = {}
        self.must_decline = self._must_decline()

    def expected(self, flags):
        if flags not in self.want:
            self.want[flags] = _chk().j2t_batch(self.fl, self.msgs, flags, nthreads=8)
        return self.want[flags]

    def _must_decline(self):
        """Messages whose number the fast parser declines (num_class of the
        host build); without a compiler, the elfail and mid tokens in "d"."""
        try:
            import test_num_host as H
            if not os.path.exists(H.B.HIPCC):
                raise OSError("no compiler")
            with tempfile.TemporaryDirectory() as d:
                num = H.Num(H.build_num(os.path.join(d, "libnum.so"), ("-shared",)))
                declines = {}
                for _, _, t in self.tok:
                    if t not in declines:
                        declines[t] = not num.cls(t.encode())[3]
            return sum(declines[t] for _, _, t in self.tok)
        except (OSError, ImportError, subprocess.CalledProcessError):
            return sum(c in ("elfail", "mid") and f == "d" for c, f, _ in self.tok)

    def bad(self, flags, extra):
        rets, outs = self.expected(flags)
        got, gr = _raw_batch(self.fl, self.msgs, flags | extra)
        return [(i, self.tok[i][0], self.msgs[i][:70], hex(int(gr[i])), hex(int(rets[i])))
                for i in range(len(self.msgs)) if int(gr[i]) != int(rets[i]) or got[i] != outs[i]]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


ROUTES = {  # name: (flag bits, knobs)
    "flat": (FLAT, {"wave_min": FAR}),
    "small": (NO_FLAT, {"wave_min": FAR}),
    "wave-occ4": (0, {"wave_min": 0, "wave_occ": 4}),
    "wave-occ5": (0, {"wave_min": 0, "wave_occ": 5}),
    "lane": (NO_WAVE, {}),
    "exact": (NO_FAST, {}),
    "hybrid": (0, {}),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_j2t_tokens_in_every_field(corpus, route, knob):
    extra, knobs = ROUTES[route]
    for k, v in knobs.items():
        knob(k, v)
    ctx = conv.default_context()
    n = len(corpus.msgs)
    for flags in FLAGS:
        ctx.stats(reset=True)
        bad = corpus.bad(flags, extra)
        bails, _ = ctx.stats(reset=True)
        print("%s flags %#x: %d messages, %d bails, %d must decline" % (route, flags, n, bails, corpus.must_decline))
        assert not bad, (route, hex(flags), len(bad), bad[:4])
        if route in ("flat", "small"):
            # every decline of these kernels is a bail; wave_min keeps the long messages here too
            assert bails >= corpus.must_decline, (route, bails, corpus.must_decline)
            assert bails * 2 < n, (route, bails, n)
        elif route.startswith("wave"):
            # the wave kernel parses the numbers its fast parser declines itself (vnumber_slow, one
            # lane at a time): only the messages that end in an error are redone by the exact machine
            errors = int(np.count_nonzero(corpus.expected(flags)[0]))
            assert bails >= errors, (route, bails, errors)
            assert bails * 2 < n, (route, bails, n)


def thinned(k=300):
    """About k tokens, every class in proportion but none under 24."""
    toks = numgen.j2t_tokens()
    n = Counter(c for c, _ in toks)
    step = {c: max(1, n[c] // max(24, k * n[c] // len(toks))) for c in n}
    out = numgen.thin(toks, (), step)
    assert set(c for c, _ in out) == set(n)
    return out


def container_desc():
    """test_gpu_flat.test_decimal_map_keys_and_values_vs_oracle's descriptor."""
    return T.struct_type("M", [
        T.FieldDescriptor(1, "md", T.map_of(T.builtin("i64"), T.builtin("double")), T.OPTIONAL),
        T.FieldDescriptor(2, "ld", T.list_of(T.builtin("double")), T.OPTIONAL),
        T.FieldDescriptor(3, "mi", T.map_of(T.builtin("double"), T.builtin("i32")), T.OPTIONAL),
    ])


def _compare(fl, msgs, flags, extra=0):
    rets, outs = _chk().j2t_batch(fl, msgs, flags, nthreads=8)
    got, gr = _raw_batch(fl, msgs, flags | extra)
    return [(i, msgs[i][:70], hex(int(gr[i])), hex(int(rets[i])))
            for i in range(len(msgs)) if int(gr[i]) != int(rets[i]) or got[i] != outs[i]]


@pytest.mark.parametrize("route", ["wave", "lane"])
def test_j2t_tokens_in_containers(route, knob):
    fl = T.flatten(container_desc())
    msgs = []
    for _, v in thinned():
        msgs.append(('{"md":{"%s":%s,"7":1.25},"ld":[%s,0.5]}' % (v, v, v)).encode())
        msgs.append(('{"mi":{"%s":1,"%s7":2},"ld":[1.5,%s]}' % (v, v, v)).encode())
    if route == "wave":
        knob("wave_min", 0)
    for flags in FLAGS:
        bad = _compare(fl, msgs, flags, NO_WAVE if route == "lane" else 0)
        assert not bad, (route, hex(flags), len(bad), bad[:4])


@pytest.mark.parametrize("root", ["double", "i64"])
@pytest.mark.parametrize("route", ["wave", "lane", "hybrid"])
def test_j2t_tokens_as_root_scalar(root, route, knob):
    """The message is the token: it ends where the message ends, and the last
    one where the batch ends."""
    fl = T.flatten(T.builtin(root))
    toks = [t for _, t in thinned()]
    if route == "wave":
        knob("wave_min", 0)
    for flags in FLAGS:
        for k, last in enumerate((toks[0], "9007199254740993", "1.5", "12345678901234567890.5", "1e", "-")):
            head = toks if k == 0 else toks[:40]  # the whole set once; then only the batch's end changes
            msgs = [t.encode() for t in head] + [last.encode()]
            bad = _compare(fl, msgs, flags, NO_WAVE if route == "lane" else 0)
            assert not bad, (root, route, hex(flags), last, len(bad), bad[:4])


# ---------------------------------------------------------------- t2j ----

@pytest.fixture(scope="module")
def t2j_chk():
    o = oracle.RefT2JOracle()
    if o is None:
        pytest.skip("oracle/_ref not built")
    return o


WIRE = {"double": (4, ">d"), "i64": (10, ">q"), "i32": (8, ">i"), "i16": (6, ">h"), "byte": (3, ">b")}


def _wrap(v, bits):
    """v modulo 2^bits as a signed value: what the narrow field holds."""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _values(kind):
    if kind == "double":
        return [v for _, v in numgen.t2j_doubles()]
    bits = {"i64": 64, "i32": 32, "i16": 16, "byte": 8}[kind]
    return [_wrap(v, bits) for v in numgen.t2j_ints()]


def _list_msgs(kind, per=40):
    tt, fmt = WIRE[kind]
    vals = _values(kind)
    return [b"\x0f\x00\x01" + bytes([tt]) + struct.pack(">i", len(vals[a:a + per])) +
            b"".join(struct.pack(fmt, v) for v in vals[a:a + per]) + b"\x00" for a in range(0, len(vals), per)]


@pytest.mark.parametrize("kind", list(WIRE))
@pytest.mark.parametrize("wmin", [0, 1], ids=["lane", "wave"])
def test_t2j_lists(t2j_chk, kind, wmin, knob):
    knob("t2j_wave_min", wmin)
    fl = T.flatten(T.struct_type("L", [T.FieldDescriptor(1, "v", T.list_of(T.builtin(kind)), T.OPTIONAL)]))
    msgs = _list_msgs(kind)
    for opts in (0, I64S, NULLNAN):
        bad = compare(t2j_chk, fl, msgs, opts)
        assert not bad, (kind, wmin, opts, len(bad), bad[:3])


@pytest.mark.parametrize("kind", list(WIRE))
@pytest.mark.parametrize("wmin", [0, 1], ids=["lane", "wave"])
def test_t2j_single_values(t2j_chk, kind, wmin, knob):
    """Each value alone in a one-field struct, 64 messages a batch: every
    value at the start of an output slot (the lane writer's pair phase, the
    wave kernel's first page) as well as in mid-stream above."""
    knob("t2j_wave_min", wmin)
    fl = T.flatten(T.struct_type("S", [T.FieldDescriptor(1, "v", T.builtin(kind), T.OPTIONAL)]))
    tt, fmt = WIRE[kind]
    msgs = [bytes([tt]) + b"\x00\x01" + struct.pack(fmt, v) + b"\x00" for v in _values(kind)]
    for opts in (0, I64S, NULLNAN):
        for a in range(0, len(msgs), 64):
            bad = compare(t2j_chk, fl, msgs[a:a + 64], opts)
            assert not bad, (kind, wmin, opts, a, len(bad), bad[:3])
