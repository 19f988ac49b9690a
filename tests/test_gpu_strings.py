"""GPU: string unquote, quote and base64 both ways on the corpora of strgen.py
(validated on the CPU by test_strings_oracle.py and test_str_host.py), byte
for byte and status word for status word against the compiled reference (the
C restatement when oracle/_ref is absent, and for DG_F_VALIDATE_UTF8, which is
the restatement's alone).

j2t: every item as a STRING or binary field of a flat struct, before a ','
and before a '}', on each route -- flat, small, wave (both instances, also
behind a 600-byte pad field), lane, exact and the default routing -- under
flags 0x1, 0x41 (NO_BASE64) and 0x1 | VALIDATE_UTF8, with the bail counters
saying that what the fast routines must decline went to the exact machine and
the rest did not; then as map keys, struct keys, map values and list elements,
as a STRING root, and with escaped keys round the lane's key buffer.

t2j: every byte string alone, in lists, as map key and value and as a binary,
on the lane kernel at spread 1, 2 and 4 and on the wave kernel; and both round
trips."""
import os
import struct
import tempfile
import time

import numpy as np
import pytest

import oracle
import strgen
import test_strings_oracle as M
from dynamicgo_amd import conv, thrift as T
from test_gpu_parity import _raw_batch
from test_gpu_t2j import gpu_t2j

pytestmark = pytest.mark.gpu

NO_FAST, NO_WAVE, FLAT, NO_FLAT = 1 << 17, 1 << 18, 1 << 19, 1 << 21
F_STR, F_NOB64, F_UTF8 = M.F_STR, M.F_NOB64, M.F_UTF8
FLAGS = (F_STR, F_NOB64, F_UTF8)
NOB64_T2J = M.NOB64_T2J
FAR = 1 << 30  # wave_min: no message is long enough for the wave kernel
WS_KEYCAP, DEEP_KEYCAP, FL_NESC = 1024, 1 << 20, 8
DG_ST_DEEP, ERR_OOM_KEY = 0xF1, 18


def _chk(flags):
    return oracle.PortOracle() if flags >> 16 else (oracle.RefOracle() or oracle.PortOracle())


_HOST = []


def _host_lib():
    """test_str_host's build of the routines (for str_class); None only where
    there is no compiler. A failed import or build fails the test."""
    if not _HOST:
        import test_str_host as H
        if not os.path.exists(H.B.HIPCC):
            _HOST.append(None)
        else:
            _HOST.append(H.Str(H.build_str(os.path.join(tempfile.mkdtemp(), "libstr.so"), ("-shared",))))
    return _HOST[0]


class Corpus:
    """One route's batch (route_messages of the thinned corpus), what the
    reference makes of it (once per flag word), and how many of its messages
    the fast routines must decline."""

    def __init__(self, pad):
        items = M.route_items()
        self.rows = M.route_messages(items[::3] if pad else items, pad)
        self.msgs = [m for _, _, m in self.rows]
        self.fl = T.flatten(M.str_desc())
        self.want = {}
        self._decline = {}

    def expected(self, flags):
        if flags not in self.want:
            self.want[flags] = _chk(flags).j2t_batch(self.fl, self.msgs, flags, nthreads=8)
        return self.want[flags]

    def must_decline(self, flags):
        """Messages whose string the fast routines decline (str_class of the
        host build: a decline bit, or an unclosed string); without a compiler,
        the messages that end in an error."""
        if flags in self._decline:
            return self._decline[flags]
        lib = _host_lib()
        if lib is None:
            n = int(np.count_nonzero(self.expected(flags)[0]))
        else:
            import test_str_host as H
            n = 0
            for it, field, m in self.rows:
                binary = field == "bin" and not flags & 0x40
                s = m.index(b'"' + field.encode() + b'":"') + len(field) + 4
                k = lib.cls(m, s, binary)
                n += k == H.UNCLOSED or bool(k & (H.B_DECLINES if binary else H.U_DECLINES))
        self._decline[flags] = n
        return n

    def bad(self, flags, extra):
        rets, outs = self.expected(flags)
        got, gr = _raw_batch(self.fl, self.msgs, flags | extra)
        return [(i, self.rows[i][0].fam, self.msgs[i][:70], hex(int(gr[i])), hex(int(rets[i])))
                for i in range(len(self.msgs)) if int(gr[i]) != int(rets[i]) or got[i] != outs[i]]


@pytest.fixture(scope="module")
def corpus():
    return Corpus(False)


@pytest.fixture(scope="module")
def padded():
    return Corpus(True)


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
def test_j2t_items_in_fields(corpus, padded, route, knob):
    extra, knobs = ROUTES[route]
    for k, v in knobs.items():
        knob(k, v)
    ctx = conv.default_context()
    t0 = time.time()
    for cp in (corpus, padded) if route.startswith("wave") or route == "hybrid" else (corpus,):
        n = len(cp.msgs)
        for flags in FLAGS:
            ctx.stats(reset=True)
            bad = cp.bad(flags, extra)
            bails, _ = ctx.stats(reset=True)
            errors = int(np.count_nonzero(cp.expected(flags)[0]))
            print("%s flags %#x: %d messages, %d bails, %d errors" % (route, flags, n, bails, errors))
            assert not bad, (route, hex(flags), len(bad), bad[:4])
            if flags >> 16:
                # the extension is outside the fast kernels' flag set: the exact machine takes every
                # message on every route, and nothing is counted as a bail
                assert bails == 0, (route, hex(flags), bails)
            elif route in ("flat", "small"):
                # every decline of these kernels is a bail; wave_min keeps the long messages here too
                must = cp.must_decline(flags)
                assert bails >= must, (route, hex(flags), bails, must)
                assert bails * 2 < n, (route, hex(flags), bails, n)
            elif route.startswith("wave"):
                # only the messages that end in an error must be redone by the exact machine
                assert bails >= errors, (route, hex(flags), bails, errors)
                assert bails * 2 < n, (route, hex(flags), bails, n)
    # the count family over a key and two values: FL_NESC is a message's, not a string's
    cm = strgen.count_messages()
    msgs = [m for m, _, _ in cm]
    fl = corpus.fl
    for flags in FLAGS:
        want_r, want_o = _chk(flags).j2t_batch(fl, msgs, flags, nthreads=4)
        assert not np.count_nonzero(want_r)
        ctx.stats(reset=True)
        got, gr = _raw_batch(fl, msgs, flags | extra)
        bails, _ = ctx.stats(reset=True)
        bad = [(msgs[i], hex(int(gr[i]))) for i in range(len(msgs)) if int(gr[i]) or got[i] != want_o[i]]
        assert not bad, (route, hex(flags), len(bad), bad[:4])
        kept = sum(k for _, _, k in cm)
        print("%s flags %#x: %d count messages, %d bails, %d kept" % (route, flags, len(msgs), bails, kept))
        if route == "flat" and not flags >> 16:
            # the table declines more than FL_NESC backslashes (9 and 10 of the kept kinds among them), an
            # escaped key, \\" and surrogates, and keeps the rest: both bounds, so the count is exact
            assert bails >= len(msgs) - kept, (hex(flags), bails, len(msgs) - kept)
            assert bails <= len(msgs) - kept, (hex(flags), bails, len(msgs) - kept)
    print("%s: %.2f s" % (route, time.time() - t0))


def test_flat_kernel_keeps_the_escapes_its_table_holds(knob):
    """At most FL_NESC escapes, no surrogate, no invalid escape, no escaped
    key, no \\" or \\\\ (a backslash before a quote or a backslash declines in
    the structure phase): the flat kernel converts the message itself."""
    knob("wave_min", FAR)
    fl = T.flatten(M.str_desc())
    msgs = []
    for it in strgen.j2t_strings():
        if it.fam in ("esc", "uni", "phase", "count") and it.imp[0] == "ok" and b"\\ud" not in it.body.lower() and \
                b'\\"' not in it.body and b"\\\\" not in it.body and it.body.count(b"\\") <= FL_NESC:
            msgs += [M.wrap(it, "str", True)[0], M.wrap(it, "str", False)[0]]
    split = [m for m, _, kept in strgen.count_messages() if kept]
    # 7 and 8 backslashes over two values among them, each in three splits
    assert sum(m.count(b"\\") == 7 for m in split) == 3 and sum(m.count(b"\\") == FL_NESC for m in split) == 3
    msgs += split
    assert len(msgs) > 3000 and max(len(m) for m in msgs) < 200
    rets, outs = _chk(F_STR).j2t_batch(fl, msgs, F_STR, nthreads=8)
    assert not np.count_nonzero(rets)
    ctx = conv.default_context()
    ctx.stats(reset=True)
    got, gr = _raw_batch(fl, msgs, F_STR | FLAT)
    bails, _ = ctx.stats(reset=True)
    bad = [(msgs[i], hex(int(gr[i]))) for i in range(len(msgs)) if int(gr[i]) or got[i] != outs[i]]
    assert not bad, (len(bad), bad[:4])
    assert bails == 0, bails


def _compare(fl, msgs, flags, extra=0):
    rets, outs = _chk(flags).j2t_batch(fl, msgs, flags, nthreads=8)
    got, gr = _raw_batch(fl, msgs, flags | extra)
    return [(i, msgs[i][:70], hex(int(gr[i])), hex(int(rets[i])))
            for i in range(len(msgs)) if int(gr[i]) != int(rets[i]) or got[i] != outs[i]]


CONTAINER_ROUTES = {"wave": (0, {"wave_min": 0}), "lane": (NO_WAVE, {}), "exact": (NO_FAST, {}), "hybrid": (0, {})}


def _small_items():
    return [it for it in M.route_items() if it.fam in ("esc", "uni", "sur", "count", "raw", "b64len")]


@pytest.mark.parametrize("route", list(CONTAINER_ROUTES))
def test_j2t_items_in_containers(route, knob):
    """The keys family as map keys; esc, uni and sur as map values and list
    elements (and the base64 lengths as elements of a list<binary>)."""
    extra, knobs = CONTAINER_ROUTES[route]
    for k, v in knobs.items():
        knob(k, v)
    fl = T.flatten(M.cont_desc())
    msgs = M.container_messages(strgen.key_bodies()[::2] + _small_items()[::2])
    msgs += [b'{"lb":["' + it.body + b'","QUJD"]}' for it in strgen.j2t_b64() if it.fam in ("b64len", "b64bits")]
    assert 3000 < len(msgs) < 9000
    for flags in FLAGS:
        bad = _compare(fl, msgs, flags, extra)
        assert not bad, (route, hex(flags), len(bad), bad[:4])


@pytest.mark.parametrize("route", ["flat", "small", "wave-occ4", "lane", "exact", "hybrid"])
def test_j2t_items_as_struct_keys(route, knob):
    """Escaped keys that name a field once unquoted, that name none, and that
    end in each error class."""
    extra, knobs = ROUTES[route]
    for k, v in knobs.items():
        knob(k, v)
    fl = T.flatten(M.str_desc())
    msgs = M.key_messages(strgen.key_bodies())
    for flags in (F_STR, F_UTF8):
        bad = _compare(fl, msgs, flags, extra)
        assert not bad, (route, hex(flags), len(bad), bad[:4])


@pytest.mark.parametrize("route", ["wave", "lane", "hybrid"])
def test_j2t_string_root(route, knob):
    """The message is the string, quoted and unquoted: it ends where the
    message ends, and the last one where the batch ends."""
    fl = T.flatten(T.builtin("string"))
    if route == "wave":
        knob("wave_min", 0)
    items = _small_items() + [it for it in M.route_items() if it.fam == "phase"][::4]
    for flags in FLAGS:
        for last in (b'"a\\n"', b'"\\ud83d\\ude00"', b'"abc\\', b'"\\u00e', b"plain", b'"'):
            msgs = M.root_messages(items if last == b'"a\\n"' else items[:40]) + [last]
            bad = _compare(fl, msgs, flags, NO_WAVE if route == "lane" else 0)
            assert not bad, (route, hex(flags), last, len(bad), bad[:4])


def test_long_strings_on_the_wave_kernel(knob):
    """The wave page's escape count shortcut (16 383 simple escapes: cn =
    32 766, applies; one more byte, or 16 384 escapes: not), one escape in
    33 000 bytes, and escapes across the 256-byte scan chunks, on both
    instances and behind a pad."""
    fl = T.flatten(M.str_desc())
    rows = M.route_messages(strgen.long_strings()) + M.route_messages(strgen.long_strings()[4:], pad=True)
    msgs = [m for _, _, m in rows]
    assert max(len(m) for m in msgs) < 34000
    for occ in (4, 5):
        knob("wave_min", 0)
        knob("wave_occ", occ)
        for flags in (F_STR, F_NOB64):
            bad = _compare(fl, msgs, flags)
            assert not bad, (occ, hex(flags), len(bad), bad[:3])


# ------------------------------------------------------- escaped keys ----

@pytest.mark.parametrize("route", ["lane", "exact", "hybrid"])
def test_escaped_keys_round_the_key_buffer(route, knob):
    """Escaped keys of unquoted length 1023, 1024, 1025 and 2048 as a map key
    and as an unknown field name: like the reference, and the deep pass takes
    exactly the messages whose key outgrows the lane's buffer (WS_KEYCAP)."""
    extra = {"lane": NO_WAVE, "exact": NO_FAST, "hybrid": 0}[route]
    ctx = conv.default_context()
    keys = strgen.long_keys()
    for fl, msgs in ((T.flatten(M.cont_desc()), [b'{"ms":{"' + it.body + b'":"v"},"str":"s"}' for it in keys]),
                     (T.flatten(M.str_desc()), [b'{"' + it.body + b'":"v","req":1}' for it in keys])):
        ctx.stats(reset=True)
        bad = _compare(fl, msgs, F_STR, extra)
        _, deeps = ctx.stats(reset=True)
        assert not bad, (route, len(bad), bad[:3])
        assert deeps == sum(len(it.imp[1]) > WS_KEYCAP for it in keys), (route, deeps)


def test_escaped_key_past_the_deep_key_buffer():
    """One escaped key that unquotes to more than DEEP_KEYCAP (1 MiB): the
    deep pass's buffer overflows too. The reference grows its key cache on
    ERR_OOM_KEY and converts the message; the library's buffers are fixed, so
    the message ends with that code (18), value = the key's JSON bytes beyond
    the buffer, and never with the internal DG_ST_DEEP."""
    fl = T.flatten(M.cont_desc())
    key = b"\\n" + b"k" * DEEP_KEYCAP
    msgs = [b'{"ms":{"a":"b"}}', b'{"ms":{"' + key + b'":"v"}}', b'{"str":"x"}']
    got, gr = _raw_batch(fl, msgs, F_STR | NO_WAVE)
    rets, outs = _chk(F_STR).j2t_batch(fl, msgs, F_STR)
    assert (int(gr[0]), got[0]) == (int(rets[0]), outs[0]) and (int(gr[2]), got[2]) == (int(rets[2]), outs[2])
    assert int(rets[1]) == 0  # the reference converts it
    print("status of the message with a key past DEEP_KEYCAP: %#x" % int(gr[1]))
    assert int(gr[1]) & 0xFF != DG_ST_DEEP, hex(int(gr[1]))
    assert int(gr[1]) == ERR_OOM_KEY | (len(key) - DEEP_KEYCAP) << 8, hex(int(gr[1]))


# ---------------------------------------------------------------- t2j ----

T2J_ROUTES = {"lane-1": {"t2j_wave_min": 0, "t2j_spread": 1}, "lane-2": {"t2j_wave_min": 0, "t2j_spread": 2},
              "lane-4": {"t2j_wave_min": 0, "t2j_spread": 4}, "wave": {"t2j_wave_min": 1}, "wave-default": {}}
PADSTR = b"p" * 600


def _t2j_cases(pad):
    """[(thrift, JSON under 0, JSON under NO_BASE64)] of every t2j item; pad:
    behind a 600-byte string field (past the wave kernel's default threshold)."""
    out = []
    for it in strgen.t2j_strings() + strgen.t2j_binaries():
        for m, j0, j1 in M.t2j_messages(it):
            if pad:
                m = b"\x0b\x00\x05" + struct.pack(">i", 600) + PADSTR + m
                if b"\x0b\x00\x05" in m[607:]:
                    continue  # qtail's own "nx" field: one per message
                j0, j1 = (b'{"nx":"' + PADSTR + b'",' + j[1:] for j in (j0, j1))
            out.append((m, j0, j1))
    return out


@pytest.mark.parametrize("route", list(T2J_ROUTES))
def test_t2j_items(route, knob):
    for k, v in T2J_ROUTES[route].items():
        knob(k, v)
    fl = T.flatten(M.t2j_desc())
    cases = _t2j_cases(route == "wave-default")
    if route == "wave-default":
        cases = cases[::2]
    chk = oracle.RefT2JOracle()
    side = T.flatten_t2j(fl)
    for opts, col in ((0, 1), (NOB64_T2J, 2)):
        outs, rets = gpu_t2j(fl, [c[0] for c in cases], opts)
        bad = [(c[0][:40], o[:60], c[col][:60], hex(int(r))) for c, o, r in zip(cases, outs, rets)
               if int(r) != 0 or o != c[col]]
        assert not bad, (route, opts, len(bad), bad[:4])
        if chk is not None:  # the constructed text is the reference's (all of it on the CPU; a sample here)
            for c in cases[::97]:
                assert chk.t2j(fl, side, c[0], opts) == (0, c[col])


def test_round_trips(knob):
    """t2j of j2t's output and j2t of t2j's output, for every well-formed item."""
    fs, ft = T.flatten(M.str_desc()), T.flatten(M.t2j_desc())
    rows = [r for r in M.route_messages(M.route_items()) if r[0].imp and r[0].imp[0] == "ok" and r[0].fam != "long"
            and r[2].endswith(b'"}')]
    rows = [r for r in rows if (r[0].fam in M.B64_FAMILIES) == (r[1] == "bin")]
    thr, rets = _raw_batch(fs, [m for _, _, m in rows], F_STR)
    assert not np.count_nonzero(rets)
    js, jr = gpu_t2j(fs, thr, 0)
    for (it, field, m), j, r in zip(rows, js, jr):
        text = M.m_b64encode(it.imp[1]) if field == "bin" else M.m_quote(it.imp[1])
        assert int(r) == 0 and j == b'{"req":1,"' + field.encode() + b'":' + text + b"}", (m[:60], j[:60])
    cases = [c for it in strgen.t2j_strings() + strgen.t2j_binaries() for c in M.t2j_messages(it)]
    for opts, flags, col in ((0, F_STR, 1), (NOB64_T2J, F_NOB64, 2)):
        js, jr = gpu_t2j(ft, [c[0] for c in cases], opts)
        assert not np.count_nonzero(jr)
        back, br = _raw_batch(ft, js, flags)
        bad = [(c[0][:40], j[:60], b[:40], hex(int(r))) for c, j, b, r in zip(cases, js, back, br)
               if int(r) != 0 or b != c[0]]
        assert not bad, (opts, len(bad), bad[:4])
