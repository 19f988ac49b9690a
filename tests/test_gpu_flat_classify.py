"""GPU: the flat kernel's structure phase (fl_classify.h in j2t_flat.h) where
its masks can go wrong: a delimiter on either side of a 64-byte lane border or
of a dword / dword-pair border, a message at every arena alignment, string
bodies of the class bytes' +1 neighbours and high-bit twins, escapes across a
lane border. Exact against the oracle, and the well-formed messages must stay
on the flat kernel: a misclassified message would decline to the list pass,
which converts it correctly and would hide the fault."""
import random
import re

import pytest

from dynamicgo_amd import conv, thrift as T, workloads as W
from test_gpu_flat import FLAT, _compare

pytestmark = pytest.mark.gpu


def five_desc():
    return T.struct_type("Five", [T.FieldDescriptor(k + 1, c, T.builtin("string"), T.OPTIONAL)
                                  for k, c in enumerate("abcde")] +
                         [T.FieldDescriptor(6, "z", T.builtin("binary"), T.OPTIONAL)])


def _simple(body):
    return b'{"StringField":"' + body + b'","I32Field":7}'


def _five(body):
    return b'{"a":"' + body + b'","b":"q","z":"QUJD"}'


SHAPES = [(W.simple_desc, _simple), (five_desc, _five)]


FL_MAXTASK = 320  # j2t_flat.h: a block of 64 messages with more chunk tasks declines some (test_gpu_flat_tasks.py)


def _spread(msgs):
    """long and short messages alternate, so that no block of 64 holds only long strings"""
    s = sorted(msgs, key=len)
    return [s[i // 2] if i % 2 == 0 else s[len(s) - 1 - i // 2] for i in range(len(s))]


def _exact_and_flat(fl, msgs):
    assert len(msgs) <= 512 and max(map(len, msgs)) <= 256
    for b in range(0, len(msgs), 64):  # a body over 8 bytes is a chunk task per 32 bytes: every block within the cap
        bodies = [v for m in msgs[b:b + 64] for v in re.findall(rb':"((?:[^"\\]|\\.)*)"', m)]
        assert sum((len(v) + 31) // 32 for v in bodies if len(v) > 8) <= FL_MAXTASK, b
    ctx = conv.default_context()
    ctx.stats(reset=True)
    bad = _compare(fl, msgs, 0x1 | FLAT)
    bails, _ = ctx.stats(reset=True)
    assert not bad, (len(bad), bad[:4])
    assert bails == 0, bails


@pytest.mark.parametrize("shape", [0, 1], ids=["simple", "five"])
def test_delimiters_cross_every_lane_and_dword_border(shape):
    """A string grown a byte at a time: its closing quote, the comma, the next
    key's quotes and its colon each stand at 63 and 64, 127 and 128, 191 and
    192, and at every position mod 8."""
    td, make = SHAPES[shape]
    fl = T.flatten(td())
    room = 256 - len(make(b""))
    msgs = [make(b"a" * k) for k in range(room + 1)]
    quote = {m.index(b'","') for m in msgs}  # the closing quote; the comma, the key and the colon follow it
    assert {63, 64, 127, 128, 191, 192} <= quote and {p % 8 for p in quote} == set(range(8))
    _exact_and_flat(fl, _spread(msgs))


def test_every_arena_alignment():
    """The message starts at each arena offset mod 8 (the length of the
    message before it), with delimiters on both sides of each lane border."""
    fl = T.flatten(W.simple_desc())
    probes = [_simple(b"a" * k) for k in (0, 9, 46, 47, 48, 49, 110, 111, 112, 113, 174, 175, 176, 177)]
    msgs, at, seen = [], 0, set()
    for a in range(8):
        for p in probes:
            fill = b'{"ByteField":1}'
            fill += b" " * ((a - at - len(fill)) % 8)
            msgs += [fill, p]
            at += len(fill)
            seen.add((at % 8, len(p)))
            at += len(p)
    assert seen == {(a, len(p)) for a in range(8) for p in probes}
    _exact_and_flat(fl, msgs)


@pytest.mark.parametrize("shape", [0, 1], ids=["simple", "five"])
def test_neighbour_and_high_bit_twin_bodies(shape):
    """Bodies of the class bytes + 1 (# - ; ]), of their twins with bit 7 set
    (0xA2 0xAC 0xBA 0xDC, as valid UTF-8) and of commas and colons inside the
    string: none is a delimiter."""
    td, make = SHAPES[shape]
    fl = T.flatten(td())
    rng = random.Random(7100 + shape)
    pieces = ["#", "-", ";", "]", "¢", "¬", "º", "ܢ", "ܬ", "ܺ", ",", ":", "a"]
    assert {b for p in pieces for b in p.encode()} >= {0x23, 0x2D, 0x3B, 0x5D, 0xA2, 0xAC, 0xBA, 0xDC, 0x2C, 0x3A}
    room = 256 - len(make(b""))
    msgs = []
    for p in pieces:  # each alone, at every seventh length
        for k in range(0, room // len(p.encode()) + 1, 7):
            msgs.append(make((p * k).encode()))
    while len(msgs) < 512:
        body = b""
        want = rng.randint(0, room)
        while True:
            nx = rng.choice(pieces).encode()
            if len(body) + len(nx) > want:
                break
            body += nx
        msgs.append(make(body))
    _exact_and_flat(fl, _spread(msgs[:512]))


def test_escapes_straddle_each_lane_border():
    """A simple escape and a \\u escape with every split of their bytes
    across bytes 63/64, 127/128 and 191/192, and wholly on either side."""
    fl = T.flatten(W.simple_desc())
    head = len(b'{"StringField":"')
    msgs = []
    for esc in (b"\\n", b"\\u00e9", b"\\u4e2d"):
        for border in (64, 128, 192):
            for start in range(border - len(esc), border + 1):
                msgs.append(_simple(b"a" * (start - head) + esc + b"bc"))
                msgs.append(_simple(b"a" * (start - head) + esc))
    _exact_and_flat(fl, msgs)
