"""CPU: the lane writers themselves -- Out (dynamicgo_amd/csrc/j2t_device.h)
and JOut (t2j_device.h), the code the small, lane and exact-machine kernels
and the t2j lane pass store through -- built for the host by jout_host.cpp and
compared with a byte-at-a-time model: after any sequence of wle / w8 /
set_len and a finish, the buffer holds bytes [0, min(len, cap)) of the logical
output, `len` is the logical length, and nothing outside [base, base + cap)
was stored to. Every cap from 0 to 48, at an 8-aligned base in both 16-byte
phases (JOut's pair stores start 8 bytes before the word that completes a
pair) and at unaligned bases (wide == false: byte stores)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
WLE, W8, SET_LEN, FINISH = range(4)
GUARD = 32
FILL = 0xC3
OUT, JOUT = 0, 1


def build_jout(out, extra=()):
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC",
                    "-Wno-ignored-attributes", *extra, "-o", out, os.path.join(HERE, "jout_host.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def jout(tmp_path_factory):
    """jout(which, base_mod16, cap, ops) -> (len, the cap bytes, front guard, back guard)"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host writers with" % B.HIPCC)
    lib = C.CDLL(build_jout(str(tmp_path_factory.mktemp("jout") / "libjout.so"), ("-shared",)))
    lib.jout_run.restype = C.c_uint64
    lib.jout_run.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]

    def run(which, mod16, cap, ops):
        raw = np.full(2 * GUARD + cap + 32, FILL, dtype=np.uint8)
        lo = (-(raw.ctypes.data + GUARD) + mod16) % 16  # base = data + lo + GUARD is mod16 (mod 16)
        base = raw.ctypes.data + lo + GUARD
        assert base % 16 == mod16
        o = np.array(ops, dtype=np.uint64).reshape(-1, 3)
        n = int(lib.jout_run(which, base, cap, o.ctypes.data, len(o)))
        return n, raw[lo + GUARD:lo + GUARD + cap].tobytes(), raw[:lo + GUARD].tobytes(), raw[lo + GUARD + cap:].tobytes()

    return run


def model(ops):
    """The logical output, one byte at a time."""
    out = bytearray()
    for op, a, v in ops:
        if op == WLE:
            out += bytes((v >> (8 * j)) & 0xFF for j in range(a))
        elif op == W8:
            out.append(v & 0xFF)
        elif op == SET_LEN:
            assert a <= len(out)
            del out[a:]
    return bytes(out)


def random_ops(rng, max_ops):
    ops, n = [], 0
    for _ in range(rng.randint(1, max_ops)):
        r = rng.random()
        if r < 0.15 and n:
            x = rng.randint(0, n)
            ops.append((SET_LEN, x, 0))
            n = x
        elif r < 0.3:
            ops.append((W8, 1, rng.randrange(256)))
            n += 1
        else:
            k = rng.randint(1, 8)
            ops.append((WLE, k, rng.getrandbits(64)))  # the bytes past k must not get out
            n += k
    return ops + [(FINISH, 0, 0)]


def check(jout, which, mod16, cap, ops):
    want = model(ops)
    n, buf, front, back = jout(which, mod16, cap, ops)
    keep = min(len(want), cap)
    what = ("JOut" if which else "Out", mod16, cap, ops)
    assert n == len(want), what
    assert buf[:keep] == want[:keep], what
    assert front == bytes([FILL]) * len(front) and back == bytes([FILL]) * len(back), what


@pytest.mark.parametrize("which", [OUT, JOUT], ids=["Out", "JOut"])
@pytest.mark.parametrize("mod16", [0, 8, 1, 4, 7, 9, 12, 15])
def test_seeded_sequences_every_cap(jout, which, mod16):
    rng = random.Random(100 * which + mod16)
    over = tight = total = 0
    for cap in range(49):
        for _ in range(12):
            ops = random_ops(rng, 12)
            need = len(model(ops))
            over += need > cap
            tight += 0 <= cap - need < 8
            total += 1
            check(jout, which, mod16, cap, ops)
    assert over * 4 >= total and tight * 20 >= total, (over, tight, total)


@pytest.mark.parametrize("which", [OUT, JOUT], ids=["Out", "JOut"])
@pytest.mark.parametrize("mod16", [0, 8, 3])
def test_every_length_against_every_cap(jout, which, mod16):
    """A plain run of n bytes (as 8-byte and shorter writes, and byte by
    byte) for every n and cap up to 48: cap - need takes every value from -48
    to 48, so each store sits at every distance from the slot's end."""
    for n in range(49):
        body = [(WLE, 8, 0x0807060504030201 + 0x0808080808080808 * k) for k in range(n // 8)]
        if n % 8:
            body.append((WLE, n % 8, 0xF7F6F5F4F3F2F1F0))
        single = [(W8, 1, 0x30 + j) for j in range(n)]
        for cap in range(49):
            check(jout, which, mod16, cap, body + [(FINISH, 0, 0)])
            check(jout, which, mod16, cap, single + [(FINISH, 0, 0)])


@pytest.mark.parametrize("which", [OUT, JOUT], ids=["Out", "JOut"])
@pytest.mark.parametrize("mod16", [0, 8, 5])
def test_truncation_to_every_length(jout, which, mod16):
    """set_len(x) for every x <= len, then more bytes: the words (JOut: the
    pairs) already stored are taken back, those still held are kept."""
    for n in (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 33, 40):
        first = [(W8, 1, 0x41 + j % 26) for j in range(n)]
        for x in range(n + 1):
            for more in (0, 1, 8, 17):
                ops = first + [(SET_LEN, x, 0)] + [(W8, 1, 0x61 + j % 26) for j in range(more)] + [(FINISH, 0, 0)]
                for cap in (0, x, max(x - 1, 0), x + more, x + more + 1, n, 48):
                    check(jout, which, mod16, cap, ops)
