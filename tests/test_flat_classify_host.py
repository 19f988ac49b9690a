"""CPU: the flat kernel's structure-phase classification (fl_classify.h), built
for the host by flat_classify_host.cpp, against a byte-at-a-time model.

Every byte value at every one of the 64 positions, over backgrounds of 'a',
the four class bytes (quote, comma, colon, backslash), their +1 neighbours,
their high-bit twins, 0x00 and 0xFF: the flag formula is exact only if a match
never flags the byte beside it and a byte >= 0x80 never matches. Then 10^5
random blocks over that alphabet, and the flag and pack routines on their own.

The same file built alone with -DCLS_MAIN under ASan + UBSan runs the
exhaustive part from heap blocks of exactly 64 bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = (0x22, 0x2C, 0x3A, 0x5C)  # Q C K B, the order of cls_blocks' columns
ALPHABET = [ord("a"), *CLASSES, 0x23, 0x2D, 0x3B, 0x5D, 0xA2, 0xAC, 0xBA, 0xDC, 0x00, 0xFF]


def build_cls(out, extra=()):
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC",
                    "-Wno-ignored-attributes", *extra, "-o", out, os.path.join(HERE, "flat_classify_host.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the classification with" % B.HIPCC)
    lib = C.CDLL(build_cls(str(tmp_path_factory.mktemp("cls") / "libcls.so"), ("-shared",)))
    lib.cls_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.cls_blocks.restype = C.c_uint64
    lib.cls_eq.argtypes = [C.c_uint32, C.c_uint32]
    lib.cls_eq.restype = C.c_uint32
    lib.cls_pack8.argtypes = [C.c_uint32, C.c_uint32]
    lib.cls_pack8.restype = C.c_uint32
    return lib


def model(blocks):
    """[n, 5]: the four masks a byte at a time (bit b = byte b), and whether a backslash is there"""
    bit = np.uint64(1) << np.arange(64, dtype=np.uint64)
    out = np.zeros((len(blocks), 5), dtype=np.uint64)
    for k, c in enumerate(CLASSES):
        out[:, k] = ((blocks == c) * bit).sum(axis=1, dtype=np.uint64)
    out[:, 4] = out[:, 3] != 0
    return out


def run(lib, blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    out = np.zeros((len(blocks), 5), dtype=np.uint64)
    assert lib.cls_blocks(blocks.ctypes.data, len(blocks), out.ctypes.data) == 0  # with and without the backslash mask
    return out


def test_every_byte_at_every_position_over_every_background(lib):
    vals = np.arange(256, dtype=np.uint8)
    for bg in ALPHABET:
        blocks = np.full((64, 256, 64), bg, dtype=np.uint8)
        for p in range(64):
            blocks[p, :, p] = vals
        blocks = blocks.reshape(-1, 64)
        got, want = run(lib, blocks), model(blocks)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (hex(bg), len(bad), [(int(i) // 256, int(i) % 256) for i in bad[:6]])


def test_random_blocks_over_the_alphabet(lib):
    rng = np.random.default_rng(20250)
    blocks = np.array(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), size=(100000, 64))]
    got, want = run(lib, blocks), model(blocks)
    assert (got == want).all(), int((got != want).any(axis=1).sum())
    assert (want[:, :4] != 0).any(axis=0).all() and (want[:, 4] == 0).any()  # every mask is exercised


def test_flag_and_pack_on_their_own(lib):
    """fl_eq on every byte at every position beside every alphabet neighbour;
    fl_pack8 on all 256 flag patterns: byte i of the pair at bit 7 + i."""
    for c in CLASSES:
        cc = c * 0x01010101
        for nb in ALPHABET:
            for p in range(4):
                for v in range(256):
                    x = (nb * 0x01010101 & ~(0xFF << 8 * p)) | v << 8 * p
                    want = sum(0x80 << 8 * i for i in range(4) if (x >> 8 * i) & 0xFF == c)
                    assert lib.cls_eq(x, cc) == want, (hex(c), hex(x))
    for pat in range(256):
        f0 = sum(0x80 << 8 * i for i in range(4) if pat >> i & 1)
        f1 = sum(0x80 << 8 * i for i in range(4) if pat >> (4 + i) & 1)
        assert lib.cls_pack8(f0, f1) == pat << 7, pat


def test_sanitizer_program_reports_nothing(tmp_path):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s" % B.HIPCC)
    exe = build_cls(str(tmp_path / "cls_main"), ("-DCLS_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                                 "-fno-sanitize-recover=undefined"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        (r.returncode, r.stderr[-2000:])
    assert r.stdout.startswith("%d blocks, 0 bad" % (len(ALPHABET) * 64 * 256)), r.stdout
