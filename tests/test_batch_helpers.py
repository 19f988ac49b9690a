"""dynamicgo_amd/_batch.py without a GPU: the arena, the retry, the split."""
import ctypes as C

import numpy as np
import pytest

from dynamicgo_amd import _batch, _lib


def test_arena_and_split():
    msgs = [b"ab", b"", b"cde"]
    a, off = _batch.arena(msgs)
    assert a.tobytes() == b"abcde" + bytes(16) and off.dtype == np.uint64 and off.tolist() == [0, 2, 2, 5]
    assert _batch.split(a, off) == msgs
    a, off = _batch.arena([])
    assert a.tobytes() == bytes(16) and off.tolist() == [0] and _batch.split(a, off) == []


def test_until_fits_retries_at_exactly_need():
    need, caps = C.c_uint64(0), []

    def call(cap):  # an entry that needs 100, then finds it needs 130
        caps.append(cap)
        need.value = 100 if cap < 100 else 130
        return (-3 if cap < need.value else 0), cap

    assert _batch.until_fits(call, 10, need) == 130 and caps == [10, 100, 130]
    with pytest.raises(_lib.DGError):  # DG_E_NOMEM without a larger need is an error, not a loop
        _batch.until_fits(lambda cap: (-3, cap), 200, need)
