"""CPU: the offset arithmetic of tests/faroff.py. Nothing is allocated."""
import numpy as np
import pytest

import faroff as F

LENS = {
    "mixed": [5, 0, 1, 17, 300, 0, 4, 1, 64, 9],
    "ones": [1] * 12 + [4] + [1] * 12,
    "with-long": [12, 40, 7, 70000, 9, 9, 0, 33],
    "tight-slots": [0, 8, 16, 24, 8, 0, 8, 128, 8],
}


def pivot_of(lens):
    """the first message past the middle that is long enough to straddle with delta = -3"""
    return next(i for i in range(len(lens) // 2, len(lens)) if lens[i] > 3)


@pytest.mark.parametrize("name", list(LENS))
@pytest.mark.parametrize("delta", [0, -3])
@pytest.mark.parametrize("B", F.BOUNDS)
def test_place(B, delta, name):
    lens = LENS[name]
    p = pivot_of(lens)
    off = F.place(lens, B, p, delta)
    assert off.dtype == np.int64 and len(off) == len(lens) + 1
    assert np.diff(off).tolist() == lens
    assert off[p] == B + delta
    assert (off[1:p + 1] <= B).all() and (off[p + 1:] > B).all()
    if delta:
        assert off[p] < B < off[p + 1]
    for guard, tail in ((F.GUARD, 0), (0, F.TAIL)):
        wins = F.check_layout(off, B, guard, tail)
        assert wins[0][:2] == ("real", 0) and wins[0][2] == off[0] - guard and wins[0][3] == off[-1] + guard + tail
        assert len(wins) == (3 if B == 2 ** 32 else 2)
        for _, shift, lo, hi in wins[1:]:
            assert shift in (-2 ** 32, -2 ** 31) and lo < hi


@pytest.mark.parametrize("B", F.BOUNDS)
def test_aliases_are_what_32_bit_arithmetic_gives(B):
    """every offset of a window at or past 2^31: its uint32 / sign-extended
    int32 value, and for B = 2^32 its value mod 2^31, lies in an alias window
    at the same distance from the window's start"""
    off = F.place([40, 3, 9, 200, 1], B, 2, -3)
    wins = F.windows(off, B, guard=F.GUARD)
    lo, hi = wins[0][2:]
    for o in sorted({lo, lo + 1, B - 1, B, B + 1, hi - 1} & set(range(lo, hi))):
        if o < 2 ** 31:
            continue
        slips = {int(np.int64(o).astype(np.int32))} if o < 2 ** 32 else {int(np.uint64(o).astype(np.uint32))}
        if B == 2 ** 32:
            slips.add(o % 2 ** 31)
        for s in slips:
            hit = [(sh, alo, ahi) for _, sh, alo, ahi in wins[1:] if alo <= s < ahi]
            assert len(hit) == 1 and hit[0][0] == s - o, (hex(o), hex(s), hit)
    assert F.alias_windows(64, 5000, B) == []  # a near window has no alias


def test_near():
    off = F.near([3, 0, 5])
    assert off.tolist() == [64, 67, 67, 72] and off.dtype == np.int64


def test_message_at():
    off = F.place([4, 6, 0, 2], 2 ** 32, 1, -3)
    assert F.message_at(off, int(off[0]) - 2).startswith("the front guard, 2 ")
    assert F.message_at(off, int(off[1]) + 3) == "message 1, slot byte 3 of 6"
    assert F.message_at(off, int(off[3])) == "message 3, slot byte 0 of 2"  # the empty message 2 holds no byte
    assert F.message_at(off, int(off[4]) + 1) == "the tail guard, +1"


@pytest.mark.parametrize("B", F.BOUNDS)
def test_wrong_placements_are_rejected(B):
    lens = [10, 20, 30, 40]
    good = F.place(lens, B, 2, -3)
    F.check_layout(good, B)
    with pytest.raises(AssertionError, match="straddles"):  # a boundary between two messages is fine; none here
        F.check_layout(good + 100, B)
    with pytest.raises(AssertionError, match="wholly below"):
        F.check_layout(F.place(lens, B, 0, -3), B)
    with pytest.raises(AssertionError, match="wholly above"):
        F.check_layout(F.place(lens[:3] + [0], B, 2, -3), B)
    with pytest.raises(AssertionError, match="leaves the arena"):  # a window reaching below arena byte 0
        F.check_layout(np.array([-F.PAD + 10, B - 3, B + 5, B + 9], dtype=np.int64), B)
    with pytest.raises(AssertionError, match="leaves the arena"):  # ... and one past its end
        F.check_layout(np.array([B - 40, B - 3, B + 5, 2 ** 32 + F.ROOM], dtype=np.int64), B)
    # an alias window overlapping the real one: a batch 2^31 (2^32) bytes long reaches its own alias
    far = 2 ** 31 if B == 2 ** 32 else 2 ** 32
    with pytest.raises(AssertionError, match="overlaps"):
        F.check_layout(np.array([B - far + F.GUARD, B - 3, B + 5, B + 9], dtype=np.int64), B)
    # a second window (a value arena) on an alias of the messages
    with pytest.raises(AssertionError, match="overlaps"):
        F.check_layout(good, B, others=[(int(good[3]) - 2 ** 32, int(good[3]) - 2 ** 32 + 8)])
    F.check_layout(good, B, others=[(2 ** 32 + (1 << 20), 2 ** 32 + (1 << 20) + 500)])
