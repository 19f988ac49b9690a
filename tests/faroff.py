"""Layouts for the far-offset tests (test_gpu_far_offsets.py): small batches
placed in two large arenas so that their 64-bit byte offsets straddle B = 2^31
or B = 2^32. Pure numpy; torch only moves windows to and from the device.

The base pointer handed to the library is arena[PAD:], PAD = 2^31, so offset o
is arena byte PAD + o and the view covers offsets [-2^31, 2^32 + ROOM). What a
32-bit slip makes of an offset o >= 2^31 stays inside the allocation:

  o - 2^32   int32(o) sign-extended for o < 2^32, uint32(o) for o >= 2^32
  o - 2^31   o mod 2^31 for 2^31 <= o < 2^32 (B = 2^32 only; above 2^32 it is
             o - 2^32 again)

These are the aliases of a window. On the input side every alias holds a
decoy: as many bytes of the same batch reversed, so a truncated read returns
plausible bytes of the wrong message. On the output side the slots, 64 guard
bytes on each side and the same ranges at the aliases are prefilled with FILL,
and after the run everything but the slots must still be FILL. A kernel that
truncates or sign-extends an offset in use therefore gives a wrong answer in
memory the test owns, never a fault.

The arenas are never touched as a whole: fill and read back windows only."""
import numpy as np

PAD = 2 ** 31
SPAN = 2 ** 32
ROOM = 2 << 20
ARENA_BYTES = PAD + SPAN + ROOM
GUARD = 64
TAIL = 16  # readable bytes the kernels may load behind the last input message
NEAR = 64  # off[0] of a near placement
FILL = 0xC3
BOUNDS = (2 ** 31, 2 ** 32)


# ------------------------------------------------------------ offset arithmetic
def near(lens):
    """off (int64, n + 1) of a batch that starts at NEAR"""
    off = np.full(len(lens) + 1, NEAR, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=off[1:])
    off[1:] += NEAR
    return off


def place(lens, B, pivot, delta):
    """off (int64, n + 1), messages back to back, message `pivot` starting at
    B + delta: with delta = 0 a message starts exactly at B, with a small
    negative delta (and a pivot longer than -delta) it straddles B. The
    messages before the pivot lie wholly below B, those after it above."""
    lens = np.asarray(lens, dtype=np.int64)
    assert 0 <= pivot < len(lens) and delta <= 0
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    off += B + delta - off[pivot]
    return off


def alias_windows(lo, hi, B):
    """[(name, shift, lo', hi')]: where a 32-bit slip sends the offsets of
    [lo, hi); offset o of the window maps to o + shift."""
    out = []
    a = max(lo, 2 ** 31)
    if a < hi:
        out.append(("alias -2^32", -2 ** 32, a - 2 ** 32, hi - 2 ** 32))
    if B == 2 ** 32:
        b = min(hi, 2 ** 32)
        if a < b:
            out.append(("alias mod 2^31", -2 ** 31, a - 2 ** 31, b - 2 ** 31))
    return out


def windows(off, B, guard=GUARD, tail=0):
    """[(name, shift, lo, hi)] of a placement: the real window (the batch with
    `guard` bytes in front and guard + tail behind) and its aliases"""
    lo, hi = int(off[0]) - guard, int(off[-1]) + guard + tail
    return [("real", 0, lo, hi)] + alias_windows(lo, hi, B)


def check_layout(off, B, guard=GUARD, tail=0, others=()):
    """What keeps a far placement from being vacuous or unsafe: a message
    straddles B or starts exactly at it, a message lies wholly on each side,
    every window and alias window is inside the arena, and no two windows
    overlap. others: further (lo, hi) windows in the same arena (offsets)."""
    off = np.asarray(off, dtype=np.int64)
    assert B in BOUNDS, B
    assert (np.diff(off) >= 0).all(), "offsets must not fall"
    a, e = off[:-1], off[1:]
    assert ((a < B) & (e > B)).any() or (a == B).any(), "no message straddles %#x or starts at it" % B
    assert ((e <= B) & (a < B)).any(), "no message wholly below %#x" % B
    assert ((a >= B) & (e > a)).any(), "no message wholly above %#x" % B
    wins = windows(off, B, guard, tail)
    for lo, hi in others:
        wins += [("other", 0, int(lo), int(hi))] + alias_windows(int(lo), int(hi), B)
    for name, _, lo, hi in wins:
        assert 0 <= PAD + lo and PAD + hi <= ARENA_BYTES, "%s window [%#x, %#x) leaves the arena" % (name, lo, hi)
    for k, (na, _, la, ha) in enumerate(wins):
        for nb, _, lb, hb in wins[k + 1:]:
            assert ha <= lb or hb <= la, "%s window [%#x, %#x) overlaps %s window [%#x, %#x)" % (na, la, ha, nb, lb, hb)
    return wins


def message_at(off, o):
    """the index of the message (slot) holding offset o, for failure texts"""
    off = np.asarray(off)
    if o < off[0]:
        return "the front guard, %d before slot 0" % (off[0] - o)
    if o >= off[-1]:
        return "the tail guard, +%d" % (o - off[-1])
    i = int(np.searchsorted(off, o, side="right")) - 1
    return "message %d, slot byte %d of %d" % (i, o - off[i], off[i + 1] - off[i])


# --------------------------------------------------------------------- arenas
class Arena:
    """One 6 GiB + 2 MiB device allocation; .base is the view the library
    gets. All accessors take offsets relative to .base."""

    def __init__(self, device="cuda"):
        import torch
        self.t = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=device)
        self.base = self.t[PAD:]
        assert self.base.data_ptr() % 16 == 0

    def free(self):
        self.base = self.t = None

    def _view(self, lo, hi):
        assert 0 <= PAD + lo <= PAD + hi <= ARENA_BYTES, (lo, hi)
        return self.t[PAD + lo:PAD + hi]

    def write(self, lo, data):
        import torch
        data = np.array(data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8))  # writable
        if len(data):
            self._view(lo, lo + len(data)).copy_(torch.from_numpy(data))

    def fill(self, lo, hi, byte=FILL):
        if hi > lo:
            self._view(lo, hi).fill_(byte)

    def read(self, lo, hi):
        return self._view(lo, hi).cpu().numpy()

    # ---- input side
    def put_input(self, off, msgs, B, tail_byte=0xAA):
        """the batch at [off[0], off[n]) with TAIL readable bytes behind it,
        and the decoy (the batch reversed) at every alias of that window"""
        data = np.frombuffer(b"".join(msgs) + bytes([tail_byte]) * TAIL, dtype=np.uint8)
        decoy = np.frombuffer(b"".join(reversed(msgs)) + bytes([tail_byte ^ 0xFF]) * TAIL, dtype=np.uint8)
        lo = int(off[0])
        assert len(data) == int(off[-1]) - lo + TAIL
        self.write(lo, data)
        for _, shift, alo, ahi in alias_windows(lo, lo + len(data), B):
            self.write(alo, decoy[alo - shift - lo:ahi - shift - lo])

    # ---- output side
    def prefill(self, off, B, guard=GUARD):
        for _, _, lo, hi in windows(off, B, guard):
            self.fill(lo, hi)

    def collect(self, off, B, guard=GUARD, what="output"):
        """the bytes of [off[0], off[n]) after the run; the guards and every
        alias window must still be FILL"""
        lo, hi = int(off[0]), int(off[-1])
        got = self.read(lo - guard, hi + guard)
        for name, g, at in (("front guard", got[:guard], lo - guard), ("tail guard", got[guard + hi - lo:], hi)):
            bad = np.nonzero(g != FILL)[0]
            assert bad.size == 0, "%s: a store in the %s of the real window, at offset %#x (%s)" % (
                what, name, at + int(bad[0]), message_at(off, at + int(bad[0])))
        for name, shift, alo, ahi in alias_windows(lo - guard, hi + guard, B):
            bad = np.nonzero(self.read(alo, ahi) != FILL)[0]
            if bad.size:
                o = alo + int(bad[0])
                raise AssertionError("%s: a store in the %s window at offset %#x, the alias of %#x (%s)" % (
                    what, name, o, o - shift, message_at(off, o - shift)))
        return got[guard:guard + hi - lo]
