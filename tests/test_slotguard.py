"""CPU: the slot-bound harness (tests/slotguard.py) against a model kernel in
numpy -- it passes a writer that keeps to its slots, and catches a single
stray byte on either side of a tested slot, 8 bytes before it, in the arena
guards, a status word that is not written, a wrong overflow report and a
miscounted d_pending -- and the inputs of tests/test_gpu_slots.py: every
route's (message, capacity) pairs hold the shares of overflows and of tight
fits that the GPU tests rely on, from the oracle's results alone."""
import numpy as np
import pytest

import oracle
import slotguard as SG

SPACER, SPACER_OUT = b".", b"s"


def convert(m):
    """The model's operation: a message's bytes upper-cased; "!..." fails."""
    m = bytes(m)
    if m == SPACER:
        return 0, SPACER_OUT
    if m.startswith(b"!"):
        return 0x102, b""
    return 0, m.upper()


def model(stray=None, keep_ret=False, overflow_len=0, pend=0):
    def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
        src, ino, out, oo = d_src.numpy(), d_in.numpy(), d_out.numpy(), d_oo.numpy()
        for i in range(n):
            m = src[ino[i]:ino[i + 1]].tobytes()
            ret, o = convert(m)
            base, cap = int(oo[i]), int(oo[i + 1] - oo[i])
            k = min(cap, len(o))
            out[base:base + k] = np.frombuffer(o[:k], dtype=np.uint8)
            if m != SPACER and stray is not None and (stray >= 0 or len(o) >= 8):
                out[base + cap + stray if stray >= 0 else base + stray] = 0x77
            if len(o) > cap:
                ret, ol = SG.OVERFLOW | (len(o) << 40), len(o) + overflow_len
                d_pend[0] += 1 + pend
            else:
                ol = len(o)
            if not (keep_ret and m != SPACER):
                d_ret[i] = ret
            d_ol[i] = ol
    return launch


def items():
    msgs = [b"a", b"hello, world", b"0123456789abcdef0123", b"!bad", b"x" * 40]
    return SG.items_for(msgs, convert, phases=(0, 8))


def test_layout():
    its = items()
    sw = SG.Sandwich(its, SPACER)
    assert len(sw.msgs) == 2 * len(its) + 1 and sw.off[0] == SG.GUARD and sw.size == sw.off[-1] + SG.GUARD
    for k, i in enumerate(sw.tested):
        assert sw.off[i] % 16 == its[k].phase and sw.off[i + 1] - sw.off[i] == its[k].cap
        assert sw.off[i] - sw.off[i - 1] >= SG.SPACER and sw.off[i + 2] - sw.off[i + 1] >= SG.SPACER
    assert SG.slot_caps(20) == [0, 11, 12, 13, 19, 20, 21, 27, 28] and SG.slot_caps(1) == [0, 1, 2, 8, 9]
    assert SG.slot_caps(0) == [0, 1, 7, 8]
    SG.assert_shares(its)


def test_a_writer_that_keeps_to_its_slots_passes():
    SG.check(model(), items(), SPACER, SPACER_OUT, "cpu")


@pytest.mark.parametrize("what,kw", [
    ("control", dict(stray=1)),        # behind the slot, the first byte the next spacer does not write itself
    ("control", dict(stray=7)),
    ("control", dict(stray=-1)),       # the byte before the slot
    ("control", dict(stray=-8)),       # a pair store that starts 8 bytes early
    ("depend on the prefill", dict(keep_ret=True)),
    ("DG_ST_OUT_OVERFLOW", dict(overflow_len=1)),
    ("d_pending", dict(pend=1)),
])
def test_a_single_stray_byte_is_caught(what, kw):
    with pytest.raises(AssertionError, match=what):
        SG.check(model(**kw), items(), SPACER, SPACER_OUT, "cpu")


def test_a_store_in_the_arena_guards_is_caught():
    def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
        model()(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend)
        d_out[int(d_oo[n]) + 5] = 1
    with pytest.raises(AssertionError, match="tail guard"):
        SG.check(launch, items(), SPACER, SPACER_OUT, "cpu")


def test_route_inputs_hold_their_shares():
    """Every route of test_gpu_slots.py: at least 25 % of its (message,
    capacity) pairs overflow and at least 25 % fit with less than 8 bytes to
    spare, by the oracle alone."""
    if oracle.ref_lib_path() is None:
        pytest.skip("oracle/_ref not built")
    import test_gpu_slots as S
    for route in S.J2T_ROUTES:
        _, _, its = S.j2t_items(route)
        SG.assert_shares(its)
        assert len(its) >= 20, route
    for which in S.T2J_SETS:
        _, its = S.t2j_items(which)
        SG.assert_shares(its)
