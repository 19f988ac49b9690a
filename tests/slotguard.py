"""Slot-bound harness for the kernels that write into caller-given slots
(dg_j2t_batch_device, dg_t2j_batch_device, the pack kernels). Pure Python +
torch: the kernel under test comes in as a `launch` callback.

Written-byte mask. Every launch runs twice on the same inputs, the output
arena prefilled 0x5A the first time and 0xA5 the second. A byte that differs
between the two results was never stored to; a byte that is equal in both was.
That is the exact set of bytes the launch wrote, with no assumption about what
a kernel may write inside its own slot. Status words and lengths (prefilled
the same way) must be identical in both runs.

Sandwich layout. The slot table is contiguous by the ABI, so guards are slots
of spacer messages: spacer, tested, spacer, tested, ..., spacer, with 64 guard
bytes in front of slot 0 and 64 behind the last slot. A spacer's slot has 64
bytes plus what brings the tested slot behind it to the wanted alignment: an
8-aligned base, for t2j in the wanted 16-byte phase (0 or 8). A tested slot
has exactly its capacity, so the spacer behind an odd capacity starts at an
odd address; its output is 1-2 bytes.

Control launch. The same slot table with every tested message replaced by a
spacer. Outside the tested slots, under each prefill, the arena must be
byte-identical to the control launch: any stray store of a tested message
shows, the one that lands in the front bytes of the next spacer and the one
that lands 8 bytes before its own slot included."""
import numpy as np

GUARD = 64
SPACER = 64
FILLS = (0x5A, 0xA5)
OVERFLOW = 0xF0  # DG_ST_OUT_OVERFLOW


def slot_caps(need):
    """The capacities a tested message of `need` output bytes is run with."""
    out = []
    for c in (0, need - 9, need - 8, need - 7, need - 1, need, need + 1, need + 7, need + 8):
        if c >= 0 and c not in out:
            out.append(c)
    return out


class Item:
    """A tested message in a slot of `cap` bytes; (ret, out) is what the
    oracle gives the message alone. phase: the slot base modulo 16 (0 or 8;
    another value for an unaligned base), None = 8-aligned in either phase."""

    def __init__(self, msg, cap, ret, out, phase=None):
        self.msg, self.cap, self.ret, self.out, self.phase = bytes(msg), int(cap), int(ret), bytes(out), phase

    @property
    def keeps(self):  # the message has output (a success, or an error that keeps its bytes)
        return self.ret == 0 or len(self.out) > 0

    @property
    def overflows(self):
        return self.keeps and self.cap < len(self.out)

    @property
    def tight(self):
        return self.keeps and 0 <= self.cap - len(self.out) < 8


def items_for(msgs, oracle, phases=(None,)):
    """Every message at every capacity of slot_caps (and slot phase)."""
    items = []
    for m in msgs:
        ret, out = oracle(m)
        need = len(out) if (ret == 0 or out) else 0
        for ph in phases:
            items += [Item(m, c, ret, out, ph) for c in slot_caps(need)]
    return items


def shares(items):
    """(share of overflows, share that fit with less than 8 bytes to spare),
    from the oracle's results alone."""
    n = max(len(items), 1)
    return sum(it.overflows for it in items) / n, sum(it.tight for it in items) / n


def assert_shares(items):
    over, tight = shares(items)
    assert over >= 0.25 and tight >= 0.25, "the inputs do not exercise the bounds: %.2f overflow, %.2f tight" % (over, tight)


class Sandwich:
    """msgs / off: the batch and its slot table (offsets into an arena whose
    base is 16-aligned; off[0] = GUARD); tested[k] = the batch index of item k."""

    def __init__(self, items, spacer):
        self.items, self.spacer = items, bytes(spacer)
        msgs, off, tested = [], [GUARD], []
        pos = GUARD
        for it in items:
            if it.phase is None:
                pad = -(pos + SPACER) % 8
            else:
                pad = (it.phase - (pos + SPACER)) % 16
            msgs.append(self.spacer)
            pos += SPACER + pad
            off.append(pos)
            assert pos % 8 == 0 if it.phase is None else pos % 16 == it.phase
            tested.append(len(msgs))
            msgs.append(it.msg)
            pos += it.cap
            off.append(pos)
        msgs.append(self.spacer)
        pos += SPACER
        off.append(pos)
        self.msgs, self.off, self.tested = msgs, np.array(off, dtype=np.int64), tested
        self.size = pos + GUARD
        self.inside = np.zeros(self.size, dtype=bool)  # the tested slots
        for k in tested:
            self.inside[off[k]:off[k + 1]] = True

    def slot_of(self, byte):
        if byte < GUARD:
            return "the front guard, %d before slot 0" % (GUARD - byte)
        if byte >= self.off[-1]:
            return "the tail guard, +%d" % (byte - self.off[-1])
        i = int(np.searchsorted(self.off, byte, side="right")) - 1
        return "slot %d (%s) +%d of %d" % (i, "tested" if i in self.tested else "spacer", byte - self.off[i],
                                           self.off[i + 1] - self.off[i])


def in_arena(msgs, pad=64):
    lens = np.fromiter((len(m) for m in msgs), dtype=np.int64, count=len(msgs))
    off = np.zeros(len(msgs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return np.frombuffer(b"".join(msgs) + b"\0" * pad, dtype=np.uint8).copy(), off


class Run:
    def __init__(self, out, out_len, ret, pending):
        self.out, self.out_len, self.ret, self.pending = out, out_len, ret, pending


def launch_twice(launch, msgs, off, size, device, tail=None, fills=FILLS):
    """launch(d_src, d_in_off, n, d_out, d_out_off, d_out_len, d_ret,
    d_pending) enqueues one conversion of the batch (torch tensors on
    `device`; d_out_off are offsets into d_out). Returns the Run of each
    prefill. tail: bytes to put behind the last message, in front of the
    input arena's zero padding."""
    import torch
    a, in_off = in_arena(msgs)
    if tail is not None:  # the bytes behind the last message
        a[int(in_off[-1]):int(in_off[-1]) + len(tail)] = np.frombuffer(tail, dtype=np.uint8)
    n = len(msgs)
    d_src = torch.from_numpy(a).to(device)
    d_in = torch.from_numpy(in_off).to(device)
    d_oo = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).to(device)
    runs = []
    for fill in fills:
        d_out = torch.full((size,), fill, dtype=torch.uint8, device=device)
        assert d_out.data_ptr() % 16 == 0
        d_ol = torch.full((n,), fill * 0x01010101 - (1 << 32) if fill & 0x80 else fill * 0x01010101, dtype=torch.int32,
                          device=device)
        d_ret = torch.full((n,), fill * 0x0101010101010101 - (1 << 64) if fill & 0x80 else fill * 0x0101010101010101,
                           dtype=torch.int64, device=device)
        d_pend = torch.zeros(4, dtype=torch.int32, device=device)
        launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend)
        if torch.device(device).type != "cpu":
            torch.cuda.synchronize()
        runs.append(Run(d_out.cpu().numpy(), d_ol.cpu().numpy().view(np.uint32).copy(),
                        d_ret.cpu().numpy().view(np.uint64).copy(), int(d_pend[0])))
    return runs


def written(runs):
    """The bytes the launch stored to."""
    return runs[0].out == runs[1].out


def check(launch, items, spacer, spacer_out, device, pending=True, max_report=6, spacer_ret=0):
    """Run the sandwich and its control and assert the expectations; returns
    (sandwich, runs). Failures are collected and raised together. (spacer_ret,
    spacer_out): what the oracle gives the spacer alone; a spacer that fails
    (no output at all) guards as well as one that writes 1-2 bytes."""
    sw = Sandwich(items, spacer)
    spacer_out = bytes(spacer_out)
    runs = launch_twice(launch, sw.msgs, sw.off, sw.size, device)
    ctrl = launch_twice(launch, [sw.spacer] * len(sw.msgs), sw.off, sw.size, device)
    bad = []

    def fail(msg):
        if len(bad) < max_report:
            bad.append(msg)

    for name, rr in (("sandwich", runs), ("control", ctrl)):
        if not np.array_equal(rr[0].ret, rr[1].ret) or not np.array_equal(rr[0].out_len, rr[1].out_len):
            k = int(np.nonzero((rr[0].ret != rr[1].ret) | (rr[0].out_len != rr[1].out_len))[0][0])
            fail("%s: status / out_len of message %d depend on the prefill (not written?): %x/%d vs %x/%d" %
                 (name, k, rr[0].ret[k], rr[0].out_len[k], rr[1].ret[k], rr[1].out_len[k]))
    wc = written(ctrl)
    for lo, hi in ((0, GUARD), (sw.size - GUARD, sw.size)):
        for b in np.nonzero(wc[lo:hi])[0][:2]:
            fail("control: a store in %s" % sw.slot_of(lo + int(b)))
    # outside the tested slots: identical to the control launch under each prefill
    for k, fill in enumerate(FILLS):
        stray = np.nonzero((runs[k].out != ctrl[k].out) & ~sw.inside)[0]
        for b in stray[:max_report]:
            i = int(np.searchsorted(sw.off, b, side="right")) - 1
            near = [t for t in sw.tested if abs(t - i) <= 1]
            what = ", ".join("cap %d need %d msg %r" % (sw.items[sw.tested.index(t)].cap,
                                                        len(sw.items[sw.tested.index(t)].out),
                                                        sw.items[sw.tested.index(t)].msg[:48]) for t in near)
            fail("prefill %#x: byte %d in %s is %#x, control %#x; tested neighbours: %s" %
                 (fill, int(b), sw.slot_of(int(b)), runs[k].out[b], ctrl[k].out[b], what))
    r = runs[0]
    n_over = 0
    for i in range(len(sw.msgs)):
        base, cap = int(sw.off[i]), int(sw.off[i + 1] - sw.off[i])
        if i in sw.tested:
            it = sw.items[sw.tested.index(i)]
            ret, out, keeps, what = it.ret, it.out, it.keeps, "msg %r cap %d (need %d, base %% 16 = %d)" % (
                it.msg[:60], cap, len(it.out), base % 16)
        else:
            ret, out, keeps, what = spacer_ret, spacer_out, spacer_ret == 0, "spacer %d" % i
        got_ret, got_len = int(r.ret[i]), int(r.out_len[i])
        if keeps and cap < len(out):
            n_over += 1
            if got_ret & 0xFF != OVERFLOW or got_len != len(out):
                fail("%s: want DG_ST_OUT_OVERFLOW with out_len %d, got %#x / %d" % (what, len(out), got_ret, got_len))
        elif keeps:
            got = r.out[base:base + len(out)].tobytes()
            if got_ret != ret or got_len != len(out) or got != out:
                d = next((j for j in range(len(out)) if got[j] != out[j]), -1)
                fail("%s: want %#x / %d, got %#x / %d, first wrong byte %d" % (what, ret, len(out), got_ret, got_len, d))
        elif got_ret != ret or got_len != 0:
            fail("%s: want %#x / 0, got %#x / %d" % (what, ret, got_ret, got_len))
    if pending:
        for rr in runs:
            if rr.pending != n_over:
                fail("d_pending counted %d messages, %d overflowed" % (rr.pending, n_over))
    assert not bad, "\n".join(bad)
    return sw, runs
