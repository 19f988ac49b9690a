"""GPU: every device entry point with 64-bit byte offsets past 2 GiB and 4 GiB.

The ABI puts no bound on d_in_off, d_out_off, d_val_off or d_dst_off, and a
j2t batch with 1 GiB of JSON already has its last slots past 4 GiB
(dg_slot_bound). Here small batches of the per-kernel tests' generators are
placed in two 6 GiB arenas (tests/faroff.py) so that their offsets straddle
B = 2^32 (input far, output far, both far with a message straddling B and with
one starting exactly at it) and B = 2^31 (both far). A `(uint32_t)` or
`(int32_t)` on an offset or on a 32-bit scan of positions reads a decoy or
writes an alias window that the test owns and checks: a wrong answer naming
the message and the window, not a fault.

Every result is compared with the operation's checker (oracle.py for j2t and
t2j, tgetref, cutref, editref, editmref, kidsref), never with a near-offset
run of the kernel. What keeps a case from being vacuous is asserted from the
checker and the layout alone: at least half the messages succeed, at least one
fails, one slot is one byte short, a message takes the deep pass where the
operation has one, and the pivot, the short slot and the deep message lie on
the far side of B.

Out of scope: the host entries (they rebase on in_off[0] before the upload),
the aggregator and the pipeline (they lay out their own arenas), and
dg_j2t_batch_device_hm / _cb (the same kernels through the same Params)."""
import random
import struct
import types

import numpy as np
import pytest

import cutgen
import cutref
import editgen
import editmgen
import editmref as M
import editref as E
import faroff as F
import kidsgen as KG
import t2jgen
import tgetgen as TG
import tgetref as R
from dynamicgo_amd import _lib, conv, thrift as T
from test_gpu_slots import FLAT, J2T_ROUTES, NO_FLAT, NO_WAVE, j2t_oracle, t2j_oracle
from test_gpu_tget import FUZZ_SETS, expect as tget_expect, same as tget_same, to_paths

pytestmark = pytest.mark.gpu

G31, G32 = 2 ** 31, 2 ** 32
# (which side is far, B, delta): near means off[0] = 64
PLACEMENTS = [("in", G32, -3), ("out", G32, -3), ("both", G32, -3), ("both", G32, 0), ("both", G31, -3)]
PL_IDS = ["in@4G", "out@4G", "both@4G-3", "both@4G+0", "both@2G-3"]
IN_PLACEMENTS = [("in", G32, -3), ("in", G32, 0), ("in", G31, -3)]  # for the operations without output slots
IN_IDS = ["4G-3", "4G+0", "2G-3"]
OVERFLOW = 0xF0  # DG_ST_OUT_OVERFLOW, DG_CUT_E_OVERFLOW, DG_EDIT_E_OVERFLOW
FULL = (1 << 64) - 1
VAL_AT = G32 + (1 << 20)  # the far value arena of the edits: in the input arena, clear of the messages and their aliases


@pytest.fixture(scope="module")
def arenas():
    import torch
    torch.cuda.reset_peak_memory_stats()
    a = types.SimpleNamespace(inp=F.Arena(), out=F.Arena())
    yield a
    print("\nfar offsets: peak device memory %.2f GiB" % (torch.cuda.max_memory_allocated() / 2 ** 30))
    a.inp.free()
    a.out.free()
    del a
    torch.cuda.empty_cache()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ batches
class Batch:
    """msgs with their slot sizes and what the checker expects in each slot:
    exps[i] = (ret, mask of the compared ret bits, out_len, bytes, clean, class)
    -- clean: from which slot byte on the fill must be kept, None: no promise;
    class: "ok", "over" (the slot is too small) or "err", by the checker"""

    def __init__(self, msgs, caps, exps, pivot, short, aligned=False, deep=None):
        self.msgs, self.caps, self.exps, self.pivot, self.short, self.aligned, self.deep = msgs, caps, exps, pivot, short, \
            aligned, deep
        self.n_over = sum(1 for e in exps if e[5] == "over")
        n = len(msgs)
        ok = sum(1 for e in exps if e[5] == "ok")
        assert 64 <= n <= 300, n
        assert 2 * ok >= n, "%d of %d messages succeed" % (ok, n)
        assert any(e[5] == "err" for e in exps), "no message fails"
        assert short > pivot and exps[short][5] == "over" and exps[short][2] == caps[short] + 1, "no slot one byte short"
        assert deep is None or deep > pivot, "the deep message is not on the far side"
        assert len(msgs[pivot]) > 3 and caps[pivot] > 8, "the pivot cannot straddle"


def choose(oks, needs, msgs, aligned=False):
    """(pivot, short): the first message from a third of the batch on that can
    straddle B on both sides, and the first one behind it whose slot can be one
    byte short (with 8-aligned slot bases: one that needs 8 k + 1 bytes)"""
    n = len(msgs)
    pivot = next(i for i in range(n // 3, n) if oks[i] and needs[i] > 8 and len(msgs[i]) > 3)
    short = next(i for i in range(pivot + 1, n) if oks[i] and needs[i] >= 1 and (not aligned or needs[i] % 8 == 1))
    return pivot, short


def caps_for(needs, short, aligned=False):
    """slot sizes: the need plus 0, 1, 8 or 13 bytes (8-aligned bases: the need
    rounded up to 8, plus 8 for every other message); need - 1 for `short`"""
    if aligned:
        caps = [(v + 7) // 8 * 8 + 8 * (i % 2) for i, v in enumerate(needs)]
    else:
        caps = [v + (0, 1, 8, 13)[i % 4] for i, v in enumerate(needs)]
    caps[short] = needs[short] - 1
    assert not aligned or caps[short] % 8 == 0
    return caps


def conv_batch(msgs, want, aligned=False, deep=None):
    """j2t / t2j: (ret, out) of the oracle; a message that keeps output in a
    slot too small for it reports DG_ST_OUT_OVERFLOW and the bytes it needs"""
    keeps = [r == 0 or len(o) > 0 for r, o in want]
    needs = [len(o) if k else 0 for (r, o), k in zip(want, keeps)]
    pivot, short = choose([r == 0 for r, _ in want], needs, msgs, aligned)
    caps = caps_for(needs, short, aligned)
    exps = []
    for (r, o), k, cap in zip(want, keeps, caps):
        if k and cap < len(o):
            exps.append((OVERFLOW, 0xFF, len(o), b"", None, "over"))
        else:
            exps.append((r, FULL, len(o) if k else 0, o if k else b"", None, "ok" if r == 0 else "err"))
    return Batch(msgs, caps, exps, pivot, short, aligned, deep)


def cut_batch(msgs, want, deep=None):
    needs = [len(o) if r == 0 else 0 for r, o in want]
    pivot, short = choose([r == 0 for r, _ in want], needs, msgs)
    caps = caps_for(needs, short)
    exps = []
    for (r, o), cap in zip(want, caps):
        if r == 0 and cap < len(o):
            exps.append((cutref.E_OVERFLOW | len(o) << 32, FULL, len(o), b"", None, "over"))
        else:  # on success no byte at or beyond out_len is written
            exps.append((r, FULL, len(o) if r == 0 else 0, o if r == 0 else b"", len(o) if r == 0 else None,
                         "ok" if r == 0 else "err"))
    return Batch(msgs, caps, exps, pivot, short, deep=deep)


def edit_batch(case, ref):
    """edit / editm: the checker applies the slot sizes itself; a message that
    fails or overflows writes nothing"""
    want = case.want()
    oks = [r & 0xFF == 0 for r, _ in want]
    needs = [len(o) if k else 0 for (r, o), k in zip(want, oks)]
    pivot, short = choose(oks, needs, case.msgs)
    caps = caps_for(needs, short)
    exps = [(r, FULL, ref.out_len(r, o), o if r & 0xFF == 0 else b"", len(o) if r & 0xFF == 0 else 0,
             "ok" if r & 0xFF == 0 else "over" if r & 0xFF == OVERFLOW else "err") for r, o in case.want(caps)]
    return Batch(case.msgs, caps, exps, pivot, short)


# ------------------------------------------------------------------ running
def offsets(lens, far, pl, pivot, delta=None):
    _, B, d = pl
    return F.place(lens, B, pivot, d if delta is None else delta) if far else F.near(lens)


def run_slots(ar, b, pl, launch, what, others=(), slip=0):
    """One launch of launch(src, d_in_off, n, out, d_out_off, d_out_len,
    d_ret) over the batch under the placement -> (in_off, out_off, the bytes of
    the real output window, out_len, ret), the guards and aliases checked.
    slip: added to the slot table the kernel gets (test_the_checks_catch_*)."""
    import torch
    mode, B, delta = pl
    in_far, out_far = mode != "out", mode != "in"
    in_off = offsets([len(m) for m in b.msgs], in_far, pl, b.pivot)
    out_off = offsets(b.caps, out_far, pl, b.pivot, -8 if b.aligned and delta else None)
    if in_far:
        F.check_layout(in_off, B, guard=0, tail=F.TAIL, others=others)
    if out_far:
        F.check_layout(out_off, B)
        assert not b.aligned or (out_off % 8 == 0).all()
    ar.inp.put_input(in_off, b.msgs, B)
    ar.out.prefill(out_off, B)
    n = len(b.msgs)
    d_in, d_oo = torch.from_numpy(in_off).cuda(), torch.from_numpy(out_off + slip).cuda()
    d_ol = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_ret = torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    launch(ar.inp.base, d_in, n, ar.out.base, d_oo, d_ol, d_ret)
    torch.cuda.synchronize()
    out = ar.out.collect(out_off, B, what=what)
    return in_off, out_off, out, d_ol.cpu().numpy().view(np.uint32), d_ret.cpu().numpy().view(np.uint64)


def check_slots(b, out_off, out, ol, ret, what):
    bad = []
    o0 = int(out_off[0])
    for i, (r, mask, n_out, data, clean, _) in enumerate(b.exps):
        a, e = int(out_off[i]), int(out_off[i + 1])
        slot = out[a - o0:e - o0]
        where = "%s: message %d (%r...), real slot [%#x, %#x)" % (what, i, b.msgs[i][:24], a, e)
        got_r, got_n = int(ret[i]), int(ol[i])
        if (got_r & mask) != (r & mask) or got_n != n_out:
            bad.append("%s: checker %#x / %d, got %#x / %d" % (where, r & mask, n_out, got_r & mask, got_n))
        elif slot[:len(data)].tobytes() != data:
            d = next(j for j in range(len(data)) if slot[j] != data[j])
            bad.append("%s: first wrong byte %d of %d" % (where, d, len(data)))
        elif clean is not None and (slot[clean:] != F.FILL).any():
            bad.append("%s: a store at slot byte %d, at or beyond the %d it may write" % (
                where, clean + int(np.nonzero(slot[clean:] != F.FILL)[0][0]), clean))
    assert not bad, "\n".join(bad[:6] + ["(%d messages in all)" % len(bad)])


def run_and_check(ar, b, pl, launch, what, others=()):
    in_off, out_off, out, ol, ret = run_slots(ar, b, pl, launch, what, others)
    check_slots(b, out_off, out, ol, ret, what)
    return in_off, out_off, out, ol, ret


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------- j2t
FAR_J2T_ROUTES = ["flat", "flat-wrapped", "small", "wave-occ4", "lane", "lane-deep"]
BAD_JSON = [b'{"a":[1,}', b'{"a"']
LONG_AT = 60  # where the long message sits: behind the pivot, inside a block of short ones


def j2t_batch(route, long=False):
    mk, flags, _, msgs_fn, _, _ = J2T_ROUTES[route]
    fl = T.flatten(mk())
    pure = flags & ~(FLAT | NO_FLAT | NO_WAVE)
    base = msgs_fn()
    msgs = [base[k % len(base)] for k in range(72)] + BAD_JSON
    if long:  # 70 000 bytes: longer than the flat kernel's 16 KiB stage and the small kernel's
        key = b"StringField" if route == "flat" else b"String"
        msgs.insert(LONG_AT, b'{"' + key + b'":"' + bytes(97 + k % 26 for k in range(70000)) + b'"}')
    orc = j2t_oracle(fl, pure)
    want = [orc(m) for m in msgs]
    deep = None
    if route == "lane-deep":  # 20 levels of lists: past the lane kernel's frames, redone by the deep pass
        deep = max(i for i, m in enumerate(msgs) if m.count(b"[") == 20 and want[i][0] == 0)
    b = conv_batch(msgs, want, deep=deep)
    assert not long or (b.pivot < LONG_AT and want[LONG_AT][0] == 0 and len(msgs[LONG_AT]) > 70000)
    return fl, flags, b


def j2t_launch(fl, flags, max_len, d_pend):
    ctx = conv.default_context()
    dh = ctx.desc(fl)

    def launch(src, d_in, n, out, d_oo, d_ol, d_ret):
        _lib.check(_lib.lib().dg_j2t_batch_device_ml(ctx.h, dh, fl.root_type, src.data_ptr(), d_in.data_ptr(), n, flags,
                                                     out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(),
                                                     d_pend.data_ptr(), stream(), max_len))
    return launch


def run_j2t(ar, route, pl, knob, long=False):
    import torch
    fl, flags, b = cached(("j2t", route, long), lambda: j2t_batch(route, long))
    for k, v in J2T_ROUTES[route][2].items():
        knob(k, v)
    d_pend = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = run_and_check(ar, b, pl, j2t_launch(fl, flags, max(len(m) for m in b.msgs), d_pend), "j2t " + route)
    assert int(d_pend[0]) == b.n_over, "d_pending counted %d messages, %d overflow" % (int(d_pend[0]), b.n_over)
    return b, res


@pytest.mark.parametrize("pl", PLACEMENTS, ids=PL_IDS)
@pytest.mark.parametrize("route", FAR_J2T_ROUTES)
def test_j2t(arenas, knob, route, pl):
    run_j2t(arenas, route, pl, knob)


@pytest.mark.parametrize("route", ["flat", "small"])
def test_j2t_long_message_between_short_ones(arenas, knob, route):
    """The block's span misses the LDS stage, so every short message is staged
    on its own from its far address (j2t_flat.h `if (!staged)`, j2t_small.h
    `if (!staged)`)."""
    run_j2t(arenas, route, ("both", G32, -3), knob, long=True)


# ---------------------------------------------------------------------- t2j
def t2j_batch(kind):
    rng = random.Random(31)
    if kind == "all-types":
        td = t2jgen.all_types_desc()
        good = [m for m in (t2jgen.gen_thrift(rng, td) for _ in range(200)) if 8 < len(m) <= 600][:88]
        msgs = good + [t2jgen.mutate(rng, m) for m in good[:12]]
        deep = None
    else:  # chains: depth 13 and 14 pass the 12 LDS frames and are redone by the deep pass
        td = t2jgen.chain_desc()
        msgs = [t2jgen.chain_thrift(1 + k % 14) for k in range(70)] + [t2jgen.chain_thrift(13)[:-1], t2jgen.chain_thrift(3)[:-2]]
        deep = max(i for i, m in enumerate(msgs) if m == t2jgen.chain_thrift(13))
    fl = T.flatten(td)
    orc = t2j_oracle(fl, 0)
    want = [orc(m) for m in msgs]
    assert deep is None or want[deep][0] == 0
    return fl, conv_batch(msgs, want, aligned=True, deep=deep)


def t2j_launch(fl, max_len):
    ctx = conv.default_context()
    dh = ctx.desc_t2j(fl)

    def launch(src, d_in, n, out, d_oo, d_ol, d_ret):
        _lib.check(_lib.lib().dg_t2j_batch_device_ml(ctx.h, dh, fl.root_type, src.data_ptr(), d_in.data_ptr(), n, 0,
                                                     out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(),
                                                     stream(), max_len))
    return launch


@pytest.mark.parametrize("pl", PLACEMENTS, ids=PL_IDS)
@pytest.mark.parametrize("route", ["lane-spread1", "lane-spread4", "wave", "deep"])
def test_t2j(arenas, knob, route, pl):
    """t2j slot bases are 8-aligned by the ABI: the output pivot starts 8
    bytes below B where the input pivot starts 3 below."""
    fl, b = cached(("t2j", route == "deep"), lambda: t2j_batch("chain" if route == "deep" else "all-types"))
    if route == "wave":
        knob("t2j_wave_min", 1)
    elif route != "deep":
        knob("t2j_wave_min", 0)
        knob("t2j_spread", int(route[-1]))
    run_and_check(arenas, b, pl, t2j_launch(fl, max(len(m) for m in b.msgs)), "t2j " + route)


# --------------------------------------------------------------------- tget
TGET_DEEP = ("SLMSESLMSELS", "e")  # 12 containers and a list of strings: 13 frames under f1, 8 fit the LDS
TGET_ONE = [(R.FIELD, 1)]  # the P = 1 path: the chain in the chain messages, a scalar (where set) in the others


def tget_batch(P):
    rng = random.Random(41)
    td = t2jgen.all_types_desc()
    good = [m for m in (t2jgen.gen_thrift(rng, td) for _ in range(200)) if 8 < len(m) <= 600][:80]
    chains = [TG.chain_message(*TG.random_chain(rng, d)) for d in (3, 5, 9, 10, 12, 14)]
    msgs = good[:40] + chains[:3] + good[40:] + [t2jgen.mutate(rng, m) for m in good[:16]] + chains[3:] + \
        [TG.chain_message(*TGET_DEEP)]
    paths = [TGET_ONE] if P == 1 else FUZZ_SETS[0]
    want = tget_expect(msgs, paths)
    n = len(msgs)
    pivot = next(i for i in range(n // 3, n) if len(msgs[i]) > 3)
    deep_path = TGET_ONE if P == 1 else []
    assert deep_path in paths and TG.chain_frames(*TGET_DEEP, deep_path) > TG.LDS_FRAMES and n - 1 > pivot
    assert want["status"][n - 1, paths.index(deep_path)] == R.OK
    ok = (want["status"] == R.OK).mean()
    assert 64 <= n <= 300 and (ok >= 0.5 if P == 1 else ok >= 0.25), ok  # half of the (message, path) pairs; of 8 fuzz
    assert (want["status"] == R.E_READ).any()                           # paths a message has about a third
    assert (want["start"][pivot + 1:][want["status"][pivot + 1:] == R.OK] > 0).any()
    return msgs, paths, want, pivot


def run_tget(ar, P, pl, slip=0):
    import torch
    from dynamicgo_amd import generic as X
    msgs, paths, want, pivot = cached(("tget", P), lambda: tget_batch(P))
    _, B, _ = pl
    n = len(msgs)
    in_off = offsets([len(m) for m in msgs], True, pl, pivot)
    F.check_layout(in_off, B, guard=0, tail=F.TAIL)
    ar.inp.put_input(in_off, msgs, B)
    d_in = torch.from_numpy(in_off + slip).cuda()
    q, guard = n * P, 64
    rec = torch.full((q + guard, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    voff = torch.full((q + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    vlen = torch.full((q + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with X.PathSet(to_paths(paths)) as ps:
        X.get_by_path_device(ps, ar.inp.base, d_in, n, rec, voff, vlen, max_len=max(len(m) for m in msgs))
        torch.cuda.synchronize()
    h_rec, h_voff, h_vlen = rec.cpu().numpy(), voff.cpu().numpy(), vlen.cpu().numpy()
    assert (h_rec[q:] == 0x5A5A5A5A).all() and (h_voff[q:] == 0x5A5A5A5A5A5A5A5A).all() and (h_vlen[q:] == 0x5A5A5A5A).all()
    tget_same(h_rec[:q].view(X.REC_DTYPE).reshape(n, P), want, "tget P = %d, input at %#x" % (P, B))
    ok = want["status"] == R.OK
    want_voff = in_off[:-1, None].astype(np.int64) + want["start"].astype(np.int64)
    bad = np.argwhere(h_voff[:q].reshape(n, P) != want_voff)
    assert bad.size == 0, "tget: d_val_off of (message, path) %s is %#x, in_off + start is %#x" % (
        bad[0].tolist(), h_voff[:q].reshape(n, P)[tuple(bad[0])], want_voff[tuple(bad[0])])
    assert (h_vlen[:q].reshape(n, P) == np.where(ok, want["end"] - want["start"], 0)).all()
    return msgs, want, in_off, voff, vlen


@pytest.mark.parametrize("pl", IN_PLACEMENTS, ids=IN_IDS)
@pytest.mark.parametrize("P", [1, 8])
def test_tget(arenas, P, pl):
    msgs, want, in_off, voff, vlen = run_tget(arenas, P, pl)
    if P != 1:
        return
    # the documented chain: (arena base, d_val_off, d_val_len) of a P = 1 run packs the found values back to back
    import torch
    n = len(msgs)
    raws = [R.raw(m, R.Rec(*w.tolist())) for m, w in zip(msgs, want[:, 0])]
    packed = b"".join(raws)
    assert 2 * sum(1 for r in raws if r) >= n
    dst = torch.full((len(packed) + 2 * F.GUARD,), F.FILL, dtype=torch.uint8, device="cuda")
    dst_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().dg_pack_device_scan(conv.default_context().h, arenas.inp.base.data_ptr(), voff.data_ptr(),
                                              vlen.data_ptr(), n, dst[F.GUARD:].data_ptr(), dst_off.data_ptr(), stream()))
    torch.cuda.synchronize()
    check_packed(dst.cpu().numpy(), packed, "pack_scan of the found values")
    assert dst_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in raws])]).tolist()


def check_packed(buf, expect, what, lens=None):
    """buf: GUARD fill bytes, the packed bytes, GUARD fill bytes"""
    g = F.GUARD
    assert (buf[:g] == F.FILL).all() and (buf[g + len(expect):] == F.FILL).all(), what + ": a store outside [0, total)"
    got = buf[g:g + len(expect)].tobytes()
    if got != expect:
        d = next(j for j in range(len(expect)) if got[j] != expect[j])
        where = "" if lens is None else " (%s)" % F.message_at(np.concatenate([[0], np.cumsum(lens)]), d)
        raise AssertionError("%s: first wrong packed byte %d of %d%s" % (what, d, len(expect), where))


# ---------------------------------------------------------------------- cut
CUT_DEEP = "SSSSSSSSSS"  # 11 cut containers under Wide.node: the lane route holds 8 frames, the rest is queued for a wave


def cut_batch_for(opts):
    wide, narrow = cutgen.pair()
    good, bad = cutgen.fuzz()
    short_enough = [i for i, m in enumerate(good) if 3 < len(m) <= 600][:100]
    deep = b"\x0c\x00\x0f" + cutgen.chain_message(CUT_DEEP) + b"\x0b\x00\x0b\x00\x00\x00\x01r\x00"
    assert cutgen.chain_containers(CUT_DEEP) + 1 > cutgen.LDS_FRAMES
    msgs = [good[i] for i in short_enough] + [bad[i] for i in short_enough[:20]] + [deep]
    want = cutgen.expect(msgs, wide, narrow, opts)
    assert want[-1][0] == 0
    return cut_batch(msgs, want, deep=len(msgs) - 1)


@pytest.fixture(scope="module")
def cut_plan():
    from dynamicgo_amd import generic as X
    p = X.CutPlan(*cutgen.pair())
    yield p
    p.close()


@pytest.mark.parametrize("pl", PLACEMENTS, ids=PL_IDS)
@pytest.mark.parametrize("opts", [0, cutref.WRITE_DEFAULT], ids=["plain", "write-default"])
@pytest.mark.parametrize("route", [("lane", 1 << 40), ("wave", 0)], ids=["lane", "wave"])
def test_cut(arenas, knob, cut_plan, route, opts, pl):
    from dynamicgo_amd import generic as X
    b = cached(("cut", opts), lambda: cut_batch_for(opts))
    knob("cut_wave_min", route[1])
    ml = max(len(m) for m in b.msgs)

    def launch(src, d_in, n, out, d_oo, d_ol, d_ret):
        X.marshal_to_device(cut_plan, src, d_in, n, out, d_oo, d_ol, d_ret, opts, max_len=ml)

    run_and_check(arenas, b, pl, launch, "cut %s, opts %d" % (route[0], opts))


# --------------------------------------------------------------------- edit
def pick_msgs(n_all):
    """100 of the generator's unmutated messages and 28 of the mutated ones (the second half of its batch)"""
    half = n_all // 2
    return list(range(100)) + list(range(half, half + 28))


def place_values(ar, values):
    """The per-message values in the input arena, far too: a window of their
    own at VAL_AT, so every val_off has bit 32 set, with the values reversed as
    the decoy at its alias -> (val_off, the window)."""
    off = np.full(len(values) + 1, VAL_AT, dtype=np.int64)
    np.cumsum([len(v) for v in values], out=off[1:])
    off[1:] += VAL_AT
    ar.inp.write(int(off[0]), b"".join(values) + b"\xAA" * F.TAIL)
    lo, hi = int(off[0]), int(off[-1]) + F.TAIL
    for _, shift, alo, ahi in F.alias_windows(lo, hi, G32):  # the decoy: the values reversed
        decoy = np.frombuffer(b"".join(reversed(values)) + b"\x55" * F.TAIL, dtype=np.uint8)
        ar.inp.write(alo, decoy[alo - shift - lo:ahi - shift - lo])
    return off, (lo, hi)


EDIT_KINDS = {"replace": 0, "insert": 4, "unset": 16}  # indexes into editgen.fuzz_cases(): f7 (a replace where the
# field is there), field 999 with values of up to 300 bytes, unset f7


def edit_case(kind):
    cases = cached("edit-fuzz", editgen.fuzz_cases)
    c = cases[EDIT_KINDS[kind]]
    c = c.sub(pick_msgs(len(c.msgs)))
    assert (c.op == E.SET_OP and isinstance(c.values, list)) or (kind == "unset" and c.op == E.UNSET_OP)
    b = edit_batch(c, E)
    outcomes = {E.outcome(c.op, r) for r, _ in c.want()}
    assert {"replace": "replaced", "insert": "inserted", "unset": "deleted"}[kind] in outcomes, outcomes
    return c, b


@pytest.mark.parametrize("pl", PLACEMENTS, ids=PL_IDS)
@pytest.mark.parametrize("kind", list(EDIT_KINDS))
def test_edit(arenas, knob, kind, pl):
    import torch
    from dynamicgo_amd import generic as X
    from test_gpu_edit import ROUTES, plan_of
    c, b = cached(("edit", kind), lambda: edit_case(kind))
    ml = max(len(m) for m in c.msgs)
    d_vo, others, val_len = None, (), 0
    if c.op == E.SET_OP:
        val_off, win = place_values(arenas, c.values)
        d_vo, others, val_len = torch.from_numpy(val_off).cuda(), (win,), max(len(v) for v in c.values)
    with plan_of(c) as plan:
        def launch(src, d_in, n, out, d_oo, d_ol, d_ret):
            X.edit_device(plan, src, d_in, n, c.val_type, src if d_vo is not None else None, d_vo, out, d_oo, d_ol, d_ret,
                          root_type=c.root_type, val_len=val_len, max_len=ml)

        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            run_and_check(arenas, b, pl, launch, "edit %s, %s route" % (kind, name), others)


# -------------------------------------------------------------------- editm
def editm_case(kind):
    base = cached("editm-fuzz", editmgen.fuzz_cases)[0]
    msgs = [base.msgs[i] for i in pick_msgs(len(base.msgs))]
    n, rng = len(msgs), random.Random(51)

    def per_msg(lo, hi):
        return [editgen.wstr(bytes(rng.randrange(256) for _ in range(rng.randrange(lo, hi)))) for _ in range(n)]

    if kind == "set":  # K = 4, every value per message: two replaces where the field is there, two inserts
        items = [((R.FIELD, 18), per_msg(0, 40), R.STRING), ((R.FIELD, 900), per_msg(0, 300), R.STRING),
                 ((R.FIELD, 22), [struct.pack(">d", rng.random()) for _ in range(n)], R.DOUBLE),
                 ((R.FIELD, 901), per_msg(0, 20), R.STRING)]
        c = editmgen.ManyCase(M.SET_OP, [], items, msgs, what="set four children, per-message values")
    else:
        c = editmgen.ManyCase(M.UNSET_OP, [], [((R.FIELD, 18),), ((R.FIELD, 22),)], msgs)
    return c, edit_batch(c, M)


@pytest.mark.parametrize("pl", PLACEMENTS, ids=PL_IDS)
@pytest.mark.parametrize("kind", ["set", "unset"])
def test_editm(arenas, knob, kind, pl):
    import torch
    from dynamicgo_amd import generic as X
    from test_gpu_editm import ROUTES, plan_of
    c, b = cached(("editm", kind), lambda: editm_case(kind))
    n, ml = len(c.msgs), max(len(m) for m in c.msgs)
    d_vo, others, val_lens = None, (), [0] * c.k
    if c.op == M.SET_OP:
        flat = [c.value(i, j) for i in range(n) for j in range(c.k)]  # message-major
        val_off, win = place_values(arenas, flat)
        d_vo, others = torch.from_numpy(val_off).cuda(), (win,)
        val_lens = [max(len(c.value(i, j)) for i in range(n)) for j in range(c.k)]
    with plan_of(c) as plan:
        def launch(src, d_in, n_, out, d_oo, d_ol, d_ret):
            X.edit_many_device(plan, src, d_in, n_, c.val_types, src if d_vo is not None else None, d_vo, val_lens, out,
                               d_oo, d_ol, d_ret, root_type=c.root_type, max_len=ml)

        for name, wm, lanes in ROUTES:
            knob("edit_wave_min", wm)
            knob("edit_lanes", lanes)
            run_and_check(arenas, b, pl, launch, "editm %s, %s route" % (kind, name), others)


# --------------------------------------------------------------------- kids
KIDS_PATH = [(R.FIELD, 1)]
KIDS_DEEP = ("S" * 12, "e")  # 11 levels below the node under f1: 8 fit the LDS (9 in recursive mode)


def kids_batch(recurse):
    rng = random.Random(61)
    wide = [m for k, m in KG.wide_messages().items() if " x 1000" not in k]  # the nodes of the wide route, up to 65 children
    chains = [TG.chain_message(k, lf) for k, lf in KG.lds_chains()[::2]]
    td = t2jgen.all_types_desc()
    scal = [m for m in (t2jgen.gen_thrift(rng, td) for _ in range(60)) if 8 < len(m) <= 600][:12]  # f1 is no container
    msgs = wide[:15] + chains[:10] + scal + wide[15:] + chains[10:] + [TG.chain_message(*KIDS_DEEP)]
    want = KG.expect(msgs, KIDS_PATH, recurse)
    n = len(msgs)
    pivot = next(i for i in range(n // 3, n) if len(msgs[i]) > 3)
    st = want[0]["status"]
    assert 64 <= n <= 300 and 2 * int((st == R.OK).sum()) >= n and (st != R.OK).any() and (st == R.E_READ).any()
    assert st[n - 1] == R.OK and n - 1 > pivot and len(KIDS_DEEP[0]) - 1 > KG.LDS_LEVELS + 1
    assert int(want[0]["count"][pivot + 1:].max()) >= 64  # a node of the wide route on the far side
    return msgs, want, pivot


@pytest.mark.parametrize("pl", IN_PLACEMENTS, ids=IN_IDS)
@pytest.mark.parametrize("recurse", [False, True], ids=["one-level", "recursive"])
@pytest.mark.parametrize("wide_min", [1, 0], ids=["wide", "lanes"])
def test_kids(arenas, knob, wide_min, recurse, pl):
    """a count-only call, then the emit with counted=True"""
    import torch
    from dynamicgo_amd import generic as X
    msgs, want, pivot = cached(("kids", recurse), lambda: kids_batch(recurse))
    knob("kids_wide_min", wide_min)
    _, B, _ = pl
    n, ml = len(msgs), max(len(m) for m in msgs)
    in_off = offsets([len(m) for m in msgs], True, pl, pivot)
    F.check_layout(in_off, B, guard=0, tail=F.TAIL)
    arenas.inp.put_input(in_off, msgs, B)
    d_in = torch.from_numpy(in_off).cuda()
    total, guard = int(want[1][-1]), 64
    head = torch.full((n + 1, 4), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    rec_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    recs = torch.full((total + guard, 8), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    with X.PathSet(to_paths([KIDS_PATH])) as ps:
        X.children_device(ps, arenas.inp.base, d_in, n, head, rec_off, None, 0, recurse=recurse, max_len=ml)
        torch.cuda.synchronize()
        assert int(rec_off[n]) == total, "the count-only call: %d records, checker %d" % (int(rec_off[n]), total)
        X.children_device(ps, arenas.inp.base, d_in, n, head, rec_off, recs, total, recurse=recurse, counted=True, max_len=ml)
        torch.cuda.synchronize()
    h, r = head.cpu().numpy(), recs.cpu().numpy()
    assert (h[n:].view(np.uint8) == 0xA5).all() and (r[total:].view(np.uint8) == 0xA5).all(), "a store past the outputs"
    got = (h[:n].copy().view(X.KIDS_HEAD_DTYPE).reshape(n), rec_off.cpu().numpy().astype(np.uint64),
           r[:total].copy().view(X.KIDS_REC_DTYPE).reshape(-1))
    KG.same(got, want, "kids, input at %#x" % B)


# --------------------------------------------------------------------- pack
def far_j2t_outputs(ar, knob, B):
    """a flat j2t run with its slots across B (the input near): the batch, its
    out_off, and the lengths to pack (0 for what failed or overflowed, as the
    header asks of the caller) with the checker's bytes"""
    import torch
    b, (_, out_off, _, ol, ret) = run_j2t(ar, "flat", ("out", B, -3), knob)
    keep = [e[3] if e[5] == "ok" else b"" for e in b.exps]
    lens = np.array([len(k) for k in keep], dtype=np.int64)
    assert (lens > 0).sum() * 2 >= len(lens) and (lens[b.pivot + 1:] > 0).any() and (lens == 0).any()
    return b, out_off, ol, ret, keep, lens


@pytest.mark.parametrize("B", F.BOUNDS, ids=["2G", "4G"])
def test_pack(arenas, knob, B):
    """dg_pack_device: source slots far, and the caller's d_dst_off shifted
    across B as well, the destination in the other arena"""
    import torch
    b, out_off, _, _, keep, lens = far_j2t_outputs(arenas, knob, B)
    n = len(keep)
    pivot = next(i for i in range(n // 3, n) if lens[i] > 3)
    dst_off = F.place(lens, B, pivot, -3)
    F.check_layout(dst_off, B)
    arenas.inp.prefill(dst_off, B)
    d_oo, d_do = torch.from_numpy(out_off).cuda(), torch.from_numpy(dst_off).cuda()
    d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
    _lib.check(_lib.lib().dg_pack_device(conv.default_context().h, arenas.out.base.data_ptr(), d_oo.data_ptr(), d_len.data_ptr(),
                                         n, arenas.inp.base.data_ptr(), d_do.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = arenas.inp.collect(dst_off, B, what="pack").tobytes()
    want = b"".join(keep)
    if got != want:
        d = next(j for j in range(len(want)) if got[j] != want[j])
        raise AssertionError("pack: first wrong byte at destination offset %#x (%s)" % (
            int(dst_off[0]) + d, F.message_at(dst_off, int(dst_off[0]) + d)))


@pytest.mark.parametrize("B", F.BOUNDS, ids=["2G", "4G"])
def test_pack_scan_and_framed(arenas, knob, B):
    """source slots far; the kernels compute the positions, so the destination is near"""
    import torch
    b, out_off, ol, ret, keep, lens = far_j2t_outputs(arenas, knob, B)
    n = len(keep)
    ctx, L = conv.default_context(), _lib.lib()
    d_oo = torch.from_numpy(out_off).cuda()
    d_len = torch.from_numpy(lens.astype(np.int32)).cuda()
    d_ol, d_ret = torch.from_numpy(ol.view(np.int32)).cuda(), torch.from_numpy(ret.view(np.int64)).cuda()
    hdr, ftr = bytes(range(0x80, 0x8D)), b"\x00"
    framed = [hdr + k + ftr if e[5] == "ok" else b"" for k, e in zip(keep, b.exps)]
    for what, parts in (("pack_scan", keep), ("pack_framed", framed)):
        want = b"".join(parts)
        dst = torch.full((len(want) + 2 * F.GUARD,), F.FILL, dtype=torch.uint8, device="cuda")
        d_do = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        if what == "pack_scan":
            _lib.check(L.dg_pack_device_scan(ctx.h, arenas.out.base.data_ptr(), d_oo.data_ptr(), d_len.data_ptr(), n,
                                             dst[F.GUARD:].data_ptr(), d_do.data_ptr(), stream()))
        else:  # the kernel's own lengths and status words: an overflowed message's out_len holds what it needs
            _lib.check(L.dg_pack_device_framed(ctx.h, arenas.out.base.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(),
                                               d_ret.data_ptr(), n, hdr, len(hdr), ftr, len(ftr), dst[F.GUARD:].data_ptr(),
                                               d_do.data_ptr(), stream()))
        torch.cuda.synchronize()
        plens = [len(p) for p in parts]
        check_packed(dst.cpu().numpy(), want, what, plens)
        assert d_do.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(plens)]).tolist(), what


def test_pack_scan_lengths_of_one_wave_pass_4_gib(arenas, knob):
    """dg_pack_scan_kernel scans the lengths of the 64 messages a wave holds:
    two messages of 2^31 + 8 bytes make that sum pass 2^32, while out_len
    allows 2^32 - 1 for each. Their source bytes are whatever the arena holds;
    the first and last 4 KiB of each are compared with the source. The 62
    messages of a j2t run behind them must sit at the uint64 prefix sum. A
    32-bit scan puts them 2^32 lower, inside the same allocation."""
    import torch
    BIG, WIN = G31 + 8, 4096
    b, (_, out_off, _, _, _) = run_j2t(arenas, "flat", ("out", G32, 0), knob)
    first = len(b.msgs) - 62  # the last 62 messages: their slots lie on both sides of 2^32
    assert first < b.pivot
    keep = [e[3] if e[5] == "ok" else b"" for e in b.exps][first:first + 62]
    assert len(keep) == 62 and sum(1 for k in keep if k) >= 31
    # the two big sources: 2 GiB + 8 of the output arena each, read only (they overlap each other, not the j2t slots)
    src_off = np.concatenate([[64, G31 - (1 << 20)], out_off[first:first + 62]]).astype(np.int64)
    assert int(src_off[1]) + BIG <= int(out_off[0]) - F.GUARD
    lens = np.array([BIG, BIG] + [len(k) for k in keep], dtype=np.uint64)
    want_off = np.zeros(65, dtype=np.uint64)
    np.cumsum(lens, out=want_off[1:])
    total = int(want_off[-1])
    assert total > G32 and total + F.GUARD <= G32 + F.ROOM and int(lens[:2].sum()) >= G32
    dst = arenas.inp  # positions [0, total); what a 32-bit scan gives, pos - 2^32, is inside it too
    small_lo, small_hi = int(want_off[2]), total
    dst.fill(small_lo, small_hi + F.GUARD)
    d_so = torch.from_numpy(src_off).cuda()
    d_len = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).cuda()
    d_do = torch.full((65,), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().dg_pack_device_scan(conv.default_context().h, arenas.out.base.data_ptr(), d_so.data_ptr(),
                                              d_len.data_ptr(), 64, dst.base.data_ptr(), d_do.data_ptr(), stream()))
    torch.cuda.synchronize()
    got_off = d_do.cpu().numpy().view(np.uint64)
    bad = np.nonzero(got_off != want_off)[0]
    assert bad.size == 0, "dst_off[%d] is %#x, the uint64 prefix sum %#x" % (bad[0], got_off[bad[0]], want_off[bad[0]])
    got = dst.read(small_lo, small_hi + F.GUARD)
    assert (got[small_hi - small_lo:] == F.FILL).all(), "a store behind the packed bytes"
    want = b"".join(keep)
    if got[:len(want)].tobytes() != want:
        d = next(j for j in range(len(want)) if got[j] != want[j])
        raise AssertionError("the small messages are not at the uint64 positions: first wrong byte at %#x (%s)" % (
            small_lo + d, F.message_at(want_off.astype(np.int64), small_lo + d)))
    for k in (0, 1):  # the big messages: their first and last 4 KiB
        for at in (0, BIG - WIN):
            s, d = int(src_off[k]) + at, int(want_off[k]) + at
            assert (arenas.out.read(s, s + WIN) == dst.read(d, d + WIN)).all(), "message %d, bytes [%#x, %#x)" % (k, at, at + WIN)


# ------------------------------------------------- the checks themselves
def test_the_checks_catch_a_truncated_output_offset(arenas, knob, cut_plan):
    """What a kernel that dropped bit 32 of out_off would do, done from
    outside: the correct kernel gets the slot table 2^32 lower. Every store
    lands in the alias window, and the check names it."""
    from dynamicgo_amd import generic as X
    b = cached(("cut", 0), lambda: cut_batch_for(0))
    knob("cut_wave_min", 1 << 40)

    def launch(src, d_in, n, out, d_oo, d_ol, d_ret):
        X.marshal_to_device(cut_plan, src, d_in, n, out, d_oo, d_ol, d_ret, 0, max_len=max(len(m) for m in b.msgs))

    with pytest.raises(AssertionError, match=r"a store in the alias -2\^32 window at offset .* \(message \d+, slot byte"):
        run_slots(arenas, b, ("both", G32, -3), launch, "cut with a slipped slot table", slip=-G32)


def test_the_checks_catch_a_truncated_input_offset(arenas):
    """... and of in_off: the kernel reads the decoy, and the records differ
    from the checker's at a named (message, path)."""
    with pytest.raises(AssertionError, match=r"differs at \(message, path\)"):
        run_tget(arenas, 8, ("in", G32, -3), slip=-G32)
