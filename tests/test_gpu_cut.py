"""GPU: batched MarshalTo (dynamicgo_amd.generic over dg_cut_*) against the
pure-Python restatement of the reference in cutref.py. Every case runs on both
routes (the cut_wave_min knob: 0 sends every message to the wave route, a huge
value none but those the lane route's 8 frames cannot hold), and the bytes,
out_len and ret of every message are compared with the checker's. Every device
run also checks the memory contract: nothing stored in front of the first slot
or behind the last, and nothing at or beyond out_len in a slot that succeeded."""
import random

import numpy as np
import pytest

import cutgen as G
import cutref as R
import slotguard as SG

pytestmark = pytest.mark.gpu

LANE, WAVE = 1 << 40, 0  # cut_wave_min for the two routes
ROUTES = (("lane", LANE), ("wave", WAVE))
FILL, GUARD = 0xEE, 64


def run_device(msgs, plan, opts=0, caps=None, max_len=None):
    """dg_cut_batch_device over torch tensors -> [(ret, out)], out_len. caps: the slot sizes, back to back (so
    slot bases are unaligned); None: dg_cut_slot_bound rounded up to 16."""
    import torch
    from dynamicgo_amd import generic as X
    n = len(msgs)
    in_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(m) for m in msgs], out=in_off[1:])
    if caps is None:
        caps = [(plan.slot_bound(len(m), opts) + 15) & ~15 for m in msgs]
    out_off = np.full(n + 1, GUARD, dtype=np.int64)
    np.cumsum(caps, out=out_off[1:])
    out_off[1:] += GUARD
    arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_in, d_oo = torch.from_numpy(in_off).cuda(), torch.from_numpy(out_off).cuda()
    d_out = torch.full((int(out_off[n]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_ol = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    d_ret = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    ml = max((len(m) for m in msgs), default=0) if max_len is None else max_len
    X.marshal_to_device(plan, arena, d_in, n, d_out, d_oo, d_ol, d_ret, opts, max_len=ml)
    torch.cuda.synchronize()
    out, ol, ret = d_out.cpu().numpy(), d_ol.cpu().numpy().view(np.uint32), d_ret.cpu().numpy().view(np.uint64)
    assert (out[:GUARD] == FILL).all() and (out[int(out_off[n]):] == FILL).all(), "a store outside the slots"
    res = []
    for i in range(n):
        a, e = int(out_off[i]), int(out_off[i + 1])
        r = int(ret[i])
        if r == 0:
            assert int(ol[i]) <= e - a, i
            assert (out[a + int(ol[i]):e] == FILL).all(), "message %d: a store at or beyond out_len" % i
            res.append((0, out[a:a + int(ol[i])].tobytes()))
        else:
            assert int(ol[i]) == (r >> 32 if r & 0xFF == R.E_OVERFLOW else 0), (i, hex(r), int(ol[i]))
            res.append((r, b""))
    return res


def same(got, want, msgs, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, message %d (%r...): got %x / %d bytes, checker %x / %d bytes" % (
            what, i, msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))


def on_both_routes(knob, plan, msgs, want, opts=0, caps=None):
    for name, wm in ROUTES:
        knob("cut_wave_min", wm)
        same(run_device(msgs, plan, opts, caps), want, msgs, "%s route, opts %d" % (name, opts))


@pytest.fixture(scope="module")
def plans():
    from dynamicgo_amd import generic as X
    made = {}

    def get(name):
        if name not in made:
            made[name] = X.CutPlan(*{"pair": G.pair, "node": G.node_pair, "run": G.run_pair, "grow": G.grow_pair}[name]())
        return made[name]

    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def fuzz_want():
    """the checker over the fuzz corpus (messages + mutated copies) under each option word, computed once"""
    wide, narrow = G.pair()
    msgs, bad = G.fuzz()
    return msgs + bad, {o: G.expect(msgs + bad, wide, narrow, o) for o in G.ALL_OPTS}


# -------------------------------------------------------------------- fuzz
def test_fuzz_corpus(fuzz_want):
    """from the checker alone: at least half of the unmutated messages cut under the default options, and
    every status but OVERFLOW and DEPTH occurs"""
    msgs, want = fuzz_want
    assert sum(r == 0 for r, _ in want[0][:G.FUZZ_N]) * 2 >= G.FUZZ_N
    assert {r & 0xFF for o in G.ALL_OPTS for r, _ in want[o]} == {R.OK, R.E_READ, R.E_TYPE, R.E_UNKNOWN, R.E_REQUIRED}


@pytest.mark.parametrize("opts", G.ALL_OPTS)
def test_fuzz(knob, plans, fuzz_want, opts):
    msgs, want = fuzz_want
    on_both_routes(knob, plans("pair"), msgs, want[opts], opts)


def test_fuzz_host_entry(knob, plans, fuzz_want):
    from dynamicgo_amd import generic as X
    msgs, want = fuzz_want
    names = {R.OK: None, R.E_READ: "ErrRead", R.E_TYPE: "ErrDismatchType", R.E_UNKNOWN: "ErrUnknownField",
             R.E_REQUIRED: "ErrMissRequiredField"}
    for opts in (X.CutOptions(), X.CutOptions(write_default=True, disallow_unknown=True),
                 X.CutOptions(not_check_requireness=True)):
        for _, wm in ROUTES + (("default", 4096),):
            knob("cut_wave_min", wm)
            res = X.marshal_to_batch(msgs, plans("pair"), opts=opts)
            same([(r.status | r.aux << 32, r.raw) for r in res], want[opts.word()], msgs, "host entry")
            assert [r.error for r in res] == [names[w & 0xFF] for w, _ in want[opts.word()]]
    # descriptors instead of a plan
    wide, narrow = G.pair()
    res = X.marshal_to_batch(msgs[:10], wide, narrow)
    same([(r.status | r.aux << 32, r.raw) for r in res], want[0][:10], msgs, "host entry, descriptors")


@pytest.mark.parametrize("n", (1, 63, 64, 65, 256, 257))
def test_batch_sizes(knob, plans, fuzz_want, n):
    msgs, want = fuzz_want
    pick = list(range(0, 2 * n, 2)) if 2 * n <= len(msgs) else list(range(n))  # unmutated and mutated ones
    on_both_routes(knob, plans("pair"), [msgs[i] for i in pick], [want[1][i] for i in pick], 1)


# ------------------------------------------------------------- run lengths
def test_run_lengths_and_alignments(knob, plans):
    """every kept-run length around the 16-byte windows and the 1024-byte wave stride, at every source and
    destination misalignment (slot bases are 16-aligned here, so the prefix sets the destination's)"""
    w, n = G.run_pair()
    msgs = G.run_messages()
    want = G.expect(msgs, w, n)
    assert all(r == 0 for r, _ in want) and len(msgs) == len(G.RUN_LENGTHS) * 256
    on_both_routes(knob, plans("run"), msgs, want)
    # the same messages in exact-size slots back to back: every slot base alignment too
    on_both_routes(knob, plans("run"), msgs[::7], want[::7], caps=[len(o) for _, o in want[::7]])


# ------------------------------------------------------------------ nesting
@pytest.mark.parametrize("opts", (0, R.WRITE_DEFAULT))
def test_chains_around_the_lds_frames(knob, plans, opts):
    node, node_n = G.node_pair()
    rng = random.Random(21)
    msgs = [G.chain_message(k) for d in (7, 8, 9) for k in G.chains_of(d, rng, 8)]
    want = G.expect(msgs, node, node_n, opts)
    assert all(r == 0 for r, _ in want)
    on_both_routes(knob, plans("node"), msgs, want, opts)


def test_chains_around_max_depth(knob, plans):
    from dynamicgo_amd.generic import CUT_MAX_DEPTH
    node, node_n = G.node_pair()
    rng = random.Random(22)
    depths = [d for d in (CUT_MAX_DEPTH - 1, CUT_MAX_DEPTH, CUT_MAX_DEPTH + 1) for _ in range(4)]
    msgs = [G.chain_message(k) for d in depths[::4] for k in G.chains_of(d, rng, 4)]
    want = G.expect(msgs, node, node_n, R.WRITE_DEFAULT)
    assert [r for r, _ in want] == [R.E_DEPTH if d > CUT_MAX_DEPTH else 0 for d in depths]
    on_both_routes(knob, plans("node"), msgs, want, R.WRITE_DEFAULT)


def test_dropped_value_at_the_skip_limit(knob, plans):
    wide, narrow = G.pair()
    msgs = [G.deep_drop_message(d) for d in (7, 8, 9, 1022, 1023, 1024)]
    want = G.expect(msgs, wide, narrow)
    assert [r for r, _ in want] == [0, 0, 0, 0, 0, R.E_READ]
    on_both_routes(knob, plans("pair"), msgs, want)


# -------------------------------------------------------------------- slots
SPACER = b"\x0b\x00\x0b\x00\x00\x00\x00\x00"  # req_s = "": cut to itself


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_slot_bounds_and_neighbours(knob, plans, fuzz_want, route):
    """tight slots, guard bytes and neighbour independence (slotguard), the checker as the oracle"""
    from dynamicgo_amd import generic as X
    wide, narrow = G.pair()
    knob("cut_wave_min", route[1])
    msgs, want = fuzz_want
    opts = R.WRITE_DEFAULT
    by_msg = dict(zip(msgs, want[opts]))
    pick = [m for m in msgs[:G.FUZZ_N] if by_msg[m][0] == 0][:24] + [m for m in msgs[G.FUZZ_N:] if by_msg[m][0]][:4]
    items = SG.items_for(pick, lambda m: by_msg[m], phases=(None, 5))
    SG.assert_shares(items)
    plan = plans("pair")

    def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
        X.marshal_to_device(plan, d_src, d_in, n, d_out, d_oo, d_ol, d_ret, opts)

    assert R.marshal_to(SPACER, wide, narrow, opts)[0] == 0
    SG.check(launch, items, SPACER, R.marshal_to(SPACER, wide, narrow, opts)[1], "cuda", pending=False)


def test_one_byte_short(knob, plans, fuzz_want):
    """E_OVERFLOW carries the exact size in aux and out_len; the neighbours, in exact-size slots on both sides,
    are whole and nothing lies beyond their out_len (run_device checks it)"""
    msgs, want = fuzz_want
    opts = R.WRITE_DEFAULT
    ok = [(m, w) for m, w in zip(msgs, want[opts]) if w[0] == 0][:96]
    caps = [len(w[1]) - (i % 3 == 1) for i, (_, w) in enumerate(ok)]
    expect = [(R.overflow(len(w[1])), b"") if i % 3 == 1 else w for i, (_, w) in enumerate(ok)]
    on_both_routes(knob, plans("pair"), [m for m, _ in ok], expect, opts, caps)


def test_host_entry_reruns_overflows(knob, plans):
    """messages whose WriteDefault output outgrows the host entry's first slots (their length + 256)"""
    from dynamicgo_amd import generic as X
    w, n = G.grow_pair()
    msgs = [G.grow_message(k) for k in (0, 1, 11, 12, 13, 40, 300, 5)]
    want = G.expect(msgs, w, n, R.WRITE_DEFAULT)
    assert all(r == 0 for r, _ in want) and sum(len(o) > len(m) + 256 for m, (_, o) in zip(msgs, want)) >= 3
    plan = plans("grow")
    assert plan.slot_bound(100, R.WRITE_DEFAULT) == 100 * (1 + 22) and plan.slot_bound(100) == 100
    assert plan.slot_bound(100, R.WRITE_DEFAULT | R.NOT_CHECK_REQ) == 100
    for name, wm in ROUTES:
        knob("cut_wave_min", wm)
        res = X.marshal_to_batch(msgs, plan, opts=X.CutOptions(write_default=True))
        same([(r.status | r.aux << 32, r.raw) for r in res], want, msgs, "host entry, " + name)
    on_both_routes(knob, plan, msgs, want, R.WRITE_DEFAULT)  # in dg_cut_slot_bound slots: no overflow


# -------------------------------------------------------------- empty cases
def test_empty_cases(knob, plans):
    from dynamicgo_amd import generic as X
    wide, narrow = G.pair()
    plan = plans("pair")
    assert X.marshal_to_batch([], plan) == []
    assert run_device([], plan) == []
    msgs = [b"", b"\x00", b"", SPACER, b""]
    for opts in (0, R.NOT_CHECK_REQ):
        want = G.expect(msgs, wide, narrow, opts)
        assert [r & 0xFF for r, _ in want] == [R.E_READ, R.OK if opts else R.E_REQUIRED, R.E_READ, R.OK, R.E_READ]
        on_both_routes(knob, plan, msgs, want, opts)
        res = X.marshal_to_batch(msgs, plan, opts=opts)
        same([(r.status | r.aux << 32, r.raw) for r in res], want, msgs, "host entry")


def test_plan_blob_is_validated():
    from dynamicgo_amd import _lib
    from dynamicgo_amd import generic as X
    blob = bytearray(X.compile_cut(*G.pair()))
    for at, val in ((0, 0), (4, 9), (12, 0xFF), (8, 0xFFFFFF)):  # magic, version, root, total_len
        bad = bytearray(blob)
        bad[at:at + 4] = val.to_bytes(4, "little")
        with pytest.raises(_lib.DGError):
            X.CutPlan(bytes(bad))
    bad = bytearray(blob)
    bad[64 + 4:64 + 8] = (0xFFFF).to_bytes(4, "little")  # the first node's `a`
    with pytest.raises(_lib.DGError):
        X.CutPlan(bytes(bad))
