"""GPU: batched Children (dynamicgo_amd.generic over dg_kids_*) against the
pure-Python restatement of the reference in kidsref.py. Every case goes
through the host entry point and the device entry point; heads, rec_off, every
record field and the children's bytes are compared with the checker's."""
import numpy as np
import pytest

import kidsgen as KG
import kidsref as K
import tgetgen as TG
import tgetref as R
from test_gpu_tget import to_paths

pytestmark = pytest.mark.gpu

F = R.FIELD
OVERFLOW = 0xF0
GUARD = 64  # records of 0xA5 after rec_cap


class Dev:
    """One batch on the device: dg_kids_batch_device over torch tensors. The
    heads are followed by 16 guard bytes, the records by GUARD guard records."""

    def __init__(self, msgs, path, root_type=R.STRUCT, ctx=None):
        import torch
        from dynamicgo_amd import generic as G
        self.G, self.torch, self.n, self.root_type = G, torch, len(msgs), root_type
        self.ps = G.PathSet(to_paths([path]), ctx=ctx)
        in_off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum([len(m) for m in msgs], out=in_off[1:])
        self.arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        self.in_off = torch.from_numpy(in_off).cuda()
        self.max_len = max((len(m) for m in msgs), default=0)

    def buffers(self, rec_cap):
        t = self.torch
        head = t.full((self.n + 1, 4), -0x5A5A5A5B, dtype=t.int32, device="cuda")  # 0xA5A5A5A5
        rec_off = t.zeros(self.n + 1, dtype=t.int64, device="cuda")
        recs = t.full((rec_cap + GUARD, 8), -0x5A5A5A5B, dtype=t.int32, device="cuda")
        return head, rec_off, recs

    def call(self, head, rec_off, recs, rec_cap, recurse, counted=False, stream=None):
        self.G.children_device(self.ps, self.arena, self.in_off, self.n, head, rec_off, recs, rec_cap, recurse=recurse,
                               counted=counted, root_type=self.root_type, stream=stream, max_len=self.max_len)

    def read(self, head, rec_off, recs, rec_cap):
        """(head, rec_off, recs[:min(total, rec_cap)]) as numpy, after checking the guards"""
        G = self.G
        self.torch.cuda.synchronize()
        h, r = head.cpu().numpy(), recs.cpu().numpy()
        assert (h[self.n:].view(np.uint8) == 0xA5).all(), "the 16 bytes after the heads were written"
        assert (r[rec_cap:].view(np.uint8) == 0xA5).all(), "records at or past rec_cap were written"
        off = rec_off.cpu().numpy().astype(np.uint64)
        return (h[:self.n].copy().view(G.KIDS_HEAD_DTYPE).reshape(self.n), off,
                r[:min(int(off[self.n]), rec_cap)].copy().view(G.KIDS_REC_DTYPE).reshape(-1))

    def total(self, recurse):
        """a count-only call: batched Len"""
        head, rec_off, _ = self.buffers(0)
        self.call(head, rec_off, None, 0, recurse)
        self.torch.cuda.synchronize()
        return int(rec_off[self.n].item())

    def run(self, recurse, rec_cap=None):
        cap = self.total(recurse) if rec_cap is None else rec_cap
        head, rec_off, recs = self.buffers(cap)
        self.call(head, rec_off, recs, cap, recurse)
        return self.read(head, rec_off, recs, cap)

    def close(self):
        self.ps.close()


def run_host(msgs, path, recurse, root_type=R.STRUCT):
    """the host entry's arrays, after checking children_batch's objects against them and the checker's bytes"""
    from dynamicgo_amd import generic as G
    got = G.children_records(msgs, to_paths([path])[0], recurse, root_type=root_type)
    names = {R.OK: None, R.NOT_FOUND: "ErrNotFound", R.E_READ: "ErrRead", R.E_TYPE: "ErrDismatchType",
             K.UNSUPPORTED: "ErrUnsupportedType"}
    res = G.children_batch(msgs, to_paths([path])[0], recurse, root_type=root_type)
    assert len(res) == len(msgs)
    for i, (m, r) in enumerate(zip(msgs, res)):
        h, kids = K.children(m, path, recurse, root_type) if i % 16 == 0 or len(msgs) < 300 else (None, None)
        if h is None:
            continue
        assert (r.status, r.error, r.type, r.key_type, r.elem_type, r.direct) == (
            h.status, names[h.status], h.type, h.key_type, h.elem_type, h.direct), i
        assert len(r.children) == len(kids)
        for c, k in zip(r.children, kids):
            assert (c.type, c.start, c.end, c.raw, c.depth, c.n_desc) == (k.type, k.start, k.end, m[k.start:k.end], k.depth,
                                                                         k.n_desc)
            assert c.parent == (None if k.parent == K.NO_PARENT else k.parent) and c.path.kind == k.kind
            assert c.path.val == (K.key_bytes(m, k) if k.kind in (R.STRKEY, R.BINKEY) else k.key)
    return got


def check(msgs, path, recurse, want=None, root_type=R.STRUCT, nested=False):
    """nested: the messages nest beyond Python's recursion limit; the checker's part of run_host needs TG.deep_checker"""
    want = KG.expect(msgs, path, recurse, root_type) if want is None else want
    host = (lambda: run_host(msgs, path, recurse, root_type))
    KG.same(TG.deep_checker(host) if nested else host(), want, "host entry")
    d = Dev(msgs, path, root_type)
    try:
        KG.same(d.run(recurse), want, "device entry")
    finally:
        d.close()
    return want


def deep_reruns():
    """messages the deep passes reran so far on the default context (dg_ctx_counters [12]; synchronizes)"""
    import ctypes as C
    from dynamicgo_amd import _lib
    from dynamicgo_amd.conv import default_context
    out = (C.c_uint64 * 13)()
    _lib.check(_lib.lib().dg_ctx_counters(default_context().h, out, 13, 0))
    return int(out[12])


# -------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def fuzz():
    return KG.fuzz_messages(2048)


@pytest.fixture(params=[1, 0], ids=["wide", "lanes"])
def route(request, knob):
    knob("kids_wide_min", request.param)
    return request.param


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(KG.FUZZ_PATHS))
def test_fuzz(fuzz, name):
    good, bad = fuzz
    path = KG.FUZZ_PATHS[name]
    e_read = {}
    for recurse in (False, True):
        wg = check(good, path, recurse)
        wb = check(bad, path, recurse)
        e_read[recurse] = int((wb[0]["status"] == R.E_READ).sum())
        # what keeps this from being vacuous: conditions on the inputs, from the checker
        if name in KG.CONTAINER_PATHS:
            assert KG.share(wb[0], R.OK) >= 0.20 and KG.share(wb[0], R.E_READ) >= 0.40
        if name == "":
            assert KG.share(wg[0], R.OK) == 1.0
            if recurse:
                assert round(float(wg[0]["count"].mean()), 1) == 62.6 and int(wg[0]["count"].max()) == 146
            else:
                assert round(float(wg[0]["direct"].mean()), 1) == 20.9 and (wg[0]["count"] == wg[0]["direct"]).all()
        if name == "f18":
            assert int((wg[0]["status"] == K.UNSUPPORTED).sum()) == 2025
    if name == "":  # messages that are fine one level deep and ErrRead below
        assert e_read[True] > e_read[False]


def test_hand_built():
    hand = KG.hand_messages()
    msgs = list(hand.values())
    for path in ([(F, 1)], []):
        for recurse in (False, True):
            want = check(msgs, path, recurse)
            if path:
                st = dict(zip(hand, want[0]["status"].tolist()))
                assert st["list<type 5> of 0"] == st["list of -1"] == st["field type 18"] == R.E_READ
                assert st["list<list<type 5> of 0>"] == (R.E_READ if recurse else R.OK)
                assert st["i32"] == K.UNSUPPORTED and st["empty map"] == R.OK
    # containers as the root of the empty path
    for rt, ms in ((R.MAP, [hand[k][3:-8] for k in hand if k.startswith(("map", "empty map"))]),
                   (R.LIST, [hand[k][3:-8] for k in hand if k.startswith(("list", "empty list"))]),
                   (R.I32, [hand["i32"]])):
        for recurse in (False, True):
            check(ms, [], recurse, root_type=rt)


def test_every_prefix():
    msgs = KG.prefixes(KG.every_kind_message())
    for path in ([], [(F, 1)], [(F, 3)], [(F, 3), (R.STRKEY, b"k")]):
        for recurse in (False, True):
            want = check(msgs, path, recurse)
            # the whole message is fine, no prefix that ends inside the node is
            assert want[0]["status"][-1] == R.OK and want[0]["status"][0] == R.E_READ and KG.share(want[0], R.E_READ) > 0.2
            if not path:
                assert (want[0]["status"][:-1] == R.E_READ).all()


def test_chains_around_the_lds_levels():
    """the messages a lane cannot finish in its 8 LDS levels take the deep pass:
    which ones is known from how the chain is built (a field-1 struct chain of
    depth d under f1: the node plus d - 1 levels)"""
    chains = KG.lds_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    for path in KG.CHAIN_PATHS:
        for recurse in (False, True):
            check(msgs, path, recurse)
    # The deep counter moves for exactly the messages that need it, known from how a struct chain of depth d is built.
    # One-level mode skips the chain with one frame per struct: from level 1 under f1 (the node is level 0 and its d - 1
    # structs take levels 1 .. d - 1), from level 0 under the empty path (d structs, levels 0 .. d - 1); 8 levels: d <= 8.
    # Recursive mode keeps the innermost container in registers and stacks the ones around it: d - 1 under f1 (d <= 9),
    # d under the empty path, the root included (d <= 8).
    fits = {(1, False): 8, (1, True): 9, (0, False): 8, (0, True): 8}
    for (steps, recurse), most in fits.items():
        ms = [TG.chain_message("S" * d, "i") for d in (7, 8, 9, 10, 11)] + [b"\x00"] * 70
        need = sum(d > most for d in (7, 8, 9, 10, 11))
        d = Dev(ms, KG.CHAIN_PATHS[steps])
        try:
            before = deep_reruns()
            d.total(recurse)  # the count pass alone
            assert deep_reruns() - before == need, (steps, recurse)
            d.run(recurse)  # count-only, then count and emit
            assert deep_reruns() - before == 4 * need, (steps, recurse)
        finally:
            d.close()


def test_chains_around_max_skip_depth():
    chains = KG.limit_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    last_ok = {}
    for what, ms, path in (("f1", msgs, [(F, 1)]), ("as root", [m[3:-8] for m in msgs], [])):
        for kind in TG.KINDS:
            sel = [i for i, (k, _) in enumerate(chains) if k[0] == kind]
            sub, rt = [ms[i] for i in sel], msgs[sel[0]][0] if what == "as root" else R.STRUCT
            want = TG.deep_checker(lambda: KG.expect(sub, path, False, rt))
            check(sub, path, False, want, rt, nested=True)
            last_ok[what, kind] = 1018 + int((want[0]["status"] == R.OK).sum()) - 1
    for kind in TG.KINDS:  # the flip, one level apart
        assert last_ok["as root", kind] == last_ok["f1", kind] + 1
    want = TG.deep_checker(lambda: KG.expect(msgs, [], False))
    check(msgs, [], False, want, nested=True)
    rmsgs = [TG.chain_message(k, lf) for k, lf in KG.limit_chains_recursive()]
    for path in KG.CHAIN_PATHS:
        want = TG.deep_checker(lambda: KG.expect(rmsgs, path, True))
        assert 0 < KG.share(want[0], R.OK) < 1
        check(rmsgs, path, True, want, nested=True)


def test_wide_route(route):
    wide = KG.wide_messages()
    msgs = list(wide.values())
    for recurse in (False, True):
        want = check(msgs, [(F, 1)], recurse)
    cut = np.array([k.endswith("cut") for k in wide])
    assert (want[0]["status"][cut] == R.E_READ).all() and (want[0]["status"][~cut] == R.OK).all()
    assert int(want[0]["count"].max()) == 1000
    # the nodes as roots, and mixed with messages the lane route takes
    check([m[3:-8] for m, c in zip(msgs, cut) if not c and m[0] == R.LIST], [], False, root_type=R.LIST)
    mixed = msgs + list(KG.hand_messages().values())
    check(mixed, [(F, 1)], True)


def tiny_batch(n):
    """n messages of 1 and 5 bytes in a fixed pattern, and their checker answer built from the two distinct ones"""
    from dynamicgo_amd import generic as G
    kinds = [b"\x00", b"\x02\x00\x01\x01\x00", b"\x7f"]  # no child, one child, ErrRead
    pick = (np.arange(n) * 7 + np.arange(n) // 5) % 3
    ans = [KG.expect([m], [], False) for m in kinds]
    head = np.concatenate([a[0] for a in ans])[pick]
    rec_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(head["count"], out=rec_off[1:])
    recs = np.repeat(ans[1][2], int(rec_off[n]))
    return [kinds[k] for k in pick], (head, rec_off, recs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 256 * 2048 + 1])
def test_geometry(n):
    """block and wave edges of the lane kernels, one past a tile of the scan (2048 counts) and one past the 256 tile
    sums that one round of the base scan takes"""
    msgs, want = tiny_batch(n)
    assert np.array_equal(want[1][1:], np.cumsum(want[0]["count"].astype(np.uint64)))
    d = Dev(msgs, [])
    try:
        KG.same(d.run(False), want, "device entry, n = %d" % n)
    finally:
        d.close()
    if n <= 4097:
        KG.same(run_host(msgs, [], False), want, "host entry, n = %d" % n)
        # 1-byte messages alone: an empty struct or ErrRead, no record at all
        ones = [m if len(m) == 1 else b"\x7f" for m in msgs]
        want = KG.expect(ones, [], False)
        assert int(want[1][-1]) == 0
        d = Dev(ones, [])
        try:
            KG.same(d.run(False), want, "device entry, 1-byte messages, n = %d" % n)
        finally:
            d.close()


def test_field_names_resolve_through_the_descriptor(fuzz):
    import t2jgen
    from dynamicgo_amd import generic as G
    td, msgs = t2jgen.all_types_desc(), fuzz[0][:64]
    for names, path in ((["inners"], [(F, 10)]), (["node", "kids"], [(F, 17), (F, 3)])):
        got = G.children_records(msgs, [G.PathFieldName(x) for x in names], True, desc=td)
        KG.same(got, KG.expect(msgs, path, True), "names %s" % names)
    with pytest.raises(Exception, match="not defined in IDL"):
        G.children_batch(msgs, [G.PathFieldName("no such field")], desc=td)


def test_capacity(fuzz, route):
    msgs = fuzz[0][:300] + list(KG.wide_messages().values())
    for path, recurse in (([], True), ([(F, 1)], False)):
        want = KG.expect(msgs, path, recurse)
        total = int(want[1][-1])
        d = Dev(msgs, path)
        try:
            KG.same(d.run(recurse, total), want, "rec_cap = total")
            head, rec_off, recs = d.run(recurse, total - 1)
            last = int(np.nonzero(want[0]["count"])[0][-1])
            exp = want[0].copy()
            exp[last]["status"], exp[last]["count"] = OVERFLOW, 0
            lo = int(want[1][last])  # every earlier record is there, the overflowed message wrote none
            KG.same((head, rec_off, recs[:lo]), (exp, want[1], want[2][:lo]), "rec_cap = total - 1")
            assert (recs[lo:].view(np.uint8) == 0xA5).all()
            head, rec_off, recs = d.run(recurse, 0)
            exp = want[0].copy()
            exp["status"][want[0]["count"] > 0] = OVERFLOW
            exp["count"] = 0
            KG.same((head, rec_off, recs), (exp, want[1], want[2][:0]), "rec_cap = 0")
        finally:
            d.close()


def test_counted_streams_and_back_to_back(fuzz):
    import torch
    msgs = fuzz[0][:500] + [TG.chain_message("S" * 12, "e")] * 3 + list(KG.wide_messages().values())
    want = KG.expect(msgs, [], True)
    total = int(want[1][-1])
    d = Dev(msgs, [])
    e = Dev(fuzz[1][:400], [(F, 10)])
    want_e = KG.expect(fuzz[1][:400], [(F, 10)], False)
    try:
        one_shot = d.run(True, total)
        KG.same(one_shot, want, "one call")
        # count only, then emit only
        head, rec_off, recs = d.buffers(total)
        d.call(head, rec_off, None, 0, True)
        d.call(head, rec_off, recs, total, True, counted=True)
        got = d.read(head, rec_off, recs, total)
        for a, b in zip(got, one_shot):
            assert a.tobytes() == b.tobytes()
        # a side stream, and two calls on one context with nothing between them
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        b1, b2 = d.buffers(total), e.buffers(int(want_e[1][-1]))
        with torch.cuda.stream(side):
            d.call(*b1, total, True, stream=side)
        e.call(*b2, int(want_e[1][-1]), False)
        d.call(head, rec_off, recs, total, True)
        torch.cuda.synchronize()
        KG.same(d.read(*b1, total), want, "side stream")
        KG.same(e.read(*b2, int(want_e[1][-1])), want_e, "back to back, the other batch")
        KG.same(d.read(head, rec_off, recs, total), want, "back to back")
    finally:
        d.close()
        e.close()


def test_neighbours(fuzz, route):
    msgs = fuzz[0][:257] + list(KG.wide_messages().values())[:10]
    for victim in (0, 100, 256, 260):
        for junk in (b"\xff" * 40, b"\x0f\x00\x01\x0a\x7f\xff\xff\xff" + b"\0" * 24, b""):
            bad = list(msgs)
            bad[victim] = junk
            for recurse in (False, True):
                a, b = KG.expect(msgs, [], recurse), KG.expect(bad, [], recurse)
                d = Dev(bad, [])
                try:
                    got = d.run(recurse)
                finally:
                    d.close()
                KG.same(got, b, "a batch with garbage at %d" % victim)
                keep = np.arange(len(msgs)) != victim
                assert got[0][keep].tobytes() == a[0][keep].tobytes()
                assert np.array_equal(got[1][1:][keep] - got[1][:-1][keep], a[1][1:][keep] - a[1][:-1][keep])
                lo, hi = int(a[1][victim]), int(a[1][victim + 1])
                assert got[2].tobytes() == a[2][:lo].tobytes() + got[2][lo:int(got[1][victim + 1])].tobytes() + a[2][hi:].tobytes()


def test_refusals_and_empty_batch():
    from dynamicgo_amd import _lib
    from dynamicgo_amd import generic as G
    L = _lib.lib()
    head, rec_off, recs = G.children_records([], [])
    assert len(head) == 0 and rec_off.tolist() == [0] and len(recs) == 0 and G.children_batch([], []) == []
    d = Dev([b"\x00"], [])
    try:
        h, o, r = d.buffers(4)
        with G.PathSet(to_paths([[(F, 1)], [(F, 2)]])) as two:
            assert L.dg_kids_batch_device(two.ctx.h, two.h, R.STRUCT, 0, d.arena.data_ptr(), d.in_off.data_ptr(), 1, h.data_ptr(),
                                          o.data_ptr(), r.data_ptr(), 4, None, 0) == -6  # DG_E_ARG
            assert b"exactly 1" in L.dg_last_error()
        ps = d.ps
        assert L.dg_kids_batch_device(ps.ctx.h, ps.h, R.STRUCT, 0, None, d.in_off.data_ptr(), 1, h.data_ptr(), o.data_ptr(),
                                      r.data_ptr(), 4, None, 0) == -1
        assert L.dg_kids_batch_device(ps.ctx.h, ps.h, R.STRUCT, 0, d.arena.data_ptr(), d.in_off.data_ptr(), 1, None, o.data_ptr(),
                                      r.data_ptr(), 4, None, 0) == -1
        assert L.dg_kids_batch_device(ps.ctx.h, ps.h, R.STRUCT, 8, d.arena.data_ptr(), d.in_off.data_ptr(), 1, h.data_ptr(),
                                      o.data_ptr(), r.data_ptr(), 4, None, 0) == -1
        assert L.dg_kids_batch_device(ps.ctx.h, ps.h, R.STRUCT, 0, None, None, 0, None, None, None, 0, None, 0) == 0  # n = 0
        assert L.dg_kids_batch_host(ps.ctx.h, ps.h, R.STRUCT, 2, None, None, 0, None, None, None, 0, None) == -1  # COUNTED
        d.torch.cuda.synchronize()
        assert (h.cpu().numpy().view(np.uint8) == 0xA5).all()
    finally:
        d.close()
    # count only: batched Len
    msgs = [m for m in KG.wide_messages().values()][:10]
    head, rec_off, recs = G.children_records(msgs, to_paths([[(F, 1)]])[0], count_only=True)
    want = KG.expect(msgs, [(F, 1)], False)
    assert head.tobytes() == want[0].tobytes() and np.array_equal(rec_off, want[1]) and len(recs) == 0
