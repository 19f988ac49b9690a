"""GPU: the parts of the batched GetByPath kernels (tget_device.h,
tget_kern.hip, tget_host.hip) that only the device build has, against the
checker (tgetref.py), every field of every record: the deep pass with a queue
longer than its grid and frames left behind by earlier pairs, frames opened by
every container kind around the 8 LDS frames and around MaxSkipDepth, the
16-byte key compare, integer keys at the edges of their widths, partial blocks
with every path count, and launches without a synchronisation between them.
The inputs are tgetgen.py's; test_tget_walk_host.py runs the same walk over them
on the CPU. Where a test uploads its own arena, its 16 spare bytes are 0xAA."""
import random
import struct

import numpy as np
import pytest

import t2jgen
import tgetgen as TG
import tgetref as R
from test_gpu_tget import FUZZ_PATHS, check, expect, same, share, to_paths

pytestmark = pytest.mark.gpu

F, S, N = R.FIELD, R.STRKEY, R.INTKEY
GUARD = 64  # entries behind every output, which no launch may touch
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


class Upload:
    """A batch on the device: the arena with 16 bytes of 0xAA behind it, and the offsets."""

    def __init__(self, msgs):
        import torch
        self.n = len(msgs)
        self.in_off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum([len(m) for m in msgs], out=self.in_off[1:])
        self.arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\xAA" * 16, dtype=np.uint8).copy()).cuda()
        self.d_off = torch.from_numpy(self.in_off).cuda()
        self.max_len = max((len(m) for m in msgs), default=0)


class Outputs:
    """rec, val_off and val_len of n * P pairs, GUARD more entries behind each, all pre-filled with 0x5A."""

    def __init__(self, n, P):
        import torch
        self.n, self.P = n, P
        self.rec = torch.full((n * P + GUARD, 4), FILL32, dtype=torch.int32, device="cuda")
        self.voff = torch.full((n * P + GUARD,), FILL64, dtype=torch.int64, device="cuda")
        self.vlen = torch.full((n * P + GUARD,), FILL32, dtype=torch.int32, device="cuda")

    def verify(self, want, in_off, what):
        """after a synchronisation: the records, val_off and val_len against the checker's, and the guards"""
        from dynamicgo_amd.generic import REC_DTYPE
        q = self.n * self.P
        rec, voff, vlen = self.rec.cpu().numpy(), self.voff.cpu().numpy(), self.vlen.cpu().numpy()
        assert (rec[q:] == FILL32).all() and (voff[q:] == FILL64).all() and (vlen[q:] == FILL32).all(), \
            what + ": a store past the last pair"
        same(rec[:q].view(REC_DTYPE).reshape(self.n, self.P), want, what)
        ok = want["status"] == R.OK
        assert (vlen[:q].reshape(self.n, self.P) == np.where(ok, want["end"] - want["start"], 0)).all(), what
        assert (voff[:q].reshape(self.n, self.P) == in_off[:-1, None] + want["start"]).all(), what


def launch(ps, up, out, root_type=R.STRUCT, stream=None):
    from dynamicgo_amd import generic as G
    G.get_by_path_device(ps, up.arena, up.d_off, up.n, out.rec, out.voff, out.vlen, root_type=root_type,
                         stream=stream, max_len=up.max_len)


def run_guarded(msgs, paths, want, what, root_type=R.STRUCT):
    """the device entry with val_off / val_len, 0xAA behind the arena and guarded outputs"""
    import torch
    from dynamicgo_amd import generic as G
    up, out = Upload(msgs), Outputs(len(msgs), len(paths))
    with G.PathSet(to_paths(paths)) as ps:
        launch(ps, up, out, root_type)
        torch.cuda.synchronize()
    out.verify(want, up.in_off, what)


def deep_pairs(chains, paths):
    """how many (message, path) pairs open more than the 8 LDS frames, from how the chains are built"""
    return sum(TG.chain_frames(k, lf, p) > TG.LDS_FRAMES for k, lf in chains for p in paths)


def chains_of(rng, depths, count):
    return [TG.random_chain(rng, rng.choice(depths)) for _ in range(count)]


def test_deep_queue_longer_than_the_grid():
    """8 400 deep pairs: the 4 096 deep lanes go round twice and part of a third
    time, every lane over the frames its earlier pairs left."""
    rng = random.Random(21)
    deep, shallow = chains_of(rng, range(10, 15), 2100), chains_of(rng, range(0, 6), 500)
    assert deep_pairs(deep, TG.CHAIN_PATHS) == 8400 > 2 * 4096 and deep_pairs(shallow, TG.CHAIN_PATHS) == 0
    chains = deep + shallow
    rng.shuffle(chains)
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want = expect(msgs, TG.CHAIN_PATHS)
    assert share(want, R.OK) == 0.75
    check(msgs, TG.CHAIN_PATHS, want)
    run_guarded(msgs, TG.CHAIN_PATHS, want, "device entry with values")


@pytest.fixture(scope="module")
def limit_chains():
    rng = random.Random(22)
    chains = [(k * d, lf) for k in TG.KINDS for d in range(1021, 1026) for lf in TG.LEAVES]
    chains += [TG.random_chain(rng, d) for d in range(1021, 1026) for _ in range(2)]
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    return msgs, TG.deep_checker(lambda: expect(msgs, TG.CHAIN_PATHS))


def test_frame_edges_by_container(limit_chains):
    """Each way a frame is opened (struct, list, set, map by value, map by key,
    a list of strings at the bottom) and the two ways it is not (a container
    that is a multiplication, a string inside one), at 6..10 levels around the
    LDS frames and at 1021..1025 around MaxSkipDepth."""
    rng = random.Random(23)
    chains = [(k * d, lf) for k in TG.KINDS for d in range(6, 11) for lf in TG.LEAVES]
    chains += [TG.random_chain(rng, d) for d in range(6, 11) for _ in range(5)]
    n_deep = deep_pairs(chains, TG.CHAIN_PATHS)
    assert 0.25 < n_deep / (4 * len(chains)) < 0.75  # both sides of the LDS frames
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want = expect(msgs, TG.CHAIN_PATHS)
    check(msgs, TG.CHAIN_PATHS, want)
    run_guarded(msgs, TG.CHAIN_PATHS, want, "6..10 levels with values")
    msgs, want = limit_chains
    assert share(want, R.OK) >= 0.25 and share(want, R.E_READ) >= 0.25, (share(want, R.OK), share(want, R.E_READ))
    check(msgs, TG.CHAIN_PATHS, want)
    run_guarded(msgs, TG.CHAIN_PATHS, want, "1021..1025 levels with values")


def test_long_keys():
    msgs, how = TG.long_key_messages(random.Random(7), 256)
    for v in (TG.EXACT, TG.LAST, TG.LONGER, TG.SHORTER, TG.BYTE8):  # every near miss of every length that has it
        for j, key in enumerate(TG.KEYS):
            if TG.key_variant(key, v) is not None:
                assert any(h[j] == v for h in how), (v, j)
    for ps in TG.long_key_paths():
        want = expect(msgs, ps)
        for col in range(8):
            assert 0.2 < share(want[:, col], R.OK) < 0.8, (col, share(want[:, col], R.OK))
        check(msgs, ps, want)
        run_guarded(msgs, ps, want, "keys with values")
    # the map itself as the root, and as the batch's last message one whose found value ends on the arena's last byte
    roots = [m[3:-1] for m in msgs]
    for rooted in TG.long_key_paths(prefix=()):
        key = rooted[7][0][1] if rooted[7][0][0] == S else rooted[7][0][1][4:]
        last = bytes([R.STRING, R.I32]) + b"\0\0\0\1" + TG._wstr(key) + b"\x7f\xff\xff\xff"
        batch = roots + [last]
        want = expect(batch, rooted, R.MAP)
        assert want[-1, 7]["status"] == R.OK and want[-1, 7]["end"] == len(last) and share(want[-1], R.OK) == 0.125
        check(batch, rooted, want, R.MAP)
        run_guarded(batch, rooted, want, "map root", R.MAP)


def test_int_key_extremes():
    msgs = TG.int_key_messages(random.Random(8), 256)
    hits = 0
    for ps in TG.int_key_paths():
        want = expect(msgs, ps)
        hits += int((want["status"] == R.OK).sum())
        check(msgs, ps, want)
    assert hits > 256 * 21 * 0.4  # 21 keys a message at p = 0.6 (an i8 -128 also answers to 128, -1 to 255)
    # each map as the root; the batch's last message holds the width's lowest key alone, its value the arena's last
    # bytes
    for kt, fmt, keys in TG.INT_KEY_SETS:
        full = struct.pack(">bbi", kt, R.STRING, len(keys))
        full += b"".join(struct.pack(fmt, k) + TG._wstr(b"x") for k in keys)
        last = struct.pack(">bbi", kt, R.STRING, 1) + struct.pack(fmt, min(keys)) + TG._wstr(b"end")
        paths = [[(N, v)] for v in sorted(set(keys) | {128, 255, 2 ** 31})[:8]]
        want = expect([full, full[:-1], last], paths, R.MAP)
        hit = want[2][want[2]["status"] == R.OK]  # one lookup finds it (an i8 -128 as 128)
        assert len(hit) == 1 and hit[0]["end"] == len(last) and share(want[0], R.OK) >= 0.5
        check([full, full[:-1], last], paths, want, R.MAP)
        run_guarded([full, full[:-1], last], paths, want, "int-keyed map as the root", R.MAP)
    m = b"\x08\xff\xfb\0\0\0\x01" + b"\x08\x80\x00\0\0\0\x02" + b"\x08\x00\x05\0\0\0\x03" + b"\0"
    paths = [[(F, -5)], [(F, -32768)], [(F, 5)], [(F, -1)], [(F, 32767)], [(F, 251)]]
    want = expect([m], paths)
    assert want[0]["status"].tolist() == [R.OK] * 3 + [R.NOT_FOUND] * 3
    check([m], paths, want)


def test_sixteen_steps():
    msgs, paths = TG.sixteen_step_inputs()
    want = expect(msgs, paths)
    assert share(want[:2], R.OK) == 1.0 and share(want[2:], R.E_READ) > 0.5
    check(msgs, paths, want)
    run_guarded(msgs, paths, want, "16 steps with values")


PARTIAL_N = (1, 31, 33, 63, 65, 255, 257)
PARTIAL_PATHS = [FUZZ_PATHS[k] for k in ("f18", "f9.f1", "f10[1].f2", "f11[2]", "f17.f2.f2.f1", "f9[0]", "f12{1}", "")]


@pytest.fixture(scope="module")
def short_fuzz():
    rng = random.Random(24)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td, keep_p=0.3) for _ in range(max(PARTIAL_N))]
    return msgs, expect(msgs, PARTIAL_PATHS)  # path k's record does not depend on the set around it


@pytest.mark.parametrize("spread", [1, 2, 4])
def test_partial_blocks_and_every_path_count(short_fuzz, knob, spread):
    """n * P * spread is never a multiple of the block (n is odd), P runs through
    1..8, and nothing may be stored past the last pair."""
    import torch
    from dynamicgo_amd import generic as G
    msgs, want = short_fuzz
    knob("tget_spread", spread)
    ups = {n: Upload(msgs[:n]) for n in PARTIAL_N}
    for P in range(1, 9):
        with G.PathSet(to_paths(PARTIAL_PATHS[:P])) as ps:
            outs = {n: Outputs(n, P) for n in PARTIAL_N}
            for n in PARTIAL_N:
                launch(ps, ups[n], outs[n])
            torch.cuda.synchronize()
        for n in PARTIAL_N:
            outs[n].verify(want[:n, :P], ups[n].in_off, "n %d, P %d, spread %d" % (n, P, spread))


def test_back_to_back_launches():
    """Launches of one context with no synchronisation between them, on one
    stream and then alternating between two, and the alternation once more on a
    fresh context: the deep queue's two counters, the event that orders the
    streams, and the queue growing while the launch before may still fill it."""
    import torch
    from dynamicgo_amd import generic as G
    from dynamicgo_amd.conv import Context
    rng = random.Random(25)
    deep, flat = chains_of(rng, range(10, 15), 2250), chains_of(rng, range(0, 6), 60)
    p4, p3 = TG.CHAIN_PATHS, TG.CHAIN_PATHS[:3]
    plan = [(flat[:30] + deep[:10] + flat[30:], p4), (flat, p4), (deep[10:310] + flat[:7], p3), (flat[:33], p3),
            (deep + flat[:5], p4), (flat[:9] + deep[300:310], p4)]
    assert [deep_pairs(c, p) for c, p in plan] == [40, 0, 900, 0, 9000, 40]
    plan = [([TG.chain_message(k, lf) for k, lf in c], p) for c, p in plan]
    wants = [expect(m, p) for m, p in plan]
    # contexts of their own: the queue starts empty and has to grow at the third and the fifth launch
    ctxs = [Context(0), Context(0)]
    try:
        sets = [{4: G.PathSet(to_paths(p4), ctx=c), 3: G.PathSet(to_paths(p3), ctx=c)} for c in ctxs]
        ups = [Upload(m) for m, _ in plan]
        outs = [[Outputs(len(m), len(p)) for m, p in plan] for _ in range(3)]
        side = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for r, (ps, streams) in enumerate(((sets[0], [None]), (sets[0], side), (sets[1], side))):
            for j, (up, (_, p)) in enumerate(zip(ups, plan)):
                launch(ps[len(p)], up, outs[r][j], stream=streams[j % len(streams)])
        torch.cuda.synchronize()
        for r, name in enumerate(("one stream", "then two streams", "two streams, fresh context")):
            for j, up in enumerate(ups):
                outs[r][j].verify(wants[j], up.in_off, "%s, launch %d" % (name, j + 1))
        for ps in sets:
            ps[4].close()
            ps[3].close()
    finally:
        for c in ctxs:
            c.close()
