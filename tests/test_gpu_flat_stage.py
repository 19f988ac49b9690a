"""GPU: the flat kernel's prologue (j2t_flat.h, phase 0), where it can go
wrong. A block stages its JSON span, copies the descriptor's image (the blob
and the number tables, built once per descriptor: flat_image.h) and takes its
per-message offsets from one load per lane; every case here is compared byte
for byte and status for status with the reference's engine.

  block shape    n around the 64-message block, the arena starting at every
                 kind of offset into a 16-byte line
  staging        a block too long to stage between two staged ones
  wrapped mode   Mixed's flat member, a partial last block, misaligned
  output slots   tight, odd bases, guard slots between (tests/slotguard.py)
  tables         number tokens that read each table of the image, at the
                 window's seams and the exact-power path
  descriptors    blobs that take one, two and more 16-byte loads per thread,
                 at FL_DESC and just past it
  ownership      two descriptors alternating, device- and host-created
                 descriptors, one destroyed before the next is made"""
import ctypes as C
import random

import numpy as np
import pytest

import descgen
import numgen
import oracle
import slotguard as SG
from dynamicgo_amd import _lib, conv, thrift as T, workloads as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAT = 1 << 19  # DG_F_FLAT_PATH
FL_DESC = 16 * 1024


def _chk():
    return oracle.RefOracle() or oracle.PortOracle()


_expect_cache = {}


def _expect(fl, msgs, flags):
    """The oracle's (rets, outs) of a batch, computed once per (descriptor, batch, flags)."""
    key = (fl.blob, tuple(msgs), flags & 0xFFFF)
    if key not in _expect_cache:
        _expect_cache[key] = _chk().j2t_batch(fl, msgs, flags & 0xFFFF)
    return _expect_cache[key]


def _device(fl, msgs, flags, lead=0, ctx=None, dh=None):
    """dg_j2t_batch_device over the messages laid out back to back behind
    `lead` bytes of another message's tail, each in a roomy 8-aligned slot:
    (status words, out_len, the bytes of each slot)."""
    import torch
    ctx = ctx or conv.default_context()
    dh = dh or ctx.desc(fl)
    n = len(msgs)
    lens = np.fromiter((len(m) for m in msgs), dtype=np.int64, count=n)
    in_off = np.full(n + 1, lead, dtype=np.int64)
    np.cumsum(lens, out=in_off[1:])
    in_off[1:] += lead
    a = np.frombuffer((b'{"ByteField":1} , ' * 2)[-lead:] * (lead > 0) + b"".join(msgs) + b"\0" * 64, dtype=np.uint8).copy()
    assert a.size == int(in_off[-1]) + 64
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((lens * 4 + 64 + 7) // 8 * 8, out=out_off[1:])
    d_src, d_in, d_oo = (torch.from_numpy(x).to(DEV) for x in (a, in_off, out_off))
    assert d_src.data_ptr() % 16 == 0  # `lead` is the first message's offset in its 16-byte line
    d_out = torch.full((int(out_off[-1]) + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    d_ol = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_ret = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    d_pend = torch.zeros(4, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dg_j2t_batch_device(ctx.h, dh, fl.root_type, d_src.data_ptr(), d_in.data_ptr(), n, flags,
                                              d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(),
                                              d_pend.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out, ol = d_out.cpu().numpy(), d_ol.cpu().numpy().view(np.uint32)
    ret = d_ret.cpu().numpy().view(np.uint64)
    assert int(d_pend[0]) == 0  # no slot is too small
    return ret, ol, [out[int(out_off[i]):int(out_off[i]) + min(int(ol[i]), int(out_off[i + 1] - out_off[i]))].tobytes()
                     for i in range(n)]


def _same(fl, msgs, flags, **kw):
    """The launch against the oracle; returns the mismatches."""
    er, eo = _expect(fl, msgs, flags)
    ret, ol, outs = _device(fl, msgs, flags, **kw)
    bad = []
    for i in range(len(msgs)):
        keeps = int(er[i]) == 0 or len(eo[i]) > 0
        want = eo[i] if keeps else b""
        if int(ret[i]) != int(er[i]) or int(ol[i]) != len(want) or outs[i] != want:
            bad.append((i, msgs[i][:80], hex(int(ret[i])), hex(int(er[i])), int(ol[i]), len(want)))
    return bad


@pytest.fixture(scope="module")
def simple():
    return T.flatten(W.simple_desc())


@pytest.fixture(scope="module")
def c2():
    return W.gen_flat_batch(random.Random(42), 129)


# ---------------------------------------------------------------- block shape and alignment
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_block_counts_and_partial_last_blocks(simple, c2, n):
    for flags in (0x1, 0x1 | FLAT):
        bad = _same(simple, c2[:n], flags)
        assert not bad, (n, hex(flags), bad[:4])


@pytest.mark.parametrize("lead", [0, 1, 7, 9, 15, 17])
def test_arena_alignment(simple, c2, lead):
    """base = lo & ~15 and the clamp of the last 16-byte load depend on where
    the first message starts in its line; 65 messages: a full block and a
    block of one"""
    for n in (65, 1):
        bad = _same(simple, c2[:n], 0x1, lead=lead)
        assert not bad, (lead, n, bad[:4])


# ---------------------------------------------------------------- staged and unstaged blocks
def test_unstaged_block_between_staged_ones(simple, c2):
    """Block 1 holds a ~20 KB message between 63 small ones: its span does
    not fit the stage, so its messages are copied one by one from the offsets
    the block loaded; blocks 0 and 2 are staged. The long message converts by
    its own route."""
    long_msg = ('{"I32Field":7,"StringField":"%s","ByteField":1}' % ("abcdefghij" * 2000)).encode()
    msgs = c2[:64] + c2[64:95] + [long_msg] + c2[95:127] + c2[:64]
    assert len(msgs) == 192 and msgs[95] is long_msg  # the middle of block 1
    for lead in (0, 11):
        bad = _same(simple, msgs, 0x1, lead=lead)
        assert not bad, (lead, bad[:4])
    er, eo = _expect(simple, msgs, 0x1)
    assert int(er[95]) == 0 and len(eo[95]) > 20000


# ---------------------------------------------------------------- wrapped mode
def test_wrapped_mode_partial_block_misaligned():
    fl = T.flatten(W.mixed_desc())
    rng = random.Random(9)
    msgs = [b'{"Flat":' + W.simple_obj(rng).encode() + b"}" for _ in range(65)]
    msgs = [m for m in msgs if len(m) <= 256] + [b'{"Flat":{"ByteField":1}}'] * 65
    msgs = msgs[:65]
    for lead in (5, 0):
        bad = _same(fl, msgs, 0x1, lead=lead)
        assert not bad, (lead, bad[:4])
    ctx = conv.default_context()
    ctx.stats(reset=True)
    _device(fl, msgs, 0x1, lead=5)
    assert ctx.stats(reset=True)[0] * 4 <= len(msgs)  # converted by the flat kernel, not handed on


# ---------------------------------------------------------------- output offsets
def test_output_slots_tight_odd_and_guarded(simple, c2):
    """64 messages in slots of exactly their size or one byte more, each
    slot's base at an odd address of its 16-byte line, guard slots between
    (the sandwich and its control launch of tests/slotguard.py): 129 messages,
    three blocks, the last of one message whose end is the table's final
    entry."""
    import torch
    chk = _chk()
    ctx = conv.default_context()
    dh = ctx.desc(simple)
    for flags in (0x1, 0x1 | FLAT):
        items = []
        for k, m in enumerate(c2[:64]):
            ret, out = chk.j2t(simple, m, flags & 0xFFFF)
            assert ret == 0
            items.append(SG.Item(m, len(out) + (k & 1), ret, out, phase=(2 * k + 1) % 16))
        spacer = b'{"ByteField":7}'
        sret, sout = chk.j2t(simple, spacer, flags & 0xFFFF)

        def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
            _lib.check(_lib.lib().dg_j2t_batch_device(ctx.h, dh, simple.root_type, d_src.data_ptr(), d_in.data_ptr(), n,
                                                      flags, d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(),
                                                      d_ret.data_ptr(), d_pend.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
        sw, runs = SG.check(launch, items, spacer, sout, DEV, spacer_ret=sret)
        assert len(sw.msgs) == 129 and all(int(sw.off[t]) % 2 == 1 for t in sw.tested)


# ---------------------------------------------------------------- tables from the image
def number_tokens():
    i64 = ["1", "10", "9", "123456789012345678", "999999999999999999", "1234567890123456789", "9223372036854775807",
           "-9223372036854775808", "9223372036854775808", "-9223372036854775809", "-1", "0"]
    i64 += ["1" + "0" * k for k in range(1, 20)] + ["9" * k for k in range(1, 20)]  # every entry of p10u
    dbl = ["1.5e-41", "1.5e-40", "1.5e+23", "1.5e+24", "7e-41", "7e-40", "7e23", "7e24",  # both sides of the window
           "1e22", "1e23", "123456789012345e22", "123456789012345e-22", "1e-22", "1e-23",  # the exact-power path
           "1.7976931348623157e308", "4.9e-324", "0.1", "2.5", "-0.0"]
    dbl += ["1e%d" % k for k in range(-23, 38)]  # every entry of p10d, both ways
    dbl += ["3.%se%d" % ("14159265358979" [:k % 14 + 1], k) for k in range(-42, 26)]  # every entry of the window
    dbl += ["12345678.12345678", "0.000001", "123456789012345.6789", "1234567890.123456789"]
    seams = [t for t, e in numgen.seam_cases() if e in (-41, -40, 23, 24)]  # the window's seams, numgen's own tokens
    dbl += seams[::max(1, len(seams) // 64)]
    return i64, dbl


def test_number_tables_from_the_image(simple):
    i64, dbl = number_tokens()
    msgs = []
    for t in i64 + dbl:
        msgs.append(('{"I64Field":%s}' % t).encode())
        msgs.append(('{"DoubleField":%s}' % t).encode())
        msgs.append(('{"ByteField":1,"I64Field":%s,"DoubleField":%s,"I32Field":2}' % (i64[len(msgs) % len(i64)], t)).encode())
    msgs = [m for m in msgs if len(m) <= 256]
    er, eo = _expect(simple, msgs, 0x1)
    assert sum(int(r) == 0 for r in er) * 2 > len(msgs)  # most convert: the tables are read
    ctx = conv.default_context()
    for flags in (0x1, 0x1 | FLAT):
        bad = _same(simple, msgs, flags, lead=3)
        assert not bad, (hex(flags), len(bad), bad[:4])
    ctx.stats(reset=True)
    good = [m for m, r in zip(msgs, er) if int(r) == 0]
    _device(simple, good, 0x1 | FLAT)
    bails = ctx.stats(reset=True)[0]
    assert bails * 4 <= len(good), (bails, len(good))  # the flat kernel's own parser took them


# ---------------------------------------------------------------- descriptor sizes
SIZES = {"two loads per thread": 6144, "more than two": 12288, "just under FL_DESC": FL_DESC - 8,
         "FL_DESC": FL_DESC, "just over FL_DESC": FL_DESC + 8}


@pytest.fixture(scope="module")
def sized_messages():
    return [m for m, _ in descgen.sizes_messages()][:200]


@pytest.mark.parametrize("what", list(SIZES))
def test_descriptor_sizes(sized_messages, what):
    target = SIZES[what]
    fl = T.flatten(descgen.sized_desc(target))
    assert len(fl.blob) == target
    ctx = conv.default_context()
    for flags in (0x1, 0x1 | FLAT):
        bad = _same(fl, sized_messages, flags, lead=9)
        assert not bad, (what, hex(flags), bad[:4])
    er, _ = _expect(fl, sized_messages, 0x1)
    good = [m for m, r in zip(sized_messages, er) if int(r) == 0]
    ctx.stats(reset=True)
    _device(fl, good, 0x1)
    bails = ctx.stats(reset=True)[0]
    assert bails < len(good) and len(good) * 2 > len(sized_messages), (what, bails, len(good))


# ---------------------------------------------------------------- image ownership
def test_two_descriptors_alternate_on_one_context(simple, c2):
    fl2 = T.flatten(descgen.sized_desc(12288))
    m2 = [m for m, _ in descgen.sizes_messages()][:130]
    ctx = conv.Context(0)
    try:
        for _ in range(3):
            assert not _same(simple, c2, 0x1, ctx=ctx)
            assert not _same(fl2, m2, 0x1, ctx=ctx)
    finally:
        ctx.close()


def _create(ctx, fl, device):
    import torch
    h = C.c_void_p()
    if device:
        d_blob = torch.frombuffer(bytearray(fl.blob), dtype=torch.uint8).to(DEV)
        _lib.check(_lib.lib().dg_desc_create_device(ctx.h, d_blob.data_ptr(), d_blob.numel(), C.byref(h)))
        del d_blob
        torch.cuda.synchronize()
    else:
        _lib.check(_lib.lib().dg_desc_create(ctx.h, fl.blob, len(fl.blob), C.byref(h)))
    return h


def test_host_and_device_created_descriptors_agree(simple, c2):
    ctx = conv.Context(0)
    try:
        hs = [_create(ctx, simple, dev) for dev in (False, True)]
        res = [_device(simple, c2, 0x1, lead=7, ctx=ctx, dh=h) for h in hs]
        assert list(res[0][0]) == list(res[1][0]) and list(res[0][1]) == list(res[1][1]) and res[0][2] == res[1][2]
        assert not _same(simple, c2, 0x1, lead=7, ctx=ctx, dh=hs[1])
        for h in hs:
            _lib.lib().dg_desc_destroy(h)
    finally:
        ctx.close()


def test_descriptor_destroyed_and_another_created(simple, c2):
    fl2 = T.flatten(descgen.sized_desc(6144))
    m2 = [m for m, _ in descgen.sizes_messages()][:130]
    ctx = conv.Context(0)
    try:
        for fl, msgs in ((simple, c2), (fl2, m2), (simple, c2[:65]), (fl2, m2[:1])):
            h = _create(ctx, fl, False)
            assert not _same(fl, msgs, 0x1, ctx=ctx, dh=h)
            _lib.lib().dg_desc_destroy(h)
    finally:
        ctx.close()
