"""GPU: every kernel that writes into caller-given slots, at tight slots.

Each route's messages run in one sandwich batch (tests/slotguard.py): every
message at capacities 0, need-9, need-8, need-7, need-1, need, need+1, need+7
and need+8, between spacer slots, the arena prefilled two ways, against a
control launch. A message that fits must equal the oracle's, one that does not
must report DG_ST_OUT_OVERFLOW with the bytes it needs, and no launch may
store a byte outside a message's own slot. Where dg_ctx_stats can tell, the
route's own kernel must convert the exactly fitting messages itself: as many
hand-offs to the exact machine at cap == need as with 64 bytes to spare.

j2t slot bases are 8-aligned in the sandwich (the fast case of
include/dgj2t.h; the spacer behind an odd capacity starts unaligned, and so
do the back-to-back exact slots of the hand-off count, which the ABI allows),
t2j slot bases 8-aligned in both 16-byte phases.

Two of the bounds cannot be told apart from a stricter one by any output:
j2t_flat.h's per-field `off + F.size >= cap` (with `>` the field ends exactly
at cap, and the STOP check `len <= cap` still declines the message to the list
pass, which reports the overflow), and t2j_wave.h's `O + tot > cap` (with `>=`
an exactly fitting message is redone by the lane pass with the same bytes, and
no counter of the context counts t2j hand-offs)."""
import base64
import random
import struct

import numpy as np
import pytest

import oracle
import slotguard as SG
import t2jgen
from dynamicgo_amd import _lib, conv, thrift as T, workloads as W

pytestmark = pytest.mark.gpu

if oracle.ref_lib_path() is None:
    pytest.skip("oracle/_ref not built", allow_module_level=True)

DEV = "cuda:0"
FLAT, NO_FLAT, NO_WAVE = 1 << 19, 1 << 21, 1 << 18
CONV_EXC = 1 << 9


# ---------------------------------------------------------------- launches
def j2t_launch(flat, flags):
    import torch
    ctx = conv.default_context()
    dh = ctx.desc(flat)

    def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
        _lib.check(_lib.lib().dg_j2t_batch_device(ctx.h, dh, flat.root_type, d_src.data_ptr(), d_in.data_ptr(), n, flags,
                                                  d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(),
                                                  d_pend.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return launch


def t2j_launch(flat, opts):
    import torch
    ctx = conv.default_context()
    dh = ctx.desc_t2j(flat)

    def launch(d_src, d_in, n, d_out, d_oo, d_ol, d_ret, d_pend):
        _lib.check(_lib.lib().dg_t2j_batch_device(ctx.h, dh, flat.root_type, d_src.data_ptr(), d_in.data_ptr(), n, opts,
                                                  d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    return launch


def j2t_oracle(flat, flags):
    chk = oracle.RefOracle()
    return lambda m: chk.j2t(flat, m, flags)


def t2j_oracle(flat, opts):
    chk = oracle.RefT2JOracle()
    side = T.flatten_t2j(flat)
    return lambda m: chk.t2j(flat, side, m, opts)


def handoffs(launch, items, spare):
    """(bails, deeps) of dg_ctx_stats over the two launches of the items'
    messages alone (no spacers), each in a slot of exactly need + spare bytes,
    the slots back to back (so at any byte alignment, which the j2t ABI
    allows); every message must convert."""
    ctx = conv.default_context()
    off = np.cumsum([SG.GUARD] + [len(it.out) + spare for it in items])
    ctx.stats(reset=True)
    runs = SG.launch_twice(launch, [it.msg for it in items], off, int(off[-1]) + SG.GUARD, DEV)
    bails, deeps = ctx.stats(reset=True)
    for i, it in enumerate(items):
        assert int(runs[0].ret[i]) == it.ret and int(runs[0].out_len[i]) == len(it.out), (it.msg, hex(int(runs[0].ret[i])))
        assert runs[0].out[off[i]:off[i] + len(it.out)].tobytes() == it.out, it.msg
    return bails, deeps


def exact_fit_stays(launch, items):
    """The messages that convert, once each, at cap == need and at need + 64:
    the same number of hand-offs to the exact machine, and not all of them."""
    seen, uniq = set(), []
    for it in items:
        if it.ret == 0 and it.msg not in seen:
            seen.add(it.msg)
            uniq.append(it)
    roomy = handoffs(launch, uniq, 64)
    exact = handoffs(launch, uniq, 0)
    assert exact == roomy, "hand-offs (bails, deeps) at cap == need %r, with 64 bytes to spare %r" % (exact, roomy)
    assert roomy[0] < 2 * len(uniq), "every message went to the list pass: %r of 2 x %d" % (roomy, len(uniq))
    return roomy


# ---------------------------------------------------------------- j2t inputs
def _b64(n_chars):
    raw = bytes(range(65, 65 + n_chars // 4 * 3))
    return base64.b64encode(raw).decode()


def flat_messages():
    rng = random.Random(5)
    msgs = [b'{"ByteField":7}', b'{"I32Field":-5,"ByteField":1}', b'{"I32Field":1}', b'{"StringField":"a"}',
            b'{"ByteField":1,"I64Field":-2,"DoubleField":1.5,"I32Field":3,"StringField":"s","BinaryField":"aGk="}',
            b'{"ByteField":1,"x":0,"I64Field":-2,"DoubleField":1.5,"I32Field":3,"StringField":"s","BinaryField":"aGk=","y":1}']
    for n in (0, 8, 9, 16, 17, 32, 33):  # both sides of FL_INLINE (8) and the 32-byte chunk task
        msgs.append(b'{"StringField":"' + bytes(97 + i % 26 for i in range(n)) + b'","I32Field":1}')
    for n in (0, 8, 12, 16, 20, 32, 36):  # base64 text comes in fours
        msgs.append(b'{"BinaryField":"' + _b64(n).encode() + b'","I32Field":1}')
    for e in range(5):  # escape-table sizes 0-4
        msgs.append(b'{"StringField":"ab' + b"\\n" * e + b'cd","ByteField":2}')
    msgs += W.gen_flat_batch(rng, 3) + W.gen_flat_batch_shuffled(rng, 5)
    msgs.append(b'{"I32Field":1,"StringField":"pad to eight"}')
    return msgs


def wrap_messages():
    rng = random.Random(6)
    msgs = [b'{"Flat":{"ByteField":7}}', b'{"other":{"I32Field":-5,"ByteField":1}}', b'{"Flat":{"I32Field":1}}',
            b' { "Flat" :\n{"StringField":"abcdefghijklmnopq","I32Field":1} } ', b'{"Other":{"StringField":"abc"}}',
            b'{"Flat":{"BinaryField":"QUJDREVGR0hJSktM","ByteField":1}}']
    while len(msgs) < 14:
        m = (b'{"Flat":%s}' if len(msgs) % 2 else b'{"other":%s}') % W.simple_obj(rng).encode()
        if len(m) <= 256:
            msgs.append(m)
    return msgs


def _simple(**kw):
    d = {"ByteField": 1, "I64Field": 2, "DoubleField": 1.5, "I32Field": 3, "StringField": "s", "BinaryField": "aGk="}
    d.update(kw)
    return d


def nest_messages():
    import json
    rng = random.Random(7)
    msgs = [b'{"I32":5}', b'{"String":"abc","I64":-1}', b'{"ListI32":[1,2,3],"Byte":9}',
            b'{"MapStringString":{"k":"v","kk":"vv"},"Double":2.5}', b'{"SimpleStruct":{"ByteField":1,"StringField":"xy"}}',
            json.dumps({"ListSimple": [_simple(), _simple(StringField="abcdefghi")], "I32": 7}).encode(),
            b'{"ListString":["a","bb",""],"Binary":"AAEC"}', b'{"MapI32I64":{"1":2,"-3":4}}', b'{"ListI32":[]}']
    msgs += [W.nesting_obj(rng).encode() for _ in range(3)]
    return msgs


def wave_messages():
    import json
    msgs = nest_messages()[:7]
    for n in (7, 8, 9, 63, 64, 65):  # around the copy chunk task
        msgs.append(b'{"String":"' + bytes(97 + i % 26 for i in range(n)) + b'","I32":1}')
    # two pages: more than 64 value entries, so a small capacity trips on the first page, a tight one on the second
    msgs.append(json.dumps({"ListI32": list(range(100)), "String": "tail"}).encode())
    msgs.append(json.dumps({"ListString": ["s%d" % i for i in range(90)], "I64": 5}).encode())
    return msgs


def lane_messages():
    return nest_messages()[:8] + [b'{"Str\\u0069ng":"escaped key","I32":2}']


def deep_list_desc(levels):
    t = T.builtin("i64")
    for _ in range(levels):
        t = T.list_of(t)
    return T.struct_type("Deep", [T.FieldDescriptor(1, "l", t, T.OPTIONAL), T.FieldDescriptor(2, "n", T.builtin("i32"), T.OPTIONAL)])


def _wrap_desc():
    from test_gpu_flat import _wrap_desc as w
    return w()


J2T_ROUTES = {
    # name: (descriptor, flags, knobs, messages, extra capacities as fractions of need, check the hand-offs)
    "flat": (W.simple_desc, 1 | FLAT, {}, flat_messages, (), True),
    "flat-wrapped": (_wrap_desc, 1 | FLAT, {}, wrap_messages, (), True),
    "small": (W.nesting_desc, 1 | NO_FLAT, {"wave_min": 1 << 20}, nest_messages, (), True),
    "wave-occ4": (W.nesting_desc, 1, {"wave_min": 0, "wave_occ": 4}, wave_messages, (0.3, 0.6), True),
    "wave-occ5": (W.nesting_desc, 1, {"wave_min": 0, "wave_occ": 5}, wave_messages, (0.3, 0.6), True),
    "lane": (W.nesting_desc, 1 | NO_WAVE, {"small_mpw": 0}, lane_messages, (), True),
    "lane-deep": (lambda: deep_list_desc(20), 1 | NO_WAVE, {"small_mpw": 0},
                  lambda: [b'{"l":' + b"[" * 20 + b"1,2" + b"]" * 20 + b',"n":3}', b'{"n":3}',
                           b'{"l":' + b"[" * 20 + b"]" * 20 + b"}"], (), False),
}


def j2t_items(route):
    mk, flags, knobs, msgs, fracs, _ = J2T_ROUTES[route]
    fl = T.flatten(mk())
    pure = flags & ~(FLAT | NO_FLAT | NO_WAVE)
    orc = j2t_oracle(fl, pure)
    items = SG.items_for(msgs(), orc)
    for m in msgs():
        ret, out = orc(m)
        if ret == 0 and len(out) > 400:  # the two-page messages: trip on the first page with a capacity above 0
            items += [SG.Item(m, int(len(out) * f) // 8 * 8, ret, out) for f in fracs]
    return fl, pure, items


@pytest.mark.parametrize("route", list(J2T_ROUTES))
def test_j2t_tight_slots(route, knob):
    _, flags, knobs, _, _, stays = J2T_ROUTES[route]
    fl, pure, items = j2t_items(route)
    SG.assert_shares(items)
    ret, spacer_out = j2t_oracle(fl, pure)(b"{}")
    assert ret == 0 and spacer_out == b"\x00"
    for k, v in knobs.items():
        knob(k, v)
    launch = j2t_launch(fl, flags)
    SG.check(launch, items, b"{}", spacer_out, DEV)
    if stays:
        exact_fit_stays(launch, items)
    elif route == "lane-deep":
        bails, deeps = handoffs(launch, [it for it in items if it.cap == len(it.out) + 8 and it.ret == 0], 8)
        assert deeps > 0, "the 20-level message did not reach the deep pass"


@pytest.mark.parametrize("route", ["flat", "flat-wrapped", "small", "wave-occ4", "wave-occ5", "lane"])
def test_j2t_unaligned_slot_bases(route, knob):
    """include/dgj2t.h: a j2t slot may start at any byte. The same capacities
    with the tested slots at bases 1, 4, 7 and 14 modulo 16: the lane writer
    stores bytes there, the wave and flat writers their edge words in parts."""
    mk, flags, knobs, msgs, _, _ = J2T_ROUTES[route]
    fl = T.flatten(mk())
    orc = j2t_oracle(fl, 1)
    items = SG.items_for([m for m in msgs() if len(m) < 400][:12], orc, phases=(1, 4, 7, 14))
    SG.assert_shares(items)
    for k, v in knobs.items():
        knob(k, v)
    SG.check(j2t_launch(fl, flags), items, b"{}", b"\x00", DEV)


# ---------------------------------------------------------------- t2j inputs
def desc_e():
    return T.struct_type("E", [
        T.FieldDescriptor(1, "m", T.map_of(T.builtin("string"), T.builtin("string")), T.OPTIONAL),
        T.FieldDescriptor(2, "b", T.builtin("binary"), T.OPTIONAL),
        T.FieldDescriptor(3, "s", T.builtin("string"), T.OPTIONAL)])


def desc_n():
    return T.struct_type("N", [T.FieldDescriptor(1, "d", T.list_of(T.builtin("double")), T.OPTIONAL),
                               T.FieldDescriptor(2, "i", T.list_of(T.builtin("i64")), T.OPTIONAL),
                               T.FieldDescriptor(3, "s", T.list_of(T.builtin("string")), T.OPTIONAL),
                               T.FieldDescriptor(4, "b", T.list_of(T.builtin("binary")), T.OPTIONAL)])


def _str(b):
    return struct.pack(">i", len(b)) + b


def e_messages():
    """Strings of control bytes (6 JSON bytes per input byte), lengths 0-20:
    `need` crosses every pair phase; a map, a binary."""
    msgs = [b"\x0b\x00\x03" + _str(b"\x01" * k) + b"\x00" for k in range(21)]
    msgs.append(b"\x0d\x00\x01\x0b\x0b" + struct.pack(">i", 2) + _str(b'k"1') + _str(b"v\n") + _str(b"key2") + _str(b"") +
                b"\x0b\x00\x02" + _str(bytes(range(17))) + b"\x00")
    return msgs


def n_messages():
    ds = [0.1, -1.5e300, 5e-324, 123456789.125, 1e21, -0.0]
    iv = [0, -1, 1 << 62, -(1 << 63), 99999999]
    ss = [b"", b"a", b'q"\\', "é中".encode(), b"x" * 40]
    m = b"\x0f\x00\x01\x04" + struct.pack(">i", len(ds)) + b"".join(struct.pack(">d", d) for d in ds)
    m2 = b"\x0f\x00\x02\x0a" + struct.pack(">i", len(iv)) + b"".join(struct.pack(">q", v) for v in iv)
    m3 = b"\x0f\x00\x03\x0b" + struct.pack(">i", len(ss)) + b"".join(_str(s) for s in ss)
    m4 = b"\x0f\x00\x04\x0b" + struct.pack(">i", 3) + _str(b"") + _str(b"\x00\x01") + _str(bytes(range(40)))
    return [m + b"\x00", m2 + b"\x00", m3 + m4 + b"\x00", m + m2 + m3 + m4 + b"\x00"]


def all_types_messages():
    td = t2jgen.all_types_desc()
    rng = random.Random(13)
    msgs = []
    while len(msgs) < 8:
        m = t2jgen.gen_thrift(rng, td)
        if len(m) > 8:
            msgs.append(m)
    return msgs


T2J_SETS = {"all-types": (t2jgen.all_types_desc, all_types_messages), "E": (desc_e, e_messages), "N": (desc_n, n_messages)}


def t2j_items(which, opts=0):
    mk, msgs = T2J_SETS[which]
    fl = T.flatten(mk())
    return fl, SG.items_for(msgs(), t2j_oracle(fl, opts), phases=(0, 8))


def run_t2j(fl, items, opts=0):
    SG.assert_shares(items)
    ret, spacer_out = t2j_oracle(fl, opts)(b"\x00")
    assert (ret, spacer_out) == (0, b"{}") or (ret & 0xFF, spacer_out) == (6, b"")  # All: its REQUIRED field is missing
    return SG.check(t2j_launch(fl, opts), items, b"\x00", spacer_out, DEV, pending=False, spacer_ret=ret)


@pytest.mark.parametrize("which", list(T2J_SETS))
@pytest.mark.parametrize("route", ["lane-spread1", "lane-spread2", "lane-spread4", "wave"])
def test_t2j_tight_slots(route, which, knob):
    """The lane pass at each spread (JOut: aligned 16-byte pair stores that
    start 8 bytes before the word completing a pair) and the wave kernel
    (`O + tot > cap` per page, its bails redone by the lane pass)."""
    if route == "wave":
        knob("t2j_wave_min", 1)  # every message longer than a spacer
    else:
        knob("t2j_wave_min", 0)
        knob("t2j_spread", int(route[-1]))
    fl, items = t2j_items(which)
    run_t2j(fl, items)


@pytest.mark.parametrize("depth", [13, 40])
def test_t2j_deep_pass_tight_slots(depth):
    """Chains past the 12 LDS frames are redone by the deep pass, through the
    same writer, into the same slot."""
    fl = T.flatten(t2jgen.chain_desc())
    msgs = [t2jgen.chain_thrift(depth), t2jgen.chain_thrift(2), t2jgen.chain_thrift(depth)[:-1]]
    run_t2j(fl, SG.items_for(msgs, t2j_oracle(fl, 0), phases=(0, 8)))


def test_t2j_rolled_back_field_tight_slots():
    """JOut::set_len after pairs were stored: with DG_T2J_CONVERT_EXC the
    result struct's success field (`{"success":{"Msg":"","Code":202,...`, 16
    bytes and more, so whole pairs are in memory) is dropped with set_len(0)
    when the exception field arrives (t2j_device.h, `o.set_len(0); exc =
    true;`), and the exception's JSON is written over it from byte 0; the
    message ends DG_T2J_E_EXCEPTION (11) and keeps that JSON."""
    from test_t2j_oracle import _example3_svc, exception_result_thrift
    fl = T.flatten(_example3_svc().functions()["ExampleMethod"].response())
    m = exception_result_thrift()
    succ_only = m[:m.index(b"\x0c\x00\x01")] + b"\x00"
    orc = t2j_oracle(fl, CONV_EXC)
    ret, out = orc(m)
    assert ret & 0xFF == 11 and out == b'{"code":400,"msg":"this is an exception"}'
    assert len(orc(succ_only)[1]) >= 32  # what is rolled back spans more than one pair
    run_t2j(fl, SG.items_for([m, succ_only], orc, phases=(0, 8)), CONV_EXC)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_t2j_batch_sizes_around_the_wave_grouping(n, knob):
    """n tested messages (2n + 1 with the spacers) around the 16 messages a
    wave takes at spread 4 and the 64 at spread 1."""
    fl, items = t2j_items("E")
    rng = random.Random(n)
    over = [it for it in items if it.overflows]
    tight = [it for it in items if it.tight]
    pick = [rng.choice(over if k % 2 else tight) for k in range(n)]
    for spread in (1, 4):
        knob("t2j_wave_min", 0)
        knob("t2j_spread", spread)
        if n > 1:
            SG.assert_shares(pick)
        SG.check(t2j_launch(fl, 0), pick, b"\x00", b"{}", DEV, pending=False)


# ---------------------------------------------------------------- pack kernels
def _pack_inputs(kind):
    """A sandwich batch's slots, lengths and status words on the device, and
    the oracle's outputs."""
    import torch
    if kind == "j2t":
        fl, pure, items = j2t_items("flat")
        sw, runs = SG.check(j2t_launch(fl, 1 | FLAT), items, b"{}", b"\x00", DEV)
        spacer_out = b"\x00"
    else:
        fl = T.flatten(T.struct_type("P", [T.FieldDescriptor(1, "a", T.builtin("i32"), T.OPTIONAL),
                                           T.FieldDescriptor(2, "s", T.builtin("string"), T.OPTIONAL)]))
        msgs = [b"\x08\x00\x01" + struct.pack(">i", v) + b"\x00" for v in (1, 12, 123, -1234)]  # 7, 8, 9, 11 bytes
        msgs += [b"\x0b\x00\x02" + _str(b"x" * k) + b"\x00" for k in (0, 3, 10, 30)] + [b"\x08\x00\x01\x00"]
        items = SG.items_for(msgs, t2j_oracle(fl, 0), phases=(0, 8))
        sw, runs = SG.check(t2j_launch(fl, 0), items, b"\x00", b"{}", DEV, pending=False)
        spacer_out = b"{}"
    r = runs[0]
    want = []
    for i in range(len(sw.msgs)):
        out = sw.items[sw.tested.index(i)].out if i in sw.tested else spacer_out
        want.append(out if int(r.ret[i]) == 0 else None)
    lens = {len(w) if w is not None else 0 for w in want}
    assert {0, len(spacer_out), 8, 9} <= lens and any(v % 8 for v in lens) and (kind == "j2t" or 7 in lens), sorted(lens)
    dev = torch.device(DEV)
    return (sw, r, want, torch.from_numpy(r.out).to(dev), torch.from_numpy(sw.off).to(dev),
            torch.from_numpy(r.out_len.view(np.int32)).to(dev), torch.from_numpy(r.ret.view(np.int64)).to(dev))


def _pack_twice(call, total, n):
    """call(d_dst, d_dst_off) packs into d_dst; both prefills -> the two
    destinations (64 guard bytes on both sides) and dst_off."""
    import torch
    got = []
    for fill in SG.FILLS:
        buf = torch.full((total + 2 * SG.GUARD,), fill, dtype=torch.uint8, device=DEV)
        d_doff = torch.full((n + 1,), -1, dtype=torch.int64, device=DEV)
        call(buf[SG.GUARD:], d_doff)
        torch.cuda.synchronize()
        got.append((buf.cpu().numpy(), d_doff.cpu().numpy()))
    return got


def _check_packed(got, expect, doff_want):
    total = len(expect)
    (a, da), (b, db) = got
    wr = a == b
    assert wr[SG.GUARD:SG.GUARD + total].all(), "bytes of [0, total) not written: %r" % np.nonzero(
        ~wr[SG.GUARD:SG.GUARD + total])[0][:8]
    assert not wr[:SG.GUARD].any() and not wr[SG.GUARD + total:].any(), "stores outside [0, %d): %r" % (
        total, np.nonzero(wr)[0][[0, -1]] - SG.GUARD)
    assert a[SG.GUARD:SG.GUARD + total].tobytes() == expect
    if doff_want is not None:
        assert np.array_equal(da, doff_want) and np.array_equal(db, doff_want)


@pytest.mark.parametrize("kind", ["j2t", "t2j"])
def test_pack_kernels_write_exactly_the_packed_bytes(kind):
    """dg_pack_device and dg_pack_device_scan over a sandwich batch's slots
    (lengths 0, 1 or 2, 7, 8, 9 and others that are no multiple of 8; the
    messages that failed or overflowed cleared to 0, as the header asks of the
    caller): the oracle's outputs back to back, and not a byte more."""
    import torch
    sw, r, want, d_out, d_oo, d_ol, d_ret = _pack_inputs(kind)
    n = len(want)
    ctx, L, st = conv.default_context(), _lib.lib(), torch.cuda.current_stream().cuda_stream
    lens = np.array([len(w) if w is not None else 0 for w in want], dtype=np.int64)
    d_len0 = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    doff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=doff[1:])
    expect = b"".join(w for w in want if w is not None)
    assert len(expect) == doff[-1]

    def plain(d_dst, d_doff):
        d_doff.copy_(torch.from_numpy(doff).to(DEV))
        _lib.check(L.dg_pack_device(ctx.h, d_out.data_ptr(), d_oo.data_ptr(), d_len0.data_ptr(), n, d_dst.data_ptr(),
                                    d_doff.data_ptr(), st))

    def scan(d_dst, d_doff):
        _lib.check(L.dg_pack_device_scan(ctx.h, d_out.data_ptr(), d_oo.data_ptr(), d_len0.data_ptr(), n,
                                         d_dst.data_ptr(), d_doff.data_ptr(), st))

    _check_packed(_pack_twice(plain, len(expect), n), expect, doff)
    _check_packed(_pack_twice(scan, len(expect), n), expect, doff)


@pytest.mark.parametrize("ftr_len", [0, 1])
@pytest.mark.parametrize("hdr_len", [1, 8, 13])
def test_pack_framed_writes_exactly_the_framed_bytes(hdr_len, ftr_len):
    """dg_pack_device_framed with the kernel's own lengths and status words:
    hdr + body + ftr for every message that converted, nothing for one that
    failed or overflowed (whose out_len holds the bytes it needs)."""
    import torch
    sw, r, want, d_out, d_oo, d_ol, d_ret = _pack_inputs("j2t")
    n = len(want)
    assert any(w is None and int(r.out_len[i]) > 0 for i, w in enumerate(want))
    hdr, ftr = bytes(range(0x80, 0x80 + hdr_len)), b"\x00" * ftr_len
    ctx, L, st = conv.default_context(), _lib.lib(), torch.cuda.current_stream().cuda_stream
    lens = np.array([len(w) + hdr_len + ftr_len if w is not None else 0 for w in want], dtype=np.int64)
    doff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=doff[1:])
    expect = b"".join(hdr + w + ftr for w in want if w is not None)

    def framed(d_dst, d_doff):
        _lib.check(L.dg_pack_device_framed(ctx.h, d_out.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(), n,
                                           hdr, hdr_len, ftr, ftr_len, d_dst.data_ptr(), d_doff.data_ptr(), st))

    _check_packed(_pack_twice(framed, len(expect), n), expect, doff)
