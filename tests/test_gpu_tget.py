"""GPU: batched GetByPath (dynamicgo_amd.generic over dg_tget_*) against the
pure-Python restatement of the reference in tgetref.py. Every case goes
through the host entry point and the device entry point, and every record
field and the value bytes are compared with the checker's."""
import os
import random
import struct

import numpy as np
import pytest

import t2jgen
import tgetref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F, I, S, N, B = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
LDS_FRAMES = 8  # TG_LDS_DEPTH (dynamicgo_amd/csrc/tget_device.h)

# the issue's paths over t2jgen.all_types_desc(): f18, f9.f1, f10[1].f2, f11[2], f17.f2.f2.f1, f17.f3[0].f1,
# f32767, f1000, f19[3], f15{1}, f9[0], f12{1} and the empty path
FUZZ_PATHS = {
    "f18": [(F, 18)], "f9.f1": [(F, 9), (F, 1)], "f10[1].f2": [(F, 10), (I, 1), (F, 2)], "f11[2]": [(F, 11), (I, 2)],
    "f17.f2.f2.f1": [(F, 17), (F, 2), (F, 2), (F, 1)], "f17.f3[0].f1": [(F, 17), (F, 3), (I, 0), (F, 1)],
    "f32767": [(F, 32767)], "f1000": [(F, 1000)], "f19[3]": [(F, 19), (I, 3)], "f15{1}": [(F, 15), (N, 1)],
    "f9[0]": [(F, 9), (I, 0)], "f12{1}": [(F, 12), (N, 1)], "": [],
}
# 13 paths in 16 slots. On well-formed messages only f9[0] (an index step on a struct) reads wrong bytes
# (E_READ, 28 % of its records) and only f12{1} (an int key on a string-keyed map) is E_TYPE (61 %), so the three
# spare slots go to them: f9[0] three times, one set holding it twice (5.5 % of all records), f12{1} twice (7.6 %).
FUZZ_SETS = [
    [FUZZ_PATHS[k] for k in ("f18", "f9.f1", "f10[1].f2", "f11[2]", "f17.f2.f2.f1", "f9[0]", "f12{1}", "")],
    [FUZZ_PATHS[k] for k in ("f17.f3[0].f1", "f32767", "f1000", "f19[3]", "f15{1}", "f9[0]", "f12{1}", "f9[0]")],
]


def to_paths(paths):
    from dynamicgo_amd import generic as G
    mk = {F: G.PathFieldId, I: G.PathIndex, S: G.PathStrKey, N: G.PathIntKey, B: G.PathBinKey}
    return [[mk[k](v) for k, v in p] for p in paths]


def expect(msgs, paths, root_type=R.STRUCT):
    """The checker's records, (len(msgs), len(paths)) of generic.REC_DTYPE."""
    from dynamicgo_amd.generic import REC_DTYPE
    out = np.zeros((len(msgs), len(paths)), dtype=REC_DTYPE)
    for i, m in enumerate(msgs):
        for k, p in enumerate(paths):
            out[i, k] = tuple(R.get_by_path(m, p, root_type))
    return out


def share(rec, status):
    return float((rec["status"] == status).mean())


def run_device(msgs, paths, root_type=R.STRUCT, vals=False, max_len=None):
    """dg_tget_batch_device over torch tensors -> records (and val_off, val_len, in_off)."""
    import torch
    from dynamicgo_amd import generic as G
    n = len(msgs)
    with G.PathSet(to_paths(paths)) as ps:
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(m) for m in msgs], out=in_off[1:])
        arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        d_off = torch.from_numpy(in_off).cuda()
        rec = torch.zeros((max(n, 1), ps.count, 4), dtype=torch.int32, device="cuda")
        voff = torch.zeros(max(n, 1) * ps.count, dtype=torch.int64, device="cuda") if vals else None
        vlen = torch.zeros(max(n, 1) * ps.count, dtype=torch.int32, device="cuda") if vals else None
        ml = max((len(m) for m in msgs), default=0) if max_len is None else max_len
        G.get_by_path_device(ps, arena, d_off, n, rec, voff, vlen, root_type=root_type, max_len=ml)
        torch.cuda.synchronize()
        out = rec.cpu().numpy().view(G.REC_DTYPE).reshape(max(n, 1), ps.count)[:n]
        if vals:
            return out, voff.cpu().numpy(), vlen.cpu().numpy(), in_off
        return out


def same(got, want, what):
    for f in want.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, "%s: field %s differs at (message, path) %s: got %s, checker %s" % (
            what, f, bad[:5].tolist(), got[f][tuple(bad[0])], want[f][tuple(bad[0])])


def check(msgs, paths, want, root_type=R.STRUCT, device=True):
    """host entry (records and .raw through get_by_path_batch) and device entry against the checker's records"""
    from dynamicgo_amd import generic as G
    res = G.get_by_path_batch(msgs, to_paths(paths), root_type=root_type)
    got = np.zeros(want.shape, dtype=G.REC_DTYPE)
    for i, row in enumerate(res):
        for k, r in enumerate(row):
            got[i, k] = (r.start, r.end, r.type, r.status, r.step, r.aux)
            w = R.Rec(*want[i, k].tolist())
            assert r.raw == R.raw(msgs[i], w), (i, k)
            assert r.error == {R.OK: None, R.NOT_FOUND: "ErrNotFound", R.E_READ: "ErrRead",
                               R.E_TYPE: "ErrDismatchType"}[w.status]
    same(got, want, "host entry")
    if device:
        same(run_device(msgs, paths, root_type), want, "device entry")


# ------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def fuzz():
    rng = random.Random(1234)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(2048)]
    return msgs, [expect(msgs, ps) for ps in FUZZ_SETS]


@pytest.fixture(scope="module")
def mutated():
    rng = random.Random(1234)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(2048)]
    mrng = random.Random(4321)
    msgs = [t2jgen.mutate(mrng, m) for m in msgs]
    return msgs, [expect(msgs, ps) for ps in FUZZ_SETS]


STR_KEYS = ["a", "b", "c"] + ["k%d" % i for i in range(8)]
INT_KEYS = list(range(-2, 6))
_PK = {R.BYTE: ">b", R.I16: ">h", R.I32: ">i", R.I64: ">q"}


def _wstr(s):
    s = s.encode()
    return struct.pack(">i", len(s)) + s


def keyed_message(rng):
    """A struct of maps with keys from small fixed sets, so fixed keys hit:
    1 map<string,i32>, 2 map<i8,string>, 3 map<i16,i64>, 4 map<i32,struct{1:i32}>,
    5 map<i64,list<i32>>, 6 map<string,map<string,string>>; each key kept with p = 1/2."""
    out = bytearray()

    def hdr(fid, kt, vt, keys):
        out.extend(struct.pack(">bhbbi", R.MAP, fid, kt, vt, len(keys)))

    ks = [k for k in STR_KEYS if rng.random() < 0.5]
    rng.shuffle(ks)
    hdr(1, R.STRING, R.I32, ks)
    for k in ks:
        out.extend(_wstr(k) + struct.pack(">i", rng.randrange(-99, 99)))
    for fid, kt in ((2, R.BYTE), (3, R.I16), (4, R.I32), (5, R.I64)):
        ki = [k for k in INT_KEYS if rng.random() < 0.5]
        rng.shuffle(ki)
        hdr(fid, kt, {2: R.STRING, 3: R.I64, 4: R.STRUCT, 5: R.LIST}[fid], ki)
        for k in ki:
            out.extend(struct.pack(_PK[kt], k))
            if fid == 2:
                out.extend(_wstr("v%d" % k))
            elif fid == 3:
                out.extend(struct.pack(">q", k * 1000))
            elif fid == 4:
                out.extend(struct.pack(">bhi", R.I32, 1, k) + b"\x00")
            else:
                out.extend(struct.pack(">bi", R.I32, 2) + struct.pack(">ii", k, -k))
    ks = [k for k in STR_KEYS if rng.random() < 0.5]
    hdr(6, R.STRING, R.MAP, ks)
    for k in ks:
        inner = [j for j in STR_KEYS[:4] if rng.random() < 0.5]
        out.extend(_wstr(k) + struct.pack(">bbi", R.STRING, R.STRING, len(inner)))
        for j in inner:
            out.extend(_wstr(j) + _wstr(j.upper()))
    out.append(0)
    return bytes(out)


KEY_SETS = [
    [[(F, 1), (S, b"a")], [(F, 1), (S, b"zz")], [(F, 2), (N, 3)], [(F, 2), (N, -1)], [(F, 3), (N, -2)],
     [(F, 4), (N, 2)], [(F, 5), (N, -1)], [(F, 4), (B, b"\x00\x00\x00\x02")]],
    [[(F, 1), (B, b"\x00\x00\x00\x01a")], [(F, 6), (S, b"k1"), (S, b"b")], [(F, 1), (N, 1)], [(F, 4), (S, b"a")],
     [(F, 4), (B, b"\x00\x00\x00\x09")], [(F, 5), (N, 5)], [(F, 2), (N, 255)], [(F, 4), (N, 2), (F, 1)]],
]


# ------------------------------------------------------------------- cases
def test_known_answers():
    with open(os.path.join(GOLDEN, "example2.bin"), "rb") as fh:
        buf = fh.read()
    assert len(buf) == 1326
    paths = [[(F, 3), (F, 8), (I, 1)], [(F, 3), (F, 12), (N, 2)], [(F, 3), (F, 9), (S, b"b")], [(F, 1)],
             [(F, 3), (F, 7)], [(F, 255)], [(F, 3), (F, 9), (S, b"aa")], [(F, 3), (F, 8), (I, 999)]]
    from dynamicgo_amd import generic as G
    r = G.get_by_path_batch([buf], to_paths(paths))[0]
    assert (r[0].status, r[0].type, r[0].start, r[0].end, r[0].raw) == (R.OK, R.I32, 93, 97, b"\0\0\0\0")
    assert (r[1].status, r[1].type, r[1].raw) == (R.OK, R.STRING, b"\0\0\0\x01B")
    assert (r[2].status, r[2].type, r[2].raw) == (R.OK, R.STRING, b"\0\0\0\x01B")
    assert r[3].raw == b"\0\0\0\x05hello"
    assert r[4].raw == b"\0\0\0\x06" + "你好".encode()
    assert (r[5].status, r[5].type, r[5].start, r[5].end) == (R.OK, R.STRUCT, 1233, 1325)
    assert (r[6].status, r[6].type, r[6].start, r[6].error) == (R.NOT_FOUND, R.MAP, 110, "ErrNotFound")
    assert (r[7].status, r[7].type, r[7].start) == (R.NOT_FOUND, R.LIST, 89)
    check([buf], paths, expect([buf], paths))
    rest = [[(F, 222)], []]
    r = G.get_by_path_batch([buf], to_paths(rest))[0]
    assert r[0].status == R.NOT_FOUND and (r[1].status, r[1].start, r[1].end) == (R.OK, 0, 1326)
    check([buf], rest, expect([buf], rest))


def test_fuzz(fuzz):
    msgs, wants = fuzz
    allrec = np.concatenate([w.ravel() for w in wants])
    for st in (R.OK, R.NOT_FOUND, R.E_READ, R.E_TYPE):  # a broken generator cannot hide a class
        assert share(allrec, st) >= 0.05, (st, share(allrec, st))
    for ps, want in zip(FUZZ_SETS, wants):
        check(msgs, ps, want)


@pytest.mark.parametrize("spread", [1, 2, 4])
def test_fuzz_every_lane_spacing(fuzz, knob, spread):
    msgs, wants = fuzz
    knob("tget_spread", spread)
    for ps, want in zip(FUZZ_SETS, wants):
        same(run_device(msgs, ps), want, "spread %d" % spread)


def test_lane_spacing_from_max_len(fuzz):
    """the spacing the launch picks by itself from max_len: <= 512, ~1 KB, unknown"""
    msgs, wants = fuzz
    for ml in (512, 1224, 0):
        same(run_device(msgs, FUZZ_SETS[0], max_len=ml), wants[0], "max_len %d" % ml)


def test_map_keys():
    rng = random.Random(99)
    msgs = [keyed_message(rng) for _ in range(512)]
    wants = [expect(msgs, ps) for ps in KEY_SETS]
    allrec = np.concatenate([w.ravel() for w in wants])
    assert share(allrec, R.OK) >= 0.20 and share(allrec, R.NOT_FOUND) >= 0.20
    # what the set is there for: hits and misses of each key kind, E_TYPE both ways, the unsigned byte key
    a, b = wants
    for col in (0, 2, 4, 5, 6, 7):
        assert 0.2 < share(a[:, col], R.OK) < 0.8
    assert share(a[:, 1], R.NOT_FOUND) == 1.0
    assert share(a[:, 3], R.OK) == 0.0  # INTKEY -1 on an i8-keyed map never hits (ReadInt: int(byte))
    assert share(b[:, 6], R.OK) > 0.2   # ... and 255 hits the key byte 0xFF
    assert share(b[:, 2], R.E_TYPE) == 1.0 and share(b[:, 3], R.E_TYPE) == 1.0
    assert share(b[:, 0], R.OK) > 0.2 and share(b[:, 4], R.NOT_FOUND) == 1.0
    for ps, want in zip(KEY_SETS, wants):
        check(msgs, ps, want)


def test_malformed(mutated):
    msgs, wants = mutated
    allrec = np.concatenate([w.ravel() for w in wants])
    assert share(allrec, R.E_READ) >= 0.20 and share(allrec, R.OK) >= 0.05
    for ps, want in zip(FUZZ_SETS, wants):
        check(msgs, ps, want)


def test_message_bounds():
    """A message cut at every offset, followed by a message that begins with
    exactly the missing bytes: the bytes past d_in_off[i+1] are not message i's."""
    m = (struct.pack(">bhi", R.I32, 1, 7) + struct.pack(">bh", R.STRING, 2) + _wstr("hello!") +
         struct.pack(">bhbi", R.LIST, 3, R.I16, 3) + struct.pack(">hhh", 1, 2, 3) + struct.pack(">bhh", R.I16, 4, 9) +
         b"\x00")
    assert len(m) == 40
    msgs = []
    for cut in range(40):
        msgs += [m[:cut], m[cut:]]
    paths = [[], [(F, 4)], [(F, 3), (I, 2)], [(F, 2)]]
    want = expect(msgs, paths)
    assert (want[0::2, 0]["status"] == R.E_READ).all()  # the whole struct of a cut message: never OK
    assert (want[0::2, 1]["status"] == R.OK).sum() == 1  # field 4 is whole only when just the STOP is missing
    check(msgs, paths, want)
    # values that end exactly at the message's last byte, and the one-byte message 00
    lst = struct.pack(">bi", R.I32, 3) + struct.pack(">iii", 1, 2, 3)
    msgs, paths = [lst, lst[:-1], lst + b"\x01"], [[], [(I, 2)], [(I, 3)]]
    want = expect(msgs, paths, R.LIST)
    assert tuple(want[0, 1].tolist())[:4] == (13, 17, R.I32, R.OK) and want[1, 1]["status"] == R.E_READ
    check(msgs, paths, want, R.LIST)
    want = expect(msgs, paths, R.SET)
    assert want[0, 2]["type"] == R.SET and want[0, 2]["status"] == R.NOT_FOUND
    check(msgs, paths, want, R.SET)
    msgs, paths = [b"\x00", b"", b"\x00\x00"], [[], [(F, 1)]]
    want = expect(msgs, paths)
    assert tuple(want[0, 0].tolist())[:4] == (0, 1, R.STRUCT, R.OK) and want[0, 1]["status"] == R.NOT_FOUND
    check(msgs, paths, want)


def test_depth():
    ds = [LDS_FRAMES, LDS_FRAMES + 1, LDS_FRAMES + 2, 1000, 1022, 1023, 1024, 1025, 1030]
    msgs = [t2jgen.chain_thrift(d) for d in ds]
    paths = [[(F, 2)], [(F, 2), (F, 2), (F, 2), (F, 1)]]
    want = expect(msgs, paths)
    # skipping field 2's value opens d - 1 nested structs: MaxSkipDepth lets 1023 through
    assert want[:, 0]["status"].tolist() == [R.OK] * 7 + [R.E_READ] * 2
    assert want[:, 1]["status"].tolist() == [R.NOT_FOUND] * 8 + [R.E_READ]
    check(msgs, paths, want)


def test_eight_paths_equal_eight_calls(fuzz):
    from dynamicgo_amd import generic as G
    msgs, wants = fuzz
    msgs = msgs[:512]
    ps = FUZZ_SETS[1]
    all8 = G.get_by_path_records(msgs, to_paths(ps))
    for k, p in enumerate(ps):
        one = G.get_by_path_records(msgs, to_paths([p]))
        assert (one[:, 0] == all8[:, k]).all(), k
        same(run_device(msgs, [p]), wants[1][:512, k:k + 1], "single path %d" % k)


def test_empty_batch():
    from dynamicgo_amd import generic as G
    assert G.get_by_path_batch([], to_paths([[(F, 1)]])) == []
    assert run_device([], [[(F, 1)], []]).shape == (0, 2)


def test_path_create_rejects_broken_blobs():
    import ctypes as C
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import default_context
    L, ctx = _lib.lib(), default_context()

    def create(blob):
        h = C.c_void_p()
        rc = L.dg_path_create(ctx.h, bytes(blob), len(blob), C.byref(h))
        if rc == 0:
            assert L.dg_path_count(h) == struct.unpack_from("<I", blob, 12)[0]
            L.dg_path_destroy(h)
        return rc, (L.dg_last_error() or b"").decode()

    good = bytearray(G.compile_paths(to_paths([[(F, 1), (I, 2), (S, b"key")], []])))
    assert create(good)[0] == 0
    off_steps = struct.unpack_from("<I", good, 20)[0]

    def patched(at, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, v)
        return b

    nine = bytearray(G.compile_paths(to_paths([[(F, 1)]] * 8)))
    struct.pack_into("<I", nine, 12, 9)
    for blob, text in ((patched(0, "<I", 0x12345678), "magic"), (patched(4, "<I", 2), "version"),
                       (nine, "9 paths"), (patched(12, "<I", 0), "0 paths"),
                       (patched(36, "<I", 17), "17 steps"),                       # path 0's step count
                       (patched(off_steps + 16, "<I", 9), "unknown kind"),        # step 1's kind
                       (patched(off_steps + 16 + 8, "<q", -1), "negative index"),  # step 1's value
                       (patched(off_steps + 8, "<q", 70000), "field id"),         # step 0's value
                       (patched(off_steps + 32 + 4, "<I", 4), "outside the pool"),  # step 2's key length
                       (patched(off_steps + 32 + 8, "<q", 1), "outside the pool"),  # step 2's key offset
                       (good[:-1], "outside the blob"), (good[:16], "no header")):
        rc, err = create(blob)
        assert rc == -6 and text in err, (text, rc, err)  # DG_E_ARG


def test_pack_found_values(fuzz):
    """d_val_off / d_val_len of a P = 1 run are what dg_pack_device_scan takes."""
    import torch
    from dynamicgo_amd import _lib
    from dynamicgo_amd.conv import default_context
    msgs, wants = fuzz
    path = FUZZ_PATHS["f10[1].f2"]
    want = wants[0][:, 2]
    rec, voff, vlen, in_off = run_device(msgs, [path], vals=True)
    same(rec, want.reshape(-1, 1), "device entry")
    raws = [R.raw(m, R.Rec(*w.tolist())) for m, w in zip(msgs, want)]
    assert 0 < sum(1 for r in raws if r) < len(msgs)
    assert vlen.tolist() == [len(r) for r in raws]
    assert voff.tolist() == [int(in_off[i]) + int(want[i]["start"]) for i in range(len(msgs))]
    n = len(msgs)
    arena = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_voff, d_vlen = torch.from_numpy(voff).cuda(), torch.from_numpy(vlen).cuda()
    dst = torch.zeros(sum(len(r) for r in raws) + 64, dtype=torch.uint8, device="cuda")
    dst_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ctx = default_context()
    _lib.check(_lib.lib().dg_pack_device_scan(ctx.h, arena.data_ptr(), d_voff.data_ptr(), d_vlen.data_ptr(), n,
                                              dst.data_ptr(), dst_off.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    packed = b"".join(raws)
    assert dst_off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in raws])]).tolist()
    assert dst.cpu().numpy().tobytes()[:len(packed)] == packed
