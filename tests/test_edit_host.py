"""CPU: the edit checker (editref.py) pinned to the reference's own tests and to
hand-written messages, dg_edit_create's refusals, the slot bound, and the
decision function of dynamicgo_amd/csrc/edit_device.h and the many-edit's
splice with one item (editm_device.h), as dg_edit_* runs them, built for the
host (edit_host.cpp: every route, lane by lane) against the
checker, once more as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import editgen as G
import editref as E
import tgetref as R
from conftest import GOLDEN
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as X

F, I, S, N, BK = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
HERE = os.path.dirname(os.path.abspath(__file__))


def example2():
    with open(os.path.join(GOLDEN, "example2.bin"), "rb") as fh:
        return fh.read()


def whole(b, root_type=R.STRUCT):
    """the message skips cleanly to its end"""
    p = R.Proto(b)
    p.skip_type(root_type)
    return p.read == len(b)


def count_at(b, path):
    r = R.get_by_path(b, path)
    assert r.status == R.OK and r.type in (R.LIST, R.SET, R.MAP)
    at = r.start + (2 if r.type == R.MAP else 1)
    return struct.unpack(">i", b[at:at + 4])[0]


# ------------------------------------------------------------- known answers
def test_set_by_path_known_answers():
    """TestSetByPath (thrift/generic/value_test.go:768-887) on example2: Subfix = 32767, Base = 255 with
    Extra = 6, InnerBase = 3 with ListInt32 = 8, A = 2"""
    b = example2()

    def set_(b, path, val, t, existed):
        ret, out = E.set_by_path(b, path, val, t)
        assert ret == E.word(E.OK, existed=existed), hex(ret)
        got = R.get_by_path(out, path)
        assert whole(out)
        return out, got

    # replace
    out, got = set_(b, [(F, 32767)], struct.pack(">d", -0.1), R.DOUBLE, True)
    assert R.raw(out, got) == struct.pack(">d", -0.1) and len(out) == len(b)
    zh = G.wstr("中文".encode())
    extra_b = [(F, 255), (F, 6), (S, b"b")]
    out, got = set_(out, extra_b, zh, R.STRING, True)
    assert R.raw(out, got) == zh
    out2, got = set_(out, extra_b, zh, R.STRING, True)
    assert out2 == out  # set twice = set once
    idx2 = [(F, 3), (F, 8), (I, 2)]
    n0 = count_at(out, idx2[:-1])
    out, got = set_(out, idx2, struct.pack(">i", -(1 << 31) + 1), R.I32, True)
    assert R.raw(out, got) == struct.pack(">i", -(1 << 31) + 1) and count_at(out, idx2[:-1]) == n0
    # insert
    assert R.get_by_path(out, [(F, 2)]).status == R.NOT_FOUND
    out, got = set_(out, [(F, 2)], struct.pack(">i", -1024), R.I32, False)
    assert R.raw(out, got) == struct.pack(">i", -1024) and out[:7] == b"\x08\x00\x02" + struct.pack(">i", -1024)
    extra_x = [(F, 255), (F, 6), (S, b"x")]
    zb = G.wstr("中文\bb".encode())
    n0 = count_at(out, extra_x[:-1])
    out, got = set_(out, extra_x, zb, R.STRING, False)
    assert R.raw(out, got) == zb and count_at(out, extra_x[:-1]) == n0 + 1
    far = [(F, 3), (F, 8), (I, 1024)]
    n0 = count_at(out, far[:-1])
    for k, v in enumerate((0x1234567, 0x7654321)):
        ret, out = E.set_by_path(out, far, struct.pack(">i", v), R.I32)
        assert ret == E.word(E.OK) and whole(out)
        first = R.get_by_path(out, far[:-1] + [(I, 0)])  # the insert reads back at index 0
        assert R.raw(out, first) == struct.pack(">i", v) and count_at(out, far[:-1]) == n0 + 1 + k
    # a wrong type
    assert E.set_by_path(b, [(F, 32767)], struct.pack(">i", 1), R.I32) == (E.word(E.E_TYPE, R.DOUBLE), b"")


def test_unset_by_path_known_answers():
    """TestUnsetByPath (value_test.go:689-745): Base.Caller = 255.2, InnerBase.ListInt32's last element,
    InnerBase.MapStringString["a"] = 3.9, InnerBase.MapInt32String[1] = 3.12"""
    b = example2()
    ret, out = E.unset_by_path(b, [(F, 255), (F, 2)])
    assert ret == E.word(E.OK, existed=True) and whole(out)
    assert R.get_by_path(out, [(F, 255), (F, 2)]).status == R.NOT_FOUND
    lst = [(F, 3), (F, 8)]
    n = count_at(b, lst)
    for path in (lst + [(I, n - 1)], [(F, 3), (F, 9), (S, b"a")], [(F, 3), (F, 12), (N, 1)]):
        n0 = count_at(b, path[:-1])
        assert R.get_by_path(b, path).status == R.OK
        ret, out = E.unset_by_path(b, path)
        assert ret == E.word(E.OK, existed=True) and whole(out)
        assert R.get_by_path(out, path).status == R.NOT_FOUND and count_at(out, path[:-1]) == n0 - 1
    # composition: unset then set gives the front-insert form
    ret, out = E.unset_by_path(b, [(F, 1)])
    ret, out = E.set_by_path(out, [(F, 1)], G.wstr(b"hello"), R.STRING)
    assert ret == E.word(E.OK) and out[:12] == b"\x0b\x00\x01" + G.wstr(b"hello") and len(out) == len(b)


# ---------------------------------------------------------------- deviations
I32_7 = struct.pack(">i", 7)
NESTED = G.field(R.I32, 1, I32_7) + G.field(R.STRUCT, 2, G.field(R.I32, 1, I32_7) + b"\x00") + b"\x00"
MAP16 = G.field(R.MAP, 1, struct.pack(">bbi", R.I16, R.I32, 1) + struct.pack(">hi", 5, 9)) + b"\x00"
DEVIATIONS = [
    # 1: a missing field of a nested struct goes to the front of THAT struct (the Go: byte 0 of the message)
    (E.SET_OP, NESTED, [(F, 2), (F, 9)], I32_7, R.I32,
     (E.word(E.OK), NESTED[:10] + b"\x08\x00\x09" + I32_7 + NESTED[10:])),
    # 2: an int key at the width of the map's key type, I16 (the Go: ToRaw(I32), four bytes)
    (E.SET_OP, MAP16, [(F, 1), (N, -2)], I32_7, R.I32,
     (E.word(E.OK), MAP16[:5] + struct.pack(">i", 2) + b"\xff\xfe" + I32_7 + MAP16[9:])),
    # 3: an insert of another type than the container's elements
    (E.SET_OP, MAP16, [(F, 1), (N, 6)], b"\x01", R.BOOL, (E.word(E.E_TYPE, R.I32), b"")),
    (E.SET_OP, struct.pack(">bi", R.I64, 0), [(I, 0)], I32_7, R.I32, (E.word(E.E_TYPE, R.I64), b"")),
    # 4: unset of an absent map key (the Go: deletes the last entry, count - 1)
    (E.UNSET_OP, MAP16, [(F, 1), (N, 6)], b"", 0, (E.word(E.NOT_FOUND), b"")),
    (E.UNSET_OP, struct.pack(">bbi", R.I16, R.I32, 0), [(N, 6)], b"", 0, (E.word(E.NOT_FOUND), b"")),
    # 5: keys match as the lookup matches them: 255 hits the I08 key 0xFF, -1 does not
    (E.UNSET_OP, struct.pack(">bbi", R.BYTE, R.BYTE, 1) + b"\xff\x07", [(N, 255)], b"", 0,
     (E.word(E.OK, existed=True), struct.pack(">bbi", R.BYTE, R.BYTE, 0))),
    (E.UNSET_OP, struct.pack(">bbi", R.BYTE, R.BYTE, 1) + b"\xff\x07", [(N, -1)], b"", 0, (E.word(E.NOT_FOUND), b"")),
    # 6: unset below a value that is no container (the Go: silently nothing)
    (E.UNSET_OP, NESTED, [(F, 1), (F, 1)], b"", 0, (E.word(E.E_TYPE, R.I32), b"")),
    (E.UNSET_OP, NESTED, [(F, 2), (I, 0)], b"", 0, (E.word(E.E_TYPE, R.STRUCT), b"")),
    # not deviations: a missing parent is no error for unset and ErrNotFound for set
    (E.UNSET_OP, NESTED, [(F, 3), (F, 1)], b"", 0, (E.word(E.OK), NESTED)),
    (E.SET_OP, NESTED, [(F, 3), (F, 1)], I32_7, R.I32, (E.word(E.NOT_FOUND), b"")),
    # int32(size + 1) wraps
    (E.SET_OP, struct.pack(">bi", R.BYTE, 0x7FFFFFFF) + b"\x09", [(I, 0x7FFFFFFF)], b"\x07", R.BYTE,
     (E.word(E.OK), struct.pack(">bI", R.BYTE, 0x80000000) + b"\x07\x09")),
]


def root_of(msg, path):
    return {F: R.STRUCT, I: R.LIST}.get(path[0][0], R.MAP)


def test_deviations_byte_for_byte():
    for op, msg, path, val, t, want in DEVIATIONS:
        assert len(msg) < 40
        assert E.edit(op, msg, path, val, t, root_of(msg, path)) == want, (op, path)


# ------------------------------------------------------ refusals and bounds
def test_create_refusals_need_no_device():
    """the blob is judged before the context: DG_E_ARG (-6) with dg_path_create's texts, and for the empty
    path and two paths; a good blob then fails on the null context (DG_E_INVALID, -1)"""
    from dynamicgo_amd import _lib
    L = _lib.lib()

    def create(blob, op=X.EDIT_SET):
        h = C.c_void_p()
        rc = L.dg_edit_create(None, bytes(blob), len(blob), op, C.byref(h))
        assert not h.value
        return rc, (L.dg_last_error() or b"").decode()

    good = bytearray(X.compile_paths([G.paths_of([(F, 1), (I, 2), (S, b"key")])]))
    assert create(good)[0] == -1 and create(good, 3) == (-1, "unknown edit op 3")
    rc, err = create(X.compile_paths([[]]))
    assert rc == -6 and "empty path" in err
    rc, err = create(X.compile_paths([G.paths_of([(F, 1)]), G.paths_of([(F, 2)])]))
    assert rc == -6 and "2 paths" in err
    off_steps = struct.unpack_from("<I", good, 20)[0]

    def patched(at, fmt, val):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, val)
        return b

    for blob, text in ((patched(0, "<I", 0), "magic"), (patched(4, "<I", 9), "magic or version"),
                       (patched(12, "<I", 0), "0 paths"), (patched(12, "<I", 9), "9 paths"),
                       (patched(36, "<I", 17), "17 steps"), (patched(32, "<I", 5), "outside the table"),
                       (patched(off_steps, "<I", 9), "unknown kind"), (patched(off_steps + 4, "<I", 3), "key_len"),
                       (patched(off_steps + 16 + 8, "<q", -1), "negative index"),
                       (patched(off_steps + 8, "<q", 70000), "field id"),
                       (patched(off_steps + 32 + 4, "<I", 4), "outside the pool"),
                       (patched(off_steps + 32 + 8, "<q", 1), "outside the pool"),
                       (good[:-1], "outside the blob"), (good[:16], "no header")):
        rc, err = create(blob)
        assert rc == -6 and text in err, (text, rc, err)
    with pytest.raises(ValueError):
        X.EditPlan([], X.EDIT_SET)


def test_slot_bound_is_the_longest_output():
    """editref.slot_bound (what dg_edit_slot_bound must return: test_gpu_edit compares them) is reached by an
    insert and never passed; for INTKEY the widest key type reaches it"""
    i64map = struct.pack(">bbi", R.I64, R.I32, 0)
    reach = [([(F, 5)], b"\x00", R.STRUCT), ([(I, 9)], struct.pack(">bi", R.I32, 0), R.LIST),
             ([(S, b"abcde")], struct.pack(">bbi", R.STRING, R.I32, 0), R.MAP), ([(N, 3)], i64map, R.MAP),
             ([(BK, b"\0\0\0\0\0\0\0\x03")], i64map, R.MAP)]
    for path, msg, root in reach:
        ret, out = E.edit(E.SET_OP, msg, path, I32_7, R.I32, root)
        assert ret == E.word(E.OK) and len(out) == E.slot_bound(E.SET_OP, path, len(msg), 4), path
    for c in G.fuzz_cases() + G.count_cases() + G.smallest_cases():
        for i, (ret, out) in enumerate(c.want()):
            assert len(out) <= E.slot_bound(c.op, c.path, len(c.msgs[i]), len(c.value(i)) if c.op == E.SET_OP else 0)


def test_fuzz_shares():
    """from the checker alone: every outcome class is at least 5 % of the fuzz cases"""
    sh = G.shares(G.fuzz_cases())
    for k in ("replaced", "inserted", "deleted", "ErrNotFound", "ErrRead", "ErrDismatchType"):
        assert sh.get(k, 0) >= 0.05, (k, sh)


# --------------------------------------------- decision + splice, on the host
def build_host(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "edit_host.cpp")],
                   check=True)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """host(case, route, caps=None) -> [(ret, out)] with the guard bytes around every slot checked"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host edit with" % B.HIPCC)
    lib = C.CDLL(build_host(str(tmp_path_factory.mktemp("edit") / "libedit.so"), ("-shared",)))
    lib.edit_msg.restype = None
    lib.edit_msg.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p,
                             C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

    def run(case, route, caps=None):
        blob = G.pair_blob(case.path) + b"\0" * 16
        res = []
        ret, ol = C.c_uint64(0), C.c_uint32(0)
        for i, m in enumerate(case.msgs):
            v = case.value(i) if case.op == E.SET_OP else b""
            cap = caps[i] if caps is not None else E.slot_bound(case.op, case.path, len(m), len(v))
            out = C.create_string_buffer(b"\xEE" * (cap + 32), cap + 32)
            lib.edit_msg(m + b"\xAA" * 16, len(m), blob, case.op, case.root_type, case.val_type, v + b"\xBB" * 16, len(v),
                         route, C.cast(C.byref(out, 16), C.c_char_p), cap, C.byref(ret), C.byref(ol))
            raw = out.raw
            assert raw[:16] == b"\xEE" * 16 and raw[16 + cap:] == b"\xEE" * 16, "a store outside the slot"
            ok = ret.value & 0xFF == E.OK
            used = ol.value if ok else 0
            assert raw[16 + used:16 + cap] == b"\xEE" * (cap - used), "a store beyond out_len, or by a failed message"
            assert ol.value == E.out_len(ret.value, raw[16:16 + used])
            res.append((ret.value, raw[16:16 + used]))
        return res

    return run


def both(host, case, caps=None):
    want = case.want(caps)
    for route in (0, 1, 2, 3):  # lane, wave, 4 and 16 lanes a message
        got = host(case, route, caps)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s, route %d, message %d (%r...): got %x / %d bytes, checker %x / %d" % (
                case.what, route, i, case.msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))
    return want


def test_host_deviations(host):
    for op, msg, path, val, t, want in DEVIATIONS:
        assert both(host, G.Case(op, path, [msg], t, val, root_of(msg, path))) == [want]


def test_host_known_answers(host):
    b = example2()
    for path, val, t in (([(F, 32767)], struct.pack(">d", -0.1), R.DOUBLE), ([(F, 255), (F, 6), (S, b"b")], G.wstr(b"xy"), R.STRING),
                         ([(F, 255), (F, 6), (S, b"x")], G.wstr(b"xy"), R.STRING), ([(F, 3), (F, 8), (I, 1024)], I32_7, R.I32),
                         ([(F, 2)], I32_7, R.I32), ([(F, 3), (F, 12), (N, 77)], G.wstr(b""), R.STRING)):
        assert both(host, G.Case(E.SET_OP, path, [b], t, val))[0][0] & 0xFF == E.OK
    for path in ([(F, 255), (F, 2)], [(F, 3), (F, 8), (I, 2)], [(F, 3), (F, 9), (S, b"a")], [(F, 3), (F, 12), (N, 1)]):
        assert both(host, G.Case(E.UNSET_OP, path, [b]))[0][0] == E.word(E.OK, existed=True)


def test_host_fuzz(host):
    for c in G.fuzz_cases():
        both(host, c.sub(range(0, len(c.msgs), 3)))


def test_host_alignment_sweep(host):
    both(host, G.sweep_case())


def test_host_counts_and_smallest(host):
    for c in G.count_cases() + G.smallest_cases():
        both(host, c)


def test_host_deep_values(host):
    for c in G.deep_cases():
        both(host, c)


def test_host_slots(host):
    """a slot of exactly the needed size takes the message; one byte less is E_OVERFLOW with the size and no byte stored"""
    for c in G.fuzz_cases()[::4] + G.count_cases()[:2]:
        c = c.sub(range(0, len(c.msgs), 5))
        need = [len(o) for _, o in c.want()]
        assert both(host, c, need) == c.want()
        short = [max(n - 1, 0) for n in need]
        want = both(host, c, short)
        assert all(w[0] == E.overflow(n) for w, n, (r, _) in zip(want, need, c.want()) if r & 0xFF == E.OK and n)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """edit_host.cpp as a program (-DEDIT_MAIN) built with AddressSanitizer and UBSan: every message and value
    in a heap block of len + 16 bytes, every slot in one of exactly its size (the needed size, or one byte less
    for every fourth message), the blob in one of its length + 16. All four routes run on every message; the counts
    it prints are the checker's."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host edit with" % B.HIPCC)
    exe = build_host(str(tmp_path / "edit"), ("-DEDIT_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                                "-fno-sanitize-recover=undefined"))
    fz = G.fuzz_cases()
    sw = G.sweep_case()
    cases = [c.sub(range(k % 4, len(c.msgs), 4)) for k, c in enumerate(fz)] + [sw.sub(range(0, len(sw.msgs), 3))] + \
        G.count_cases() + G.smallest_cases() + G.deep_cases()
    files, count, existed, total, n_msgs = [], {}, 0, 0, 0
    for k, c in enumerate(cases):
        caps = [max(len(out) - (1 if i % 4 == 3 else 0), 0) for i, (_, out) in enumerate(c.want())]
        for ret, out in c.want(caps):
            count[ret & 0xFF] = count.get(ret & 0xFF, 0) + 1
            existed += bool(ret & E.EXISTED)
            total += len(out)
        files.append(str(tmp_path / ("corpus%d.bin" % k)))
        G.write_corpus(files[-1], c, caps)
        n_msgs += len(c.msgs)
    assert count.get(E.E_OVERFLOW, 0) > 100
    out = subprocess.run([exe, *files], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "%d messages; OK %d (existed %d), NOT_FOUND %d, E_READ %d, E_TYPE %d, E_OVERFLOW %d; %d bytes" % (
        n_msgs, count.get(E.OK, 0), existed, count.get(E.NOT_FOUND, 0), count.get(E.E_READ, 0), count.get(E.E_TYPE, 0),
        count.get(E.E_OVERFLOW, 0), total), out
