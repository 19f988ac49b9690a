"""CPU: the many-edit checker (editmref.py) pinned to the reference's TestSetMany,
to the single-edit checker (chained editref calls) and to hand-written messages;
dg_editm_create's refusals; the slot bound; the generator's shares; and the
combine and splice of dynamicgo_amd/csrc/editm_device.h built for the host
(editm_host.cpp: every route, lane by lane) against the checker, once more as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import editgen as G
import editmgen as MG
import editmref as M
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
    p = R.Proto(b)
    p.skip_type(root_type)
    return p.read == len(b)


def count_at(b, path):
    r = R.get_by_path(b, path)
    assert r.status == R.OK and r.type in (R.LIST, R.SET, R.MAP)
    at = r.start + (2 if r.type == R.MAP else 1)
    return struct.unpack(">i", b[at:at + 4])[0]


@pytest.fixture(scope="module")
def corpus():
    """every generated case with the checker's answers, computed once"""
    cases = {"fuzz": MG.fuzz_cases(), "adjacency": MG.adjacency_cases(), "phase": [MG.phase_case()],
             "unit": MG.unit_cases(), "count": MG.count_cases(), "failure": MG.failure_cases()}
    for cs in cases.values():
        for c in cs:
            c.want()
    return cases


# ------------------------------------------------------------- known answers
def test_set_many_known_answers():
    """TestSetMany (thrift/generic/value_test.go:535-687) on example2: A = 2 is not there, InnerBase = 3 with
    ListInt32 = 8, Msg = 1, Subfix = 32767, Base = 255 with its six fields"""
    b = example2()
    i32 = struct.pack(">i", -1024)
    # field 2 inserted
    assert R.get_by_path(b, [(F, 2)]).status == R.NOT_FOUND
    ret, out = M.edit_many(M.SET_OP, b, [], [((F, 2), i32, R.I32)])
    assert ret == M.word(M.OK) and whole(out) and out[:7] == b"\x08\x00\x02" + i32
    assert R.raw(out, R.get_by_path(out, [(F, 2)])) == i32
    # two Index(1024) inserts read back at indexes 0 and 1, the length + 2
    lst = [(F, 3), (F, 8)]
    n0 = count_at(b, lst)
    v1, v2 = struct.pack(">i", 0x1234567), struct.pack(">i", 0x7654321)
    ret, out = M.edit_many(M.SET_OP, b, lst, [((I, 1024), v1, R.I32), ((I, 1024), v2, R.I32)])
    assert ret == M.word(M.OK) and whole(out) and count_at(out, lst) == n0 + 2 and len(out) == len(b) + 8
    assert R.raw(out, R.get_by_path(out, lst + [(I, 0)])) == v1 and R.raw(out, R.get_by_path(out, lst + [(I, 1)])) == v2
    assert R.raw(out, R.get_by_path(out, lst + [(I, 2)])) == R.raw(b, R.get_by_path(b, lst + [(I, 0)]))
    # fields 1 and 32767 replaced
    msg, dbl = G.wstr(b"hello"), struct.pack(">d", -255.0001)
    ret, out = M.edit_many(M.SET_OP, b, [], [((F, 1), msg, R.STRING), ((F, 32767), dbl, R.DOUBLE)])
    assert ret == M.word(M.OK, mask=3) and whole(out)
    assert R.raw(out, R.get_by_path(out, [(F, 1)])) == msg and R.raw(out, R.get_by_path(out, [(F, 32767)])) == dbl
    # the six Base fields replaced by themselves: identical bytes
    items = []
    for fid in range(1, 7):
        r = R.get_by_path(b, [(F, 255), (F, fid)])
        assert r.status == R.OK
        items.append(((F, fid), R.raw(b, r), r.type))
    ret, out = M.edit_many(M.SET_OP, b, [(F, 255)], items)
    assert ret == M.word(M.OK, mask=0x3F) and out == b


def test_equals_chained_single_edits(corpus):
    """wherever no item fails or overlaps another, the many-edit is the chain of single edits editref checks:
    SET the found items, then the missing ones in reverse item order; UNSET descending by span start"""
    compared = {M.SET_OP: 0, M.UNSET_OP: 0}
    for cs in corpus.values():
        for c in cs:
            for i, (ret, out) in enumerate(c.want()):
                if M.status_of(ret) != M.OK:
                    continue
                ok, chain = M.chained(c.op, c.msgs[i], c.parent, c.items_for(i), c.root_type)
                if ok is None:
                    continue
                assert ok and chain == out, (c.what, i)
                compared[c.op] += 1
    assert compared[M.SET_OP] > 1500 and compared[M.UNSET_OP] > 500, compared


def test_one_item_is_the_single_edit_word_for_word():
    for c in G.fuzz_cases():
        for i in range(len(c.msgs)):
            got = M.edit_many(c.op, c.msgs[i], c.path[:-1], [(c.path[-1], c.value(i), c.val_type)], c.root_type)
            assert got == c.want()[i], (c.what, i)


I32_7 = struct.pack(">i", 7)
TWO = G.field(R.I32, 1, I32_7) + G.field(R.STRING, 2, G.wstr(b"two")) + b"\x00"
MAP_A = struct.pack(">bbi", R.STRING, R.I32, 2) + G.wstr(b"a") + I32_7 + G.wstr(b"b") + I32_7
LIST3 = struct.pack(">bi", R.I32, 3) + I32_7 * 3
HAND = [
    # 8: a replace checks the wire type (replaceMany would write a string over the i32)
    (M.SET_OP, TWO, [], [((F, 2), G.wstr(b"x"), R.STRING), ((F, 1), G.wstr(b"x"), R.STRING)], R.STRUCT,
     (M.word(M.E_TYPE, R.I32, item=1), b"")),
    # 9: overlapping items (the Go writes a corrupt buffer): the second of the pair, in message order, is reported
    (M.SET_OP, MAP_A, [], [((S, b"a"), I32_7, R.I32), ((BK, G.wstr(b"a")), I32_7, R.I32)], R.MAP, (M.word(M.E_SAME, item=1), b"")),
    (M.SET_OP, LIST3, [], [((I, 1), I32_7, R.I32), ((I, 0), I32_7, R.I32), ((I, 1), I32_7, R.I32)], R.LIST,
     (M.word(M.E_SAME, item=2), b"")),
    (M.UNSET_OP, LIST3, [], [((I, 2),), ((I, 2),)], R.LIST, (M.word(M.E_SAME, item=1), b"")),
    # ... but two missing duplicates are a legal double insert, in item order
    (M.SET_OP, LIST3, [], [((I, 9), b"\0\0\0\1", R.I32), ((I, 9), b"\0\0\0\2", R.I32)], R.LIST,
     (M.word(M.OK), struct.pack(">bi", R.I32, 5) + b"\0\0\0\1\0\0\0\2" + I32_7 * 3)),
    # the first failing item in item order wins, whatever the later ones are
    (M.SET_OP, TWO, [], [((F, 1), I32_7, R.I32), ((F, 2), I32_7, R.I32), ((F, 1), G.wstr(b""), R.STRING)], R.STRUCT,
     (M.word(M.E_TYPE, R.STRING, item=1), b"")),
    (M.UNSET_OP, TWO, [], [((F, 9),), ((F, 1),)], R.STRUCT, (M.word(M.NOT_FOUND, item=0), b"")),
    # a replace and an insert, the insert in front whatever the item order; UNSET on the original indexes
    (M.SET_OP, LIST3, [], [((I, 0), b"\0\0\0\1", R.I32), ((I, 3), b"\0\0\0\2", R.I32)], R.LIST,
     (M.word(M.OK, mask=1), struct.pack(">bi", R.I32, 4) + b"\0\0\0\2\0\0\0\1" + I32_7 * 2)),
    (M.UNSET_OP, struct.pack(">bi", R.BYTE, 4) + b"abcd", [], [((I, 0),), ((I, 1),)], R.LIST,
     (M.word(M.OK, mask=3), struct.pack(">bi", R.BYTE, 2) + b"cd")),
    (M.UNSET_OP, TWO, [(F, 7)], [((F, 1),), ((F, 2),)], R.STRUCT, (M.word(M.OK), TWO)),
]


def test_hand_written_messages():
    for op, msg, parent, items, root, want in HAND:
        items = [(it[0], it[1] if len(it) > 1 else b"", it[2] if len(it) > 2 else 0) for it in items]
        assert M.edit_many(op, msg, parent, items, root) == want, (op, parent, items)
    with pytest.raises(ValueError):  # 10: mixed step classes are refused before any message is read
        M.edit_many(M.SET_OP, TWO, [], [((F, 1), I32_7, R.I32), ((I, 0), I32_7, R.I32)])


# ------------------------------------------------------ refusals and bounds
def test_create_refusals_need_no_device():
    """the blob is judged before the context: DG_E_ARG (-6) with dg_path_create's texts and the many-edit's
    own; a good blob then fails on the null context (DG_E_INVALID, -1)"""
    from dynamicgo_amd import _lib
    L = _lib.lib()

    def create(blob, op=X.EDIT_SET):
        h = C.c_void_p()
        rc = L.dg_editm_create(None, bytes(blob), len(blob), op, C.byref(h))
        assert not h.value
        return rc, (L.dg_last_error() or b"").decode()

    good = MG.items_blob([(F, 1), (S, b"key")], [(I, 2), (I, 5), (I, 2)])
    assert create(good)[0] == -1 and create(good, 3) == (-1, "unknown edit op 3")
    assert create(MG.items_blob([], [(S, b"a"), (N, 1), (BK, b"abcd")]))[0] == -1  # the key kinds may mix
    for paths, text in (
            ([[]], "empty path"),
            ([G.paths_of([(F, k)]) for k in range(8)], "8 items"),
            ([G.paths_of([(F, 1), (F, 2)]), G.paths_of([(F, 2)])], "unequal length"),
            ([G.paths_of([(F, 1), (F, 2)]), G.paths_of([(F, 3), (F, 2)])], "differ before their last step"),
            ([G.paths_of([(S, b"ab"), (F, 2)]), G.paths_of([(S, b"ac"), (F, 2)])], "differ before their last step"),
            ([G.paths_of([(F, 1), (F, 2)]), G.paths_of([(F, 1), (I, 2)])], "mixed step classes"),
            ([G.paths_of([(I, 1)]), G.paths_of([(N, 1)])], "mixed step classes")):
        rc, err = create(X.compile_paths(paths))
        assert rc == -6 and text in err, (text, rc, err)
    b = bytearray(good)
    struct.pack_into("<I", b, 0, 0)
    rc, err = create(b)
    assert rc == -6 and "magic" in err
    rc, err = create(good[:-1])
    assert rc == -6 and "outside the blob" in err
    for bad in ([], [X.PathFieldId(k) for k in range(8)], [X.PathFieldId(1), X.PathIndex(1)]):
        with pytest.raises(ValueError):
            X.EditManyPlan([], bad, X.EDIT_SET)


def test_slot_bound_is_the_longest_output(corpus):
    """editmref.slot_bound (what dg_editm_slot_bound must return: test_gpu_editm compares them) is reached by K
    inserts and never passed; for INTKEY the widest key type reaches it"""
    i64map = struct.pack(">bbi", R.I64, R.I32, 0)
    reach = [([(F, 5), (F, 6), (F, 7)], b"\x00", R.STRUCT), ([(I, 9), (I, 9)], struct.pack(">bi", R.I32, 0), R.LIST),
             ([(S, b"abcde"), (BK, G.wstr(b"xy")), (S, b"")], struct.pack(">bbi", R.STRING, R.I32, 0), R.MAP),
             ([(N, 3), (BK, b"\0\0\0\0\0\0\0\x03"), (N, 4)], i64map, R.MAP)]
    for steps, msg, root in reach:
        items = [(st, I32_7, R.I32) for st in steps]
        ret, out = M.edit_many(M.SET_OP, msg, [], items, root)
        assert ret == M.word(M.OK) and len(out) == M.slot_bound(M.SET_OP, items, len(msg)), steps
    for cs in corpus.values():
        for c in cs:
            for i, (ret, out) in enumerate(c.want()):
                assert len(out) <= c.bound(i)


SHARED = ("all replaced", "all inserted", "mixed", "dropped", "ErrNotFound", "ErrRead", "ErrDismatchType")


def test_fuzz_shares(corpus):
    """from the checker alone: every outcome class is at least 5 % of the (message, item set) cases, and K = 1,
    2, 3, 5 and 7 each appear"""
    sh = MG.shares(corpus["fuzz"])
    for k in SHARED:
        assert sh.get(k, 0) >= 0.05, (k, sh)
    assert {c.k for c in corpus["fuzz"]} >= {1, 2, 3, 5, 7}
    assert {st[0] for c in corpus["fuzz"] for st in c.steps} == {F, I, S, N, BK}
    assert any(not c.shared for c in corpus["fuzz"]) and any(c.shared and c.op == M.SET_OP for c in corpus["fuzz"])


# --------------------------------------------- combine + splice, on the host
def build_host(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "editm_host.cpp")],
                   check=True)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """host(case, route, caps=None) -> [(ret, out)] with the guard bytes around every slot checked"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host many-edit with" % B.HIPCC)
    lib = C.CDLL(build_host(str(tmp_path_factory.mktemp("editm") / "libeditm.so"), ("-shared",)))
    lib.editm_msg.restype = None
    lib.editm_msg.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                              C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_int, C.c_char_p, C.c_uint64,
                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

    def run(case, route, caps=None):
        blob = MG.set_blob(case.parent, case.steps) + b"\0" * 16
        k = case.k
        vt = (C.c_uint32 * k)(*case.val_types)
        res = []
        ret, ol = C.c_uint64(0), C.c_uint32(0)
        for i, m in enumerate(case.msgs):
            vs = [case.value(i, j) if case.op == M.SET_OP else b"" for j in range(k)]
            bufs = [C.create_string_buffer(v + b"\xBB" * 16, len(v) + 16) for v in vs]
            vp = (C.c_void_p * k)(*[C.addressof(b) for b in bufs])
            vl = (C.c_uint64 * k)(*map(len, vs))
            cap = caps[i] if caps is not None else case.bound(i)
            out = C.create_string_buffer(b"\xEE" * (cap + 32), cap + 32)
            lib.editm_msg(m + b"\xAA" * 16, len(m), blob, case.op, case.root_type, vt, vp, vl, route,
                          C.cast(C.byref(out, 16), C.c_char_p), cap, C.byref(ret), C.byref(ol))
            raw = out.raw
            assert raw[:16] == b"\xEE" * 16 and raw[16 + cap:] == b"\xEE" * 16, "a store outside the slot"
            ok = ret.value & 0xFF == M.OK
            used = ol.value if ok else 0
            assert raw[16 + used:16 + cap] == b"\xEE" * (cap - used), "a store beyond out_len, or by a failed message"
            assert ol.value == M.out_len(ret.value, raw[16:16 + used])
            res.append((ret.value, raw[16:16 + used]))
        return res

    return run


def every_route(host, case, caps=None):
    want = case.want(caps)
    for route in (0, 1, 2, 3):  # lane, wave, 4 and 16 lanes a message
        got = host(case, route, caps)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s, route %d, message %d (%r...): got %x / %d bytes, checker %x / %d" % (
                case.what, route, i, case.msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))
    return want


def test_host_hand_written(host):
    for op, msg, parent, items, root, want in HAND:
        assert every_route(host, MG.ManyCase(op, parent, items, [msg], root)) == [want]


def test_host_known_answers(host):
    b = example2()
    i32 = struct.pack(">i", 0x1234567)
    c = MG.ManyCase(M.SET_OP, [(F, 3), (F, 8)], [((I, 1024), i32, R.I32), ((I, 0), i32, R.I32), ((I, 1024), i32[::-1], R.I32)], [b])
    assert every_route(host, c)[0][0] == M.word(M.OK, mask=2)
    c = MG.ManyCase(M.SET_OP, [], [((F, 1), G.wstr(b"hello"), R.STRING), ((F, 2), i32, R.I32),
                                   ((F, 32767), struct.pack(">d", 1.5), R.DOUBLE)], [b])
    assert every_route(host, c)[0][0] == M.word(M.OK, mask=5)
    c = MG.ManyCase(M.UNSET_OP, [(F, 255)], [((F, k),) for k in range(1, 7)], [b])
    assert every_route(host, c)[0][0] == M.word(M.OK, mask=0x3F)


def test_host_fuzz(host, corpus):
    for c in corpus["fuzz"]:
        every_route(host, c)


def test_host_sweeps(host, corpus):
    for name in ("adjacency", "unit", "count", "failure"):
        for c in corpus[name]:
            every_route(host, c)
    ph = corpus["phase"][0]
    want = every_route(host, ph)
    assert all(r == M.word(M.OK, mask=7) for r, _ in want)
    assert {len(o) % 16 for _, o in want} == set(range(16)) and any(len(o) > 1024 for _, o in want)
    assert {R.get_by_path(m, [(F, 2)]).start % 16 for m in ph.msgs} == set(range(16))


def test_host_slots(host, corpus):
    """a slot of exactly the needed size takes the message; one byte less is E_OVERFLOW with the size and no byte stored"""
    for c in corpus["fuzz"][::3] + corpus["count"][:2] + corpus["adjacency"][:3]:
        c = c.sub(range(0, len(c.msgs), 4))
        need = [len(o) for _, o in c.want()]
        assert every_route(host, c, need) == c.want()
        short = [max(n - 1, 0) for n in need]
        want = every_route(host, c, short)
        assert all(w[0] == M.overflow(n) for w, n, (r, _) in zip(want, need, c.want()) if r & 0xFF == M.OK and n)


def test_stand_alone_program_under_sanitizers(tmp_path, corpus):
    """editm_host.cpp as a program (-DEDITM_MAIN) built with AddressSanitizer and UBSan: every message and value
    in a heap block of len + 16 bytes, every slot in one of exactly its size (the needed size, or one byte less
    for every fourth message), the blob in one of its length + 16. All four routes run on every message; the
    counts it prints are the checker's."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host many-edit with" % B.HIPCC)
    exe = build_host(str(tmp_path / "editm"), ("-DEDITM_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                                 "-fno-sanitize-recover=undefined"))
    cases = [c.sub(range(k % 4, len(c.msgs), 4)) for k, c in enumerate(corpus["fuzz"])]
    for name in ("adjacency", "phase", "unit", "count", "failure"):
        cases += corpus[name]
    files, count, existed, total, n_msgs = [], {}, 0, 0, 0
    for k, c in enumerate(cases):
        caps = [max(len(out) - (1 if i % 4 == 3 else 0), 0) for i, (_, out) in enumerate(c.want())]
        for ret, out in c.want(caps):
            count[ret & 0xFF] = count.get(ret & 0xFF, 0) + 1
            if ret & 0xFF == M.OK:
                existed += sum(M.existed_of(ret, c.k))
            total += len(out)
        files.append(str(tmp_path / ("corpus%d.bin" % k)))
        MG.write_corpus(files[-1], c, caps)
        n_msgs += len(c.msgs)
    assert count.get(M.E_OVERFLOW, 0) > 100 and count.get(M.E_SAME, 0) >= 3
    out = subprocess.run([exe, *files], check=True, capture_output=True, text=True).stdout
    assert out.strip() == ("%d messages; OK %d (existed %d), NOT_FOUND %d, E_READ %d, E_TYPE %d, E_SAME %d, "
                           "E_OVERFLOW %d; %d bytes" % (
                               n_msgs, count.get(M.OK, 0), existed, count.get(M.NOT_FOUND, 0), count.get(M.E_READ, 0),
                               count.get(M.E_TYPE, 0), count.get(M.E_SAME, 0), count.get(M.E_OVERFLOW, 0), total)), out
