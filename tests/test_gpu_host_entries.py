"""GPU: the five thrift/generic host entries (dg_tget / dg_cut / dg_edit /
dg_editm / dg_kids _batch_host) and the two conversion entries (dg_t2j /
dg_j2t _batch_host) through ctypes with an arena that does not
start at 0. The Python wrappers always pass in_off[0] = 0, so the rebasing the
entries share (csrc/host_layout.h, HostBatch; j2t's own in batch_host) is
reached only here: every
entry is called once with the messages at base 0 and once with the same
messages behind 37 bytes of 0xEE (edit and editm: per-message values behind 11
bytes); the two answers are byte-identical and the first equals the checker's
(t2j: JSON written by hand).
cut, edit, editm, t2j and j2t also answer a one-byte-short output with
DG_E_NOMEM and the size to retry with. The t2j and j2t batches each hold
messages that outgrow their first slot, so the rerun pass gathers them from
behind the padding. dg_t2j_batch_host refuses descending offsets and writes
nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

import cutgen as CG
import cutref as CR
import editgen as G
import editmref as M
import editref as E
import kidsgen as KG
import tgetref as R
from test_gpu_tget import expect as tget_expect, same as tget_same, to_paths

pytestmark = pytest.mark.gpu

F = R.FIELD
PAD, VPAD = 37, 11
NOMEM = -3  # DG_E_NOMEM


def _str(fid, s):
    return G.field(R.STRING, fid, G.wstr(s))


# five tiny messages of five lengths: field 18 alone, fields 18 and 7, no byte at all, a longer 18, 7 before 18
MSGS = [_str(18, b"r") + b"\x00", _str(18, b"") + _str(7, b"old") + b"\x00", b"", _str(18, b"r" * 20) + b"\x00",
        _str(7, b"seven") + _str(18, b"rrr") + b"\x00"]
VALS7 = [G.wstr(b"v" * k) for k in (100, 0, 5, 17, 1)]   # field 7's new value, per message
VALS18 = [G.wstr(b"w" * k) for k in (3, 40, 0, 1, 16)]  # field 18's


def arena(parts, pad):
    """(uint8 array, uint64 offsets): the parts back to back behind `pad` bytes of 0xEE, offsets from `pad`"""
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return np.frombuffer(b"\xEE" * pad + b"".join(parts) + b"\0" * 16, dtype=np.uint8), off + np.uint64(pad)


def lib():
    from dynamicgo_amd import _lib
    return _lib.lib(), _lib.check


def packed(call, n, total):
    """call(out, cap, out_off, ret, need) -> rc at total - 1 (DG_E_NOMEM, *need = total) and at total;
    (ret, out_off, out) of the call that fitted"""
    for cap, rc_want in ((total - 1, NOMEM), (total, 0)):
        out, out_off = np.zeros(max(total, 1), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        ret, need = np.zeros(n, dtype=np.uint64), C.c_uint64(0)
        rc = call(out.ctypes.data, cap, out_off.ctypes.data, ret.ctypes.data, C.byref(need))
        assert rc == rc_want and need.value == total, (cap, rc, need.value, total)
    return ret, out_off, out


def same_packed(got, want, what):
    ret, out_off, out = got
    assert list(ret) == [r for r, _ in want], what
    assert list(out_off) == list(np.concatenate([[0], np.cumsum([len(o) for _, o in want])])), what
    assert out.tobytes() == b"".join(o for _, o in want), what


def twice(run):
    """run(pad) at base 0 and behind the padding: the same bytes; the first answer"""
    first, second = run(0), run(PAD)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return first


def test_tget():
    from dynamicgo_amd import generic as X
    L, check = lib()
    paths = [[(F, 18)], [(F, 7)]]
    with X.PathSet(to_paths(paths)) as ps:
        def run(pad):
            a, off = arena(MSGS, pad)
            rec = np.zeros((len(MSGS), 2), dtype=X.REC_DTYPE)
            check(L.dg_tget_batch_host(ps.ctx.h, ps.h, R.STRUCT, a.ctypes.data, off.ctypes.data, len(MSGS),
                                       rec.ctypes.data))
            return (rec,)

        rec, = twice(run)
    want = tget_expect(MSGS, paths)
    assert {R.OK, R.NOT_FOUND, R.E_READ} <= set(want["status"].ravel().tolist())
    tget_same(rec, want, "host entry")


def test_kids():
    from dynamicgo_amd import generic as X
    L, check = lib()
    n = len(MSGS)
    want = KG.expect(MSGS, (), False)
    total = int(want[1][n])
    assert total == 6
    with X.PathSet([[]]) as ps:
        def run(pad):
            a, off = arena(MSGS, pad)
            head, rec_off = np.zeros(n, dtype=X.KIDS_HEAD_DTYPE), np.zeros(n + 1, dtype=np.uint64)
            recs, need = np.zeros(total, dtype=X.KIDS_REC_DTYPE), C.c_uint64(0)
            check(L.dg_kids_batch_host(ps.ctx.h, ps.h, R.STRUCT, 0, a.ctypes.data, off.ctypes.data, n, head.ctypes.data,
                                       rec_off.ctypes.data, recs.ctypes.data, total, C.byref(need)))
            assert need.value == total
            return head, rec_off, recs

        KG.same(twice(run), want, "host entry")


def test_cut():
    from dynamicgo_amd import generic as X
    L, _ = lib()
    wide, narrow = CG.grow_pair()
    msgs = [CG.grow_message(k) for k in (0, 1, 11, 12, 40)]
    n, opts = len(msgs), CR.WRITE_DEFAULT
    want = CG.expect(msgs, wide, narrow, opts)
    assert all(r == 0 for r, _ in want)
    total = sum(len(o) for _, o in want)
    with X.CutPlan(wide, narrow) as plan:
        # the first pass's slot overflows on exactly 2 of the 5: the second pass gathers them from the arena
        first = [min(plan.slot_bound(len(m), opts), len(m) + 256) for m in msgs]
        assert [len(o) > cap for (_, o), cap in zip(want, first)] == [False, False, False, True, True]

        def run(pad):
            a, off = arena(msgs, pad)
            return packed(lambda *o: L.dg_cut_batch_host(plan.ctx.h, plan.h, opts, a.ctypes.data, off.ctypes.data, n, *o),
                          n, total)

        same_packed(twice(run), want, "host entry")


def test_edit():
    from dynamicgo_amd import generic as X
    L, _ = lib()
    n = len(MSGS)
    want = [E.edit(E.SET_OP, m, [(F, 7)], v, R.STRING) for m, v in zip(MSGS, VALS7)]
    assert {r & 0xFF for r, _ in want} == {E.OK, R.E_READ} and len({r for r, _ in want}) == 3  # insert, replace, error
    total = sum(len(o) for _, o in want)
    with X.EditPlan([X.PathFieldId(7)], X.EDIT_SET) as p:
        def run(pad):
            a, off = arena(MSGS, pad)
            v, voff = arena(VALS7, VPAD if pad else 0)
            return packed(lambda *o: L.dg_edit_batch_host(p.ctx.h, p.h, R.STRUCT, a.ctypes.data, off.ctypes.data, n,
                                                          R.STRING, v.ctypes.data, voff.ctypes.data, 0, *o), n, total)

        same_packed(twice(run), want, "host entry")


def test_editm():
    from dynamicgo_amd import generic as X
    L, _ = lib()
    n = len(MSGS)
    want = [M.edit_many(M.SET_OP, m, [], [((F, 7), v7, R.STRING), ((F, 18), v18, R.STRING)])
            for m, v7, v18 in zip(MSGS, VALS7, VALS18)]
    assert {M.status_of(r) for r, _ in want} == {M.OK, R.E_READ} and len({r for r, _ in want}) == 3
    total = sum(len(o) for _, o in want)
    vt, vl = np.array([R.STRING, R.STRING], dtype=np.uint8), np.zeros(2, dtype=np.uint64)
    with X.EditManyPlan([], [X.PathFieldId(7), X.PathFieldId(18)], X.EDIT_SET) as p:
        def run(pad):
            a, off = arena(MSGS, pad)
            v, voff = arena([x for pair in zip(VALS7, VALS18) for x in pair], VPAD if pad else 0)  # message-major
            return packed(lambda *o: L.dg_editm_batch_host(p.ctx.h, p.h, R.STRUCT, a.ctypes.data, off.ctypes.data, n,
                                                           vt.ctypes.data, v.ctypes.data, voff.ctypes.data,
                                                           vl.ctypes.data, *o), n, total)

        same_packed(twice(run), want, "host entry")


def test_t2j():
    from dynamicgo_amd import conv, thrift as T
    L, _ = lib()
    fl = T.flatten(T.struct_type("S", [T.FieldDescriptor(1, "s", T.builtin("string"), T.OPTIONAL)]))
    ks = (0, 1, 7, 100)
    msgs = [b"\x0b\x00\x01" + struct.pack(">i", k) + b"\x01" * k + b"\x00" for k in ks] + [b"\x00"]
    want = [(0, b'{"s":"' + b"\\u0001" * k + b'"}') for k in ks] + [(0, b"{}")]
    n, total = len(msgs), sum(len(o) for _, o in want)
    # k = 100 alone (108 bytes in, 608 out, a first slot of 512) takes the rerun pass: todo = [3]
    assert (len(msgs[3]), len(want[3][1]), L.dg_t2j_slot_bound(108)) == (108, 608, 512)
    assert [len(o) > L.dg_t2j_slot_bound(len(m)) for m, (_, o) in zip(msgs, want)] == [False, False, False, True, False]
    ctx = conv.default_context()
    d = ctx.desc_t2j(fl)

    def run(pad):
        a, off = arena(msgs, pad)
        return packed(lambda *o: L.dg_t2j_batch_host(ctx.h, d, fl.root_type, a.ctypes.data, off.ctypes.data, n, 0, *o),
                      n, total)

    same_packed(twice(run), want, "host entry")


def test_t2j_refuses_descending_offsets():
    from dynamicgo_amd import conv, thrift as T
    L, _ = lib()
    fl = T.flatten(T.struct_type("S", [T.FieldDescriptor(1, "s", T.builtin("string"), T.OPTIONAL)]))
    ctx = conv.default_context()
    a = np.frombuffer(b"\x00" * 3 + b"\0" * 16, dtype=np.uint8)
    off = np.array([0, 2, 1, 3], dtype=np.uint64)  # message 1 ends before it starts
    out, out_off = np.full(64, 0xAB, dtype=np.uint8), np.full(4, 0xAB, dtype=np.uint64)
    ret, need = np.full(3, 0xAB, dtype=np.uint64), C.c_uint64(0xAB)
    rc = L.dg_t2j_batch_host(ctx.h, ctx.desc_t2j(fl), fl.root_type, a.ctypes.data, off.ctypes.data, 3, 0, out.ctypes.data,
                             64, out_off.ctypes.data, ret.ctypes.data, C.byref(need))
    assert rc == -1  # DG_E_INVALID
    assert need.value == 0xAB and all((x == 0xAB).all() for x in (out, out_off, ret))


def test_j2t():
    import oracle
    from dynamicgo_amd import conv, thrift as T
    L, _ = lib()
    fl = T.flatten(T.struct_type("Wide", [T.FieldDescriptor(i, "f%d" % i, T.builtin("i64"), T.DEFAULT)
                                          for i in range(1, 13)]))
    flags = 0x3  # allow unknown fields, write the default ones: every struct comes out as 12 fields, 133 bytes
    full = b"{" + b",".join(b'"f%d":%d' % (i, -i) for i in range(1, 13)) + b"}"
    msgs = [b"{}", full, b"[]", b'{"f3":-1}', b""]
    chk = oracle.RefOracle() or oracle.PortOracle()
    want = [chk.j2t(fl, m, flags) for m in msgs]

    def field(i, v):
        return b"\x0a" + struct.pack(">hq", i, v)

    # by hand: the fields given in the order given, then the unset ones by id
    assert want[0] == (0, b"".join(field(i, 0) for i in range(1, 13)) + b"\x00")
    assert want[1] == (0, b"".join(field(i, -i) for i in range(1, 13)) + b"\x00")
    assert want[3] == (0, field(3, -1) + b"".join(field(i, 0) for i in range(1, 13) if i != 3) + b"\x00")
    assert want[2][0] != 0 and want[2][1] == b""
    # 133 bytes outgrow dg_slot_bound of the two short structs: the rerun pass takes messages 0 and 3
    assert [r == 0 and len(o) > L.dg_slot_bound(len(m)) for m, (r, o) in zip(msgs, want)] == [True, False, False, True, False]
    n, total = len(msgs), sum(len(o) for _, o in want)
    ctx = conv.default_context()
    d = ctx.desc(fl)

    def run(pad):
        a, off = arena(msgs, pad)
        return packed(lambda *o: L.dg_j2t_batch_host(ctx.h, d, fl.root_type, a.ctypes.data, off.ctypes.data, n, flags, *o),
                      n, total)

    same_packed(twice(run), want, "host entry")
