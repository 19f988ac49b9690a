"""CPU: the path-lookup checker (tgetref.py) pinned to known answers and to the
reference's compiled skipper, the path-set blob layout and its limits, and
name resolution through the descriptor (dynamicgo_amd.generic)."""
import ctypes as C
import os
import random
import struct

import pytest

import t2jgen
import tgetgen
import tgetref as R
from conftest import GOLDEN
from dynamicgo_amd import generic as G
from dynamicgo_amd.http import ConvError

F, I, S, N, B = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY


def example2():
    with open(os.path.join(GOLDEN, "example2.bin"), "rb") as fh:
        return fh.read()


def test_checker_known_answers():
    """thrift/generic/value_test.go:339-395 over testdata/sample/example2.go:44-62"""
    b = example2()
    assert len(b) == 1326

    def get(*path):
        r = R.get_by_path(b, list(path))
        return r, R.raw(b, r)

    r, raw = get((F, 3), (F, 8), (I, 1))
    assert (r.status, r.type, r.start, r.end) == (R.OK, R.I32, 93, 97) and struct.unpack(">i", raw)[0] == 0
    r, raw = get((F, 3), (F, 12), (N, 2))
    assert (r.status, r.type, raw) == (R.OK, R.STRING, b"\0\0\0\x01B")
    r, raw = get((F, 3), (F, 9), (S, b"b"))
    assert (r.status, r.type, raw) == (R.OK, R.STRING, b"\0\0\0\x01B")
    assert get((F, 1))[1] == b"\0\0\0\x05hello"
    assert get((F, 3), (F, 7))[1][4:].decode() == "你好"
    r, _ = get((F, 255))
    assert (r.status, r.type, r.start, r.end) == (R.OK, R.STRUCT, 1233, 1325)
    r, _ = get((F, 3), (F, 9), (S, b"aa"))
    assert (r.status, r.type, r.start, r.step) == (R.NOT_FOUND, R.MAP, 110, 2)
    r, _ = get((F, 3), (F, 8), (I, 999))
    assert (r.status, r.type, r.start, r.step) == (R.NOT_FOUND, R.LIST, 89, 2)
    r, _ = get((F, 222))
    assert (r.status, r.type, r.start, r.step) == (R.NOT_FOUND, R.STRUCT, 0, 0)
    r, _ = get()
    assert (r.status, r.type, r.start, r.end) == (R.OK, R.STRUCT, 0, 1326)


def test_checker_rules():
    # LIST or SET of a missed index: the last field header's wire type, the root type without one
    lst = struct.pack(">bi", R.I32, 1) + struct.pack(">i", 5)
    assert R.get_by_path(lst, [(I, 3)], R.LIST).type == R.LIST
    assert R.get_by_path(lst, [(I, 3)], R.SET).type == R.SET
    assert R.get_by_path(struct.pack(">bh", R.SET, 1) + lst + b"\0", [(F, 1), (I, 3)]).type == R.SET
    assert R.get_by_path(struct.pack(">bh", R.LIST, 1) + lst + b"\0", [(F, 1), (I, 3)]).type == R.LIST
    # an int key on a byte-keyed map reads the byte unsigned
    m = struct.pack(">bbi", R.BYTE, R.BYTE, 1) + b"\xff\x07"
    assert R.get_by_path(m, [(N, -1)], R.MAP).status == R.NOT_FOUND
    assert R.get_by_path(m, [(N, 255)], R.MAP)[:4] == (7, 8, R.BYTE, R.OK)
    assert R.get_by_path(m, [(S, b"a")], R.MAP)[3:] == (R.E_TYPE, 0, R.BYTE)
    # invalid wire types fail in a header the search reads, not in a skipped empty list
    assert R.get_by_path(b"\x05\x00\x01", [(F, 1)]).status == R.E_READ
    assert R.get_by_path(struct.pack(">bhbi", R.LIST, 1, 5, 0) + b"\0", [(F, 2)]).status == R.NOT_FOUND
    assert R.get_by_path(struct.pack(">bhbi", R.LIST, 1, 5, 0) + b"\0", [(F, 1), (I, 0)]).status == R.E_READ
    # MaxSkipDepth: 1023 nested structs skip, 1024 do not
    assert R.get_by_path(t2jgen.chain_thrift(1023), []).status == R.OK
    assert R.get_by_path(t2jgen.chain_thrift(1024), []).status == R.E_READ


class _SkipBuf(C.Structure):
    """skipbuf_t (native/thrift_skip.c:39-45): 8 bytes"""
    _fields_ = [("t", C.c_uint8), ("k", C.c_uint8), ("v", C.c_uint8), ("n", C.c_uint32)]


def test_checker_skip_matches_compiled_reference():
    """skipType's restatement against tb_skip (native/thrift_skip.c:115) of the
    reference library build() compiles: the whole struct and each top-level
    field value of well-formed messages."""
    import oracle
    p = oracle.ref_lib_path()
    if p is None:
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    lib = C.CDLL(p)
    lib.tb_skip.restype = C.c_int64
    lib.tb_skip.argtypes = [C.POINTER(_SkipBuf), C.c_char_p, C.c_int64, C.c_uint8]
    assert C.sizeof(_SkipBuf) == 8
    st = (_SkipBuf * 1024)()
    rng = random.Random(1234)
    td = t2jgen.all_types_desc()

    def both(m):
        pr = R.Proto(m)
        pr.skip_type(R.STRUCT)
        assert pr.read == len(m) == lib.tb_skip(st, m, len(m), R.STRUCT)
        pr = R.Proto(m)
        fields = 0
        while True:
            t, _ = pr.read_field_begin()
            if t == R.STOP:
                return fields
            at = pr.read
            pr.skip_type(t)
            assert pr.read - at == lib.tb_skip(st, m[at:], len(m) - at, t), (t, at)
            fields += 1

    assert sum(both(t2jgen.gen_thrift(rng, td)) for _ in range(256)) > 2000
    # chains of every container kind (tgetgen.chain_message), 0 to 12 levels: far below either skipper's depth rule
    rng = random.Random(5)
    for d in range(13):
        for _ in range(16):
            assert both(tgetgen.chain_message(*tgetgen.random_chain(rng, d))) == 2


def test_blob_layout():
    blob = G.compile_paths([[G.PathFieldId(3), G.PathFieldId(9), G.PathStrKey("b")], [],
                            [G.PathFieldId(-5), G.PathIndex(7), G.PathIntKey(-2), G.PathBinKey(b"\0\0\0\2")]])
    magic, ver, total, n_paths, n_steps, off_steps, off_pool, pool_len = struct.unpack("<8I", blob[:32])
    assert (magic, ver, total, n_paths, n_steps) == (0x31504744, 1, len(blob), 3, 7)
    assert off_steps == 56 and off_steps % 8 == 0 and off_pool == off_steps + 16 * 7 and pool_len == 5
    assert off_pool + pool_len == total
    assert [struct.unpack_from("<II", blob, 32 + 8 * k) for k in range(3)] == [(0, 3), (3, 0), (3, 4)]
    steps = [struct.unpack_from("<IIq", blob, off_steps + 16 * k) for k in range(7)]
    assert steps == [(1, 0, 3), (1, 0, 9), (3, 1, 0), (1, 0, -5), (2, 0, 7), (4, 0, -2), (5, 4, 1)]
    assert blob[off_pool:] == b"b\0\0\0\2"


def test_blob_limits():
    one = [G.PathFieldId(1)]
    G.compile_paths([one] * 8)
    G.compile_paths([one * 16])
    with pytest.raises(ValueError):
        G.compile_paths([one] * 9)
    with pytest.raises(ValueError):
        G.compile_paths([])
    with pytest.raises(ValueError):
        G.compile_paths([one * 17])
    with pytest.raises(ValueError):
        G.PathIndex(-1)
    with pytest.raises(ValueError):
        G.compile_paths([[G.Path(G.PS_INDEX, -1)]])
    with pytest.raises(ValueError):
        G.PathFieldId(40000)


def test_name_resolution():
    td = t2jgen.all_types_desc()

    def steps(path):
        blob = G.compile_paths([path], td)
        n, off = struct.unpack_from("<I", blob, 16)[0], struct.unpack_from("<I", blob, 20)[0]
        return [struct.unpack_from("<IIq", blob, off + 16 * k)[::2] for k in range(n)]

    assert steps([G.PathFieldName("req_s")]) == [(F, 18)]
    assert steps([G.PathFieldName("inner"), G.PathFieldName("a")]) == [(F, 9), (F, 1)]
    # through a list element, a map element, and a recursive struct
    assert steps([G.PathFieldName("inners"), G.PathIndex(1), G.PathFieldName("b")]) == [(F, 10), (I, 1), (F, 2)]
    assert steps([G.PathFieldName("m_i32"), G.PathIntKey(1), G.PathFieldName("c")]) == [(F, 15), (N, 1), (F, 3)]
    assert steps([G.PathFieldId(17), G.PathFieldName("kids"), G.PathIndex(0), G.PathFieldName("next"),
                  G.PathFieldName("val")]) == [(F, 17), (F, 3), (I, 0), (F, 2), (F, 1)]
    assert steps([G.PathFieldName("m_i64"), G.PathIntKey(-3), G.PathStrKey("x")])[0] == (F, 16)
    assert steps([G.PathFieldName('q"uo\\teé\x01')]) == [(F, 7)]  # an alias is a key of the name map too
    with pytest.raises(ConvError) as e:
        G.compile_paths([[G.PathFieldName("inner"), G.PathFieldName("nope")]], td)
    assert e.value.behavior == "ErrUnknownField" and str(e.value) == "field name 'nope' is not defined in IDL"
    with pytest.raises(ConvError):  # a name of the parent struct is no name of the child
        G.compile_paths([[G.PathFieldName("inner"), G.PathFieldName("req_s")]], td)
    with pytest.raises(ConvError):
        G.compile_paths([[G.PathFieldName("req_s")]])  # a name without a descriptor
    with pytest.raises(ValueError):
        G.compile_paths([[G.PathFieldName("inners"), G.PathIndex(-1)]], td)
