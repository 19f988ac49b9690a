"""CPU: the typed-column encode itself (dynamicgo_amd/csrc/vals_device.h: vl_size
behind vl_pair, vl_head, vl_unit, vl_granule over cl_find: the code the kernels
run) built for the host by vals_host.cpp and compared, byte by byte, offset by
offset and status by status, with the checker (valsref.py) over all of
valsgen's inputs, the ones the GPU tests of test_gpu_vals.py use. Every output
is followed by 16 bytes of 0xAA that must stay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import valsgen as VG
import valsref as VR
from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("val", "len", "src", "elem_off", "elems", "present")


class ValCol(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in FIELDS]


def build_vals(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "vals_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host encode with" % B.HIPCC)


@pytest.fixture(scope="module")
def valslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_vals(str(tmp_path_factory.mktemp("vals") / "libvalshost.so"), ("-shared",)))
    lib.vals_run.restype = C.c_int
    lib.vals_run.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                             C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint32]
    lib.vals_size.restype = None
    lib.vals_size.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p]
    lib.vals_kind_ok.restype = C.c_int
    lib.vals_wire.restype = C.c_uint32
    return lib


def run(lib, case, lane, base=0, cap=None, closed=False, blocks=3, sizing=False):
    """(out with its guards, off, status) of one emulated batch; out is None when sizing"""
    _, kinds, fids, cols, n = case
    K = len(kinds)
    recs = (ValCol * K)(*[ValCol(*[c[f].ctypes.data if f in c else None for f in FIELDS]) for c in cols])
    ids = np.array(fids, dtype=np.int16) if fids is not None else None
    off = np.full(n * K + 3, 0x7777777777777777, dtype=np.uint64)
    status = np.full(n * K + 2, 0x77, dtype=np.uint8)
    want = VR.encode_batch(kinds, cols, n, fids, base)
    need = want[1][-1]
    cap = need if cap is None else cap
    out = None if sizing else np.full(max(cap, need) + 16 + 64, VG.GUARD, dtype=np.uint8)
    lib.vals_run(bytes(kinds), None if ids is None else ids.ctypes.data, K, recs, n, base,
                 None if sizing else out.ctypes.data, cap, off[1:].ctypes.data, status[1:].ctypes.data, lane, closed, blocks)
    assert off[0] == off[-1] == 0x7777777777777777 and status[0] == status[-1] == 0x77
    return out, off[1:-1], status[1:-1], want


def check(lib, case, lane, **kw):
    out, off, status, (arena, woff, wst) = run(lib, case, lane, **kw)
    base, cap = kw.get("base", 0), kw.get("cap")
    what = "%s, lane_emit %d" % (case[0], lane)
    assert off.tolist() == woff, what
    assert status.tolist() == wst, what
    if out is None:
        return
    end = woff[-1] if cap is None else min(cap, woff[-1])
    assert (out[:base] == VG.GUARD).all(), what
    assert out[base:end].tobytes() == arena[:max(end - base, 0)], what
    assert (out[max(end, base):] == VG.GUARD).all(), what


@pytest.mark.parametrize("lane", (0, 1))
def test_all_inputs_against_the_checker(valslib, lane):
    kinds_seen = set()
    for case in VG.all_cases():
        check(valslib, case, lane)
        kinds_seen |= set(case[1])
    assert {VR.BOOL, VR.I08, VR.I16, VR.I32, VR.I64, VR.DOUBLE, VR.STRING} <= kinds_seen
    assert {c | et for c in (VR.LIST, VR.SET) for et in VG.ELEM_TYPES} <= kinds_seen


def test_bases_caps_and_block_counts(valslib):
    """out_base at every residue mod 16, a cap below the need at every cut of a small batch, 1 to 5 blocks"""
    case = VG.geometry_case(7, 65)
    need = VR.encode_batch(case[1], case[3], case[4])[1][-1]
    for base in list(range(17)) + [8191, 16384]:
        check(valslib, case, 0, base=base, blocks=1 + base % 5)
    small = VG.geometry_case(7, 2, ids=True)
    snd = VR.encode_batch(small[1], small[3], small[4], small[2], 5)[1][-1]
    for cap in range(0, snd + 1):
        for lane in (0, 1):
            check(valslib, small, lane, base=5, cap=cap)
    for cap in (1, 4095, need // 2, need - 1):
        for lane in (0, 1):
            check(valslib, case, lane, cap=cap)
    check(valslib, case, 0, sizing=True)


def test_closed_form_offsets_equal_the_running_sum(valslib):
    for case in list(VG.matrix_cases()) + [c for c in VG.struct_cases() if c[0] == "struct scalars"]:
        for closed in (False, True):
            check(valslib, case, 0, base=9, closed=closed)


def test_error_cells_size_as_the_empty_value(valslib):
    out = np.zeros(4, dtype=np.uint64)
    cells = [(VR.STRING, 0x80000000), (VR.STRING, 0xFFFFFFFF), (VR.STRING, 0x7FFFFFFF), (VR.LIST | VR.I08, 2 ** 31),
             (VR.LIST | VR.I08, 2 ** 31 - 1), (VR.LIST | VR.I64, 2 ** 29), (VR.SET | VR.I64, 2 ** 29 - 1),
             (VR.LIST | VR.I32, 2 ** 30), (VR.LIST | VR.I32, 2 ** 30 - 2), (VR.SET | VR.I16, 2 ** 64 - 1),
             (VR.LIST | VR.DOUBLE, 2 ** 63)]
    flagged = 0
    for kind, cnt in cells:
        for fh, stop in ((0, 0), (3, 0), (3, 1)):
            valslib.vals_size(kind, fh, stop, 1, cnt, out.ctypes.data)
            ln, st, wcnt = VR.item_size(kind, cnt, fh, stop)
            assert out.tolist() == [ln, st, fh + (4 if kind == VR.STRING else 5), wcnt], (kind, cnt, fh, stop)
            flagged += st == VR.E_SIZE
    assert 0 < flagged < 3 * len(cells)
    # the item of 2^32 bytes exactly is flagged, one byte less is not
    assert VR.item_size(VR.LIST | VR.I08, 2 ** 31 - 1, 3, 1)[1] == VR.OK
    assert VR.item_size(VR.LIST | VR.I16, 2 ** 31 - 3)[1] == VR.OK and VR.item_size(VR.LIST | VR.I16, 2 ** 31 - 2)[1] == VR.E_SIZE


def test_kinds(valslib):
    for kind in range(256):
        assert bool(valslib.vals_kind_ok(kind)) == VR.kind_ok(kind), kind
        if VR.kind_ok(kind):
            assert valslib.vals_wire(kind) == VR.wire_type(kind)


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """vals_host.cpp as a program (-DVALS_MAIN: every input array and every output in a heap block of its own) over
    corpus files: both emits agree and the counts and the hash it prints are the checker's."""
    need_hipcc()
    files, cells, flagged, total = [], 0, 0, 0
    h = 0xCBF29CE484222325
    for j, case in enumerate(VG.all_cases(geometry_k=(3, 16), geometry_n=(65,))):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        with open(files[-1], "wb") as fh:
            fh.write(VG.corpus_bytes(case))
        arena, off, st = VR.encode_batch(case[1], case[3], case[4], case[2])
        cells, flagged, total = cells + len(st), flagged + sum(st), total + len(arena)
        for b in np.array(off, dtype=np.uint64).tobytes() + bytes(st) + arena + bytes([VG.GUARD]) * 16:
            h = ((h ^ b) * 0x100000001B3) & VR.M64
    exe = build_vals(str(tmp_path / "valshost"), ("-DVALS_MAIN",))
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    assert out.strip() == "%d cells, %d flagged, %d bytes, hash %016x" % (cells, flagged, total, h), out
