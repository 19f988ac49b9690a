"""CPU: the row-column encode itself (dynamicgo_amd/csrc/rvals_device.h:
rv_size_lane, rv_msg_lane, rv_list_head, rv_head_lane and rv_granule over
cl_find: the code the kernels run) built for the host by rvals_host.cpp and
compared, byte by byte, offset by offset and status by status, with the checker
(rvalsref.py) over all of rvalsgen's inputs, the ones the GPU tests of
test_gpu_rvals.py use. Every output lies between bytes of 0xAA that must stay,
and so does every part of the work space (rvals_run answers 1 otherwise)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rvalsgen as RG
import rvalsref as RR
import valsref as VR
from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("val", "len", "src", "elem_off", "elems", "present")


class ValCol(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in FIELDS]


def build_rvals(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "rvals_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host encode with" % B.HIPCC)


@pytest.fixture(scope="module")
def rvalslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_rvals(str(tmp_path_factory.mktemp("rvals") / "librvalshost.so"), ("-shared",)))
    lib.rvals_run.restype = C.c_int
    lib.rvals_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def wants():
    """the checker's answer per case name, computed once"""
    return {c[0]: RR.encode_batch(c[1], c[2], c[3], c[4], c[5], c[6]) for c in RG.all_cases()}


def records(cols):
    return (ValCol * len(cols))(*[ValCol(*[c[f].ctypes.data if f in c else None for f in FIELDS]) for c in cols])


def rebase(want, base):
    return want[0], [o + base for o in want[1]], want[2], want[3]


def run(lib, case, want, base=0, cap=None, blocks=3, sizing=False, route=0, cells=True):
    """(out with its guards, off, status, cell_status) of one emulated batch; out is None when sizing"""
    _, kinds, fids, cols, row_off, n, n_rows = case
    K = len(kinds)
    ids = np.array(fids, dtype=np.int16)
    kk = np.array(kinds, dtype=np.uint8)
    off = np.full(n + 3, 0x7777777777777777, dtype=np.uint64)
    status = np.full(n + 2, 0x77, dtype=np.uint8)
    cst = np.full(n_rows * K + 2 if cells else 2, 0x77, dtype=np.uint8)
    need = want[1][-1]
    cap = need if cap is None else cap
    out = None if sizing else np.full(max(cap, need) + 16 + 64, RG.GUARD, dtype=np.uint8)
    rc = lib.rvals_run(kk.ctypes.data, ids.ctypes.data, K, records(cols), row_off.ctypes.data, n, n_rows, base,
                       None if sizing else out.ctypes.data, cap, off[1:].ctypes.data, status[1:].ctypes.data,
                       cst[1:].ctypes.data if cells else None, blocks, route)
    assert rc == 0, "a guard of the work space broke"
    assert off[0] == off[-1] == 0x7777777777777777 and status[0] == status[-1] == 0x77 and cst[0] == cst[-1] == 0x77
    return out, off[1:-1], status[1:-1], cst[1:-1]


def check(lib, case, want, **kw):
    base, cap = kw.get("base", 0), kw.get("cap")
    arena, woff, wst, wcst = rebase(want, base)
    out, off, status, cst = run(lib, case, (arena, woff, wst, wcst), **kw)
    what = case[0]
    assert off.tolist() == woff, what
    assert status.tolist() == wst, what
    if kw.get("cells", True):
        assert cst.tolist() == wcst, what
    if out is None:
        return
    end = woff[-1] if cap is None else min(cap, woff[-1])
    assert (out[:base] == RG.GUARD).all(), what
    assert out[base:end].tobytes() == arena[:max(end - base, 0)], what
    assert (out[max(end, base):] == RG.GUARD).all(), what


def test_all_inputs_against_the_checker(rvalslib, wants):
    kinds_seen, statuses, cell_statuses, ks = set(), set(), set(), set()
    for case in RG.all_cases():
        want = wants[case[0]]
        check(rvalslib, case, want)
        kinds_seen |= set(case[1])
        statuses |= set(want[2])
        cell_statuses |= set(want[3])
        ks.add(len(case[1]))
    assert set(RR.ALL_KINDS) == kinds_seen
    assert statuses == {RR.OK, RR.E_SIZE, RR.E_RANGE} and cell_statuses == {RR.OK, RR.E_SIZE}
    assert {1, 2, 7, 16} <= ks


def test_the_generator_covers_what_it_says(wants):
    """from the generator and the checker alone: the row counts, the chunk counts, overlap and gaps"""
    counts = set()
    for case in RG.count_cases():
        ro = case[4].tolist()
        counts |= {b - a for a, b in zip(ro, ro[1:])}
    assert set(RG.ROW_COUNTS) | {4097} <= counts
    for chunks, case in zip((1, 2, 3), RG.chunk_cases()):
        assert (chunks - 1) * RG.CHUNK < wants[case[0]][1][-1] <= chunks * RG.CHUNK
    case = next(RG.overlap_cases())
    owners = np.zeros(case[6], dtype=int)
    for (a, b), st in zip(zip(case[4].tolist(), case[4].tolist()[1:]), wants[case[0]][2]):
        if st == RR.OK:
            owners[a:b] += 1
    assert owners.max() >= 2 and owners.min() == 0  # rows written more than once, rows nobody owns
    for case in RG.present_cases():
        K = len(case[1])
        pres = np.array([c.get("present", np.ones(case[6], dtype=np.uint8)) for c in case[3]])
        if case[0] == "presence":
            assert {tuple(pres[:, g]) for g in range(case[6])} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        assert (pres[K - 1] == 0).any()


def test_string_outputs_start_at_every_residue(wants):
    """the generator alone: over the 16 shifts, payloads start at every output residue mod 16"""
    seen, lens = set(), set()
    for case in RG.string_cases():
        if len(case[1]) != 1:
            continue
        off = wants[case[0]][1]
        col, ro = case[3][0], case[4].tolist()
        for i in range(case[5]):
            at = off[i] + RR.HDR
            for g in range(ro[i], ro[i + 1]):
                if i:
                    seen.add((at + 7) % 16)
                at += 3 + 4 + int(col["len"][g]) + 1
                lens.add(int(col["len"][g]))
            assert at == off[i + 1]
    assert seen == set(range(16))
    assert 16385 in lens


def test_bases_caps_and_block_counts(rvalslib, wants):
    """out_base at every residue mod 16, every cap from 0 to the need of a small batch, 1 to 5 blocks"""
    case = RG.geometry_case(7, 65)
    want = wants[case[0]]
    need = want[1][-1]
    for base in list(range(17)) + [8191, 16384]:
        check(rvalslib, case, want, base=base, blocks=1 + base % 5)
    small = RG.geometry_case(7, 4, n=3, seed=5)
    swant = RR.encode_batch(*small[1:])
    for cap in range(0, swant[1][-1] + 5 + 1):
        check(rvalslib, small, swant, base=5, cap=cap)
    for cap in (1, 4095, need // 2, need - 1):
        check(rvalslib, case, want, cap=cap)
    check(rvalslib, case, want, sizing=True)
    big = next(c for c in RG.count_cases() if c[0].startswith("one of 4097"))
    for blocks in (1, 2, 5):
        check(rvalslib, big, wants[big[0]], blocks=blocks)


def test_fixed_stride_route_against_the_scanned_route(rvalslib, wants):
    """the same scalar inputs by the closed form and by the scan"""
    done = 0
    for case in RG.all_cases():
        if all(k in VR.WIDTH for k in case[1]) and not any("present" in c for c in case[3]):
            for route in (0, 1):
                check(rvalslib, case, wants[case[0]], route=route, base=3 * route)
            done += 1
    assert done >= 3


def test_count_flags_in_a_sizing_call(rvalslib):
    """a count of 2^31 is E_SIZE, behind RANGE; the one-row array under n_rows = 2^31 + 8 is not read"""
    case, (woff, wst) = RG.count_flag_case()
    check(rvalslib, case, (b"", woff, wst, []), sizing=True, cells=False)


def test_stand_alone_program_reads_a_corpus(tmp_path, wants):
    """rvals_host.cpp as a program (-DRVALS_MAIN: every input array and every output in a heap block of its own),
    built with the address and undefined-behaviour sanitizers, over every generated batch as corpus files: it ends
    clean, and the counts and the hash it prints are the checker's."""
    need_hipcc()
    files, msgs, flagged, cells, cell_flagged, total = [], 0, 0, 0, 0, 0
    h = 0xCBF29CE484222325
    for j, case in enumerate(RG.all_cases()):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        with open(files[-1], "wb") as fh:
            fh.write(RG.corpus_bytes(case))
        arena, off, st, cst = wants[case[0]]
        msgs, flagged, cells = msgs + len(st), flagged + sum(s != 0 for s in st), cells + len(cst)
        cell_flagged, total = cell_flagged + sum(s != 0 for s in cst), total + len(arena)
        for b in np.array(off, dtype=np.uint64).tobytes() + bytes(st) + bytes(cst) + arena + bytes([RG.GUARD]) * 16:
            h = ((h ^ b) * 0x100000001B3) & VR.M64
    exe = build_rvals(str(tmp_path / "rvalshost"), ("-DRVALS_MAIN", "-g", "-fsanitize=address,undefined",
                                                    "-fno-sanitize-recover=undefined"))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    assert run.stdout.strip() == "%d messages, %d flagged, %d cells, %d flagged, %d bytes, hash %016x" % (
        msgs, flagged, cells, cell_flagged, total, h), run.stdout
