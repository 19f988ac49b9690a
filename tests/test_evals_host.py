"""CPU: the entry-column encode itself (dynamicgo_amd/csrc/evals_device.h:
ev_entry_size, ev_cell behind ev_pair_cell, ev_head, ev_emit over cl_find: the
code the kernels run) built for the host by evals_host.cpp and compared, byte
by byte, offset by offset and status by status, with the checker (evalsref.py)
over all of evalsgen's inputs, the ones the GPU tests of test_gpu_evals.py use.
Every output lies between bytes of 0xAA that must stay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import evalsgen as EG
import evalsref as ER
from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))


class EvalCol(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in EG.FIELDS] + [("n_ent", C.c_uint64)]


def build_evals(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "evals_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host encode with" % B.HIPCC)


@pytest.fixture(scope="module")
def evalslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_evals(str(tmp_path_factory.mktemp("evals") / "libevalshost.so"), ("-shared",)))
    lib.evals_run.restype = C.c_int
    lib.evals_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                              C.c_void_p, C.c_void_p, C.c_uint32]
    lib.evals_kind_ok.restype = C.c_int
    lib.evals_wire.restype = C.c_uint32
    lib.evals_entry_size.restype = C.c_uint32
    return lib


def records(cols):
    return (EvalCol * len(cols))(*[EvalCol(*[c[f].ctypes.data if f in c else None for f in EG.FIELDS], c["n_ent"])
                                    for c in cols])


def run(lib, case, base=0, cap=None, blocks=3, sizing=False, want=None):
    """(out with its guards, off, status, want) of one emulated batch; out is None when sizing"""
    _, kinds, fids, cols, n = case
    K = len(kinds)
    ids = np.array(fids, dtype=np.int16) if fids is not None else None
    kk = np.array(kinds, dtype=np.uint16)
    off = np.full(n * K + 3, 0x7777777777777777, dtype=np.uint64)
    status = np.full(n * K + 2, 0x77, dtype=np.uint8)
    want = want or ER.encode_batch(kinds, cols, n, fids, base)
    need = want[1][-1]
    cap = need if cap is None else cap
    out = None if sizing else np.full(max(cap, need) + 16 + 64, EG.GUARD, dtype=np.uint8)
    lib.evals_run(kk.ctypes.data, None if ids is None else ids.ctypes.data, K, records(cols), n, base,
                  None if sizing else out.ctypes.data, cap, off[1:].ctypes.data, status[1:].ctypes.data, blocks)
    assert off[0] == off[-1] == 0x7777777777777777 and status[0] == status[-1] == 0x77
    return out, off[1:-1], status[1:-1], want


def check(lib, case, **kw):
    out, off, status, (arena, woff, wst) = run(lib, case, **kw)
    base, cap = kw.get("base", 0), kw.get("cap")
    what = case[0]
    assert off.tolist() == woff, what
    assert status.tolist() == wst, what
    if out is None:
        return wst
    end = woff[-1] if cap is None else min(cap, woff[-1])
    assert (out[:base] == EG.GUARD).all(), what
    assert out[base:end].tobytes() == arena[:max(end - base, 0)], what
    assert (out[max(end, base):] == EG.GUARD).all(), what
    return wst


def test_all_inputs_against_the_checker(evalslib):
    kinds_seen, statuses = set(), set()
    for case in EG.all_cases():
        statuses |= set(check(evalslib, case))
        kinds_seen |= set(case[1])
    assert set(ER.ALL_KINDS) == kinds_seen
    assert statuses == {ER.OK, ER.E_SIZE, ER.E_RANGE}


def test_bases_caps_and_block_counts(evalslib):
    """out_base at every residue mod 16, every cap from 0 to the need of a small batch, 1 to 5 blocks"""
    case = EG.geometry_case(7, 65)
    need = ER.encode_batch(case[1], case[3], case[4])[1][-1]
    for base in list(range(17)) + [8191, 16384]:
        check(evalslib, case, base=base, blocks=1 + base % 5)
    small = EG.geometry_case(7, 2, ids=True)
    want = ER.encode_batch(small[1], small[3], small[4], small[2], 5)
    for cap in range(0, want[1][-1] + 1):
        check(evalslib, small, base=5, cap=cap, want=want)
    for cap in (1, 4095, need // 2, need - 1):
        check(evalslib, case, cap=cap)
    check(evalslib, case, sizing=True)
    big = next(c for c in EG.count_cases() if c[0].startswith("one of 4097"))
    for blocks in (1, 2, 5):
        check(evalslib, big, blocks=blocks)


def test_count_flags_in_a_sizing_call(evalslib):
    """a count of 2^31 is E_SIZE, behind RANGE; the two-entry arrays under n_ent = 2^32 - 1 are not read"""
    for ids in (False, True):
        case = EG.count_flag_case(ids)
        assert check(evalslib, case, sizing=True) == [ER.E_SIZE, ER.OK, ER.E_RANGE, ER.E_RANGE, ER.OK, ER.E_RANGE]


def test_string_outputs_start_at_every_residue():
    """the generator alone: over the 16 shifts, list elements' payloads start at every output residue mod 16"""
    seen = set()
    for case in EG.string_cases():
        off = ER.encode_batch(case[1], case[3], case[4])[1]
        col = case[3][1]
        for i in range(case[4]):
            at = off[i * 3 + 1] + 5
            for e in range(int(col["ent_off"][i]), int(col["ent_off"][i + 1])):
                seen.add((at + 4) % 16)
                at += 4 + int(col["val_len"][e])
    assert seen == set(range(16))


def test_kinds_and_entry_sizes(evalslib):
    for kind in range(0x400):
        assert bool(evalslib.evals_kind_ok(kind)) == ER.kind_ok(kind), kind
        if ER.kind_ok(kind):
            assert evalslib.evals_wire(kind) == ER.wire_type(kind)
    for kt, vt, kl, vl, want in ((11, 11, 0, 0, 8), (11, 10, 2 ** 31 - 1, 0, 2 ** 31 + 11), (11, 10, 2 ** 31, 0, 2 ** 32 - 1),
                                 (0, 11, 5, 2 ** 32 - 1, 2 ** 32 - 1), (11, 11, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 32 - 1),
                                 (8, 11, 9, 2 ** 31 - 1, 2 ** 31 + 7), (3, 2, 7, 7, 2), (10, 4, 0, 0, 16), (0, 11, 0, 7, 11)):
        assert evalslib.evals_entry_size(kt, vt, kl, vl) == want, (kt, vt, kl, vl)


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """evals_host.cpp as a program (-DEVALS_MAIN: every input array and every output in a heap block of its own),
    built with the address and undefined-behaviour sanitizers, over every generated batch as corpus files: it ends
    clean, and the counts and the hash it prints are the checker's."""
    need_hipcc()
    files, cells, flagged, total = [], 0, 0, 0
    h = 0xCBF29CE484222325
    for j, case in enumerate(EG.all_cases()):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        with open(files[-1], "wb") as fh:
            fh.write(EG.corpus_bytes(case))
        arena, off, st = ER.encode_batch(case[1], case[3], case[4], case[2])
        cells, flagged, total = cells + len(st), flagged + sum(s != 0 for s in st), total + len(arena)
        for b in np.array(off, dtype=np.uint64).tobytes() + bytes(st) + arena + bytes([EG.GUARD]) * 16:
            h = ((h ^ b) * 0x100000001B3) & ER.M64
    exe = build_evals(str(tmp_path / "evalshost"), ("-DEVALS_MAIN", "-g", "-fsanitize=address,undefined",
                                                    "-fno-sanitize-recover=undefined"))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    out = run.stdout
    assert out.strip() == "%d cells, %d flagged, %d bytes, hash %016x" % (cells, flagged, total, h), out
