"""CPU: the row-column walk itself (dynamicgo_amd/csrc/rows_device.h: the
counting and the storing sink behind kd_scan, and tg_walk over an index entry
followed by cl_cell: the code the kernels run) built for the host by
rows_host.cpp and compared, head by head, index entry by index entry and cell
by cell, with the checker (rowsref.py) over all of rowsgen's inputs, the ones the
GPU tests of test_gpu_rows.py use, and the fuzz corpus. Every message is
followed by 16 bytes of 0xAA."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import colsgen as CG
import kidsgen as KG
import rowsgen as RG
import t2jgen
import tgetgen as TG
import tgetref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import to_paths

HERE = os.path.dirname(os.path.abspath(__file__))


def build_rows(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "rows_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)


def blobs(s):
    return G.compile_paths(to_paths([s.parent])), G.compile_paths(to_paths([p for p, _ in s.columns]))


@pytest.fixture(scope="module")
def rowslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_rows(str(tmp_path_factory.mktemp("rows") / "librowshost.so"), ("-shared",)))
    common = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.rows_head.restype = lib.rows_rest.restype = C.c_int
    lib.rows_head.argtypes = common
    lib.rows_rest.argtypes = common + [C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def walk(rowslib):
    """walk(set, row_cap=None) -> ((head, row_off, index, cols) as rowsgen.arrays gives them, deep flags[n])"""
    lib = rowslib

    def run(s, cap=None):
        pb, sb = blobs(s)
        pb, sb = pb + b"\0" * 16, sb + b"\0" * 16
        P = len(s.columns)
        kinds = int.from_bytes(bytes([k for _, k in s.columns]).ljust(8, b"\0"), "little")
        heads, ents, cells, deep, base = [], [], [], [], 0
        for i, m in enumerate(s.msgs):
            buf = m + b"\xAA" * 16
            head = np.zeros(1, dtype=G.ROWS_HEAD_DTYPE)
            d = lib.rows_head(buf, len(m), pb, sb, P, s.root_type, kinds, head.ctypes.data)
            assert d >= 0
            h = head[0]
            n = int(h["count"])
            take = n if cap is None else min(n, cap)
            if h["status"] == R.OK and n:
                idx = np.full(take + 1, 0x5A, dtype=G.ROW_ENT_DTYPE)  # one guard entry behind the last
                out = np.zeros((max(take, 1), P, 7), dtype=np.uint32)
                r = lib.rows_rest(buf, len(m), pb, sb, P, s.root_type, kinds, head.ctypes.data, take, idx.ctypes.data,
                                  out.ctypes.data)
                assert r >= 0 and idx[take]["len"] == 0x5A, "a store behind the message's entries"
                d |= r << 1
                idx = idx[:take]
                idx["off"] += base  # one message is a batch of its own: into the batch's arena
                idx["msg"] = i
                out = out[:take].astype(np.uint64)
                strs = [k for k, (_, kind) in enumerate(s.columns) if kind == CG.CR.STR or kind & CG.CR.LIST]
                val = out[:, :, 5] | out[:, :, 6] << np.uint64(32)
                for k in strs:
                    val[:, k] += np.where(out[:, k, 0] == R.OK, np.uint64(base), np.uint64(0))
                ents.append(idx)
                cells.append(np.concatenate([out[:, :, :5], val[:, :, None]], axis=2))
            if h["status"] == R.OK:
                head["first"] += base
            heads.append(head)
            deep.append(d)
            base += len(m)
        head = np.concatenate(heads) if heads else np.zeros(0, dtype=G.ROWS_HEAD_DTYPE)
        index = np.concatenate(ents) if ents else np.zeros(0, dtype=G.ROW_ENT_DTYPE)
        cell = np.concatenate(cells) if cells else np.zeros((0, P, 6), dtype=np.uint64)
        counts = head["count"].astype(np.uint64) if cap is None else np.minimum(head["count"], cap).astype(np.uint64)
        got = ({f: head[f] for f in RG.HEAD_FIELDS}, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
               {f: index[f] for f in RG.ROW_FIELDS},
               [dict(zip(("status", "type", "step", "aux", "len", "val"), (cell[:, k, j] for j in range(6)))) for k in range(P)])
        return got, np.array(deep)

    return run


def check(walk, s, what):
    want = RG.expect(s)
    got, deep = walk(s)
    RG.same(got, RG.arrays(want, len(s.columns)), what)
    return want, deep


def test_every_built_set(walk):
    sets = RG.all_sets()
    seen_h, seen_c = set(), set()
    for name, s in sets.items():
        want, _ = check(walk, s, name)
        h, c = RG.statuses(want)
        seen_h |= {st for st, _ in h}
        seen_c |= {st for st, _ in c}
    assert seen_h == {R.OK, R.NOT_FOUND, R.E_READ, CG.CR.E_UNSUPPORTED} and seen_h <= seen_c
    # the values at the width edges come out of the rows as they come out of cols' cells
    want = RG.expect(sets["struct elements"])
    ints = {row[2].val for m in want for row in m.cells if row[2].status == R.OK}
    assert {0x80, 0xFF, 2 ** 64 - 2 ** 15, 2 ** 64 - 2 ** 31, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1} <= ints
    want = RG.expect(sets["lacks the next one's field"])
    col1 = [row[1].status for row in want[0].cells]  # field 2 as INT: a, b, a, c, d, a
    assert col1 == [R.NOT_FOUND, R.OK, R.NOT_FOUND, CG.CR.E_UNSUPPORTED, R.NOT_FOUND, R.NOT_FOUND]


def test_both_deep_passes(walk):
    sets, chains = RG.deep_sets()
    _, deep = check(walk, sets["above"], "above")
    frames = np.array([TG.chain_frames(k, lf, [(R.FIELD, 2)]) for k, lf in chains])
    assert ((deep & 1) == (frames > TG.LDS_FRAMES)).all() and (deep & 1).any() and not (deep & 1).all()
    want, deep = check(walk, sets["inside"], "inside")
    assert (deep & 1).any() and (deep & 2).any() and (deep >> 2).any()  # the head's, the index's and the cells' reruns
    assert any(row[0].status == R.OK and row[0].val == 9 for m in want for row in m.cells)


def test_row_cap_cuts_the_stores(walk):
    s = RG.all_sets()["geometry"]
    want = RG.arrays(RG.expect(s), len(s.columns))
    for cap in (0, 1, 64):
        got, _ = walk(s, cap)
        keep = np.concatenate([np.arange(int(a), int(a) + min(int(b - a), cap)) for a, b in zip(want[1][:-1], want[1][1:])] +
                              [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        CG.same(got[2], {f: want[2][f][keep] for f in RG.ROW_FIELDS}, "cap %d, index" % cap)
        for k, w in enumerate(want[3]):
            CG.same(got[3][k], {f: w[f][keep] for f in CG.CELL_FIELDS}, "cap %d, column %d" % (cap, k))


def test_fuzz_inputs(walk):
    """the first 400 messages of the fuzz corpus and of its mutated form, both plans"""
    msgs, bad = KG.fuzz_messages(400)
    for ms, what in ((msgs, "fuzz"), (bad, "mutated")):
        for name, (parent, cols) in RG.FUZZ_PLANS.items():
            check(walk, RG.Set(ms, parent, cols, R.STRUCT), "%s, %s" % (what, name))


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """rows_host.cpp as a program (-DROWS_MAIN: every message, blob, index array and cell array in an exactly sized
    heap block of its own) over corpus files: the counts and the sum it prints are the checker's."""
    need_hipcc()
    sets = dict(RG.all_sets())
    msgs, bad = KG.fuzz_messages(200)
    for name, (parent, cols) in RG.FUZZ_PLANS.items():
        sets["fuzz " + name] = RG.Set(msgs + bad, parent, cols, R.STRUCT)
    files, hby, cby, rows, cells, total = [], [0] * 5, [0] * 5, 0, 0, 0
    for j, (name, s) in enumerate(sets.items()):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        RG.write_corpus(files[-1], s, *blobs(s))
        for m in s.msgs:  # the program gives every message the arena offset 0
            w = RG.RR.message(m, s.parent, s.columns, s.root_type)
            hby[w.head.status] += 1
            for r, row in zip(w.rows, w.cells):
                rows += 1
                total += r.off + r.len
                for c, (_, kind) in zip(row, s.columns):
                    cells += 1
                    cby[c.status] += 1
                    if kind != CG.CR.STR and not kind & CG.CR.LIST:
                        total += c.val
    exe = build_rows(str(tmp_path / "rowshost"), ("-DROWS_MAIN",))
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    n = sum(len(s.msgs) for s in sets.values())
    want = "%d messages: OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d; %d rows, %d cells: OK %d, " \
        "NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d; sum %d;" % (n, *hby, rows, cells, *cby, total % 2 ** 64)
    assert out.startswith(want), (out, want)
