"""CPU: the map head, the map index and the storing sink of the map rows
(dynamicgo_amd/csrc/rows_device.h: rw_map_head_msg, rw_map_index_msg with its
arithmetic route, RWMapStore behind kd_scan: the code the kernels run) built for
the host by mrows_host.cpp and compared, head by head, index entry by index
entry, key by key and key length by key length, with the checker (mrowsref.py)
over all of mrowsgen's inputs, the ones the GPU tests of test_gpu_mrows.py use,
and the fuzz corpus. Every message is followed by 16 bytes of 0xAA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kidsgen as KG
import mrowsgen as MG
import rowsgen as RG
import tgetref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import to_paths

HERE = os.path.dirname(os.path.abspath(__file__))
KEY_FILL = 0x5A5A5A5A5A5A5A5A


def build_mrows(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "mrows_host.cpp")],
                   check=True)
    return out


def need_hipcc():
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)


@pytest.fixture(scope="module")
def mrowslib(tmp_path_factory):
    need_hipcc()
    lib = C.CDLL(build_mrows(str(tmp_path_factory.mktemp("mrows") / "libmrowshost.so"), ("-shared",)))
    common = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.mrows_head.restype = lib.mrows_index.restype = C.c_int
    lib.mrows_head.argtypes = common
    lib.mrows_index.argtypes = common + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def walk(mrowslib):
    """walk(set, row_cap=None, keys=True, lens=True) -> ((head, row_off, index, None, keys) as mrowsgen.arrays gives
    them, deep flags[n]); one guard entry behind every output"""
    lib = mrowslib

    def run(s, cap=None, keys=True, lens=True):
        pb = G.compile_paths(to_paths([s.parent])) + b"\0" * 16
        heads, ents, kvs, kls, deep, base = [], [], [], [], [], 0
        for i, m in enumerate(s.msgs):
            buf = m + b"\xAA" * 16
            head = np.zeros(1, dtype=G.ROWS_HEAD_DTYPE)
            d = lib.mrows_head(buf, len(m), pb, s.root_type, s.keys, head.ctypes.data)
            assert d >= 0
            h = head[0]
            n = int(h["count"])
            take = n if cap is None else min(n, cap)
            if h["status"] == R.OK and n:
                idx = np.full(take + 1, 0x5A, dtype=G.ROW_ENT_DTYPE)
                kv = np.full(take + 1, KEY_FILL, dtype=np.uint64)
                kl = np.full(take + 1, 0x5A5A5A5A, dtype=np.uint32)
                r = lib.mrows_index(buf, len(m), pb, s.root_type, s.keys, head.ctypes.data, take, idx.ctypes.data,
                                    kv.ctypes.data if keys else None, kl.ctypes.data if lens else None)
                assert r >= 0 and idx[take]["len"] == 0x5A and kv[take] == KEY_FILL and kl[take] == 0x5A5A5A5A, \
                    "a store behind the message's entries"
                assert keys or (kv == KEY_FILL).all()
                assert lens or (kl == 0x5A5A5A5A).all()
                d |= r << 1
                idx = idx[:take]
                idx["off"] += base  # one message is a batch of its own: into the batch's arena
                idx["msg"] = i
                ents.append(idx)
                kvs.append(kv[:take] + np.uint64(base if s.keys == MG.STR else 0))
                kls.append(kl[:take])
            if h["status"] == R.OK:
                head["first"] += base
            heads.append(head)
            deep.append(d)
            base += len(m)
        head = np.concatenate(heads) if heads else np.zeros(0, dtype=G.ROWS_HEAD_DTYPE)
        index = np.concatenate(ents) if ents else np.zeros(0, dtype=G.ROW_ENT_DTYPE)
        counts = head["count"].astype(np.uint64) if cap is None else np.minimum(head["count"], cap).astype(np.uint64)
        kd = {}
        if keys:
            kd["key"] = np.concatenate(kvs) if kvs else np.zeros(0, dtype=np.uint64)
        if lens:
            kd["key_len"] = np.concatenate(kls) if kls else np.zeros(0, dtype=np.uint32)
        got = ({f: head[f] for f in RG.HEAD_FIELDS}, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64),
               {f: index[f] for f in RG.ROW_FIELDS}, None, kd)
        return got, np.array(deep)

    return run


def check(walk, s, what, **kw):
    want = MG.expect(s)
    got, deep = walk(s, **kw)
    MG.same(got, MG.arrays(want, len(s.columns)), what)
    return want, deep


def test_every_built_set(walk):
    seen = set()
    for name, s in MG.all_sets().items():
        want, _ = check(walk, s, name)
        seen |= {st for st, _ in MG.statuses(want)[0]}
    assert seen == {R.OK, R.NOT_FOUND, R.E_READ, MG.MR.E_UNSUPPORTED}
    # the keys at the width edges, as ReadInt gives them: a byte unsigned, the others sign-extended
    want = MG.expect(MG.all_sets()["int key edges"])
    assert [k.val for k in want[0].keys] == [0x00, 0x7F, 0x80, 0xFF] and {k.len for k in want[0].keys} == {1}
    assert want[1].keys[0] == MG.MR.Key(2 ** 64 - 1, 2) and want[3].keys[0] == MG.MR.Key(2 ** 63, 8)
    assert want[3].keys[1] == MG.MR.Key(2 ** 63 - 1, 8)
    assert [k.val for k in want[8].keys] == [3, 3, 3, 4, 3]  # duplicate keys are kept, in wire order


def test_the_arithmetic_route_and_the_walk_agree(walk):
    """map<i32, i64> takes the arithmetic route, the same data under string keys walks: the same value spans (moved
    by the keys' length prefixes) and, as the payload, the same key bytes"""
    sets = MG.all_sets()
    a, _ = check(walk, sets["fixed maps"], "fixed")
    b, _ = check(walk, sets["fixed maps' data, string keys"], "walked")
    assert [m.head.count for m in a] == [m.head.count for m in b] and sum(m.head.count for m in a) > 400
    arena_a, arena_b = (b"".join(sets[k].msgs) for k in ("fixed maps", "fixed maps' data, string keys"))
    for ma, mb in zip(a, b):
        for ka, kb, ra, rb in zip(ma.keys, mb.keys, ma.rows, mb.rows):
            assert (ka.len, kb.len, ra.len, rb.len) == (4, 4, 8, 8)
            assert int.from_bytes(arena_b[kb.val:kb.val + 4], "big", signed=True) % 2 ** 64 == ka.val
            assert arena_a[ra.off:ra.off + 8] == arena_b[rb.off:rb.off + 8]


def test_deep_head_and_index(walk):
    sets, chains = MG.deep_sets()
    for name, s in sets.items():
        _, deep = check(walk, s, name)
        assert (deep & 1).any() and (deep & 2).any() and not (deep & 1).all()


def test_row_cap_and_null_keys(walk):
    for name in ("geometry, str keys", "fixed maps"):
        s = MG.all_sets()[name]
        want = MG.arrays(MG.expect(s), len(s.columns))
        for cap in (0, 1, 64):
            for keys, lens in ((True, True), (False, True), (True, False), (False, False)):
                got, _ = walk(s, cap, keys, lens)
                keep = np.concatenate([np.arange(int(a), int(a) + min(int(b - a), cap))
                                       for a, b in zip(want[1][:-1], want[1][1:])] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
                MG.CG.same(got[2], {f: want[2][f][keep] for f in RG.ROW_FIELDS}, "%s, cap %d, index" % (name, cap))
                MG.CG.same(got[4], {f: want[4][f][keep] for f in got[4]}, "%s, cap %d, keys" % (name, cap))


def test_fuzz_inputs(walk):
    """the first 400 messages of the fuzz corpus and of its mutated form, every plan"""
    msgs, bad = KG.fuzz_messages(400)
    for ms, what in ((msgs, "fuzz"), (bad, "mutated")):
        for name, (parent, cols, kind) in MG.FUZZ_PLANS.items():
            check(walk, MG.Set(ms, parent, cols, R.STRUCT, kind), "%s, %s" % (what, name))


def corpus_files(tmp_path):
    """the corpus files of the stand-alone program and the line the checker expects of it"""
    sets = dict(MG.all_sets())
    msgs, bad = KG.fuzz_messages(200)
    for name, (parent, cols, kind) in MG.FUZZ_PLANS.items():
        sets["fuzz " + name] = MG.Set(msgs + bad, parent, cols, R.STRUCT, kind)
    files, hby, rows, total = [], [0] * 5, 0, 0
    for j, (name, s) in enumerate(sets.items()):
        files.append(str(tmp_path / ("corpus%d.bin" % j)))
        MG.write_corpus(files[-1], s, G.compile_paths(to_paths([s.parent])))
        for m in s.msgs:  # the program gives every message the arena offset 0
            h, rws, keys, _ = MG.MR.head_rows(m, s.parent, s.keys, s.root_type)
            hby[h.status] += 1
            rows += len(rws)
            total += sum(r.off + r.len + k.val + k.len for r, k in zip(rws, keys))
    n = sum(len(s.msgs) for s in sets.values())
    want = "%d messages: OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d; %d rows; sum %d;" % (
        n, *hby, rows, total % 2 ** 64)
    return files, want


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """mrows_host.cpp as a program (-DMROWS_MAIN: every message, blob, head, index array, key array and key-length
    array in an exactly sized heap block of its own) over corpus files: the counts and the sum it prints are the
    checker's."""
    need_hipcc()
    files, want = corpus_files(tmp_path)
    exe = build_mrows(str(tmp_path / "mrowshost"), ("-DMROWS_MAIN",))
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    assert out.startswith(want), (out, want)
