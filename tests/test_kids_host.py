"""CPU: the Children walk itself (dynamicgo_amd/csrc/kids_device.h, the code
the count, emit and deep kernels run) built for the host by kids_host.cpp and
compared, head by head and record by record, with the checker (kidsref.py) over
the inputs the GPU tests of test_gpu_kids.py use; the checker against the
reference's own assertion on example2; a sanitizer run of the same file as a
stand-alone program; and the refusals of dg_kids_* that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kidsgen as KG
import kidsref as K
import tgetgen as TG
import tgetref as R
from conftest import GOLDEN
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import to_paths

HERE = os.path.dirname(os.path.abspath(__file__))
F = R.FIELD


def build_host(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "kids_host.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """walk(msgs, path, recurse, root_type) -> ((head, rec_off, recs), whether each message needed the 1024 levels)"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    lib = C.CDLL(build_host(str(tmp_path_factory.mktemp("kids") / "libkidshost.so"), ("-shared",)))
    u32, vp = C.c_uint32, C.c_void_p
    lib.kids_count.restype = lib.kids_emit.restype = C.c_int
    lib.kids_count.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, u32, u32, u32, u32, u32, vp]
    lib.kids_emit.argtypes = [C.c_char_p, C.c_uint64, u32, u32, vp, vp]

    def run(msgs, path, recurse, root_type=R.STRUCT):
        blob = G.compile_paths(to_paths([path]))
        off_steps, off_pool = np.frombuffer(blob, dtype="<u4", count=8)[5:7].tolist()
        blob += b"\0" * 16
        n = len(msgs)
        head = np.zeros(n, dtype=G.KIDS_HEAD_DTYPE)
        deep = np.zeros(n, dtype=bool)
        bufs = [m + b"\xAA" * 16 for m in msgs]
        for i, m in enumerate(msgs):
            d = lib.kids_count(bufs[i], len(m), blob, off_steps, off_pool, len(path), root_type, recurse, head[i:].ctypes.data)
            assert d >= 0
            deep[i] = d
        rec_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(head["count"], out=rec_off[1:])
        recs = np.frombuffer(bytearray(b"\xA5" * (32 * (int(rec_off[n]) + 1))), dtype=G.KIDS_REC_DTYPE)
        for i, m in enumerate(msgs):
            if head[i]["status"] == R.OK and head[i]["count"]:
                d = lib.kids_emit(bufs[i], len(m), len(path), recurse, head[i:].ctypes.data, recs[int(rec_off[i]):].ctypes.data)
                assert d == deep[i]  # both passes run the same walk
        assert recs[-1:].tobytes() == b"\xA5" * 32  # the guard record
        return (head, rec_off, recs[:-1]), deep

    return run


def test_checker_against_the_reference_assertion():
    """thrift/generic/path_test.go:51: example2 at the root has exactly 4 children"""
    with open(os.path.join(GOLDEN, "example2.bin"), "rb") as fh:
        m = fh.read()
    h, kids = K.children(m)
    assert h.status == R.OK and h.count == h.direct == 4 and h.type == R.STRUCT
    assert [(k.key, k.type) for k in kids] == [(32767, R.DOUBLE), (1, R.STRING), (3, R.STRUCT), (255, R.STRUCT)]
    assert all(k.kind == F and k.parent == K.NO_PARENT and k.depth == 1 and k.key_start == k.start - 3 for k in kids)
    assert kids[0].start == 3 and kids[-1].end == len(m) - 1 and [a.end + 3 for a in kids[:-1]] == [b.start for b in kids[1:]]
    h, deep = K.children(m, recurse=True)
    assert h.status == R.OK and h.direct == 4 and [k for k in deep if k.depth == 1] == [
        a._replace(n_desc=b.n_desc) for a, b in zip(kids, [k for k in deep if k.depth == 1])]
    assert h.count == len(deep) == 4 + sum(k.n_desc for k in deep if k.depth == 1)
    for idx, k in enumerate(deep):  # the tree the records describe: preorder, parents before children, spans nested
        if k.parent != K.NO_PARENT:
            p = deep[k.parent]
            assert k.parent < idx <= k.parent + p.n_desc and p.start <= k.start and k.end <= p.end and k.depth == p.depth + 1
    # a cross-check, not a pin: a restatement written apart from this one gave 134 records, 6 levels
    print("example2 recursive: %d records, depth %d" % (len(deep), max(k.depth for k in deep)))


def test_example2_host_walk(walk):
    with open(os.path.join(GOLDEN, "example2.bin"), "rb") as fh:
        m = fh.read()
    for path in ([], [(F, 3)], [(F, 255)], [(F, 1)]):
        for rec in (False, True):
            KG.same(walk([m], path, rec)[0], KG.expect([m], path, rec), "host walk %s %s" % (path, rec))


def test_fuzz(walk):
    """the first 512 messages of the GPU fuzz and their mutated versions over its 14 paths, both modes"""
    good, bad = KG.fuzz_messages(512)
    need_deep = []
    for name, path in KG.FUZZ_PATHS.items():
        for rec in (False, True):
            for ms, what in ((good, "good"), (bad, "mutated")):
                want = KG.expect(ms, path, rec)
                got, deep = walk(ms, path, rec)
                KG.same(got, want, "host walk %s %s %s" % (name, rec, what))
                need_deep.append(int(deep.sum()))
                if name == "" and what == "good":
                    assert KG.share(want[0], R.OK) == 1.0
                if name in KG.CONTAINER_PATHS and what == "mutated":
                    assert KG.share(want[0], R.OK) >= 0.20 and KG.share(want[0], R.E_READ) >= 0.40, (name, rec)
    print("messages that needed the 1024 levels, per (path, mode, set):", need_deep)


def test_hand_built(walk):
    hand = KG.hand_messages()
    msgs = list(hand.values())
    for path in ([(F, 1)], []):
        for rec in (False, True):
            want = KG.expect(msgs, path, rec)
            KG.same(walk(msgs, path, rec)[0], want, "host walk %s %s" % (path, rec))
    st = dict(zip(hand, KG.expect(msgs, [(F, 1)], False)[0]["status"].tolist()))
    # the headers only ReadListBegin / ReadMapBegin refuse, and the scalars
    assert st["list<type 5> of 0"] == st["map<type 5, i32> of 0"] == st["map<i32, type 9> of 0"] == R.E_READ
    assert st["list of -1"] == st["map of -1"] == st["field type 18"] == st["short string"] == R.E_READ
    assert st["i32"] == st["string"] == K.UNSUPPORTED and st["empty struct"] == st["empty list"] == st["empty map"] == R.OK
    # fine one level deep, ErrRead in recursive mode
    one = dict(zip(hand, KG.expect(msgs, [(F, 1)], False)[0]["status"].tolist()))
    rec = dict(zip(hand, KG.expect(msgs, [(F, 1)], True)[0]["status"].tolist()))
    for k in ("list<list<type 5> of 0>", "struct{list<type 7> of 0}"):
        assert one[k] == R.OK and rec[k] == R.E_READ
    # an I08 key is unsigned; keys at the extremes; BINKEY spans
    h, kids = K.children(hand["map<i08,i32>"], [(F, 1)])
    assert [k.key for k in kids] == [128, 255, 127] and all(k.kind == R.INTKEY for k in kids)
    h, kids = K.children(hand["map<i64,string>"], [(F, 1)])
    assert [k.key for k in kids] == [-2 ** 63, 2 ** 63 - 1, -1, 2 ** 32]
    h, kids = K.children(hand["map<list,list>"], [(F, 1)], True)
    assert [k.kind for k in kids if k.depth == 1] == [R.BINKEY] * 2 and h.count == 3  # keys are not descended into
    assert K.key_bytes(hand["map<list,list>"], kids[0]) == b"\x06\0\0\0\x02\0\1\0\2"  # the list<i16> key as it stands
    h, kids = K.children(hand["map<string,i32>"], [(F, 1)])
    assert [k.key for k in kids] == [0, 1, 300] and K.key_bytes(hand["map<string,i32>"], kids[1]) == b"k"


def test_every_prefix(walk):
    m = KG.every_kind_message()
    assert 70 <= len(m) <= 110
    msgs = KG.prefixes(m)
    for path in ([], [(F, 1)], [(F, 3)]):
        for rec in (False, True):
            want = KG.expect(msgs, path, rec)
            KG.same(walk(msgs, path, rec)[0], want, "host walk %s %s" % (path, rec))
    h, kids = K.children(m, [], True)
    assert h.status == R.OK and h.direct == 5 and {k.kind for k in kids} == {R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY}
    assert max(k.depth for k in kids) == 3


def test_chains_around_the_lds_levels(walk):
    chains = KG.lds_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    seen = set()
    for path in KG.CHAIN_PATHS:
        for rec in (False, True):
            got, deep = walk(msgs, path, rec)
            KG.same(got, KG.expect(msgs, path, rec), "host walk %s %s" % (path, rec))
            seen.add(bool(deep.any()) and not bool(deep.all()))
            # depth 6 fits whatever the kind, depth 10 never does
            assert not deep[[len(k) == 6 and lf == "i" for k, lf in chains]].any()
            assert deep[[len(k) == 10 and lf == "e" for k, lf in chains]].all()
    assert seen == {True}


def test_chains_around_max_skip_depth(walk):
    """The limit is the outermost skip's. Under path f1 it is GetByPath's skip
    of the node: 1023 levels including the node. Under the empty path it is each
    direct child's: 1023 levels below the node. So the same container flips
    between OK and ErrRead one level later when it is the root of the empty
    path than when path f1 leads to it; the message's root struct over it
    (the empty path on the whole message) flips where f1 does."""
    chains = KG.limit_chains()
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    last_ok = {}
    for what, ms, path in (("root struct", msgs, []), ("f1", msgs, [(F, 1)]), ("as root", [m[3:-8] for m in msgs], [])):
        status = []
        for kind in TG.KINDS:  # a chain's own top as the root: its wire type is the message's first byte
            sel = [i for i, (k, _) in enumerate(chains) if k[0] == kind]
            sub, rt = [ms[i] for i in sel], msgs[sel[0]][0] if what == "as root" else R.STRUCT
            want = TG.deep_checker(lambda: KG.expect(sub, path, False, rt))
            got, deep = walk(sub, path, False, rt)
            KG.same(got, want, "host walk %s %s" % (what, kind))
            assert deep.all()
            st = want[0]["status"].tolist()
            ok = [d for d, s_ in zip(range(1018, 1028), st) if s_ == R.OK]
            assert ok == list(range(1018, ok[-1] + 1)) and set(st) == {R.OK, R.E_READ}, (what, kind, st)
            last_ok[what, kind] = ok[-1]
            status += st
    for kind in TG.KINDS:
        assert last_ok["as root", kind] == last_ok["f1", kind] + 1 == last_ok["root struct", kind] + 1, (kind, last_ok)
    assert last_ok["f1", "S"] == 1023
    # recursive mode: the same verdicts from ONE walk, next to the limit (the checker is quadratic there)
    rchains = KG.limit_chains_recursive()
    rmsgs = [TG.chain_message(k, lf) for k, lf in rchains]
    for path in KG.CHAIN_PATHS:
        want = TG.deep_checker(lambda: KG.expect(rmsgs, path, True))
        assert [s_ == R.OK for s_ in want[0]["status"].tolist()] == [len(k) <= last_ok["f1", k[0]] for k, _ in rchains]
        got, deep = walk(rmsgs, path, True)
        KG.same(got, want, "host walk, recursive %s" % path)
        assert deep.all()


def test_wide_nodes(walk):
    wide = KG.wide_messages()
    msgs = list(wide.values())
    for rec in (False, True):
        want = KG.expect(msgs, [(F, 1)], rec)
        KG.same(walk(msgs, [(F, 1)], rec)[0], want, "host walk")
    cut = [k.endswith("cut") for k in wide]
    assert (want[0]["status"][cut] == R.E_READ).all() and (want[0]["status"][~np.array(cut)] == R.OK).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """kids_host.cpp as a program (-DKIDS_MAIN) built with the address and
    undefined-behaviour sanitizers: every message and the blob in a heap block
    of their own with 16 spare bytes, the heads and the record array in blocks
    of exactly their size. The counts it prints are the checker's."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    exe = build_host(str(tmp_path / "kids"), ("-DKIDS_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                               "-fno-sanitize-recover=undefined"))
    good, bad = KG.fuzz_messages(96)
    m = KG.every_kind_message()
    chains = [TG.chain_message(k * d, "e") for k in "SLM" for d in (7, 9, 12)] + \
             [TG.chain_message(k * d, "i") for k in "SK" for d in (1022, 1024)]
    sets = [(good + bad, []), (good + bad, [(F, 10)]), (good + bad, [(F, 17), (F, 3)]), (bad, [(F, 18)]),
            (list(KG.hand_messages().values()), [(F, 1)]), (KG.prefixes(m), []), (list(KG.wide_messages().values()), [(F, 1)])]
    files, n_msgs, total, by = [], 0, 0, [0] * 5
    for k, (msgs, path) in enumerate(sets + [(chains, []), (chains, [(F, 1)])]):
        files.append(str(tmp_path / ("corpus%d.bin" % k)))
        TG.write_corpus(files[-1], msgs, G.compile_paths(to_paths([path])))
        for rec in (False, True):
            want = TG.deep_checker(lambda: KG.expect(msgs, path, rec))
            n_msgs += len(msgs)
            total += int(want[1][-1])
            for s in range(5):
                by[s] += int((want[0]["status"] == s).sum())
    out = subprocess.run([exe] + files, check=True, capture_output=True, text=True).stdout
    assert out.startswith("%d messages, " % n_msgs) and int(out.split()[2]) > 0, out
    assert ", %d records; OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d, E_UNSUPPORTED %d" % (total, *by) in out, out


def test_refusals_without_a_device():
    """dg_kids_* judge the handles before anything touches a device"""
    from dynamicgo_amd import _lib
    L = _lib.lib()
    need = C.c_uint64(7)
    assert L.dg_kids_batch_host(None, None, R.STRUCT, 0, None, None, 0, None, None, None, 0, C.byref(need)) == -1
    assert L.dg_kids_batch_device(None, None, R.STRUCT, 0, None, None, 0, None, None, None, 0, None, 0) == -1
    assert b"null ctx/path" in L.dg_last_error()
