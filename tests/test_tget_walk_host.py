"""CPU: the path-lookup walk itself (dynamicgo_amd/csrc/tget_device.h, the code
both kernels run) built for the host by tget_walk_host.cpp and compared, record
by record, with the checker (tgetref.py) over the inputs the GPU tests of
test_gpu_tget_deep.py use: chains of every container kind around the 8 LDS
frames and around MaxSkipDepth, the 16-step path, keys around the 16-byte
compare window, integer keys at the edges of their widths, and the fuzz inputs
of test_gpu_tget.py. Every message is followed by 16 bytes of 0xAA."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import t2jgen
import tgetgen as TG
import tgetref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as G
from test_gpu_tget import FUZZ_PATHS, expect, same, share, to_paths

F, I, S, N = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY
HERE = os.path.dirname(os.path.abspath(__file__))


def build_walk(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "tget_walk_host.cpp")],
                   check=True)
    return out


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """walk(msgs, paths, root_type) -> (records as expect() gives them, whether each pair needed the 1024 frames)"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    lib = C.CDLL(build_walk(str(tmp_path_factory.mktemp("walk") / "libtgetwalk.so"), ("-shared",)))
    lib.walk.restype = C.c_int
    lib.walk.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                         C.POINTER(C.c_uint32)]

    def run(msgs, paths, root_type=R.STRUCT):
        blob = G.compile_paths(to_paths(paths))
        off_steps, off_pool = np.frombuffer(blob, dtype="<u4", count=8)[5:7].tolist()
        blob += b"\0" * 16
        rec = np.zeros((len(msgs), len(paths)), dtype=G.REC_DTYPE)
        deep = np.zeros((len(msgs), len(paths)), dtype=bool)
        out = (C.c_uint32 * 6)()
        for i, m in enumerate(msgs):
            buf = m + b"\xAA" * 16
            for k in range(len(paths)):
                deep[i, k] = lib.walk(buf, len(m), blob, off_steps, off_pool, k, root_type, out)
                rec[i, k] = tuple(out)
        return rec, deep

    return run


def test_chains_around_the_lds_frames(walk):
    rng = random.Random(11)
    chains = [TG.random_chain(rng, d) for d in range(13) for _ in range(8)]
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want = expect(msgs, TG.CHAIN_PATHS)
    assert share(want, R.OK) == 0.75 and share(want[:, 3], R.NOT_FOUND) == 1.0
    got, deep = walk(msgs, TG.CHAIN_PATHS)
    same(got, want, "host walk")
    # a pair is deep exactly when its skip opens more than the 8 LDS frames, counted from how the chain is built
    frames = np.array([[TG.chain_frames(k, lf, p) for p in TG.CHAIN_PATHS] for k, lf in chains])
    assert (deep == (frames > TG.LDS_FRAMES)).all()
    assert deep[[len(k) >= 10 for k, _ in chains]].all() and not deep[[len(k) <= 6 for k, _ in chains]].any()


def test_chains_around_max_skip_depth(walk):
    rng = random.Random(12)
    chains = [(k * d, lf) for k in TG.KINDS for d in range(1018, 1027) for lf in TG.LEAVES]
    chains += [TG.random_chain(rng, d) for d in range(1018, 1027) for _ in range(6)]
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    want = TG.deep_checker(lambda: expect(msgs, TG.CHAIN_PATHS))
    assert share(want, R.OK) > 0.25 and share(want, R.E_READ) > 0.25
    got, deep = walk(msgs, TG.CHAIN_PATHS)
    same(got, want, "host walk")
    assert deep.all()


def test_sixteen_steps(walk):
    msgs, paths = TG.sixteen_step_inputs()
    want = expect(msgs, paths)
    assert want[0, 0]["status"] == R.OK and want[0, 0]["type"] == R.LIST and want[1, 0]["type"] == R.LIST
    assert share(want[:2], R.OK) == 1.0 and share(want[2:], R.E_READ) > 0.5
    got, deep = walk(msgs, paths)
    same(got, want, "host walk")
    # what is left to skip after n steps: 16 - n containers and the leaf's frame, 10 more in the long chain
    assert deep[0].tolist() == [17 - len(p) > TG.LDS_FRAMES for p in paths]
    assert deep[1].tolist() == [27 - len(p) > TG.LDS_FRAMES for p in paths] == [True] * 8


def test_long_keys(walk):
    msgs, how = TG.long_key_messages(random.Random(7), 256)
    for ps in TG.long_key_paths():
        want = expect(msgs, ps)
        for col in range(8):
            assert 0.2 < share(want[:, col], R.OK) < 0.8, (col, share(want[:, col], R.OK))
        same(walk(msgs, ps)[0], want, "host walk")
    # the key map as the root
    roots = [m[3:-1] for m in msgs]
    for ps in TG.long_key_paths(prefix=()):
        same(walk(roots, ps, R.MAP)[0], expect(roots, ps, R.MAP), "host walk, map root")
    for v in (TG.EXACT, TG.LAST, TG.LONGER, TG.SHORTER, TG.BYTE8):
        for j, key in enumerate(TG.KEYS):
            if TG.key_variant(key, v) is not None:
                assert any(h[j] == v for h in how), (v, j)


def test_int_key_extremes(walk):
    msgs = TG.int_key_messages(random.Random(8), 256)
    hits = 0
    for ps in TG.int_key_paths():
        want = expect(msgs, ps)
        hits += int((want["status"] == R.OK).sum())
        same(walk(msgs, ps)[0], want, "host walk")
    assert hits > 256 * 21 * 0.4  # 21 keys a message at p = 0.6 (an i8 -128 also answers to 128, -1 to 255)
    # a negative field id, and the ids around it
    m = b"\x08\xff\xfb\0\0\0\x01" + b"\x08\x80\x00\0\0\0\x02" + b"\x08\x00\x05\0\0\0\x03" + b"\0"
    paths = [[(F, -5)], [(F, -32768)], [(F, 5)], [(F, -1)], [(F, 32767)], [(F, 251)]]
    want = expect([m], paths)
    assert want[0]["status"].tolist() == [R.OK] * 3 + [R.NOT_FOUND] * 3 and want[0]["start"].tolist()[:3] == [3, 10, 17]
    same(walk([m], paths)[0], want, "host walk")


def test_fuzz_inputs_and_their_deep_share(walk):
    """The first 600 messages of test_gpu_tget.py's fuzz and mutated sets over
    its 13 paths. The deep counts are why test_gpu_tget_deep.py exists: the
    generator nests too little for the deep pass."""
    rng, mrng = random.Random(1234), random.Random(4321)
    td = t2jgen.all_types_desc()
    msgs = [t2jgen.gen_thrift(rng, td) for _ in range(600)]
    bad = [t2jgen.mutate(mrng, m) for m in msgs]
    paths = list(FUZZ_PATHS.values())
    counts = []
    for ms in (msgs, bad):
        n = 0
        for ps in (paths[:8], paths[8:]):
            got, deep = walk(ms, ps)
            same(got, expect(ms, ps), "host walk")
            n += int(deep.sum())
        counts.append(n)
    assert counts == FUZZ_DEEP, counts


def test_stand_alone_program_reads_a_corpus(tmp_path):
    """tget_walk_host.cpp as a program (-DWALK_MAIN: every message and the blob
    in a heap block of their own, 16 spare bytes each) over a corpus file: the
    status counts it prints are the checker's."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    rng = random.Random(13)
    chains = [TG.random_chain(rng, d) for d in (0, 3, 8, 9, 12, 1022, 1023, 1024) for _ in range(2)]
    msgs = [TG.chain_message(k, lf) for k, lf in chains]
    msgs += [m[:len(m) // 2] for m in msgs[:6]]
    want = TG.deep_checker(lambda: expect(msgs, TG.CHAIN_PATHS))
    TG.write_corpus(str(tmp_path / "corpus.bin"), msgs, G.compile_paths(to_paths(TG.CHAIN_PATHS)))
    exe = build_walk(str(tmp_path / "tgetwalk"), ("-DWALK_MAIN",))
    out = subprocess.run([exe, str(tmp_path / "corpus.bin")], check=True, capture_output=True, text=True).stdout
    frames = [TG.chain_frames(k, lf, p) for k, lf in chains for p in TG.CHAIN_PATHS]
    assert out.startswith("%d pairs, " % want.size) and int(out.split()[2]) >= sum(f > TG.LDS_FRAMES for f in frames)
    assert out.strip().endswith("OK %d, NOT_FOUND %d, E_READ %d, E_TYPE %d" % tuple(
        int((want["status"] == s).sum()) for s in (R.OK, R.NOT_FOUND, R.E_READ, R.E_TYPE))), out


# pairs that need more than the 8 LDS frames, of 600 x 13 = 7 800 each: none of the well-formed messages', 16 of the
# mutated ones' (0.2 %)
FUZZ_DEEP = [0, 16]
