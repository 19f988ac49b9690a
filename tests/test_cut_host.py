"""CPU: the cut (batched MarshalTo). The plan compiler (generic.compile_cut):
its layout, memoisation on recursive descriptors and what it refuses. The
checker (cutref.py) on messages answered by hand. And the walk itself
(dynamicgo_amd/csrc/cut_device.h: the code both kernels run, with both frame
stores and both copy engines) built for the host by cut_walk_host.cpp and
compared with the checker, message by message, over the inputs the GPU tests of
test_gpu_cut.py use; the same file as a stand-alone program under
AddressSanitizer and UBSan over a corpus file."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import cutgen as G
import cutref as R
from dynamicgo_amd import build as B
from dynamicgo_amd import generic as X
from dynamicgo_amd import thrift as T
from dynamicgo_amd.http import ConvError

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ the plan
def parse(blob):
    h = struct.unpack("<16I", blob[:64])
    magic, version, total, root, n_nodes, off_nodes, n_fields, off_fields, n_lits, off_lits, off_pool, pool_len, U = h[:13]
    nodes = [struct.unpack_from("<6I2Q", blob, off_nodes + 40 * k) for k in range(n_nodes)]
    fields = [struct.unpack_from("<hBBI", blob, off_fields + 8 * k) for k in range(n_fields)]
    lits = [struct.unpack_from("<hHI", blob, off_lits + 8 * k) for k in range(n_lits)]
    return dict(magic=magic, version=version, total=total, root=root, nodes=nodes, fields=fields, lits=lits,
                pool=blob[off_pool:off_pool + pool_len], U=U, offs=(off_nodes, off_fields, off_lits, off_pool))


def test_plan_layout():
    wide, narrow = G.pair()
    blob = X.compile_cut(wide, narrow)
    p = parse(blob)
    assert p["magic"] == 0x31434744 and p["version"] == 1 and p["total"] == len(blob)
    assert p["offs"][0] == 64 and all(o % 8 == 0 for o in p["offs"]) and p["offs"][3] + len(p["pool"]) == len(blob)
    kind, f0, _, nf, lit0, nl, tracked, required = p["nodes"][p["root"]]
    assert kind == X.CUT_STRUCT and nf == len(wide.struct.fields)
    fl = p["fields"][f0:f0 + nf]
    assert [f[0] for f in fl] == sorted(f.id for f in wide.struct.fields)
    by_id = {f[0]: f for f in fl}
    # dropped: the five fields narrow lacks; their wire types are wide's
    assert [i for i in by_id if by_id[i][3] == X.CUT_DROP] == [1, 2, 3, 4, 5]
    assert [by_id[i][1] for i in (1, 2, 3, 4, 5)] == [8, 11, 12, 15, 13]
    # tracked fields of narrow, ascending: 11 (required), 12, 16, 17, 20, 21 (default); bit k = lit k
    ids = [l[0] for l in p["lits"][lit0:lit0 + nl]]
    assert ids == [11, 12, 16, 17, 20, 21] and tracked == 0x3F and required == 1
    assert [by_id[i][2] for i in (11, 12, 16, 17, 20)] == [0, 1, 2, 3, 4] and by_id[13][2] == X.CUT_NO_BIT
    lit = {l[0]: p["pool"][l[2]:l[2] + l[1]] for l in p["lits"][lit0:lit0 + nl]}
    assert lit[11] == b"" and lit[12] == b"\x0f\x00\x0c\x0b\0\0\0\0" and lit[16] == b"\x0d\x00\x10\x0b\x08\0\0\0\0"
    assert lit[17] == b"\x0c\x00\x11\x00" and lit[20] == b"\x04\x00\x14" + b"\0" * 8 and lit[21] == b"\x02\x00\x15\x00"
    assert p["U"] == sum(len(v) for v in lit.values())  # the root has the largest literal total
    # the children: the same-object list is a whole copy, the others are cut
    kinds = {i: p["nodes"][by_id[i][3]] for i in by_id if by_id[i][3] != X.CUT_DROP}
    assert kinds[10][:2] == (X.CUT_COPY, 15) and kinds[19][:2] == (X.CUT_COPY, 14) and kinds[18][:2] == (X.CUT_COPY, 11)
    assert kinds[7][0] == X.CUT_LIST and kinds[8][0] == X.CUT_MAP and kinds[9][0] == X.CUT_MAP and kinds[6][0] == X.CUT_STRUCT
    assert p["nodes"][kinds[8][1]][:2] == (X.CUT_COPY, 11) and p["nodes"][kinds[8][2]][0] == X.CUT_STRUCT
    assert p["nodes"][kinds[9][1]][0] == X.CUT_STRUCT and p["nodes"][kinds[9][2]][:2] == (X.CUT_COPY, 8)
    # Mid.differ: i32 against string
    mid = kinds[6]
    differ = [f for f in p["fields"][mid[1]:mid[1] + mid[3]] if f[0] == 4][0]
    assert differ[1] == 8 and p["nodes"][differ[3]][0] == X.CUT_MISMATCH


def test_plan_memoises_recursive_descriptors():
    node, node_n = G.node_pair()
    p = parse(X.compile_cut(node, node_n))
    # (Node, NodeN), its i32, its list: three nodes, and both `next` and the list's element lead back to the first
    assert len(p["nodes"]) == 3 and p["root"] == 0
    kind, f0, _, nf = p["nodes"][0][:4]
    fl = {f[0]: f for f in p["fields"][f0:f0 + nf]}
    assert fl[2][3] == 0 and p["nodes"][fl[3][3]][:2] == (X.CUT_LIST, 0) and fl[4][3] == X.CUT_DROP
    assert X.compile_cut(node, node_n) == X.compile_cut(node, node_n)


def test_same_descriptor_rule():
    assert X.same_descriptor(T.builtin("i32"), T.builtin("i32"))
    assert not X.same_descriptor(T.builtin("string"), T.builtin("binary"))  # equal type, another name
    l = T.list_of(T.builtin("i32"))
    assert X.same_descriptor(l, l) and not X.same_descriptor(l, T.list_of(T.builtin("i32")))
    # a list of a fresh list of i32: not the same object, no base type: cut entry by entry
    a, b_ = T.list_of(T.list_of(T.builtin("i32"))), T.list_of(T.list_of(T.builtin("i32")))
    p = parse(X.compile_cut(a, b_))
    assert p["nodes"][0][:2] == (X.CUT_LIST, 1) and p["nodes"][1][:2] == (X.CUT_COPY, 15)
    # list against set with the same element: skip_val's type test
    p = parse(X.compile_cut(T.struct_type("A", [G.F(1, "l", T.list_of(T.builtin("i32")))]),
                            T.struct_type("B", [G.F(1, "l", T.set_of(T.builtin("i32")))])))
    assert [n[0] for n in p["nodes"]] == [X.CUT_STRUCT, X.CUT_MISMATCH]


def test_what_the_compiler_refuses():
    wide, narrow = G.pair()
    with pytest.raises(ValueError, match="same struct"):
        X.compile_cut(wide, wide)
    inner = T.struct_type("I", [G.F(1, "x", T.builtin("i32"))])
    with pytest.raises(ValueError, match="same struct"):  # below the root
        X.compile_cut(T.struct_type("A", [G.F(1, "i", inner)]), T.struct_type("B", [G.F(1, "i", inner)]))
    with pytest.raises(ValueError, match="none in the from"):
        X.compile_cut(T.struct_type("A", [G.F(1, "i", T.builtin("i32"))]), T.struct_type("B", [G.F(1, "i", inner)]))
    with pytest.raises(ConvError) as e:
        X.compile_cut(wide, T.list_of(narrow))
    assert e.value.behavior == "ErrDismatchType"
    many = [G.F(i + 1, "f%d" % i, T.builtin("i32"), T.DEFAULT) for i in range(65)]
    with pytest.raises(ValueError, match="65 tracked"):
        X.compile_cut(T.struct_type("A", many), T.struct_type("B", many))
    X.compile_cut(T.struct_type("A", many[:64]), T.struct_type("B", many[:64]))
    X.compile_cut(T.struct_type("A", many), T.struct_type("B", many[:1] + [G.F(f.id, f.name, f.type) for f in many[1:]]))
    with pytest.raises(ValueError, match="negative"):
        X.compile_cut(T.struct_type("A", []), T.struct_type("B", [G.F(-1, "n", T.builtin("i32"), T.DEFAULT)]))


# ------------------------------------------------------- the checker by hand
REQ_S = b"\x0b\x00\x0b\x00\x00\x00\x01r"


def test_checker_known_answers():
    wide, narrow = G.pair()
    cut = lambda m, o=0: R.marshal_to(m, wide, narrow, o)
    # s_drop (i32) dropped, req_s and opt_i kept
    m = b"\x08\x00\x01\x00\x00\x00\x05" + REQ_S + b"\x0a\x00\x0d" + b"\x11" * 8 + b"\x00"
    assert cut(m) == (0, REQ_S + b"\x0a\x00\x0d" + b"\x11" * 8 + b"\x00")
    # every status
    assert cut(b"") == (R.E_READ, b"") and cut(REQ_S) == (R.E_READ, b"") and cut(b"\x05\x00\x01") == (R.E_READ, b"")
    assert cut(b"\x00") == (R.E_REQUIRED | 11 << 32, b"")
    assert cut(b"\x00", R.NOT_CHECK_REQ) == (0, b"\x00")
    assert cut(b"\x0b\x00\x01\x00\x00\x00\x00" + REQ_S + b"\x00") == (R.E_TYPE | 1 << 32, b"")  # s_drop as a string
    unknown = b"\x08\x03\xe8\x00\x00\x00\x01" + REQ_S + b"\x00"
    assert cut(unknown) == (0, REQ_S + b"\x00") and cut(unknown, R.DISALLOW_UNKNOWN) == (R.E_UNKNOWN | 1000 << 32, b"")
    neg = b"\x08\xff\xfb\x00\x00\x00\x01" + REQ_S + b"\x00"
    assert cut(neg, R.DISALLOW_UNKNOWN) == (R.E_UNKNOWN | 0xFFFFFFFB << 32, b"")
    # Mid.differ: i32 in from, string in to -> the pair's own ErrDismatchType, no field id
    differ = REQ_S + b"\x0c\x00\x06" + b"\x08\x00\x04\x00\x00\x00\x01" + b"\x00" + b"\x00"
    assert cut(differ) == (R.E_TYPE, b"")
    # the required field of an inner struct: Leaf.a missing in leaves[0]
    assert cut(REQ_S + b"\x0f\x00\x07\x0c\x00\x00\x00\x01" + b"\x00" + b"\x00") == (R.E_REQUIRED | 1 << 32, b"")
    # a chain of Nodes one deeper than the frames
    node, node_n = G.node_pair()
    assert R.marshal_to(G.chain_message("S" * 63), node, node_n)[0] == 0
    assert R.marshal_to(G.chain_message("S" * 64), node, node_n) == (R.E_DEPTH, b"")


def test_checker_write_default_byte_by_byte():
    wide, narrow = G.pair()
    # req_s; mid = {leaf = {a = 1}, name = "x" (dropped)}; leaves = [{a = 2, d = 3 (dropped)}]
    leaf1 = b"\x0a\x00\x01" + b"\0" * 7 + b"\x01"
    leaf2 = b"\x0a\x00\x01" + b"\0" * 7 + b"\x02" + b"\x08\x00\x04\x00\x00\x00\x03"
    m = (REQ_S + b"\x0c\x00\x06" + b"\x0c\x00\x01" + leaf1 + b"\x00" + b"\x0b\x00\x02\x00\x00\x00\x01x" + b"\x00" +
         b"\x0f\x00\x07\x0c\x00\x00\x00\x01" + leaf2 + b"\x00" + b"\x00")
    leaf_unset = b"\x0b\x00\x02\x00\x00\x00\x00" + b"\x06\x00\x05\x00\x00"  # b = "", e = 0
    want = (REQ_S + b"\x0c\x00\x06" + b"\x0c\x00\x01" + leaf1 + leaf_unset + b"\x00" + b"\x00" +
            b"\x0f\x00\x07\x0c\x00\x00\x00\x01" + b"\x0a\x00\x01" + b"\0" * 7 + b"\x02" + leaf_unset + b"\x00" +
            b"\x0f\x00\x0c\x0b\x00\x00\x00\x00" +      # def_l: an empty list of strings
            b"\x0d\x00\x10\x0b\x08\x00\x00\x00\x00" +  # def_m: an empty map<string, i32>
            b"\x0c\x00\x11\x00" +                      # def_st: a lone STOP
            b"\x04\x00\x14" + b"\0" * 8 +              # dbl
            b"\x02\x00\x15\x00" +                      # only_to
            b"\x00")
    assert R.marshal_to(m, wide, narrow, R.WRITE_DEFAULT) == (0, want)
    plain = (REQ_S + b"\x0c\x00\x06" + b"\x0c\x00\x01" + leaf1 + b"\x00" + b"\x00" +
             b"\x0f\x00\x07\x0c\x00\x00\x00\x01" + b"\x0a\x00\x01" + b"\0" * 7 + b"\x02" + b"\x00" + b"\x00")
    assert R.marshal_to(m, wide, narrow, 0) == (0, plain)
    assert R.marshal_to(m, wide, narrow, R.WRITE_DEFAULT | R.NOT_CHECK_REQ) == (0, plain)


def test_fuzz_corpus_is_worth_running():
    """what test_gpu_cut.py's fuzz asserts of its corpus, from the checker alone"""
    wide, narrow = G.pair()
    msgs, bad = G.fuzz()
    assert sum(r == 0 for r, _ in G.expect(msgs, wide, narrow)) * 2 >= len(msgs)
    seen = set()
    for o in G.ALL_OPTS:
        seen |= {r & 0xFF for r, _ in G.expect(msgs + bad, wide, narrow, o)}
    assert seen == {R.OK, R.E_READ, R.E_TYPE, R.E_UNKNOWN, R.E_REQUIRED}


# ---------------------------------------------------------- the walk, on the host
def build_walk(out, extra=()):
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", *extra, "-o", out, os.path.join(HERE, "cut_walk_host.cpp")],
                   check=True)
    return out


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """walk(msgs, blob, opts, route, caps=None, wave_min=1 << 20) -> ([(ret, out)], [declined])"""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    lib = C.CDLL(build_walk(str(tmp_path_factory.mktemp("cutwalk") / "libcutwalk.so"), ("-shared",)))
    lib.cut_msg.restype = C.c_int
    lib.cut_msg.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.c_char_p, C.c_uint64,
                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

    def run(msgs, blob, opts, route, caps=None, wave_min=1 << 20):
        blob = blob + b"\0" * 16
        res, declined = [], []
        ret, ol = C.c_uint64(0), C.c_uint32(0)
        for i, m in enumerate(msgs):
            cap = caps[i] if caps is not None else 12 * len(m) + 64
            out = C.create_string_buffer(b"\xEE" * (cap + 32), cap + 32)
            declined.append(lib.cut_msg(m + b"\xAA" * 16, len(m), blob, opts, route, wave_min,
                                        C.cast(C.byref(out, 16), C.c_char_p), cap, C.byref(ret), C.byref(ol)))
            raw = out.raw
            assert raw[:16] == b"\xEE" * 16 and raw[16 + cap:] == b"\xEE" * 16, "a store outside the slot"
            if ret.value == 0:
                assert raw[16 + ol.value:16 + cap] == b"\xEE" * (cap - ol.value), "a store beyond out_len"
            res.append((ret.value, raw[16:16 + ol.value] if ret.value == 0 else b""))
            if ret.value & 0xFF == R.E_OVERFLOW:
                assert ol.value == ret.value >> 32
            elif ret.value:
                assert ol.value == 0
        return res, declined

    return run


def both(walk, msgs, frm, to, opts=0):
    blob = X.compile_cut(frm, to)
    want = G.expect(msgs, frm, to, opts)
    for route in (1, 0):  # `declined` is the lane route's
        got, declined = walk(msgs, blob, opts, route)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "route %d, message %d (%r...): got %x / %d bytes, checker %x / %d" % (
                route, i, msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))
    return want, declined


def test_walk_fuzz(walk):
    wide, narrow = G.pair()
    msgs, bad = G.fuzz()
    for o in G.ALL_OPTS:
        both(walk, msgs + bad, wide, narrow, o)


def family_on_both_routes(walk, fam, opts_words=G.ALL_OPTS):
    unset = parse(fam.blob())["U"]  # dg_cut_slot_bound: a message of one STOP can grow by every literal
    caps = [len(m) * (1 + unset) + 64 for m in fam.msgs]
    for o in opts_words:
        for route in (1, 0):
            got, _ = walk(fam.msgs, fam.blob(), o, route, caps=caps)
            for i, (g, w) in enumerate(zip(got, fam.want(o))):
                assert g == w, "%s, opts %d, route %d, message %d (%r...): got %x / %d bytes, checker %x / %d" % (
                    fam.name, o, route, i, fam.msgs[i][:24], g[0], len(g[1]), w[0], len(w[1]))


def test_wide_corpus_is_worth_running():
    """what test_gpu_cut_shapes.py asserts of the wide structs' corpus, from the checker alone"""
    G.check_wide_corpus(G.wide_cases())
    G.check_wide_corpus(G.wide_cases(G.WIDE_GPU_NS))
    for fam in [G.staged_family(d) for d in G.STAGED_DELTAS] + [G.padded_family()]:
        fam.assert_worth_running()


@pytest.mark.parametrize("mode", G.WIDE_MODES)
def test_walk_wide_structs(walk, mode):
    """1 to 300 fields, up to 64 of them tracked: bit 63 of the live mask required and as a literal, the field
    search over more than 33 fields, ids at the int16 extremes"""
    for n, m, top in G.wide_cases():
        if m == mode:
            family_on_both_routes(walk, G.wide_family(n, m, top))


def test_walk_plans_around_the_lane_routes_lds_copy(walk):
    cap = G.lane_plan_cap()
    assert [G.tab_len(G.staged_family(d).blob()) - cap for d in G.STAGED_DELTAS] == [-8, 0, 8]
    for d in G.STAGED_DELTAS:
        family_on_both_routes(walk, G.staged_family(d))
    assert G.tab_len(G.padded_family().blob()) > 3 * cap
    family_on_both_routes(walk, G.padded_family())


def test_walk_runs_and_alignments(walk):
    w, n = G.run_pair()
    msgs = G.run_messages()
    want, _ = both(walk, msgs, w, n)
    assert all(r == 0 for r, _ in want)


def test_walk_chains_around_the_frame_limits(walk):
    node, node_n = G.node_pair()
    rng = random.Random(21)
    for depth in (7, 8, 9, X.CUT_MAX_DEPTH - 1, X.CUT_MAX_DEPTH, X.CUT_MAX_DEPTH + 1):
        kinds = G.chains_of(depth, rng)
        msgs = [G.chain_message(k) for k in kinds]
        for o in (0, R.WRITE_DEFAULT):
            want, declined = both(walk, msgs, node, node_n, o)
            assert all((r == R.E_DEPTH) == (depth > X.CUT_MAX_DEPTH) for r, _ in want)
            assert all(d == (depth > G.LDS_FRAMES) for d in declined), (depth, declined)


def test_walk_dropped_value_at_the_skip_limit(walk):
    wide, narrow = G.pair()
    msgs = [G.deep_drop_message(d) for d in (7, 8, 9, 1022, 1023, 1024)]
    want, declined = both(walk, msgs, wide, narrow)
    assert [r for r, _ in want] == [0, 0, 0, 0, 0, R.E_READ] and declined == [0, 0, 1, 1, 1, 1]


def test_walk_slots(walk):
    """a slot of exactly the needed size takes the message, one byte less is E_OVERFLOW with the size"""
    wide, narrow = G.pair()
    msgs = [m for m, (r, out) in zip(G.fuzz()[0], G.expect(G.fuzz()[0], wide, narrow, R.WRITE_DEFAULT)) if r == 0][:64]
    want = G.expect(msgs, wide, narrow, R.WRITE_DEFAULT)
    blob = X.compile_cut(wide, narrow)
    for route in (0, 1):
        got, _ = walk(msgs, blob, R.WRITE_DEFAULT, route, caps=[len(o) for _, o in want])
        assert got == want
        got, _ = walk(msgs, blob, R.WRITE_DEFAULT, route, caps=[len(o) - 1 for _, o in want])
        assert [g[0] for g in got] == [R.overflow(len(o)) for _, o in want]


def test_walk_empty_and_wave_min(walk):
    wide, narrow = G.pair()
    blob = X.compile_cut(wide, narrow)
    msgs = [b"", b"\x00", REQ_S + b"\x00"]
    want = G.expect(msgs, wide, narrow)
    assert [r & 0xFF for r, _ in want] == [R.E_READ, R.E_REQUIRED, R.OK]
    for wave_min, declined in ((0, [1, 1, 1]), (1, [0, 1, 1]), (9, [0, 0, 1]), (10, [0, 0, 0])):
        got, d = walk(msgs, blob, 0, 0, wave_min=wave_min)
        assert got == want and d == declined


def test_stand_alone_program_under_sanitizers(tmp_path):
    """cut_walk_host.cpp as a program (-DWALK_MAIN) built with AddressSanitizer
    and UBSan: every message, every slot (exactly the needed size, or one byte
    less for every fourth message) and the plan in heap blocks of their own.
    Both routes run on every message; the counts it prints are the checker's."""
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host walk with" % B.HIPCC)
    wide, narrow = G.pair()
    node, node_n = G.node_pair()
    exe = build_walk(str(tmp_path / "cutwalk"), ("-DWALK_MAIN", "-Xarch_host", "-fsanitize=address,undefined",
                                                   "-fno-sanitize-recover=undefined"))
    msgs, bad = G.fuzz()
    sets = [(msgs[:96] + bad[:96] + [G.deep_drop_message(d) for d in (9, 1023, 1024)], wide, narrow, R.WRITE_DEFAULT),
            (msgs[:48] + bad[:48], wide, narrow, R.DISALLOW_UNKNOWN),
            ([G.chain_message("S" * (d - 1)) for d in (8, 9, 64, 65)], node, node_n, R.WRITE_DEFAULT),
            (G.run_messages()[::37], *G.run_pair(), 0)]
    # 300 fields with sparse ids and 64 tracked; the fuzz shape with a plan of 16 KB
    wide300, padded = G.wide_family(300, "sparse"), G.padded_family()
    sets += [(wide300.msgs, wide300.frm, wide300.to, R.WRITE_DEFAULT), (padded.msgs, padded.frm, padded.to, R.WRITE_DEFAULT)]
    files, count, total, n_msgs = [], {}, 0, 0
    for k, (ms, frm, to, o) in enumerate(sets):
        want = G.expect(ms, frm, to, o)
        caps = [len(out) - (1 if i % 4 == 3 and out else 0) for i, (_, out) in enumerate(want)]
        for (r, out), c in zip(want, caps):
            st = R.E_OVERFLOW if r == 0 and c < len(out) else r & 0xFF
            count[st] = count.get(st, 0) + 1
            total += len(out) if st == 0 else 0
        files.append(str(tmp_path / ("corpus%d.bin" % k)))
        G.write_corpus(files[-1], ms, caps, X.compile_cut(frm, to), o)
        n_msgs += len(ms)
    out = subprocess.run([exe, *files], check=True, capture_output=True, text=True).stdout
    assert out.startswith("%d messages, " % n_msgs), out
    assert out.strip().endswith("OK %d, E_READ %d, E_TYPE %d, E_UNKNOWN %d, E_REQUIRED %d, E_DEPTH %d, E_OVERFLOW %d; %d bytes" % (
        *(count.get(s, 0) for s in (R.OK, R.E_READ, R.E_TYPE, R.E_UNKNOWN, R.E_REQUIRED, R.E_DEPTH, R.E_OVERFLOW)), total)), out
    assert count.get(R.E_OVERFLOW, 0) > 20 and count.get(R.E_DEPTH, 0) == 1
