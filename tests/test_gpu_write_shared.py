"""GPU: what the two write components (dg_vals_*, dg_evals_*) share in the host
layer, pinned per component: (a) every single-fault refusal of the create, the
device and the host entries with its return code and its full text, called
through the library where the Python wrappers would stop the call first; (b)
the host entries' two-pass contract (sizing, a cap one byte short, an exact cap,
n = 0); (c) which payload bytes a host entry uploads: a first live payload well
inside the source, empty strings whose offsets lie past the source's end, and a
flagged cell (vals) or an absent cell's entries (evals) with wild offsets, all
compared with valsref / evalsref. Every batch has n <= 3 and K <= 2.

The device-side refusals pass real device memory of zeros for everything that
is not the fault, misaligned pointers included (they point into the same
allocation), so that nothing a call could launch reads or writes elsewhere."""
import ctypes as C

import numpy as np
import pytest

import evalsgen as EG
import evalsref as ER
import valsgen as VG
import valsref as VR

pytestmark = pytest.mark.gpu

INVALID, NOMEM, ARG = -1, -3, -6  # DG_E_*
N = 3
V_FIELDS = ("val", "len", "src", "elem_off", "elems", "present")
E_FIELDS = ("ent_off", "key", "key_len", "val", "val_len", "key_src", "val_src", "present")
LIST_I64, MAP_I32_F64, MAP_STR_I64 = VR.LIST | VR.I64, ER.map_kind(ER.I32, ER.DOUBLE), ER.map_kind(ER.STRING, ER.I64)


@pytest.fixture(scope="module")
def env():
    """the library, two contexts, 8 KiB of zeroed device memory cut into 256-byte fields, and plans per kind class"""
    import torch
    from dynamicgo_amd import _lib, generic as G
    from dynamicgo_amd.conv import Context, default_context

    class Env:
        pass
    e = Env()
    e.L, e.G, e.lib, e.ctx, e.other = _lib.lib(), G, _lib, default_context(), Context(0)
    e.mem = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = int(e.mem.data_ptr())
    assert base % 256 == 0
    names = V_FIELDS + tuple("e_" + f for f in E_FIELDS) + ("out", "out_off", "status", "work")
    e.at = {f: base + 256 * k for k, f in enumerate(names)}  # work: the last field, 8192 - 256 * 17 = 3840 bytes
    e.work_bytes = 8192 - 256 * (len(names) - 1)
    e.vplans = {k: G.ValuePlan([k]) for k in (VR.I32, VR.STRING, LIST_I64)}
    e.vstruct = G.ValuePlan([VR.I32], [1])
    e.vother = G.ValuePlan([VR.I32], None, e.other)
    e.eplans = {k: G.EntryValuePlan([k]) for k in (ER.LIST_STR, MAP_I32_F64, MAP_STR_I64)}
    e.eother = G.EntryValuePlan([ER.LIST_STR], None, e.other)
    yield e
    for p in list(e.vplans.values()) + list(e.eplans.values()) + [e.vstruct, e.vother, e.eother]:
        p.close()
    e.other.close()


def answer(e, rc):
    return rc, (e.L.dg_last_error() or b"").decode() if rc else ""


def vcol(e, **over):
    """dg_val_col[1] of the zeroed device fields; over: field -> pointer (None: null)"""
    from dynamicgo_amd._lib import ValCol
    f = {k: e.at[k] for k in V_FIELDS if k != "present"}
    f.update(over)
    return (ValCol * 1)(ValCol(*[f.get(k) for k in V_FIELDS]))


def ecol(e, n_ent=2, **over):
    from dynamicgo_amd._lib import EvalCol
    f = {k: e.at["e_" + k] for k in E_FIELDS if k != "present"}
    f.update(over)
    return (EvalCol * 1)(EvalCol(*[f.get(k) for k in E_FIELDS], n_ent))


def vals_device(e, plan=None, ctx=0, cols=0, n=N, out_off=0):
    """one dg_vals_batch_device call; 0 stands for the good argument"""
    plan = e.vplans[VR.I32] if plan is None else plan
    return answer(e, e.L.dg_vals_batch_device(e.ctx.h if ctx == 0 else ctx, plan if not hasattr(plan, "h") else plan.h,
                                              vcol(e) if cols == 0 else cols, n, 0, e.at["out"], 64,
                                              e.at["out_off"] if out_off == 0 else out_off, e.at["status"], None))


def evals_device(e, plan=None, ctx=0, cols=0, n=N, out_off=0, work=0, work_bytes=None):
    plan = e.eplans[ER.LIST_STR] if plan is None else plan
    return answer(e, e.L.dg_evals_batch_device(e.ctx.h if ctx == 0 else ctx, plan if not hasattr(plan, "h") else plan.h,
                                               ecol(e) if cols == 0 else cols, n, 0, e.at["out"], 64,
                                               e.at["out_off"] if out_off == 0 else out_off, e.at["status"],
                                               e.at["work"] if work == 0 else work,
                                               e.work_bytes if work_bytes is None else work_bytes, None))


class HostCall:
    """the host arrays of one dg_*_batch_host call over n = 3 rows of zeros"""

    def __init__(self, e, evals):
        self.e, self.evals = e, evals
        self.arr = {f: np.zeros(64, dtype=np.uint64) for f in (E_FIELDS if evals else V_FIELDS)}
        self.off, self.status, self.need = np.zeros(N + 1, dtype=np.uint64), np.zeros(N, dtype=np.uint8), C.c_uint64(0)

    def cols(self, n_ent=2, **over):
        from dynamicgo_amd._lib import EvalCol, ValCol
        fields = E_FIELDS if self.evals else V_FIELDS
        f = {k: self.arr[k].ctypes.data for k in fields if k != "present"}
        f.update(over)
        vals = [f.get(k) for k in fields]
        return (EvalCol * 1)(EvalCol(*vals, n_ent)) if self.evals else (ValCol * 1)(ValCol(*vals))

    def __call__(self, plan=None, ctx=0, cols=0, n=N, off=0):
        e = self.e
        plan = (e.eplans[ER.LIST_STR] if self.evals else e.vplans[VR.I32]) if plan is None else plan
        fn = e.L.dg_evals_batch_host if self.evals else e.L.dg_vals_batch_host
        return answer(e, fn(e.ctx.h if ctx == 0 else ctx, plan if not hasattr(plan, "h") else plan.h,
                            self.cols() if cols == 0 else cols, n, None, 0, self.off.ctypes.data if off == 0 else off,
                            self.status.ctypes.data, C.byref(self.need)))


# a ------------------------------------------------------------ the reject table
def test_create_rejects(env):
    e = env
    for evals, fn, good, bad, dt in ((False, e.L.dg_vals_create, VR.I32, 12, np.uint8),
                                     (True, e.L.dg_evals_create, ER.LIST_STR, 0x41, np.uint16)):
        kinds = np.array([good] * 17, dtype=dt)
        kp = kinds.tobytes()  # dg_vals_create's kinds are declared as a byte string

        def create(ctx=e.ctx.h, kinds=kp, K=1, out=True):
            h = C.c_void_p()
            rc = fn(ctx, kinds, K, None, C.byref(h) if out else None)
            assert rc or h.value
            if h.value:
                (e.L.dg_evals_destroy if evals else e.L.dg_vals_destroy)(h)
            return answer(e, rc)

        assert create() == (0, "")
        assert create(ctx=None) == (INVALID, "null ctx/kinds/out")
        assert create(kinds=None) == (INVALID, "null ctx/kinds/out")
        assert create(out=False) == (INVALID, "null ctx/kinds/out")
        assert create(K=0) == (ARG, "0 columns (1 to 16)")
        assert create(K=17) == (ARG, "17 columns (1 to 16)")
        assert create(kinds=np.array([good, bad], dtype=dt).tobytes(), K=2) == (ARG, "column 1: unknown kind %d" % bad)


def test_vals_device_rejects(env):
    e, at = env, env.at
    assert vals_device(e) == (0, "")
    who = (INVALID, "null ctx/plan, or a plan of another context")
    assert vals_device(e, ctx=None) == who
    assert vals_device(e, plan=C.c_void_p(None)) == who
    assert vals_device(e, plan=e.vother) == who
    assert vals_device(e, cols=None) == (INVALID, "null columns")
    assert vals_device(e, cols=vcol(e, present=at["present"])) == (ARG, "column 0: d_present in a plan without field ids")
    assert vals_device(e, plan=e.vstruct, cols=vcol(e, present=at["present"])) == (0, "")
    assert vals_device(e, out_off=None) == (INVALID, "d_out_off null or not 8-byte aligned")
    assert vals_device(e, out_off=at["out_off"] + 4) == (INVALID, "d_out_off null or not 8-byte aligned")
    null = (INVALID, "column 0: null buffer")
    assert vals_device(e, cols=vcol(e, val=None)) == null
    assert vals_device(e, plan=e.vplans[VR.STRING], cols=vcol(e, val=None)) == null
    assert vals_device(e, plan=e.vplans[VR.STRING], cols=vcol(e, len=None)) == null
    assert vals_device(e, plan=e.vplans[LIST_I64], cols=vcol(e, elem_off=None)) == null
    # what a kind does not read may be null
    assert vals_device(e, cols=vcol(e, len=None, src=None, elem_off=None, elems=None)) == (0, "")
    assert vals_device(e, plan=e.vplans[LIST_I64], cols=vcol(e, val=None, len=None, src=None, elems=None)) == (0, "")
    crooked = (INVALID, "column 0: values, offsets or elements not aligned")
    for f, by in (("val", 4), ("elem_off", 4), ("elems", 4), ("len", 2)):
        assert vals_device(e, plan=e.vplans[VR.STRING], cols=vcol(e, **{f: at[f] + by})) == crooked, f
    import torch
    torch.cuda.synchronize()


def test_evals_device_rejects(env):
    e, at = env, env.at
    assert evals_device(e) == (0, "")
    who = (INVALID, "null ctx/plan, or a plan of another context")
    assert evals_device(e, ctx=None) == who
    assert evals_device(e, plan=C.c_void_p(None)) == who
    assert evals_device(e, plan=e.eother) == who
    assert evals_device(e, cols=None) == (INVALID, "null columns")
    assert evals_device(e, cols=ecol(e, present=at["e_present"])) == (ARG, "column 0: d_present in a plan without field ids")
    assert evals_device(e, cols=ecol(e, n_ent=2 ** 32)) == (ARG, "column 0: 4294967296 entries (at most 4294967295)")
    assert evals_device(e, out_off=None) == (INVALID, "d_out_off null or not 8-byte aligned")
    assert evals_device(e, out_off=at["out_off"] + 4) == (INVALID, "d_out_off null or not 8-byte aligned")
    null = (INVALID, "column 0: null buffer")
    assert evals_device(e, cols=ecol(e, ent_off=None)) == null
    assert evals_device(e, cols=ecol(e, val=None)) == null
    assert evals_device(e, cols=ecol(e, val_len=None)) == null
    assert evals_device(e, plan=e.eplans[MAP_I32_F64], cols=ecol(e, key=None)) == null
    assert evals_device(e, plan=e.eplans[MAP_I32_F64], cols=ecol(e, val=None)) == null
    assert evals_device(e, plan=e.eplans[MAP_STR_I64], cols=ecol(e, key_len=None)) == null
    # with no entries only d_ent_off is read; a fixed-stride kind reads no length
    assert evals_device(e, cols=ecol(e, n_ent=0, key=None, key_len=None, val=None, val_len=None, key_src=None, val_src=None)) == (0, "")
    assert evals_device(e, plan=e.eplans[MAP_I32_F64], cols=ecol(e, key_len=None, val_len=None, key_src=None, val_src=None)) == (0, "")
    crooked = (INVALID, "column 0: offsets, keys, values or lengths not aligned")
    for f, by in (("ent_off", 4), ("key", 4), ("val", 4), ("key_len", 2), ("val_len", 2)):
        assert evals_device(e, plan=e.eplans[MAP_STR_I64], cols=ecol(e, **{f: at["e_" + f] + by})) == crooked, f
    work = (INVALID, "d_work null or not 8-byte aligned")
    assert evals_device(e, work=None) == work
    assert evals_device(e, work=at["work"] + 4) == work
    need = int(e.L.dg_evals_work_bytes(e.eplans[ER.LIST_STR].h, N, np.array([2], dtype=np.uint64).ctypes.data))
    assert 0 < need <= e.work_bytes
    assert evals_device(e, work_bytes=need) == (0, "")
    assert evals_device(e, work_bytes=need - 1) == (NOMEM, "d_work of %d bytes, %d needed" % (need - 1, need))
    import torch
    torch.cuda.synchronize()


def test_host_rejects(env):
    e = env
    who = (INVALID, "null ctx/plan/columns, or a plan of another context")
    for evals, other in ((False, e.vother), (True, e.eother)):
        call = HostCall(e, evals)
        assert call() == (0, "")
        assert call(ctx=None) == who
        assert call(plan=C.c_void_p(None)) == who
        assert call(plan=other) == who
        assert call(cols=None) == who
        assert call(cols=call.cols(present=call.arr["present"].ctypes.data)) == \
            (ARG, "column 0: d_present in a plan without field ids")
        assert call(off=None) == (INVALID, "null buffer")
    null = (INVALID, "column 0: null buffer")
    call = HostCall(e, False)
    assert call(cols=call.cols(val=None)) == null
    assert call(plan=e.vplans[VR.STRING], cols=call.cols(len=None)) == null
    assert call(plan=e.vplans[LIST_I64], cols=call.cols(elem_off=None)) == null
    call = HostCall(e, True)
    assert call(cols=call.cols(n_ent=2 ** 32)) == (ARG, "column 0: 4294967296 entries (at most 4294967295)")
    assert call(cols=call.cols(ent_off=None)) == null
    assert call(cols=call.cols(val=None)) == null
    assert call(cols=call.cols(val_len=None)) == null
    assert call(plan=e.eplans[MAP_I32_F64], cols=call.cols(key=None)) == null
    assert call(plan=e.eplans[MAP_STR_I64], cols=call.cols(key_len=None)) == null


# b --------------------------------------------------------- the host tail
def string_case():
    return "strings", [VR.I32, VR.STRING], None, [VG.scalar_col([7, -1, 2 ** 31]), VG.string_col([b"abc", b"", b"0123456789"], 5)], N


def entry_case():
    rows = [[(1, b"one"), (-2, b"")], [], [(3, b"three, longer than a unit")]]
    return "entries", [ER.map_kind(ER.I64, ER.STRING)], None, [EG.entry_col(ER.map_kind(ER.I64, ER.STRING), rows, lead=1)], N


@pytest.mark.parametrize("evals", (False, True), ids=("vals", "evals"))
def test_host_tail_contract(env, evals):
    e, G = env, env.G
    _, kinds, fids, cols, n = entry_case() if evals else string_case()
    ref = ER if evals else VR
    arena, woff, wst = ref.encode_batch(kinds, cols, n, fids)
    pairs, want = n * len(kinds), len(arena)
    fn = e.L.dg_evals_batch_host if evals else e.L.dg_vals_batch_host
    with (G.EntryValuePlan if evals else G.ValuePlan)(kinds, fids) as plan:
        recs = plan._cols(cols)

        def call(cap, with_out=True, n=n):
            off = np.full(pairs + 1, 0x77, dtype=np.uint64)
            st = np.full(pairs, 0x77, dtype=np.uint8)
            out = np.full(cap + 16, 0xAA, dtype=np.uint8)
            need = C.c_uint64(2 ** 64 - 1)
            rc = fn(plan.ctx.h, plan.h, recs, n, out.ctypes.data if with_out else None, cap, off.ctypes.data, st.ctypes.data,
                    C.byref(need))
            return answer(e, rc), int(need.value), out, off.tolist(), st.tolist()

        ans, need, _, off, st = call(0, with_out=False)  # a sizing call
        assert ans == (0, "") and need == want and off == woff and st == wst
        ans, need, out, off, st = call(want - 1)
        assert ans == (NOMEM, "values need %d bytes" % want) and need == want and (out == 0xAA).all()
        assert off == woff and st == wst
        ans, need, out, off, st = call(want)
        assert ans == (0, "") and need == want and out[:want].tobytes() == arena and (out[want:] == 0xAA).all()
        assert off == woff and st == wst
        ans, need, out, off, st = call(want, n=0)
        assert ans == (0, "") and need == 0 and off[0] == 0 and (out == 0xAA).all()


# c ------------------------------------------------------ the payload span
def test_vals_payload_span(env):
    """column 0: the first live payload 48 bytes into the source, an empty string past the source's end, a cell flagged
    DG_VAL_E_SIZE at a wild offset; column 1: the live payloads in falling order of their offsets around an empty one"""
    G = env.G
    a = VG.string_col([b"\xEE" * 41, b"first live payload", b"", b""], 3)
    a = {"val": a["val"][1:].copy(), "len": a["len"][1:].copy(), "src": a["src"]}
    assert a["val"][0] >= 41
    a["val"][1], a["val"][2], a["len"][2] = len(a["src"]) + 12345, 2 ** 60, 0x80000000
    b = VG.string_col([b"\xEE" * 23, b"late", b"", b"an early one"], 9)
    b = {"val": b["val"][[3, 2, 1]].copy(), "len": b["len"][[3, 2, 1]].copy(), "src": b["src"]}
    b["val"][1] = 2 ** 63
    kinds, cols = [VR.STRING, VR.STRING], [a, b]
    arena, woff, wst = VR.encode_batch(kinds, cols, N)
    assert wst == [0, 0, 0, 0, VR.E_SIZE, 0]
    with G.ValuePlan(kinds) as plan:
        out, off, st = G._write_host(plan, cols, N)
    assert off.tolist() == woff and st.tolist() == wst and out.tobytes() == arena


def test_evals_payload_span(env):
    """struct mode, map<string, string>: message 0 is absent and its two entries, whose payloads lead both sources,
    carry wild offsets; message 1 holds an empty key and an empty value whose offsets lie past their sources' ends;
    message 2's payloads are the last bytes of the sources"""
    G = env.G
    kind = ER.map_kind(ER.STRING, ER.STRING)
    rows = [[(b"k" * 37, b"v" * 53), (b"absent", b"too")], [(b"", b"value of the empty key"), (b"key", b"")],
            [(b"last key", b"last value")]]
    c = EG.entry_col(kind, rows, phase=2, lead=1)
    c["present"] = np.array([0, 1, 1], dtype=np.uint8)
    for side in ("key", "val"):
        c[side] = c[side].copy()
        assert c[side][3] >= 37  # the first live payload lies well inside
        c[side][1], c[side][2] = 2 ** 60, 2 ** 63 + 5
    c["key"][3], c["val"][4] = len(c["key_src"]) + 999, len(c["val_src"]) + 2 ** 40
    arena, woff, wst = ER.encode_batch([kind], [c], N, [9])
    assert wst == [0, 0, 0] and woff[1] == 1
    with G.EntryValuePlan([kind], [9]) as plan:
        out, off, st = G._write_host(plan, [c], N)
    assert off.tolist() == woff and st.tolist() == wst and out.tobytes() == arena
