"""GPU parity over descriptor shapes: the families of descgen.py (built so
that a descriptor's shape, not the message, picks the branch -- name tables
with equal hashes and wrapping probe chains, keys at the 8- and 16-byte
seams, aliases that shadow each other, 1 .. 257 fields, struct indices around
the wave kernel's mask table, blobs at every routing threshold) on every
route of dg_j2t_batch_host and both t2j kernels, status word for status word
and byte for byte against the checker; and the routes the code's own
eligibility rules promise: plain keys of a small flat struct never leave the
fast kernels, a message that outgrows the lane kernel's requires arena is
redone by the deep pass and no other is."""
import pytest

import descgen as G
import oracle
from dynamicgo_amd import conv, thrift as T
from test_gpu_parity import _raw_batch
from test_gpu_t2j import compare as t2j_compare

pytestmark = pytest.mark.gpu

NO_FAST, NO_WAVE, FLAT, NO_FLAT = 1 << 17, 1 << 18, 1 << 19, 1 << 21
ROUTES = ("hybrid", "flat", "no-flat", "no-wave", "no-fast", "wave-all")
WREQ, WDEF, WOPT = 1 << 6, 1 << 5, 1 << 7  # DG_T2J_WRITE_*
T2J_OPTS = (0, WREQ, WDEF | WREQ | WOPT)


def flat_root(case):
    """flat_root of j2t_host.hip: a struct of at most 64 scalar or string
    fields whose blob fits the flat kernel's LDS copy (no HTTP mappings here)."""
    td = case.td
    if td.type != T.STRUCT or len(case.flat.blob) > G.kernel_const("j2t_flat.h", "FL_DESC"):
        return False
    fs = td.struct.fields
    return len(fs) <= 64 and all(f.type.type in (T.BOOL, T.BYTE, T.I16, T.I32, T.I64, T.DOUBLE, T.STRING) for f in fs)


_expected = {}


def expected(case, flags):
    key = (case.name, len(case.flat.blob), flags)
    if key not in _expected:
        chk = oracle.RefOracle() or oracle.PortOracle()
        rets, outs = chk.j2t_batch(case.flat, case.msgs, flags)
        _expected[key] = ([int(r) for r in rets], outs)
    return _expected[key]


def run_route(case, route, flags, knob, msgs=None):
    extra = {"hybrid": 0, "flat": FLAT, "no-flat": NO_FLAT, "no-wave": NO_WAVE, "no-fast": NO_FAST, "wave-all": 0}[route]
    knob("wave_min", 0 if route == "wave-all" else 512)
    outs, rets = _raw_batch(case.flat, case.msgs if msgs is None else msgs, flags | extra)
    return [int(r) for r in rets], outs


def parity(cases, route, knob, flag_words=G.FLAG_WORDS):
    bad, ran = [], 0
    for case in cases:
        if route == "flat" and not flat_root(case):
            continue
        for flags in flag_words:
            er, eo = expected(case, flags)
            rets, outs = run_route(case, route, flags, knob)
            ran += 1
            for i in range(len(case.msgs)):
                if rets[i] != er[i] or outs[i] != eo[i]:
                    bad.append((case.name, route, hex(flags), i, case.msgs[i][:80], hex(rets[i]), hex(er[i])))
    return bad, ran


@pytest.mark.parametrize("route", ROUTES)
def test_names(route, knob):
    cases, _ = G.names_family()
    bad, ran = parity(cases, route, knob)
    assert ran == len(cases) * len(G.FLAG_WORDS)  # all four are flat roots
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("route", ROUTES)
def test_aliases_and_ids(route, knob):
    cases = G.aliases_family() + G.ids_family()
    bad, ran = parity(cases, route, knob)
    assert ran == len(cases) * len(G.FLAG_WORDS)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("form", G.FORMS)
def test_counts(form, knob):
    cases = G.counts_family((form,))
    for route in ROUTES:
        bad, ran = parity(cases, route, knob)
        # flat roots: the all-scalar structs of at most 64 fields
        flat_roots = len([c for c in cases if c.props["n"] <= 64]) if form == "flat" else 0
        assert route != "flat" or ran == flat_roots * len(G.FLAG_WORDS)
        assert not bad, (route, len(bad), bad[:5])


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "flat"])
def test_structs(route, knob):
    bad, ran = parity([G.structs_case(), G.tree_case()], route, knob)
    assert ran and not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("edge", G.SIZE_EDGES)
def test_sizes(edge, knob):
    """The same batch under blobs 8 bytes below, at and 8 bytes above a
    routing threshold: identical outputs, and the checker's."""
    cases = G.sizes_family([edge - 8, edge, edge + 8])
    for route in ROUTES:
        for flags in G.FLAG_WORDS:
            got = []
            for c in cases:
                if route == "flat" and not flat_root(c):
                    continue
                got.append((c.name, run_route(c, route, flags, knob)))
            er, eo = expected(cases[0], flags)
            for name, (rets, outs) in got:
                bad = [(name, route, hex(flags), i, cases[0].msgs[i][:60], hex(rets[i]), hex(er[i]))
                       for i in range(len(er)) if rets[i] != er[i] or outs[i] != eo[i]]
                assert not bad, (len(bad), bad[:5])
    assert [flat_root(c) for c in cases] == [edge - 8 <= 16384, edge <= 16384, edge + 8 <= 16384]


def slot_bound(n):
    """dg_slot_bound of j2t_host.hip: the output slot of an n-byte message."""
    return (4 * n + 64 + 127) & ~127


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "flat"])
def test_reqarena_hands_exactly_the_too_deep_messages_to_the_deep_pass(route, knob):
    """Every flag word: 0x3, 0x83 and 0xa3 (F_WRITE_DEFAULT) make each open
    level walk its 64-word bitmap and write its 2016 unset DEFAULT fields
    (14 KB a level, up to 85 KB a message), in the lane arena up to `fit`
    levels and in the deep pass's beyond. The output buffer is sized from the
    checker's outputs; the usual 16 bytes per input byte are far too few here.

    The blob (about 260 KB) is larger than DESC_LDS_BYTES, so enqueue() has
    neither a small nor a wave stage on any route: the lane kernel over global
    memory converts the batch alone, with the fast path (hybrid, no-flat,
    no-wave, wave-all: one and the same launch) or without it (no-fast).

    deeps counts a launch's DG_ST_DEEP messages, and batch_host launches a
    second time for the messages that came back DG_ST_OUT_OVERFLOW (ret 0 and
    more bytes than dg_slot_bound of the message): a too-deep message whose
    output outgrows its slot meets the arena's end in both launches."""
    case = G.reqarena_case()
    assert not flat_root(case) and len(case.flat.blob) > G.kernel_const("j2t_machine.h", "DESC_LDS_BYTES")
    fit = case.props["fit"]
    deep = [i for i, it in enumerate(case.intents) if it.depth > fit]
    assert 0 < len(deep) < len(case.msgs) and any(it.depth == fit for it in case.intents)
    ctx = conv.default_context()
    redone_at = set()
    for flags in G.FLAG_WORDS:
        er, eo = expected(case, flags)
        slots = [slot_bound(len(m)) for m in case.msgs]
        assert all(len(o) <= s // 2 or len(o) >= 2 * s for o, s in zip(eo, slots))  # nowhere near the slot's edge
        redone = [i for i in range(len(er)) if er[i] == 0 and len(eo[i]) > slots[i]]
        if redone:
            redone_at.add(flags)
        want = len(deep) + len(set(deep) & set(redone))
        ctx.stats(reset=True)
        extra = {"hybrid": 0, "no-flat": NO_FLAT, "no-wave": NO_WAVE, "no-fast": NO_FAST, "wave-all": 0}[route]
        knob("wave_min", 0 if route == "wave-all" else 512)
        outs, rets = _raw_batch(case.flat, case.msgs, flags | extra, cap=sum(map(len, eo)) + 65536)
        _, deeps = ctx.stats(reset=True)
        bad = [(i, hex(int(rets[i])), hex(er[i]), len(outs[i]), len(eo[i])) for i in range(len(er))
               if int(rets[i]) != er[i] or outs[i] != eo[i]]
        assert not bad, (route, hex(flags), bad[:5])
        assert deeps == want, (route, hex(flags), deeps, want)
    assert redone_at == {f for f in G.FLAG_WORDS if f & G.F_WRITE_DEFAULT}


@pytest.mark.parametrize("route", ["flat", "no-flat", "no-wave", "wave-all"])
def test_plain_keys_stay_on_the_fast_route(route, knob):
    """Eligible by the code's own rules: a flat root of at most 16 names (the
    flat kernel's key table) or any number of them (its name-table lookup),
    plain keys that hit, nothing to write for unset fields (F_ALLOW_UNKNOWN
    alone), messages far below 256 bytes. fast_convert, fl_field and the wave
    kernel's lookup decline a struct field only for an escaped key, an
    unknown key (LEAN), a wide struct or -- the wave kernel, which leaves the
    order semantics to the exact machine -- one field named twice; none of
    which is here (the two-keys-of-one-field messages of the aliases family
    are left out for that reason)."""
    ctx = conv.default_context()
    cases = G.names_family()[0] + G.aliases_family() + G.ids_family()
    for case in cases:
        keep = [i for i, it in enumerate(case.intents) if it.kind == G.HIT and not it.escaped and
                b"\x00" not in case.msgs[i] and len(set(it.ids)) == len(it.ids)]
        assert len(keep) >= min(len(case.td.struct.names), 7), case.name
        msgs = [case.msgs[i] for i in keep]
        er, eo = expected(case, 0x1)
        ctx.stats(reset=True)
        rets, outs = run_route(case, route, 0x1, knob, msgs)
        bails, deeps = ctx.stats(reset=True)
        assert rets == [er[i] for i in keep] and outs == [eo[i] for i in keep], case.name
        assert (bails, deeps) == (0, 0), (case.name, route, bails, deeps)


# ------------------------------------------------------------------ t2j
@pytest.fixture(scope="module")
def t2j_chk():
    o = oracle.RefT2JOracle()
    if o is None:
        pytest.skip("oracle/_ref not built")
    return o


def t2j_cases():
    out = [(c.name, c.td, c.td.struct) for c in G.ids_family() + G.aliases_family()]
    for n in (65, 128, 129, 257):
        td, _ = G.wide_struct(n, "W%d" % n)
        out.append(("W%d" % n, td, td.struct))
    return out


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_t2j_ids_counts_aliases(t2j_chk, kernel, knob):
    knob("t2j_wave_min", 0 if kernel == "lane" else 1)
    for name, td, sd in t2j_cases():
        fl = T.flatten(td)
        msgs = G.t2j_messages(sd)
        for opts in T2J_OPTS:
            bad = t2j_compare(t2j_chk, fl, msgs, opts)
            assert not bad, (name, kernel, opts, len(bad), bad[:3])


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_t2j_sizes(t2j_chk, kernel, knob):
    """t2j's wave kernel takes blobs up to 16 384 bytes whose side table is
    at most T2W_SIDE bytes: blobs 8 bytes below, at and above the first, with
    a side table well under the second, and blobs whose side table is over."""
    knob("t2j_wave_min", 0 if kernel == "lane" else 1)
    descs = [G.chain_sized_desc(t) for t in (16376, 16384, 16392)] + [G.sized_desc(t) for t in (12288, 16384)]
    for td in descs:
        fl = T.flatten(td)
        target = len(fl.blob)
        side = len(T.flatten_t2j(fl))
        assert (side <= G.kernel_const("t2j_wave.h", "T2W_SIDE")) == (td.name == "ChainSized"), (td.name, side)
        msgs = G.t2j_messages(td.struct, limit=8)
        for opts in T2J_OPTS:
            bad = t2j_compare(t2j_chk, fl, msgs, opts)
            assert not bad, (target, kernel, opts, len(bad), bad[:3])
