"""GPU: the cut (batched MarshalTo) over plan shapes that pick a branch the
message does not: the lane route's two ways to read the plan (cut_stage_plan in
cut_kern.hip copies tables of at most CUT_LANE_PLAN bytes to LDS and reads
longer ones from device memory), at the boundary and far past it, and `to`
structs of up to 64 tracked fields (bit 63 of the live mask as a required field
and as a literal, the field search over 300 fields, ids at the int16 extremes).
The checker (cutref.py) is the yardstick; test_cut_host.py runs the same
families through the walk on the CPU, where the staging does not exist. Every
device run checks the memory contract too (test_gpu_cut.run_device)."""
import pytest

import cutgen as G
import cutref as R
from test_gpu_cut import on_both_routes

pytestmark = pytest.mark.gpu

DEFAULTS = (0, R.WRITE_DEFAULT, R.WRITE_DEFAULT | R.DISALLOW_UNKNOWN)


@pytest.fixture(scope="module")
def plan_of():
    """plan_of(family): its plan on the device, made once"""
    from dynamicgo_amd import generic as X
    made = {}

    def get(fam):
        if fam.name not in made:
            made[fam.name] = X.CutPlan(fam.blob())
        return made[fam.name]

    yield get
    for p in made.values():
        p.close()


def pick(fam, good, bad):
    """the first `good` unmutated messages and the first `bad` mutated copies: (indices, messages)"""
    idx = list(range(good)) + list(range(fam.n_good, fam.n_good + bad))
    return idx, [fam.msgs[i] for i in idx]


def run_family(knob, plan_of, fam, idx, opts_words, flat=False):
    """flat: the family's structs hold no struct, so a message grows by the literals of one STOP at the most and gets a
    slot of that size (dg_cut_slot_bound allows for a struct per byte: 1.3 MB a message with 64 literals)"""
    msgs = [fam.msgs[i] for i in idx]
    caps = [(len(m) + G.unset_bytes(fam.blob()) + 15) & ~15 for m in msgs] if flat else None
    for o in opts_words:
        want = fam.want(o)
        on_both_routes(knob, plan_of(fam), msgs, [want[i] for i in idx], o, caps)


def test_corpus():
    """from the checker alone: test_cut_host.py asserts the same without a GPU"""
    G.check_wide_corpus(G.wide_cases(G.WIDE_GPU_NS))
    for fam in [G.staged_family(d) for d in G.STAGED_DELTAS] + [G.padded_family()]:
        fam.assert_worth_running()


@pytest.mark.parametrize("delta", G.STAGED_DELTAS)
def test_plan_at_the_edge_of_the_lds_copy(knob, plan_of, delta):
    """tables of CUT_LANE_PLAN - 8 and CUT_LANE_PLAN bytes are staged (the copy loop's last 8-byte step), CUT_LANE_PLAN
    + 8 is read where it is"""
    fam = G.staged_family(delta)
    cap, tab = G.lane_plan_cap(), G.tab_len(fam.blob())
    assert tab == cap + delta and (tab <= cap) == (delta <= 0)
    idx, _ = pick(fam, 64, 16)
    run_family(knob, plan_of, fam, idx, DEFAULTS, flat=True)


def test_fuzz_shape_with_the_plan_in_device_memory(knob, plan_of):
    """the whole shape of test_gpu_cut.py's fuzz (nesting, lists and maps of narrowed structs, a struct map key, the
    recursive Node, a mismatched field, required / default / to-only fields) under a plan the lane route cannot stage"""
    from dynamicgo_amd import generic as X
    fam = G.padded_family()
    assert G.tab_len(fam.blob()) > 3 * G.lane_plan_cap()
    assert G.tab_len(X.compile_cut(*G.pair())) <= G.lane_plan_cap()  # what test_gpu_cut.py runs is staged
    idx, _ = pick(fam, 64, 16)
    run_family(knob, plan_of, fam, idx, G.ALL_OPTS)


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_batch_sizes_with_the_plan_in_device_memory(knob, plan_of, n):
    """block edges of the lane kernel: a block with fewer live messages than lanes skips the staging as one"""
    fam = G.padded_family()
    assert G.tab_len(fam.blob()) > G.lane_plan_cap() and 2 * G.PAD_N >= n
    idx = [k // 2 + (k % 2) * fam.n_good for k in range(n)]  # unmutated and mutated ones in turn
    run_family(knob, plan_of, fam, idx, (R.WRITE_DEFAULT,))


@pytest.mark.parametrize("n", G.WIDE_GPU_NS)
def test_wide_structs(knob, plan_of, n):
    """64 tracked fields at n = 64 (every field of `to`), 65 (one more), 129 and 300; the plans of 64 and 65 fields are
    staged in LDS, those of 129 lie on both sides of CUT_LANE_PLAN, those of 300 are read from device memory"""
    cases = G.wide_cases((n,))
    assert len(cases) >= 3
    if n >= 129:
        assert any(len(G.tracked_ids(G.wide_family(*c).to)) == 64 and c[1] != "dense" for c in cases)
    sides = set()
    for c in cases:
        fam = G.wide_family(*c)
        sides.add(G.tab_len(fam.blob()) <= G.lane_plan_cap())
        run_family(knob, plan_of, fam, range(len(fam.msgs)), G.ALL_OPTS, flat=True)
    assert sides == {64: {True}, 65: {True}, 129: {True, False}, 300: {False}}[n]


def test_one_byte_short_with_wide_and_unstaged_plans(knob, plan_of):
    """exact-size slots back to back, every third one a byte short: E_OVERFLOW with the size in aux and out_len, whole
    neighbours on both sides (run_device checks that nothing lies beyond their out_len)"""
    opts = R.WRITE_DEFAULT
    for fam in (G.padded_family(), G.wide_family(300, "sparse"), G.wide_family(300, "sparse", "def")):
        ok = [(m, w) for m, w in zip(fam.msgs, fam.want(opts)) if w[0] == 0][:96]
        assert len(ok) >= 24
        caps = [len(w[1]) - (i % 3 == 1) for i, (_, w) in enumerate(ok)]
        expect = [(R.overflow(len(w[1])), b"") if i % 3 == 1 else w for i, (_, w) in enumerate(ok)]
        on_both_routes(knob, plan_of(fam), [m for m, _ in ok], expect, opts, caps)
