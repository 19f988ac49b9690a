"""CPU: the layout arithmetic the thrift/generic host entries share
(dynamicgo_amd/csrc/host_layout.h: offsets rebased to 0, 16-byte slots, the
gather of a rerun, value offsets), run by a stand-alone program
(host_layout_host.cpp) under the address and undefined-behaviour sanitizers,
every array in a heap block of its exact size. What each routine must leave
behind is computed here with numpy."""
import os
import subprocess

import numpy as np
import pytest

from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
OK, DESCENDING, TOO_LONG = 0, 1, 2  # HL_*
SLOT_MAX = 0xFFFFFFFF
U64 = np.uint64


def line(name, nums):
    return name + " " + " ".join(str(int(x)) for x in nums)


def rebase_case(off, K=1):
    """hl_rebase: rel = off - off[0] and the longest span per residue of K, up
    to and without the first descending pair; nothing is written past it."""
    off = np.asarray(off, dtype=U64)
    count = len(off) - 1
    down = np.nonzero(off[1:] < off[:-1])[0]
    good = int(down[0]) if len(down) else count
    rel = off[:good + 1] - off[0]
    spans = off[1:good + 1] - off[:good]
    longest = [int(spans[j::K].max()) if len(spans[j::K]) else 0 for j in range(K)]
    return line("rebase", [K, count, *off, DESCENDING if len(down) else OK, good + 1, *rel, *longest])


def layout_case(in_off, caps=None, idx=None, src=False, longest=True):
    """hl_layout over the messages idx (None: all): io = their lengths summed
    up, so = their capacities (caps[i], None: no slots) rounded up to 16 and
    summed up, src = where each starts, the longest length; all of it up to and
    without the first message that descends or whose capacity is over
    0xFFFFFFFF, which is named."""
    in_off = np.asarray(in_off, dtype=U64)
    n = len(in_off) - 1
    lens = in_off[1:].astype(np.int64) - in_off[:-1].astype(np.int64)
    order = np.arange(n) if idx is None else np.asarray(idx, dtype=np.int64)
    down = lens[order] < 0
    over = np.zeros(len(order), dtype=bool) if caps is None else np.asarray(caps, dtype=object)[order] > SLOT_MAX
    stop = np.nonzero(down | over)[0]
    good = int(stop[0]) if len(stop) else len(order)
    done = order[:good]
    rc, bad, bad_cap = OK, 0, 0
    if len(stop):
        bad = int(order[good])
        rc, bad_cap = (DESCENDING, 0) if down[good] else (TOO_LONG, caps[bad])
    io = np.concatenate([[0], np.cumsum(lens[done])])
    so = [] if caps is None else np.concatenate(
        [[0], np.cumsum([(int(caps[i]) + 15) // 16 * 16 for i in done], dtype=U64)])
    starts = in_off[:-1][done] if src else []
    # the program's capacity of message i is extra[i] + the length it is handed: only the right length gives caps[i]
    extra = [0] * n if caps is None else [(int(caps[i]) - int(lens[i])) % (1 << 64) for i in range(n)]
    return line("layout", [n, *in_off, *extra, idx is not None, len(order), *([] if idx is None else order),
                           caps is not None, src, longest, rc, bad, bad_cap, len(io), *io, len(so), *so, len(starts),
                           *starts, *([max(lens[done], default=0)] if longest else [])])


def offsets(lens, base):
    return np.concatenate([[base], base + np.cumsum(np.asarray(lens, dtype=np.int64))])


def all_cases():
    rng = np.random.default_rng(7)
    out = []
    for n in (1, 2, 5):
        for base in (0, 37):
            lens = rng.integers(1, 300, n)
            some = lens.copy()
            some[::2] = 0  # zero-length messages
            for ls in (lens, some, np.zeros(n, dtype=np.int64)):
                off = offsets(ls, base)
                caps = [int(x) + int(e) for x, e in zip(ls, rng.integers(0, 64, n))]
                out.append(layout_case(off))
                out.append(layout_case(off, longest=False))  # a caller without use for the longest length
                out.append(layout_case(off, caps))
                for idx in ([], list(range(n)), sorted({0, n - 1})):  # a gather of none, of all, of the two ends
                    out.append(layout_case(off, caps, idx, src=True))
                    out.append(layout_case(off, None, idx, src=True))
            # the 32-bit limit at the first, a middle and the last message: accepted at it, refused past it
            for at in sorted({0, n // 2, n - 1}):
                caps = [int(x) + 40 for x in lens]
                for cap in (SLOT_MAX, SLOT_MAX + 1):
                    caps[at] = cap
                    out.append(layout_case(offsets(lens, base), caps))
                    out.append(layout_case(offsets(lens, base), caps, list(range(n))[::-1], src=True))
    # slot rounding at cap % 16 = 0, 1, 15
    out.append(layout_case(offsets([3, 0, 9, 30, 2, 1, 15], 37), [0, 16, 17, 31, 32, 1, 15]))
    # a descending pair at the first, a middle and the last position
    for n, at in ((1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (5, 4)):
        for base in (0, 37):
            off = offsets(np.full(n, 40), base + 100)
            off[at + 1] = off[at] - 1
            if at + 2 <= n:
                off[at + 2:] = off[at + 1] + 40 * np.arange(1, n - at)  # ascending again behind it
            out.append(layout_case(off))
            out.append(layout_case(off, [50] * n))
            out.append(rebase_case(off))
    # value offsets: K items per message, message-major
    for K in (1, 3, 7):
        for n in (1, 2, 5):
            for base in (0, 11):
                out.append(rebase_case(offsets(rng.integers(0, 90, n * K), base), K))
        off = offsets(rng.integers(1, 90, 5 * K), 11)
        off[-1] = off[-2] - 1  # the last value descends
        out.append(rebase_case(off, K))
    return out


def test_layout_under_sanitizers(tmp_path):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host program with" % B.HIPCC)
    exe = str(tmp_path / "host_layout")
    subprocess.run([B.HIPCC, "-O1", "-std=c++17", "-fPIC", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "host_layout_host.cpp")], check=True)
    cases = all_cases()
    assert any(" %d " % (SLOT_MAX + 1) in c for c in cases)
    good = str(tmp_path / "cases.txt")
    with open(good, "w") as fh:
        fh.write("\n".join(cases) + "\n")
    run = subprocess.run([exe, good], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "%d cases, 0 bad" % len(cases), (run.stdout, run.stderr)
    # the program does not pass whatever it is given: one wrong expectation per routine, and no file at all
    for name in ("rebase", "layout"):
        c = next(c for c in cases if c.startswith(name)).split()
        bad = str(tmp_path / "wrong.txt")
        with open(bad, "w") as fh:
            fh.write("\n".join(cases[:3] + [" ".join(c[:-1] + [str(int(c[-1]) + 1)])]) + "\n")
        run = subprocess.run([exe, bad], capture_output=True, text=True)
        assert run.returncode != 0 and run.stdout.strip() == "4 cases, 1 bad", (name, run.stdout, run.stderr)
    assert subprocess.run([exe, str(tmp_path / "missing.txt")], capture_output=True).returncode != 0
