#!/usr/bin/env python3
"""Times the row column writes (dg_rvals_batch_device).

    python tools/rvals_bench.py [--iters 200] [--warmup 20] [--only uniform|skew|chain]

HIP events around every launch, the compared launches alternating in one run;
the mean and p10 / p90 over the launches are reported. The bytes counted come
from the shapes, by the code below: the arena written, the offsets and statuses,
and what the per-row arrays hold (8 bytes a scalar or a string's offset, 4 a
string's length, the payload bytes).

uniform  16 384 messages x list<struct> of 4 / 64 / 1 024 rows, a plan of
         scalars {1: i64, 2: i32, 3: double} (the fixed-stride route) and a plan
         with a string {1: i64, 2: string of 8 bytes, 3: i32} (the scanned
         route). Beside each: its sizing call; the yardstick, values_device in
         struct mode over the same R rows taken as R messages (the same struct
         bytes without the list headers: what the library could do before); and
         the read side, rows_device on the lists the call itself wrote.
skew     one list of 10 000 rows among 16 383 of 4, against an even batch of
         the same rows and bytes: the ratio of the two calls shows whether rows
         placed by scans and written row-parallel do what they are for.
chain    rows_device -> torch (+ 1 on qty) -> row_values_device ->
         edit_many_device on cut_bench's mid batch (field 4, the list of item
         structs {1: i64, 2: string, 3: string, 4: i32}), timed per step.

Writes profiles/rvals_<part>.json."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import HBM_GBS, stats, timed  # noqa: E402

N = 16384
WIDTH = {2: 1, 3: 1, 4: 8, 6: 2, 8: 4, 10: 8}
PLANS = {"scalars": ([10, 8, 4], [1, 2, 3], 0), "scalars+string": ([10, 11, 8], [1, 2, 3], 8)}


def gbs(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def mean(x):
    return statistics.mean(x)


def setup():
    import torch
    from dynamicgo_amd import conv
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev, conv.default_context(), torch.cuda.current_stream()


def columns(kinds, n_rows, slen, rng, dev):
    """(device columns indexed by row, bytes read from them, a row's encoded bytes)"""
    import torch
    cols, read, row = [], 0, 1
    for kind in kinds:
        if kind == 11:
            cols.append({"val": torch.arange(n_rows, dtype=torch.int64, device=dev) * slen,
                         "len": torch.full((n_rows,), slen, dtype=torch.int32, device=dev),
                         "src": torch.from_numpy(rng.integers(1, 255, size=n_rows * slen + 16, dtype=np.uint8)).to(dev)})
            read, row = read + n_rows * (12 + slen), row + 3 + 4 + slen
        else:
            cols.append({"val": torch.from_numpy(rng.integers(0, 2 ** 62, size=n_rows, dtype=np.int64)).to(dev)})
            read, row = read + n_rows * 8, row + 3 + WIDTH[kind]
    return cols, read, row


class Batch:
    """one plan over `counts[i]` rows per message with its outputs; .call / .sizing launch it on the stream"""

    def __init__(self, kinds, ids, counts, slen, seed, ctx, dev, stream):
        import torch
        from dynamicgo_amd import generic as G
        self.G, self.stream, self.n, self.kinds, self.ids = G, stream, len(counts), kinds, ids
        self.n_rows = int(counts.sum())
        off = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(counts, out=off[1:])
        self.row_off = torch.from_numpy(off).to(dev)
        self.cols, read, self.row_bytes = columns(kinds, self.n_rows, slen, np.random.default_rng(seed), dev)
        self.need = 5 * self.n + self.n_rows * self.row_bytes
        self.plan = G.RowValuePlan(kinds, ids, ctx=ctx)
        self.out = torch.zeros(self.need + 16, dtype=torch.uint8, device=dev)
        self.off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.st = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.cst = torch.zeros(self.n_rows * len(kinds), dtype=torch.uint8, device=dev)
        self.work = torch.zeros(self.plan.work_bytes(self.n, self.n_rows), dtype=torch.uint8, device=dev)
        self.moved = read + self.need + 17 * (self.n + 1) + self.n_rows * len(kinds)

    def call(self):
        self.G.row_values_device(self.plan, self.cols, self.row_off, self.n, self.n_rows, self.out, self.off, self.work, self.st,
                                 self.cst, cap=self.need, stream=self.stream)

    def sizing(self):
        self.G.row_values_device(self.plan, self.cols, self.row_off, self.n, self.n_rows, None, self.off, self.work, self.st,
                                 self.cst, cap=0, stream=self.stream)

    def check(self, what):
        if int(self.off[-1].item()) != self.need or self.st.any().item() or self.cst.any().item():
            raise SystemExit("%s: the arena's end (%d, %d expected) or a status is wrong" % (what, int(self.off[-1].item()), self.need))


def vals_yardstick(b, ctx, dev):
    """values_device in struct mode over b's rows as n_rows messages: (call, check)"""
    import torch
    G = b.G
    K, R = len(b.kinds), b.n_rows
    vp = G.ValuePlan(b.kinds, b.ids, ctx=ctx)
    need = R * b.row_bytes
    out = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    off = torch.zeros(R * K + 1, dtype=torch.int64, device=dev)
    st = torch.zeros(R * K, dtype=torch.uint8, device=dev)

    def call():
        G.values_device(vp, b.cols, R, out, off, st, cap=need, stream=b.stream)

    def check(what):
        if int(off[-1].item()) != need:
            raise SystemExit("%s: the yardstick's arena ends at %d, %d expected" % (what, int(off[-1].item()), need))
        first = 5 + b.row_bytes  # message 0's first row against the yardstick's first message
        if b.n_rows and int(b.row_off[1].item()) and not torch.equal(b.out[5:first], out[:b.row_bytes]):
            raise SystemExit("%s: the two writers disagree on the first row" % what)

    return call, check, need + 8 * (R * K + 1) + R * K


def reader(b, ctx, dev):
    """rows_device over the lists batch b has written (root_type LIST, the empty parent)"""
    import torch
    G = b.G
    b.call()
    torch.cuda.synchronize()
    names = {10: "int", 8: "int", 4: "float64", 11: "str"}
    plan = G.RowPlan((), [([G.PathFieldId(f)], names[k]) for f, k in zip(b.ids, b.kinds)], ctx=ctx)
    P, R = len(b.kinds), max(b.n_rows, 1)
    head = torch.zeros((b.n, 4), dtype=torch.int32, device=dev)
    row_off = torch.zeros(b.n + 1, dtype=torch.int64, device=dev)
    index = torch.zeros((R, 4), dtype=torch.int32, device=dev)
    val, cell = (torch.zeros((P, R), dtype=torch.int64, device=dev) for _ in range(2))
    lens = torch.zeros((P, R), dtype=torch.int32, device=dev)
    max_len = int(np.diff(b.off.cpu().numpy()).max())

    def read():
        G.rows_device(plan, b.out, b.off, b.n, head, row_off, index, val, cell, lens, row_cap=R, root_type=G.LIST,
                      stream=b.stream, max_len=max_len)

    def verify(what):
        if int(row_off[-1].item()) != b.n_rows or (cell.view(torch.uint8)[:, :b.n_rows * 8:8] != 0).any().item():
            raise SystemExit("%s: the read side found %d rows of %d, or a cell that is not OK" % (
                what, int(row_off[-1].item()), b.n_rows))
        if not torch.equal(val[0, :b.n_rows], b.cols[0]["val"]):
            raise SystemExit("%s: the read side's first column is not the input" % what)

    return read, verify


def uniform(args):
    dev, ctx, stream = setup()
    out = {"iters": args.iters, "messages": N, "roofline_gbs": HBM_GBS, "sets": {}}
    for pname, (kinds, ids, slen) in PLANS.items():
        for rows in (4, 64, 1024):
            b = Batch(kinds, ids, np.full(N, rows, dtype=np.int64), slen, rows + slen, ctx, dev, stream)
            yard, ycheck, ymoved = vals_yardstick(b, ctx, dev)
            read, verify = reader(b, ctx, dev)
            t = timed(stream, args.iters, args.warmup, [b.call, b.sizing, yard, read])
            name = "%s x %d rows" % (pname, rows)
            b.check(name), ycheck(name), verify(name)
            res = {"rows": b.n_rows, "string_bytes": slen, "bytes_moved": b.moved, "arena_bytes": b.need, "call_ms": stats(t[0]),
                   "sizing_ms": stats(t[1]), "vals_struct_mode_ms": stats(t[2]), "read_side_ms": stats(t[3]),
                   "call_gbs": gbs(b.moved, mean(t[0])), "call_over_roofline": round(gbs(b.moved, mean(t[0])) / HBM_GBS, 4),
                   "call_over_vals_struct_mode": round(mean(t[0]) / mean(t[2]), 4),
                   "call_over_read_side": round(mean(t[0]) / mean(t[3]), 4)}
            out["sets"][name] = res
            print(name, res["call_ms"]["mean"], res["vals_struct_mode_ms"]["mean"], res["read_side_ms"]["mean"], flush=True)
            del b, yard, ycheck, read, verify
    out["method"] = ("HIP events around every launch; the call, its sizing call, values_device in struct mode over the same "
                     "rows as R messages and the read side (rows_device, root_type LIST, on the lists the call wrote) "
                     "alternate on one stream")
    return out


def skew(args):
    dev, ctx, stream = setup()
    kinds, ids, slen = PLANS["scalars+string"]
    counts = np.full(N, 4, dtype=np.int64)
    counts[N // 2] = 10000
    total = int(counts.sum())
    even = np.full(N, total // N, dtype=np.int64)
    even[:total - int(even.sum())] += 1
    bs, be = Batch(kinds, ids, counts, slen, 1, ctx, dev, stream), Batch(kinds, ids, even, slen, 1, ctx, dev, stream)
    ts, te = timed(stream, args.iters, args.warmup, [bs.call, be.call])
    bs.check("skewed"), be.check("even")
    assert bs.n_rows == be.n_rows and bs.need == be.need
    ss, se = stats(ts), stats(te)
    ratio = mean(ts) / mean(te)
    return {"iters": args.iters, "messages": N, "rows": bs.n_rows, "arena_bytes": bs.need, "skewed_ms": ss, "even_ms": se,
            "skewed_over_even": round(ratio, 4),
            "ratio_inside_both_p10_p90": bool(se["p10"] <= ss["mean"] <= se["p90"] and ss["p10"] <= se["mean"] <= ss["p90"]),
            "method": "HIP events around every launch; one list of 10 000 rows among 16 383 of 4, and an even batch of the same "
                      "rows and bytes, alternate on one stream"}


def chain(args):
    import torch
    from cut_bench import DISTINCT, SETS, gen_message
    from kids_bench import Batch as Msgs
    dev, ctx, stream = setup()
    n, items, slen = SETS["mid"]
    rng = random.Random(7)
    base = [gen_message(rng, items, slen) for _ in range(min(DISTINCT, n))]
    m = Msgs(torch, dev, base, n // len(base))
    from dynamicgo_amd import generic as G
    fid = G.PathFieldId
    rp = G.RowPlan([fid(4)], [([fid(1)], "int"), ([fid(2)], "str"), ([fid(3)], "str"), ([fid(4)], "int")], ctx=ctx)
    wp = G.RowValuePlan([10, 11, 11, 8], [1, 2, 3, 4], ctx=ctx)
    mp = G.EditManyPlan([], [fid(4)], G.EDIT_SET, ctx=ctx)
    head = torch.zeros((m.n, 4), dtype=torch.int32, device=dev)
    row_off = torch.zeros(m.n + 1, dtype=torch.int64, device=dev)
    G.rows_device(rp, m.src, m.in_off, m.n, head, row_off, stream=stream, max_len=m.max_len)
    torch.cuda.synchronize()
    R = int(row_off[-1].item())
    val, cell = (torch.zeros((4, R), dtype=torch.int64, device=dev) for _ in range(2))
    lens = torch.zeros((4, R), dtype=torch.int32, device=dev)
    need = m.total  # the lists are part of the messages
    ev = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    ev_off = torch.zeros(m.n + 1, dtype=torch.int64, device=dev)
    work = torch.zeros(wp.work_bytes(m.n, R), dtype=torch.uint8, device=dev)
    slot = (m.max_len + 79) & ~15
    d_oo = torch.arange(m.n + 1, dtype=torch.int64, device=dev) * slot
    out = torch.zeros(m.n * slot + 64, dtype=torch.uint8, device=dev)
    ol = torch.zeros(m.n, dtype=torch.int32, device=dev)
    ret = torch.zeros(m.n, dtype=torch.int64, device=dev)
    qty = [val[3]]

    def rows():
        G.rows_device(rp, m.src, m.in_off, m.n, head, row_off, None, val, cell, lens, row_cap=R, stream=stream, max_len=m.max_len)

    def torch_op():
        qty[0] = val[3] + 1

    def rvals():
        cols = [{"val": val[0]}, {"val": val[1], "len": lens[1], "src": m.src}, {"val": val[2], "len": lens[2], "src": m.src},
                {"val": qty[0]}]
        G.row_values_device(wp, cols, row_off, m.n, R, ev, ev_off, work, cap=need, stream=stream)

    def editm():
        G.edit_many_device(mp, m.src, m.in_off, m.n, [wp.wire_type], ev, ev_off, [0], out, d_oo, ol, ret, stream=stream)

    tr, tt, tv, tm = timed(stream, args.iters, args.warmup, [rows, torch_op, rvals, editm])
    if (ret & 0xFF).any().item() or (cell.view(torch.uint8)[:, ::8] != 0).any().item():  # the low byte is the status
        raise SystemExit("chain: an edit failed or a cell is not OK")
    if not torch.equal(ol.to(torch.int64), m.in_off[1:] - m.in_off[:-1]):
        raise SystemExit("chain: a message changed its length though only qty changed")
    whole = mean(tr) + mean(tt) + mean(tv) + mean(tm)
    return {"iters": args.iters, "messages": m.n, "rows": R, "thrift_bytes": m.total, "values_bytes": int(ev_off[-1].item()),
            "rows_ms": stats(tr), "torch_ms": stats(tt), "rvals_ms": stats(tv), "editm_ms": stats(tm), "chain_ms": round(whole, 5),
            "chain_over_editm_alone": round(whole / mean(tm), 4),
            "method": "HIP events around every step; rows_device (full call), a torch + 1 on qty, row_values_device and "
                      "edit_many_device on cut_bench's mid batch in turn on one stream; edit_many_device alone is the last step"}


PARTS = {"uniform": uniform, "skew": skew, "chain": chain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=sorted(PARTS))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in [args.only] if args.only else list(PARTS):
        res = PARTS[name](args)
        path = os.path.join(args.out_dir, "rvals_%s.json" % name)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({name: {k: v for k, v in res.items() if k != "sets"}}), flush=True)


if __name__ == "__main__":
    main()
