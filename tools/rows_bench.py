#!/usr/bin/env python3
"""Times row columns (dg_rows_batch_device) device-resident.

    python tools/rows_bench.py [--iters 30] [--warmup 5] [--sets small,mid,large]

1. cut_bench's three batches (about 200 B x 65 536, about 1 KB x 65 536, about
   85 KB x 4 096), parent = field 4, the list of item structs {1: i64 sku,
   2: string title, 3: string internal, 4: i32 qty}, with 1 row column (sku as
   int) and with 4 (sku as int, title as str, qty as int, and LEN of the item
   itself, which a struct does not take: the walk still runs to the element's
   end. The item has no double field). Three rows calls: heads + scan (the
   sizing call), heads + scan + index (cells NULL, d_index given) and the full
   call; the index pass and the cell pass are their differences.
2. 16 384 messages of one list<struct> of exactly 4 / 64 / 1 024 such items.
3. 16 384 messages of one list<i64> of 1 024: the index pass writes its entries
   by arithmetic from the message's lane; beside it the kids emit on its lane
   route and on its record-parallel route.

Two yardsticks from existing code run in the same loop, alternating with the
rows calls: the full kids call on the same node (count + scan + emit of 32-byte
records) and the cols cell pass on parent[0].sub with the same kinds (one row
per message). HIP events around every call; mean, p10 and p90 over the calls.
Writes profiles/rows_bench.json and prints it."""
import argparse
import json
import os
import random
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import stats, timed  # noqa: E402
from cut_bench import DISTINCT, SETS, gen_message  # noqa: E402
from kids_bench import Batch  # noqa: E402


def item(rng, slen=8):
    def s(n):
        return struct.pack(">i", n) + rng.getrandbits(8 * n).to_bytes(n, "little")

    return (b"\x0a\x00\x01" + struct.pack(">q", rng.getrandbits(40)) + b"\x0b\x00\x02" + s(slen) + b"\x0b\x00\x03" + s(slen) +
            b"\x08\x00\x04" + struct.pack(">i", rng.randrange(100)) + b"\x00")


def struct_list_message(rng, k):
    return b"\x0f\x00\x04\x0c" + struct.pack(">i", k) + b"".join(item(rng) for _ in range(k)) + b"\x00"


def bench_node(G, ctx, torch, stream, b, parent, plans, args, kids_routes=False):
    """every rows call of every plan, the kids call and the cols cell pass on one batch"""
    dev = b.src.device
    n = b.n
    row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    out = {"messages": n, "thrift_bytes": b.total, "plans": {}}
    with G.PathSet([parent], ctx=ctx) as ps:
        G.children_device(ps, b.src, b.in_off, n, b.head, b.rec_off, None, 0, stream=stream, max_len=b.max_len)
        torch.cuda.synchronize()
        total = int(b.rec_off[n].item())
        recs = torch.zeros((max(total, 1), 8), dtype=torch.int32, device=dev)
        out["rows"] = total

        def kids():
            G.children_device(ps, b.src, b.in_off, n, b.head, b.rec_off, recs, total, stream=stream, max_len=b.max_len)

        for pname, cols in plans.items():
            P = len(cols)
            with G.RowPlan(parent, cols, ctx=ctx) as plan, G.ColumnPlan([(parent + [G.PathIndex(0)] + p, k) for p, k in cols],
                                                                         ctx=ctx) as cplan:
                head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
                index = torch.zeros((max(total, 1), 4), dtype=torch.int32, device=dev)
                val = torch.zeros((P, max(total, 1)), dtype=torch.int64, device=dev)
                cell = torch.zeros((P, max(total, 1)), dtype=torch.int64, device=dev)
                lens = torch.zeros((P, max(total, 1)), dtype=torch.int32, device=dev)
                cv = torch.zeros((P, n), dtype=torch.int64, device=dev)
                cc = torch.zeros((P, n), dtype=torch.int64, device=dev)
                cl = torch.zeros((P, n), dtype=torch.int32, device=dev)

                def sizing():
                    G.rows_device(plan, b.src, b.in_off, n, head, row_off, stream=stream, max_len=b.max_len)

                def indexed():
                    G.rows_device(plan, b.src, b.in_off, n, head, row_off, index, row_cap=total, stream=stream,
                                  max_len=b.max_len)

                def full():
                    G.rows_device(plan, b.src, b.in_off, n, head, row_off, index, val, cell, lens, row_cap=total,
                                  stream=stream, max_len=b.max_len)

                def cols_pass():
                    G.columns_device(cplan, b.src, b.in_off, n, cv, cc, cl, stream=stream, max_len=b.max_len)

                ts, ti, tf, tk, tc = timed(stream, args.iters, args.warmup, [sizing, indexed, full, kids, cols_pass])
                if int(row_off[n].item()) != total:
                    raise SystemExit("rows counts %d rows, kids %d children" % (int(row_off[n].item()), total))
                ok = float((cell.view(torch.uint8)[:, :total * 8:8] == 0).float().mean().item()) if total else 0.0
                m = {k: statistics.mean(v) for k, v in (("s", ts), ("i", ti), ("f", tf), ("k", tk), ("c", tc))}
                out["plans"][pname] = {
                    "columns": P, "ok_cell_share": round(ok, 4),
                    "rows_heads_scan_ms": stats(ts), "rows_heads_scan_index_ms": stats(ti), "rows_full_ms": stats(tf),
                    "kids_full_ms": stats(tk), "cols_cell_pass_parent0_ms": stats(tc),
                    "index_pass_ms": round(m["i"] - m["s"], 5), "cell_pass_ms": round(m["f"] - m["i"], 5),
                    "cell_pass_ns_per_row": round((m["f"] - m["i"]) * 1e6 / max(total, 1), 3),
                    "cols_ns_per_message": round(m["c"] * 1e6 / n, 3),
                    "heads_scan_index_over_kids_full": round(m["i"] / m["k"], 4),
                    "rows_full_mrow_s": round(total / (m["f"] * 1e-3) / 1e6, 1),
                }
        if kids_routes:
            routes = {}
            keep = ctx.get_knob("kids_wide_min")
            for route, wm in (("lane", 0), ("wide", 1)):
                ctx.set_knob("kids_wide_min", wm)
                routes["kids_emit_%s_ms" % route] = stats(timed(stream, args.iters, args.warmup, [
                    lambda: G.children_device(ps, b.src, b.in_off, n, b.head, b.rec_off, recs, total, counted=True,
                                              stream=stream, max_len=b.max_len)])[0])
            ctx.set_knob("kids_wide_min", keep)
            out["kids_emit_routes"] = routes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", default="small,mid,large")
    args = ap.parse_args()
    import torch
    from dynamicgo_amd import conv, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = conv.Context(dev.index)
    stream = torch.cuda.current_stream()
    fid = G.PathFieldId
    one = {"p1": [([fid(1)], "int")]}
    four = {"p4": [([fid(1)], "int"), ([fid(2)], "str"), ([fid(4)], "int"), ([], "len")]}
    result = {"iters": args.iters, "sets": {}}
    for name in [s for s in args.sets.split(",") if s]:
        n, items, slen = SETS[name]
        rng = random.Random(7)
        base = [gen_message(rng, items, slen) for _ in range(min(DISTINCT, n))]
        b = Batch(torch, dev, base, n // len(base))
        result["sets"][name] = bench_node(G, ctx, torch, stream, b, [fid(4)], {**one, **four}, args)
        print(name, json.dumps(result["sets"][name]), flush=True)
        del b
    for k in (4, 64, 1024):
        rng = random.Random(k)
        b = Batch(torch, dev, [struct_list_message(rng, k) for _ in range(64)], 16384 // 64)
        key = "16384 x list<struct> of %d" % k
        result["sets"][key] = bench_node(G, ctx, torch, stream, b, [fid(4)], {**one, **four}, args)
        print(key, json.dumps(result["sets"][key]), flush=True)
        del b
    b = Batch(torch, dev, [b"\x0f\x00\x01\x0a" + struct.pack(">i", 1024) + bytes(range(256)) * 32 + b"\x00"], 16384)
    key = "16384 x list<i64> of 1024"
    result["sets"][key] = bench_node(G, ctx, torch, stream, b, [fid(1)], {"p1": [([], "int")]}, args, kids_routes=True)
    print(key, json.dumps(result["sets"][key]), flush=True)
    result["method"] = ("HIP events around every call; the three rows calls (heads + scan; + index; the full call), the "
                        "full kids call on the same node and the cols cell pass on parent[0].sub with the same kinds "
                        "alternate on one stream; mean, p10 and p90 over the calls; index pass and cell pass are "
                        "differences of the means")
    result["not_measured"] = ["mixed list lengths in one batch", "a 10 000-item list holding one lane of the index pass",
                              "the host entry end to end", "an element-parallel index route for fixed-size elements"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rows_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
