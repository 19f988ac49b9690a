#!/usr/bin/env python3
"""Times map rows (dg_rows_map_batch_device) against list rows
(dg_rows_batch_device) on the same structs, device-resident.

    python tools/mrows_bench.py [--iters 30] [--warmup 5]

1. 16 384 messages of one map<i32, struct> of exactly 4 / 64 / 1 024 entries,
   the structs rows_bench's items {1: i64 sku, 2: string title, 3: string
   internal, 4: i32 qty}; beside each the same structs as one list<struct>
   (rows_bench's batch). Plans of 1 column (sku as int) and of 4 (sku, title,
   qty, LEN of the item itself).
2. The same with string keys of 8 bytes.
3. 16 384 messages of one map<i32, i64> of 1 024 entries, whose index entries
   and keys are arithmetic, beside list<i64> of 1 024.

Per batch and plan three calls each of the map plan and of the list plan, all six
alternating on one stream: heads + scan (the sizing call), heads + scan + index
(cells NULL; the map call with d_key and d_key_len) and the full call. HIP events
around every call. The ratio map / list is taken per round (the two calls of a
round run back to back) and reported as mean, p10 and p90 over the rounds.
Writes profiles/mrows_bench.json and prints it."""
import argparse
import json
import os
import random
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import stats, timed  # noqa: E402
from kids_bench import Batch  # noqa: E402
from rows_bench import item  # noqa: E402

# what the map calls were expected to cost against the list calls, written down before the first run: the walk reads
# one key more per entry (one more window beside the four fields of an item) and stores 12 bytes more per row; the
# cell pass is shared
EXPECTED = {
    "heads_scan": "1.05 - 1.25 with i32 keys, 1.1 - 1.35 with string keys (one more read per entry in the head's walk)",
    "heads_scan_index": "1.1 - 1.35 (the same read again and 28 instead of 16 bytes stored per row)",
    "full": "1.05 - 1.2 at 1 column, 1.02 - 1.1 at 4 (the unchanged cell pass dilutes it)",
    "fixed map<i32, i64> against list<i64>": "heads + scan about 1.0 (a multiplication in both); heads + scan + index "
                                             "1.5 - 2.5: the list's entries are stores alone, the map's need a 16-byte "
                                             "load per entry for the key and store 28 bytes instead of 16",
}


def map_message(rng, k, string_keys):
    key = (lambda j: struct.pack(">i", 8) + b"key%05d" % j) if string_keys else (lambda j: struct.pack(">i", j * 7 - 100))
    return (b"\x0d\x00\x04" + (b"\x0b" if string_keys else b"\x08") + b"\x0c" + struct.pack(">i", k) +
            b"".join(key(j) + item(rng) for j in range(k)) + b"\x00")


def list_message(rng, k):
    return b"\x0f\x00\x04\x0c" + struct.pack(">i", k) + b"".join(item(rng) for _ in range(k)) + b"\x00"


def ratio(a, b):
    """per-round ratios a / b: mean, p10, p90"""
    r = [x / y for x, y in zip(a, b)]
    q = statistics.quantiles(r, n=10)
    return {"mean": round(statistics.mean(r), 4), "p10": round(q[0], 4), "p90": round(q[-1], 4)}


def bench_pair(G, ctx, torch, stream, mb, lb, parent, keys, plans, args):
    """the map plan on batch mb against the list plan on batch lb (the same values), every plan"""
    dev = mb.src.device
    n = mb.n
    out = {"messages": n, "map_thrift_bytes": mb.total, "list_thrift_bytes": lb.total, "plans": {}}
    for pname, cols in plans.items():
        P = len(cols)
        with G.RowPlan(parent, cols, ctx=ctx, keys=keys) as mp, G.RowPlan(parent, cols, ctx=ctx) as lp:
            m_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            l_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            G.rows_device(mp, mb.src, mb.in_off, n, head, m_off, stream=stream)
            G.rows_device(lp, lb.src, lb.in_off, n, head, l_off, stream=stream)
            torch.cuda.synchronize()
            total = int(m_off[n].item())
            if total != int(l_off[n].item()) or not total:
                raise SystemExit("the map plan counts %d rows, the list plan %d" % (total, int(l_off[n].item())))
            index = torch.zeros((total, 4), dtype=torch.int32, device=dev)
            key = torch.zeros(total, dtype=torch.int64, device=dev)
            klen = torch.zeros(total, dtype=torch.int32, device=dev)
            val = torch.zeros((P, total), dtype=torch.int64, device=dev)
            cell = torch.zeros((P, total), dtype=torch.int64, device=dev)
            lens = torch.zeros((P, total), dtype=torch.int32, device=dev)

            def call(plan, b, off, level):
                kw = {"keys": key, "key_lens": klen} if plan is mp and level else {}
                if level == 0:
                    return lambda: G.rows_device(plan, b.src, b.in_off, n, head, off, stream=stream, max_len=b.max_len)
                if level == 1:
                    return lambda: G.rows_device(plan, b.src, b.in_off, n, head, off, index, row_cap=total, stream=stream,
                                                 max_len=b.max_len, **kw)
                return lambda: G.rows_device(plan, b.src, b.in_off, n, head, off, index, val, cell, lens, row_cap=total,
                                             stream=stream, max_len=b.max_len, **kw)

            calls = [call(p, b, o, lv) for lv in range(3) for p, b, o in ((mp, mb, m_off), (lp, lb, l_off))]
            t = timed(stream, args.iters, args.warmup, calls)
            ok = float((cell.view(torch.uint8)[:, :total * 8:8] == 0).float().mean().item())
            r = {"columns": P, "rows": total, "ok_cell_share": round(ok, 4)}
            for lv, name in enumerate(("heads_scan", "heads_scan_index", "full")):
                r["map_%s_ms" % name] = stats(t[2 * lv])
                r["list_%s_ms" % name] = stats(t[2 * lv + 1])
                r["map_over_list_%s" % name] = ratio(t[2 * lv], t[2 * lv + 1])
            r["map_full_mrow_s"] = round(total / (statistics.mean(t[4]) * 1e-3) / 1e6, 1)
            out["plans"][pname] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dynamicgo_amd import conv, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = conv.Context(dev.index)
    stream = torch.cuda.current_stream()
    fid = G.PathFieldId
    plans = {"p1": [([fid(1)], "int")],
             "p4": [([fid(1)], "int"), ([fid(2)], "str"), ([fid(4)], "int"), ([], "len")]}
    result = {"iters": args.iters, "expected_before_the_run": EXPECTED, "sets": {}}
    for keys in ("int", "str"):
        for k in (4, 64, 1024):
            mb = Batch(torch, dev, [map_message(random.Random(k * 64 + j), k, keys == "str") for j in range(64)], 16384 // 64)
            lb = Batch(torch, dev, [list_message(random.Random(k * 64 + j), k) for j in range(64)], 16384 // 64)
            name = "16384 x map<%s, struct> of %d" % ("string" if keys == "str" else "i32", k)
            result["sets"][name] = bench_pair(G, ctx, torch, stream, mb, lb, [fid(4)], keys, plans, args)
            print(name, json.dumps(result["sets"][name]), flush=True)
            del mb, lb
    body = bytes(range(256)) * 32
    mb = Batch(torch, dev, [b"\x0d\x00\x01\x08\x0a" + struct.pack(">i", 1024) +
                            b"".join(struct.pack(">i", j) + body[8 * j:8 * j + 8] for j in range(1024)) + b"\x00"], 16384)
    lb = Batch(torch, dev, [b"\x0f\x00\x01\x0a" + struct.pack(">i", 1024) + body + b"\x00"], 16384)
    name = "16384 x map<i32, i64> of 1024"
    result["sets"][name] = bench_pair(G, ctx, torch, stream, mb, lb, [fid(1)], "int", {"p1": [([], "int")]}, args)
    print(name, json.dumps(result["sets"][name]), flush=True)
    result["method"] = ("HIP events around every call; per batch and plan the map plan's and the list plan's three calls "
                        "(heads + scan; + index, the map call with d_key and d_key_len; the full call) alternate on one "
                        "stream; map / list per round, then mean, p10 and p90 over the rounds")
    result["not_measured"] = ["mixed map sizes in one batch", "a map of 10 000 entries holding one lane of the head and the index",
                              "the host entry end to end", "keys longer than 8 bytes", "d_key or d_key_len NULL",
                              "a wave per long map"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mrows_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
