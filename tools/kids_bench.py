#!/usr/bin/env python3
"""Times batched Children (dg_kids_batch_device, the reference's Node.Children
behind GetByPath) device-resident: the count pass, the scan and the emit pass
apart and together, against the path lookup of the same one path
(dg_tget_batch_device: a comparable walk) and a plain device-to-device copy of
the same input bytes.

    python tools/kids_bench.py [--iters 30] [--warmup 5] [--sets small,mid,large]

The batches are cut_bench's: about 200 B x 65 536, about 1 KB x 65 536, about
85 KB x 4 096. The node is field 4, the list of item structs, in one-level and
in recursive mode, and the message's root. HIP events around every call, the
median of --iters calls. The count pass alone is a call without records under
the kids_no_scan knob; count + scan the same call without the knob (the scan is
their difference); the emit pass alone a DG_KIDS_F_COUNTED call. kids_wide_min
is swept over 0 / 16 / 64 / 256 / 1024 on 4 096 messages holding a list<i64> of
10 000 elements and on the ~1 KB batch (node: field 6.2, a list<i64> of 3, and
field 4); since neither batch has nodes between 3 and 10 000 children, the two
routes are also timed on 16 384 messages of one list<i64> of 4 to 1 024
elements. Writes profiles/kids_bench.json and prints it.
"""
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

from cut_bench import DISTINCT, SETS, d2d_copy_fn, gen_message, timed  # noqa: E402

WIDE_SWEEP = (0, 16, 64, 256, 1024)


class Batch:
    def __init__(self, torch, dev, base, reps):
        n = len(base) * reps
        lens = np.tile(np.fromiter((len(m) for m in base), dtype=np.int64, count=len(base)), reps)
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=in_off[1:])
        self.n, self.total, self.max_len, self.median_len = n, int(in_off[n]), int(lens.max()), int(np.median(lens))
        self.src = torch.from_numpy(np.frombuffer(b"".join(base) * reps + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        self.in_off = torch.from_numpy(in_off).to(dev)
        self.head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self.rec_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)


def time_children(G, ctx, torch, stream, b, path, recurse, iters, warmup):
    """count / count + scan / emit / all of one (batch, path, mode), as ms medians and rates"""
    with G.PathSet([path], ctx=ctx) as ps:
        def call(recs, cap, counted=False):
            G.children_device(ps, b.src, b.in_off, b.n, b.head, b.rec_off, recs, cap, recurse=recurse, counted=counted,
                              stream=stream, max_len=b.max_len)

        call(None, 0)
        torch.cuda.synchronize()
        total = int(b.rec_off[b.n].item())
        ok = int((b.head.view(torch.uint8)[:, 15] == 0).sum().item())
        recs = torch.zeros((max(total, 1), 8), dtype=torch.int32, device=b.src.device)
        r = {"records": total, "ok_messages": ok}
        ctx.set_knob("kids_no_scan", 1)
        r["count_ms"] = statistics.median(timed(lambda: call(None, 0), stream, iters, warmup))
        ctx.set_knob("kids_no_scan", 0)
        r["count_scan_ms"] = statistics.median(timed(lambda: call(None, 0), stream, iters, warmup))
        r["scan_ms"] = r["count_scan_ms"] - r["count_ms"]
        r["emit_ms"] = statistics.median(timed(lambda: call(recs, total, True), stream, iters, warmup))
        r["all_ms"] = statistics.median(timed(lambda: call(recs, total), stream, iters, warmup))
        r["count_gbs"] = round(b.total / (r["count_ms"] * 1e-3) / 1e9, 2)
        r["all_gbs"] = round(b.total / (r["all_ms"] * 1e-3) / 1e9, 2)
        r["emit_mrec_s"] = round(total / (r["emit_ms"] * 1e-3) / 1e6, 1)
        r["all_mrec_s"] = round(total / (r["all_ms"] * 1e-3) / 1e6, 1)
        for k in ("count_ms", "count_scan_ms", "scan_ms", "emit_ms", "all_ms"):
            r[k] = round(r[k], 5)
        return r


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
    copy = d2d_copy_fn()
    fid = G.PathFieldId
    default_wide = ctx.get_knob("kids_wide_min")
    result = {"iters": args.iters, "kids_wide_min_default": default_wide, "sets": {}}
    batches = {}
    for name in args.sets.split(","):
        n, items, slen = SETS[name]
        rng = random.Random(7)
        base = [gen_message(rng, items, slen) for _ in range(min(DISTINCT, n))]
        b = batches[name] = Batch(torch, dev, base, n // len(base))
        row = {"messages": b.n, "thrift_bytes": b.total, "median_len": b.median_len, "max_len": b.max_len, "children": {}}
        for pname, path in (("f4", [fid(4)]), ("root", [])):
            for recurse in (False, True):
                row["children"]["%s, %s" % (pname, "recursive" if recurse else "one level")] = time_children(
                    G, ctx, torch, stream, b, path, recurse, args.iters, args.warmup)
        d_rec = torch.zeros((b.n, 1, 4), dtype=torch.int32, device=dev)
        with G.PathSet([[fid(4)]], ctx=ctx) as ps:
            ms = statistics.median(timed(lambda: G.get_by_path_device(ps, b.src, b.in_off, b.n, d_rec, stream=stream,
                                                                      max_len=b.max_len), stream, args.iters, args.warmup))
        row["tget_f4_ms"], row["tget_f4_gbs"] = round(ms, 5), round(b.total / (ms * 1e-3) / 1e9, 2)
        d_cp = torch.empty(b.total, dtype=torch.uint8, device=dev)
        s = stream.cuda_stream
        if copy is not None:
            ms = timed(lambda: copy(d_cp.data_ptr(), b.src.data_ptr(), b.total, s), stream, args.iters, args.warmup)
            row["copy"] = "hipMemcpyAsync device to device"
        else:
            ms = timed(lambda: d_cp.copy_(b.src[:b.total]), stream, args.iters, args.warmup)
            row["copy"] = "torch copy_ device to device"
        ms = statistics.median(ms)
        row["copy_ms"], row["copy_gbs"] = round(ms, 5), round(b.total / (ms * 1e-3) / 1e9, 2)
        del d_cp
        result["sets"][name] = row
        print(name, json.dumps(row), flush=True)
    # the wide route's threshold
    big = [b"\x0f\x00\x01\x0a" + struct.pack(">i", 10000) + bytes(range(256)) * 312 + bytes(128) + b"\x00"]
    sweep = {"list<i64> x 10000, 4096 messages": (Batch(torch, dev, big, 4096), [fid(1)])}
    if "mid" in batches:
        sweep["mid, f6.f2 (list<i64> of 3)"] = (batches["mid"], [fid(6), fid(2)])
        sweep["mid, f4 (list<struct>)"] = (batches["mid"], [fid(4)])
    result["sweep_kids_wide_min"] = {}
    for sname, (b, path) in sweep.items():
        sw = result["sweep_kids_wide_min"][sname] = {}
        for wm in WIDE_SWEEP:
            ctx.set_knob("kids_wide_min", wm)
            r = time_children(G, ctx, torch, stream, b, path, False, args.iters, args.warmup)
            sw[str(wm)] = {k: r[k] for k in ("records", "emit_ms", "all_ms", "emit_mrec_s", "all_gbs")}
        print(sname, json.dumps(sw), flush=True)
    # where the routes cross: 16 384 messages of one list<i64> of k elements, the emit pass on either route
    result["crossover_list_i64"] = {}
    for k in (4, 8, 16, 32, 64, 128, 256, 1024):
        m = [b"\x0f\x00\x01\x0a" + struct.pack(">i", k) + bytes(8 * k) + b"\x00"]
        b = Batch(torch, dev, m, 16384)
        row = result["crossover_list_i64"][str(k)] = {}
        for route, wm in (("lane", 0), ("wide", 1)):
            ctx.set_knob("kids_wide_min", wm)
            r = time_children(G, ctx, torch, stream, b, [fid(1)], False, args.iters, args.warmup)
            row[route + "_emit_ms"], row[route + "_all_ms"] = r["emit_ms"], r["all_ms"]
        del b
    print("crossover", json.dumps(result["crossover_list_i64"]), flush=True)
    ctx.set_knob("kids_wide_min", default_wide)
    result["method"] = ("HIP events around every call on one stream, median of the calls; GB/s = Thrift bytes in over that "
                        "time, Mrec/s = records out over it; count = a call without records under kids_no_scan, "
                        "count_scan = the same without the knob, scan = their difference, emit = a DG_KIDS_F_COUNTED "
                        "call, all = one call; tget = dg_tget_batch_device on the same one path; the copy moves the "
                        "same input bytes once, device to device")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "kids_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
