#!/usr/bin/env python3
"""Times the batched edit (dg_edit_batch_device, the reference's SetByPath /
UnsetByPath) device-resident: the splice alone, the lookup + splice together,
the lookup alone on the same batch, and a plain device-to-device copy of the
same input bytes (the ceiling: the splice is pure data movement).

    python tools/edit_bench.py [--iters 30] [--warmup 5] [--sets small,mid,large]

The batches are cut_bench's: about 200 B x 65 536, about 1 KB x 65 536, about
85 KB x 4 096. The edits: a replace of the string field 2 by a value of the same
length (per-message values) and by one of another length (one 40-byte value for
all), an insert of the absent string field 9, an unset of the string field 3.
Per set and edit, on the lane route (edit_wave_min huge) with 1, 4 and 16 lanes
a message (edit_lanes) and on the wave route (edit_wave_min 0): GB/s of Thrift in, HIP events around every launch, the
median of --iters launches. The splice alone is timed with the edit_reuse_rec
knob (the launch skips the lookup and reuses the records of the launch before
it). The routes' outputs are compared byte for byte first. On the ~1 KB
set edit_wave_min is swept over 256, 1024, 4096, 16384 for the replace by
another length, at each edit_lanes. Writes profiles/edit_bench.json and prints it.
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

STRING = 11


def field2_len(m: bytes) -> int:
    """the length of string field 2's payload: the message starts with i64 field 1 (11 bytes), then field 2's header"""
    assert m[11:14] == b"\x0b\x00\x02"
    return struct.unpack(">i", m[14:18])[0]


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
    edits = (("replace_same_len", G.EDIT_SET, [fid(2)], "per_message"), ("replace_other_len", G.EDIT_SET, [fid(2)], 40),
             ("insert", G.EDIT_SET, [fid(9)], 16), ("unset", G.EDIT_UNSET, [fid(3)], None))
    result = {"iters": args.iters, "sets": {}}
    for name in args.sets.split(","):
        n, items, slen = SETS[name]
        rng = random.Random(7)
        base = [gen_message(rng, items, slen) for _ in range(min(DISTINCT, n))]
        reps = n // len(base)
        lens = np.fromiter((len(m) for m in base), dtype=np.int64, count=len(base)).repeat(1)
        lens = np.tile(lens, reps)
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=in_off[1:])
        total = int(in_off[n])
        d_src = torch.from_numpy(np.frombuffer(b"".join(base) * reps + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        d_in = torch.from_numpy(in_off).to(dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
        d_rec = torch.zeros((n, 2, 4), dtype=torch.int32, device=dev)
        d_cp = torch.empty(total, dtype=torch.uint8, device=dev)
        max_len = int(lens.max())

        def gbs(ms):
            return round(total / (statistics.median(ms) * 1e-3) / 1e9, 2)

        row = {"messages": n, "thrift_bytes": total, "median_len": int(np.median(lens)), "max_len": max_len, "edits": {}}
        for ename, op, path, val in edits:
            plan = G.EditPlan(path, op, ctx=ctx)
            d_val = d_vo = None
            val_len = 0
            if val == "per_message":
                vals = [struct.pack(">i", field2_len(m)) + b"V" * field2_len(m) for m in base]
                vo = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(np.tile(np.fromiter((len(v) for v in vals), dtype=np.int64, count=len(vals)), reps), out=vo[1:])
                d_val = torch.from_numpy(np.frombuffer(b"".join(vals) * reps + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
                d_vo = torch.from_numpy(vo).to(dev)
                val_len = max(len(v) for v in vals)
                slot = lens + np.diff(vo)
            elif val is not None:
                v = struct.pack(">i", val - 4) + b"W" * (val - 4)
                d_val = torch.from_numpy(np.frombuffer(v + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
                val_len = len(v)
                slot = lens + val_len + 3
            else:
                slot = lens
            out_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum((slot + 15) & ~15, out=out_off[1:])
            d_oo = torch.from_numpy(out_off).to(dev)
            d_out = torch.zeros(int(out_off[n]) + 64, dtype=torch.uint8, device=dev)

            def edit():
                G.edit_device(plan, d_src, d_in, n, STRING, d_val, d_vo, d_out, d_oo, d_ol, d_ret, val_len=val_len,
                              stream=stream, max_len=max_len)

            er = {}
            outs = {}
            for route, wm, lanes in (("lane", 1 << 40, 1), ("lane4", 1 << 40, 4), ("lane16", 1 << 40, 16), ("wave", 0, 1)):
                ctx.set_knob("edit_wave_min", wm)
                ctx.set_knob("edit_lanes", lanes)
                d_out.zero_()
                ms = timed(edit, stream, args.iters, args.warmup)
                if int(((d_ret & 0xFF) != 0).sum().item()):
                    raise SystemExit("%s, %s, %s route: some messages failed" % (name, ename, route))
                outs[route] = (d_out.clone(), d_ol.clone())
                er[route + "_total_gbs"] = gbs(ms)
                er[route + "_total_ms"] = round(statistics.median(ms), 5)
                ctx.set_knob("edit_reuse_rec", 1)  # the records of the launch above
                ms = timed(edit, stream, args.iters, args.warmup)
                ctx.set_knob("edit_reuse_rec", 0)
                er[route + "_splice_gbs"] = gbs(ms)
                er[route + "_splice_ms"] = round(statistics.median(ms), 5)
            for route in ("lane4", "lane16", "wave"):
                if not (torch.equal(outs["lane"][0], outs[route][0]) and torch.equal(outs["lane"][1], outs[route][1])):
                    raise SystemExit("%s, %s: the %s route's output differs from the lane route's" % (name, ename, route))
            er["out_bytes"] = int(outs["lane"][1].sum().item())
            del outs
            if name == "mid" and ename == "replace_other_len":
                er["sweep_edit_wave_min_splice_gbs"] = {}  # [edit_lanes][edit_wave_min]
                for lanes in (1, 4, 16):
                    ctx.set_knob("edit_lanes", lanes)
                    sw = er["sweep_edit_wave_min_splice_gbs"][str(lanes)] = {}
                    for wm in (256, 1024, 4096, 16384):
                        ctx.set_knob("edit_wave_min", wm)
                        edit()
                        ctx.set_knob("edit_reuse_rec", 1)
                        sw[str(wm)] = gbs(timed(edit, stream, args.iters, args.warmup))
                        ctx.set_knob("edit_reuse_rec", 0)
            # the lookup alone: the same (parent, full) set on the same batch
            with G.PathSet([path[:-1], path], ctx=ctx) as ps:
                ms = timed(lambda: G.get_by_path_device(ps, d_src, d_in, n, d_rec, stream=stream, max_len=max_len), stream,
                           args.iters, args.warmup)
            er["lookup_gbs"] = gbs(ms)
            er["lookup_ms"] = round(statistics.median(ms), 5)
            row["edits"][ename] = er
            plan.close()
        s = stream.cuda_stream
        if copy is not None:
            ms = timed(lambda: copy(d_cp.data_ptr(), d_src.data_ptr(), total, s), stream, args.iters, args.warmup)
            row["copy"] = "hipMemcpyAsync device to device"
        else:
            ms = timed(lambda: d_cp.copy_(d_src[:total]), stream, args.iters, args.warmup)
            row["copy"] = "torch copy_ device to device"
        row["copy_gbs"] = gbs(ms)
        row["copy_ms"] = round(statistics.median(ms), 5)
        result["sets"][name] = row
        print(name, json.dumps(row), flush=True)
    result["method"] = ("HIP events around every launch on one stream, median of the launches; GB/s = Thrift bytes in over "
                        "that time; total = lookup + splice as dg_edit_batch_device runs them, splice = the same call "
                        "with edit_reuse_rec (no lookup), lookup = dg_tget_batch_device on the (parent, full) set; the "
                        "copy moves the same input bytes once, device to device")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "edit_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
