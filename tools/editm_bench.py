#!/usr/bin/env python3
"""Times the batched many-edit (dg_editm_batch_device, the reference's SetMany)
device-resident against what it replaces: K chained single edits
(dg_edit_batch_device), each reading the output of the one before.

    python tools/editm_bench.py [--iters 30] [--warmup 5] [--sets small,mid,large]

The batches are cut_bench's (about 200 B x 65 536, about 1 KB x 65 536, about
85 KB x 4 096) with seven more string fields, 11 to 17, in front of the root's
STOP: cut_bench's root struct has only two strings, and the edit timed here
replaces K = 1, 2, 4 and 7 string fields of ONE struct by 40-byte values. Per set
and K, at the default knobs: one many-edit; the K chained edits (every stage in
exact slots, so its output is the next stage's input arena; the many-edit writes
the same slots and the two final arenas are compared byte for byte); the lookup
alone on the many-edit's K + 1 paths (dg_tget_batch_device); and a plain
device-to-device copy of the input bytes (the ceiling). The many-edit has no
knob that leaves its lookup out, so its splice is given as the call minus the
lookup alone. For K = 4 the lane route with 1, 4 and 16 lanes a message and the
wave route are timed too (edit_lanes, edit_wave_min). HIP events around every
call, the median of --iters. Writes profiles/editm_bench.json and prints it.
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
KS = (1, 2, 4, 7)
FIRST = 11  # the added string fields: FIRST .. FIRST + 6
VAL = struct.pack(">i", 36) + b"W" * 36


def with_strings(rng, m: bytes, slen: int):
    """m with seven string fields in front of its STOP; returns (message, the seven payload lengths)"""
    out, lens = bytearray(m[:-1]), []
    for k in range(7):
        n = rng.randrange(max(1, slen // 2), slen + slen // 2 + 1)
        out += struct.pack(">bhi", STRING, FIRST + k, n) + rng.getrandbits(8 * n).to_bytes(n, "little")
        lens.append(4 + n)
    return bytes(out + b"\x00"), lens


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
    defaults = {k: ctx.get_knob(k) for k in ("edit_lanes", "edit_wave_min")}
    result = {"iters": args.iters, "defaults": defaults, "sets": {}}
    for name in args.sets.split(","):
        n, items, slen = SETS[name]
        rng = random.Random(7)
        base, old = zip(*(with_strings(rng, gen_message(rng, items, slen), slen) for _ in range(min(DISTINCT, n))))
        reps = n // len(base)
        lens = np.tile(np.fromiter((len(m) for m in base), dtype=np.int64, count=len(base)), reps)
        old = np.tile(np.array(old, dtype=np.int64), (reps, 1))  # (n, 7): what each field's value takes today
        stage = [lens]  # stage[j]: every message's length after j fields were replaced
        for j in range(7):
            stage.append(stage[-1] + len(VAL) - old[:, j])
        offs = []
        for ln in stage:
            o = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(ln, out=o[1:])
            offs.append(torch.from_numpy(o).to(dev))
        total = int(lens.sum())
        cap = int(max(s.sum() for s in stage)) + 64
        d_src = torch.from_numpy(np.frombuffer(b"".join(base) * reps + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        bufs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        d_many = torch.zeros(cap, dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
        d_cp = torch.empty(total, dtype=torch.uint8, device=dev)
        max_len = int(max(s.max() for s in stage))
        d_val1 = torch.from_numpy(np.frombuffer(VAL + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        singles = [G.EditPlan([fid(FIRST + j)], G.EDIT_SET, ctx=ctx) for j in range(7)]

        def ms_of(fn):
            return round(statistics.median(timed(fn, stream, args.iters, args.warmup)), 5)

        def gbs(ms):
            return round(total / (ms * 1e-3) / 1e9, 2)

        row = {"messages": n, "thrift_bytes": total, "median_len": int(np.median(lens)), "max_len": max_len, "k": {}}
        for k in KS:
            plan = G.EditManyPlan([], [fid(FIRST + j) for j in range(k)], G.EDIT_SET, ctx=ctx)
            d_valk = torch.from_numpy(np.frombuffer(VAL * k + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
            d_rec = torch.zeros((n, k + 1, 4), dtype=torch.int32, device=dev)

            def many():
                G.edit_many_device(plan, d_src, offs[0], n, [STRING] * k, d_valk, None, [len(VAL)] * k, d_many, offs[k],
                                   d_ol, d_ret, stream=stream, max_len=max_len)

            def chain():
                src, src_off = d_src, offs[0]
                for j in range(k):
                    dst = bufs[j & 1]
                    G.edit_device(singles[j], src, src_off, n, STRING, d_val1, None, dst, offs[j + 1], d_ol, d_ret,
                                  val_len=len(VAL), stream=stream, max_len=max_len)
                    src, src_off = dst, offs[j + 1]

            for kn, v in defaults.items():
                ctx.set_knob(kn, v)
            kr = {}
            kr["many_ms"] = ms_of(many)
            want = (1 << k) - 1 << 8
            if int((d_ret != want).sum().item()):
                raise SystemExit("%s, K = %d: some messages were not replaced whole" % (name, k))
            kr["chained_ms"] = ms_of(chain)
            if int((d_ret != 0x100).sum().item()):
                raise SystemExit("%s, K = %d: a chained edit failed" % (name, k))
            end = int(stage[k].sum())
            if not torch.equal(d_many[:end], bufs[(k - 1) & 1][:end]):
                raise SystemExit("%s, K = %d: the many-edit's output differs from the chain's" % (name, k))
            with G.PathSet([[]] + [[fid(FIRST + j)] for j in range(k)], ctx=ctx) as ps:
                kr["lookup_ms"] = ms_of(lambda: G.get_by_path_device(ps, d_src, offs[0], n, d_rec, stream=stream, max_len=max_len))
            kr["splice_ms_by_difference"] = round(kr["many_ms"] - kr["lookup_ms"], 5)
            kr["many_gbs"], kr["chained_gbs"] = gbs(kr["many_ms"]), gbs(kr["chained_ms"])
            kr["speedup"] = round(kr["chained_ms"] / kr["many_ms"], 3)
            if k == 1:
                kr["dg_edit_ms"] = kr["chained_ms"]  # the chain of one is the single edit on the same batch
            if k == 4:
                kr["routes_ms"] = {}
                for route, wm, lanes in (("lane", 1 << 40, 1), ("lane4", 1 << 40, 4), ("lane16", 1 << 40, 16), ("wave", 0, 1),
                                         ("lane4_wave_min_1024", 1024, 4), ("lane4_wave_min_16384", 16384, 4)):
                    ctx.set_knob("edit_wave_min", wm)
                    ctx.set_knob("edit_lanes", lanes)
                    kr["routes_ms"][route] = ms_of(many)
                    if not torch.equal(d_many[:end], bufs[(k - 1) & 1][:end]):
                        raise SystemExit("%s, K = 4, %s: the output differs from the chain's" % (name, route))
                for kn, v in defaults.items():
                    ctx.set_knob(kn, v)
            row["k"][str(k)] = kr
            plan.close()
        s = stream.cuda_stream
        if copy is not None:
            row["copy_ms"] = ms_of(lambda: copy(d_cp.data_ptr(), d_src.data_ptr(), total, s))
            row["copy"] = "hipMemcpyAsync device to device"
        else:
            row["copy_ms"] = ms_of(lambda: d_cp.copy_(d_src[:total]))
            row["copy"] = "torch copy_ device to device"
        row["copy_gbs"] = gbs(row["copy_ms"])
        for p in singles:
            p.close()
        result["sets"][name] = row
        print(name, json.dumps(row), flush=True)
    result["method"] = ("HIP events around every call on one stream, median of the calls; many = one dg_editm_batch_device "
                        "replacing K string fields by 40-byte values; chained = K dg_edit_batch_device calls, each on the "
                        "output of the one before (exact slots); lookup = dg_tget_batch_device on the K + 1 paths; splice "
                        "= many - lookup; GB/s = Thrift bytes in over the time; the copy moves the input bytes once")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "editm_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
