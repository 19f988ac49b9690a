#!/usr/bin/env python3
"""Times the batched cut (dg_cut_batch_device, the reference's Value.MarshalTo)
device-resident, per route, next to a plain device-to-device copy of the same
input bytes (the ceiling: the cut is almost pure data movement).

    python tools/cut_bench.py [--iters 30] [--warmup 5] [--sets small,mid,large]

Three sets of generated messages over a wide order-like descriptor cut to a
narrow one (a dropped string and struct at the top, a list of structs each
narrowed by a dropped string, a map copied whole): about 200 B x 65 536, about
1 KB x 65 536, about 85 KB x 4 096. Per set: GB/s of Thrift in on the lane
route (cut_wave_min huge) and on the wave route (cut_wave_min 0), HIP events
around every launch, the median of --iters launches; the two routes' outputs
are compared byte for byte first. On the ~1 KB set cut_wave_min is swept over
256, 1024, 4096, 16384. Writes profiles/cut_bench.json and prints it.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"small": (65536, 1, 8), "mid": (65536, 10, 24), "large": (4096, 850, 32)}  # messages, items, string length
DISTINCT = 512  # generated messages per set, tiled to the set's size


def descriptors():
    from dynamicgo_amd import thrift as T
    b, F = T.builtin, T.FieldDescriptor
    item = T.struct_type("Item", [F(1, "sku", b("i64"), T.REQUIRED), F(2, "title", b("string"), T.OPTIONAL),
                                  F(3, "internal", b("string"), T.OPTIONAL), F(4, "qty", b("i32"), T.OPTIONAL)])
    item_n = T.struct_type("ItemN", [F(1, "sku", b("i64"), T.REQUIRED), F(2, "title", b("string"), T.OPTIONAL),
                                     F(4, "qty", b("i32"), T.OPTIONAL)])
    trace = T.struct_type("Trace", [F(1, "span", b("string"), T.OPTIONAL), F(2, "hops", T.list_of(b("i64")), T.OPTIONAL)])
    wide = T.struct_type("Order", [
        F(1, "id", b("i64"), T.REQUIRED), F(2, "name", b("string"), T.OPTIONAL), F(3, "debug", b("string"), T.OPTIONAL),
        F(4, "items", T.list_of(item), T.OPTIONAL), F(5, "attrs", T.map_of(b("string"), b("string")), T.OPTIONAL),
        F(6, "trace", trace, T.OPTIONAL), F(7, "score", b("double"), T.OPTIONAL)])
    narrow = T.struct_type("OrderN", [
        F(1, "id", b("i64"), T.REQUIRED), F(2, "name", b("string"), T.OPTIONAL), F(4, "items", T.list_of(item_n), T.OPTIONAL),
        F(5, "attrs", T.map_of(b("string"), b("string")), T.OPTIONAL), F(7, "score", b("double"), T.OPTIONAL)])
    return wide, narrow


def gen_message(rng, items, slen):
    def s(n):
        return struct.pack(">i", n) + rng.getrandbits(8 * n).to_bytes(n, "little")  # n >= 1

    def n_of(k):
        return rng.randrange(max(1, k // 2), k + k // 2 + 1)

    out = bytearray(b"\x0a\x00\x01" + struct.pack(">q", rng.getrandbits(62)))
    out += b"\x0b\x00\x02" + s(n_of(slen)) + b"\x0b\x00\x03" + s(n_of(2 * slen))
    k = n_of(items)
    out += b"\x0f\x00\x04\x0c" + struct.pack(">i", k)
    for _ in range(k):
        out += b"\x0a\x00\x01" + struct.pack(">q", rng.getrandbits(40)) + b"\x0b\x00\x02" + s(n_of(slen))
        out += b"\x0b\x00\x03" + s(n_of(slen)) + b"\x08\x00\x04" + struct.pack(">i", rng.randrange(100)) + b"\x00"
    out += b"\x0d\x00\x05\x0b\x0b" + struct.pack(">i", 2) + s(4) + s(n_of(slen)) + s(5) + s(n_of(slen))
    out += b"\x0c\x00\x06" + b"\x0b\x00\x01" + s(16) + b"\x0f\x00\x02\x0a" + struct.pack(">i", 3) + bytes(24) + b"\x00"
    out += b"\x04\x00\x07" + struct.pack(">d", rng.random()) + b"\x00"
    return bytes(out)


def d2d_copy_fn():
    """plain hipMemcpyAsync, device to device, from the HIP runtime torch loaded"""
    try:
        hip = C.CDLL("libamdhip64.so.7")
        f = hip.hipMemcpyAsync
    except (OSError, AttributeError):
        return None
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return lambda dst, src, n, s: f(dst, src, n, 3, s)  # hipMemcpyDeviceToDevice


def timed(fn, stream, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


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
    wide, narrow = descriptors()
    plan = G.CutPlan(wide, narrow, ctx=ctx)
    stream = torch.cuda.current_stream()
    copy = d2d_copy_fn()
    result = {"iters": args.iters, "sets": {}}
    for name in args.sets.split(","):
        n, items, slen = SETS[name]
        rng = random.Random(7)
        base = [gen_message(rng, items, slen) for _ in range(min(DISTINCT, n))]
        msgs = [base[i % len(base)] for i in range(n)]
        lens = np.fromiter((len(m) for m in msgs), dtype=np.int64, count=n)
        in_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=in_off[1:])
        out_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum((lens + 15) & ~15, out=out_off[1:])
        total = int(in_off[n])
        arena = np.frombuffer(b"".join(base) * (n // len(base)) + b"\0" * 16, dtype=np.uint8)
        d_src = torch.from_numpy(arena.copy()).to(dev)
        d_in, d_oo = torch.from_numpy(in_off).to(dev), torch.from_numpy(out_off).to(dev)
        d_out = torch.zeros(int(out_off[n]) + 64, dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
        d_cp = torch.empty(total, dtype=torch.uint8, device=dev)
        max_len = int(lens.max())

        def cut():
            G.marshal_to_device(plan, d_src, d_in, n, d_out, d_oo, d_ol, d_ret, 0, stream=stream, max_len=max_len)

        def gbs(ms):
            return round(total / (statistics.median(ms) * 1e-3) / 1e9, 2)

        row = {"messages": n, "thrift_bytes": total, "median_len": int(np.median(lens)), "max_len": max_len}
        outs = {}
        for route, wm in (("lane", 1 << 40), ("wave", 0)):
            ctx.set_knob("cut_wave_min", wm)
            d_out.zero_()
            ms = timed(cut, stream, args.iters, args.warmup)
            if int((d_ret != 0).sum().item()):
                raise SystemExit("%s, %s route: some messages failed" % (name, route))
            outs[route] = (d_out.clone(), d_ol.clone())
            row[route + "_gbs"] = gbs(ms)
            row[route + "_ms_median"] = round(statistics.median(ms), 5)
            row[route + "_ms_min"] = round(min(ms), 5)
        if not (torch.equal(outs["lane"][0], outs["wave"][0]) and torch.equal(outs["lane"][1], outs["wave"][1])):
            raise SystemExit("%s: the routes' outputs differ" % name)
        row["out_bytes"] = int(outs["lane"][1].sum().item())
        del outs
        if name == "mid":
            row["sweep_cut_wave_min_gbs"] = {}
            for wm in (256, 1024, 4096, 16384):
                ctx.set_knob("cut_wave_min", wm)
                row["sweep_cut_wave_min_gbs"][str(wm)] = gbs(timed(cut, stream, args.iters, args.warmup))
        s = stream.cuda_stream
        if copy is not None:
            ms = timed(lambda: copy(d_cp.data_ptr(), d_src.data_ptr(), total, s), stream, args.iters, args.warmup)
            row["copy"] = "hipMemcpyAsync device to device"
        else:
            ms = timed(lambda: d_cp.copy_(d_src[:total]), stream, args.iters, args.warmup)
            row["copy"] = "torch copy_ device to device"
        row["copy_gbs"] = gbs(ms)
        result["sets"][name] = row
        print(name, json.dumps(row), flush=True)
    result["method"] = ("HIP events around every launch on one stream, median of the launches; GB/s = Thrift bytes in "
                        "over that time; the copy moves the same input bytes once, device to device")
    plan.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cut_bench.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
