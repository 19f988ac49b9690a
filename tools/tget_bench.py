#!/usr/bin/env python3
"""Times the batched path lookup (dg_tget_batch_device) against t2j
(dg_t2j_batch_device_ml) on the same Thrift batch, alternating the two in one
run: the t2j-c2 and t2j-c3 batches of bench.py (the C2 / C3 JSON batches of
dynamicgo_amd.workloads converted to Thrift once on the GPU).

    python tools/tget_bench.py [--config t2j-c3|t2j-c2] [--iters 200] [--warmup 20]

Writes profiles/tget_<config>.json: per path set the lookup's time per launch
(HIP events, mean and median over --iters launches), t2j's time over the same
alternation, their ratio, the bytes a lookup has to read (the headers on the
walk, counted by a host walk over a sample of the batch, not the message
size), and the host-to-host call next to the same run's copy bound.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXED = {2: 1, 3: 1, 4: 8, 6: 2, 8: 4, 10: 8}
STRING, STRUCT, MAP, SET, LIST = 11, 12, 13, 14, 15


class Walk:
    """The bytes and dependent reads of one lookup on a well-formed message:
    every header the walk has to look at (3 per field, 4 per string size, 5 / 6
    per list / map header), none of the bytes it steps over."""

    def __init__(self, b):
        self.b, self.p, self.bytes, self.reads = b, 0, 0, 0

    def hdr(self, k):
        self.bytes += k
        self.reads += 1
        self.p += k

    def skip(self, t, own_read=True):
        b = self.b
        if t in FIXED:
            self.p += FIXED[t]
        elif t == STRING:
            n = struct.unpack_from(">I", b, self.p)[0]
            self.bytes += 4
            self.reads += own_read  # a field's string size sits in the field header's window
            self.p += 4 + n
        elif t == STRUCT:
            while True:
                ft = b[self.p]
                if ft == 0:
                    self.hdr(1)
                    return
                self.hdr(3)
                self.skip(ft, False)
        elif t == MAP:
            kt, vt, n = b[self.p], b[self.p + 1], struct.unpack_from(">i", b, self.p + 2)[0]
            self.bytes += 6
            self.reads += own_read
            self.p += 6
            if kt in FIXED and vt in FIXED:
                self.p += n * (FIXED[kt] + FIXED[vt])
            else:
                for _ in range(n):
                    self.skip(kt)
                    self.skip(vt)
        else:
            vt, n = b[self.p], struct.unpack_from(">i", b, self.p + 1)[0]
            self.bytes += 5
            self.reads += own_read
            self.p += 5
            if vt in FIXED:
                self.p += n * FIXED[vt]
            else:
                for _ in range(n):
                    self.skip(vt)

    def lookup(self, path):
        """path of ("f", id) / ("i", index) steps; False when a step misses"""
        t = STRUCT
        for kind, v in path:
            if kind == "f":
                while True:
                    ft = self.b[self.p]
                    if ft == 0:
                        self.hdr(1)
                        return False
                    fid = struct.unpack_from(">h", self.b, self.p + 1)[0]
                    self.hdr(3)
                    if fid == v:
                        t = ft
                        break
                    self.skip(ft, False)
            else:
                t, n = self.b[self.p], struct.unpack_from(">i", self.b, self.p + 1)[0]
                self.hdr(5)
                if v >= n:
                    return False
                for _ in range(v):
                    self.skip(t)
        self.skip(t)
        return True


def make_batch(cfg, dev):
    """bench.py's t2j setup: the config's JSON batch -> Thrift, packed, on the device"""
    import torch
    from dynamicgo_amd import _lib, conv, workloads as W
    from dynamicgo_amd.thrift import flatten
    if cfg == "t2j-c2":
        td, msgs = W.simple_desc(), W.gen_flat_batch(random.Random(42), 65536)
    else:
        td, msgs = W.nesting_i64_desc(), W.gen_nested_batch(random.Random(43), 65536)
    arena, off = W.arena(msgs)
    flat = flatten(td)
    L = _lib.lib()
    ctx = conv.Context(dev.index)
    dh = ctx.desc_t2j(flat)
    n = len(off) - 1
    lens = np.diff(off).astype(np.int64)
    slots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((lens * 4 + 64 + 127) & ~127, out=slots[1:])
    d_json = torch.from_numpy(arena).to(dev)
    d_in = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_j2t = torch.empty(int(slots[-1]) + 64, dtype=torch.uint8, device=dev)
    d_oo = torch.from_numpy(slots).to(dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
    d_thrift = torch.zeros(int(slots[-1]) + 64, dtype=torch.uint8, device=dev)
    d_toff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.dg_j2t_batch_device(ctx.h, dh, flat.root_type, d_json.data_ptr(), d_in.data_ptr(), n, 1,
                                     d_j2t.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), d_ret.data_ptr(), None, s))
    _lib.check(L.dg_pack_device_scan(ctx.h, d_j2t.data_ptr(), d_oo.data_ptr(), d_ol.data_ptr(), n,
                                     d_thrift.data_ptr(), d_toff.data_ptr(), s))
    torch.cuda.synchronize()
    if int((d_ret != 0).sum().item()):
        raise SystemExit("the j2t setup pass failed on some messages")
    return ctx, flat, dh, n, d_thrift, d_toff


PATHS = {  # (shallow, deep, the P = 4 set)
    # NestingI64: I64; ListSimple[1].StringField (3 steps); SimpleStruct.StringField; Byte (the last field)
    "t2j-c3": ([("f", 6)], [("f", 2), ("i", 1), ("f", 5)],
               [[("f", 6)], [("f", 2), ("i", 1), ("f", 5)], [("f", 8), ("f", 5)], [("f", 14)]]),
    # Simple is flat: no path is deeper than one step; "deep" is the last field (every header walked)
    "t2j-c2": ([("f", 1)], [("f", 6)], [[("f", 1)], [("f", 2)], [("f", 5)], [("f", 6)]]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="t2j-c3", choices=sorted(PATHS))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample", type=int, default=4096, help="messages the host walk counts bytes on")
    args = ap.parse_args()
    import torch
    from dynamicgo_amd import _lib, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx, flat, dh, n, d_thrift, d_toff = make_batch(args.config, dev)
    L = _lib.lib()
    toff = d_toff.cpu().numpy().astype(np.uint64)
    thrift_bytes = int(toff[-1])
    h_thrift = d_thrift[:thrift_bytes + 64].cpu().numpy()
    tl = np.diff(toff).astype(np.int64)
    t_max = int(tl.max())
    jslots = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((tl * 3 + 64 + 127) & ~127, out=jslots[1:])
    d_out = torch.empty(int(jslots[-1]) + 64, dtype=torch.uint8, device=dev)
    d_jo = torch.from_numpy(jslots).to(dev)
    d_jl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_jr = torch.zeros(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def t2j():
        _lib.check(L.dg_t2j_batch_device_ml(ctx.h, dh, flat.root_type, d_thrift.data_ptr(), d_toff.data_ptr(), n, 0,
                                            d_out.data_ptr(), d_jo.data_ptr(), d_jl.data_ptr(), d_jr.data_ptr(), s,
                                            t_max))

    shallow, deep, four = PATHS[args.config]
    mk = {"f": G.PathFieldId, "i": G.PathIndex}
    result = {"config": args.config, "messages": n, "thrift_bytes": thrift_bytes, "max_len": t_max,
              "median_len": int(np.median(tl)), "iters": args.iters, "sets": {}}
    for name, paths in (("p1_shallow", [shallow]), ("p1_deep", [deep]), ("p4", four)):
        ps = G.PathSet([[mk[k](v) for k, v in p] for p in paths], ctx=ctx)
        P = ps.count
        d_rec = torch.zeros((n, P, 4), dtype=torch.int32, device=dev)

        def tget():
            G.get_by_path_device(ps, d_thrift, d_toff, n, d_rec, stream=stream, max_len=t_max)

        for _ in range(args.warmup):
            tget()
            t2j()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.iters)]
        for a, b, c in ev:  # lookup, then t2j, every iteration
            a.record(stream)
            tget()
            b.record(stream)
            t2j()
            c.record(stream)
        torch.cuda.synchronize()
        tg = [a.elapsed_time(b) for a, b, c in ev]
        tj = [b.elapsed_time(c) for a, b, c in ev]
        rec = d_rec.cpu().numpy().view(G.REC_DTYPE).reshape(n, P)
        # the bytes a lookup has to read, from a host walk over a sample
        step = max(1, n // args.sample)
        nb = nr = cnt = 0
        for i in range(0, n, step):
            m = h_thrift[int(toff[i]):int(toff[i + 1])].tobytes()
            for k, p in enumerate(paths):
                w = Walk(m)
                found = w.lookup(p)
                if found != (int(rec[i, k]["status"]) == 0) or (found and w.p != int(rec[i, k]["end"])):
                    raise SystemExit("message %d path %d: the host walk and the device disagree" % (i, k))
                nb += w.bytes
                nr += w.reads
            cnt += 1
        must = nb / cnt * n
        # host to host, and the copies alone over the same buffers
        h_off = toff.copy()
        h_rec = np.zeros((n, P), dtype=G.REC_DTYPE)
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            _lib.check(L.dg_tget_batch_host(ctx.h, ps.h, 12, h_thrift.ctypes.data, h_off.ctypes.data, n,
                                            h_rec.ctypes.data))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        if not (h_rec == rec).all():
            raise SystemExit("host and device entry points disagree")
        t_h = torch.from_numpy(h_thrift[:thrift_bytes])
        t_r = torch.empty(n * P * 16, dtype=torch.uint8)
        d_a = torch.empty(thrift_bytes, dtype=torch.uint8, device=dev)
        d_r = torch.empty(n * P * 16, dtype=torch.uint8, device=dev)
        cb = None
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_a.copy_(t_h)
            t_r.copy_(d_r)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            cb = dt if cb is None else min(cb, dt)
        tgm, tjm = statistics.mean(tg), statistics.mean(tj)
        result["sets"][name] = {
            "paths": [["%s%d" % (k, v) for k, v in p] for p in paths], "P": P,
            "found_share": [round(float((rec[:, k]["status"] == 0).mean()), 4) for k in range(P)],
            "tget_ms_mean": round(tgm, 5), "tget_ms_median": round(statistics.median(tg), 5),
            "tget_ms_min": round(min(tg), 5),
            "t2j_ms_mean": round(tjm, 5), "t2j_ms_median": round(statistics.median(tj), 5),
            "t2j_ms_min": round(min(tj), 5),
            "ratio_tget_over_t2j": round(tgm / tjm, 4),
            "must_read_bytes": int(must), "must_read_share_of_batch": round(must / thrift_bytes, 4),
            "dependent_reads_per_lookup": round(nr / cnt / P, 2), "sampled_messages": cnt,
            "must_read_gbs": round(must / (tgm * 1e-3) / 1e9, 2),
            "batch_gbs": round(thrift_bytes / (tgm * 1e-3) / 1e9, 2),
            "host_to_host_ms": round(best * 1e3, 3), "host_to_host_gbs": round(thrift_bytes / best / 1e9, 3),
            "copy_bound_ms": round(cb * 1e3, 3), "copy_bound_gbs": round(thrift_bytes / cb / 1e9, 3),
        }
        ps.close()
    result["method"] = ("HIP events around every launch, lookup and t2j alternating on one stream; host to host: "
                        "dg_tget_batch_host over pageable buffers, wall clock, best of 5; copy bound: the same "
                        "bytes up and the records down with nothing between, best of 5")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.path.join(ROOT, "profiles", "tget_%s.json" % args.config)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
