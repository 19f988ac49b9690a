#!/usr/bin/env python3
"""Times the entry columns (dg_ents_batch_device, dg_ents_emit_device).

    python tools/ents_bench.py [--iters 100] [--warmup 10] [--out profiles]

Built batches of 16 384 messages struct{1: X}:
  variable stride  list<string> and map<string, i64> of 4, 16 and 64 entries
                   with strings of 8 and 64 bytes
  fixed stride     map<i32, double> of 64 and 1 024 entries
Alternating in one run on one stream: the cell pass, the sizing call (the scan
alone), the emit call (scan + emit) under every setting of the "ents_stage"
knob (0 = every lane stores its entries itself; 4, 8, 16 = that many staged in
LDS a round), and as the yardstick from existing code the kids calls on the
same node: the count call and the DG_KIDS_F_COUNTED call, which walks the same
container and stores a 32-byte record per child.

HIP events around every launch. Writes <out>/ents_var.json and
<out>/ents_fixed.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import stats, timed  # noqa: E402

N = 16384
STAGES = (0, 4, 8, 16)


def be32(v):
    return np.frombuffer(int(v).to_bytes(4, "big"), dtype=np.uint8)


def batch(shape, count, slen, seed):
    """N messages struct{1: X} of `count` random entries as (arena uint8 with 16 spare bytes, in_off int64);
    shape: "list<string>", "map<string,i64>" or "map<i32,double>"; slen: the strings' length"""
    rng = np.random.default_rng(seed)
    hdr = 5 if shape == "list<string>" else 6
    ent = {"list<string>": 4 + slen, "map<string,i64>": 4 + slen + 8, "map<i32,double>": 12}[shape]
    ln = 3 + hdr + count * ent + 1
    m = np.zeros((N, ln), dtype=np.uint8)
    m[:, 2] = 1
    if shape == "list<string>":
        m[:, 0], m[:, 3] = 15, 11
    else:
        m[:, 0], m[:, 3], m[:, 4] = 13, (11 if shape == "map<string,i64>" else 8), (10 if shape == "map<string,i64>" else 4)
    m[:, 3 + hdr - 4:3 + hdr] = be32(count)
    body = rng.integers(0, 256, size=(N, count, ent), dtype=np.uint8)
    if shape != "map<i32,double>":
        body[:, :, :4] = be32(slen)
    m[:, 3 + hdr:ln - 1] = body.reshape(N, count * ent)
    return np.concatenate([m.ravel(), np.zeros(16, dtype=np.uint8)]), np.arange(N + 1, dtype=np.int64) * ln


def run(args, shape, kind, count, slen, stages):
    import torch
    from dynamicgo_amd import conv, generic as G
    dev = torch.device("cuda", 0)
    ctx = conv.default_context()
    stream = torch.cuda.current_stream()
    arena, in_off = batch(shape, count, slen, seed=count * 131 + slen)
    d_thrift, d_off = torch.from_numpy(arena).to(dev), torch.from_numpy(in_off).to(dev)
    path = [G.PathFieldId(1)]
    plan, ps = G.EntryPlan([(path, kind)], ctx=ctx), G.PathSet([path], ctx=ctx)
    n, total = N, N * count
    d_val = torch.zeros((1, n), dtype=torch.int64, device=dev)
    d_cell = torch.zeros((1, n), dtype=torch.int64, device=dev)
    d_len = torch.zeros((1, n), dtype=torch.int32, device=dev)
    d_span = torch.zeros((1, n), dtype=torch.int32, device=dev)
    d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    keys, vals = (torch.zeros(total, dtype=torch.int64, device=dev) for _ in range(2))
    klens, vlens = (torch.zeros(total, dtype=torch.int32, device=dev) for _ in range(2))
    head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    rec_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    recs = torch.zeros((total * (1 if shape == "list<string>" else 2), 8), dtype=torch.int32, device=dev)

    def cells():
        G.entries_device(plan, d_thrift, d_off, n, d_val, d_cell, d_len, d_span, stream=stream)

    def sizing():
        G.entry_emit_device(plan, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_span[0], d_eoff, stream=stream)

    def emit_at(stage):
        def emit():
            ctx.set_knob("ents_stage", stage)
            G.entry_emit_device(plan, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_span[0], d_eoff, keys, klens, vals,
                                vlens, ent_cap=total, stream=stream)
        return emit

    def kids_count():
        G.children_device(ps, d_thrift, d_off, n, head, rec_off, None, 0, stream=stream)

    def kids():
        G.children_device(ps, d_thrift, d_off, n, head, rec_off, recs, recs.shape[0], counted=True, stream=stream)

    cells()
    kids_count()
    torch.cuda.synchronize()
    n_recs = int(rec_off[n].item())
    saved = ctx.get_knob("ents_stage")
    times = timed(stream, args.iters, args.warmup, [cells, sizing] + [emit_at(s) for s in stages] + [kids_count, kids])
    ctx.set_knob("ents_stage", saved)
    if int(d_eoff[n].item()) != total:
        raise SystemExit("%s x %d: the scan counts %d entries, built %d" % (shape, count, int(d_eoff[n].item()), total))
    # spot check: the last message's last entry against the bytes
    a = int(in_off[n]) - 1
    hv, hl = int(vals[total - 1].item()), int(vlens[total - 1].item())
    if shape == "map<i32,double>":
        ok = hv == int.from_bytes(arena[a - 8:a].tobytes(), "big", signed=True)
    elif shape == "map<string,i64>":
        ok = hv == int.from_bytes(arena[a - 8:a].tobytes(), "big", signed=True) and int(klens[total - 1].item()) == slen and \
            int(keys[total - 1].item()) == a - 8 - slen
    else:
        ok = hv == a - slen and hl == slen
    if not ok:
        raise SystemExit("%s x %d: the last entry is wrong" % (shape, count))
    mean = [statistics.mean(t) for t in times]
    res = {"messages": n, "entries": total, "thrift_bytes": int(in_off[n]), "kids_records": n_recs,
           "cell_pass_ms": stats(times[0]), "scan_ms": stats(times[1]),
           "kids_count_ms": stats(times[-2]), "kids_counted_ms": stats(times[-1])}
    for j, s in enumerate(stages):
        call = mean[2 + j]
        res["emit_call_stage%d_ms" % s] = stats(times[2 + j])
        res["emit_alone_stage%d_ms" % s] = round(call - mean[1], 5)
        res["emit_call_over_kids_counted_stage%d" % s] = round(call / mean[-1], 4)
        res["full_over_kids_full_stage%d" % s] = round((mean[0] + call) / (mean[-2] + mean[-1]), 4)
    plan.close()
    ps.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    method = ("HIP events around every launch; the cell pass, the sizing call (scan alone), the emit call (scan + emit) "
              "under each ents_stage, the kids count call and the kids DG_KIDS_F_COUNTED call alternate on one stream. "
              "emit alone = emit call - scan, by the means; full = cell pass + emit call against kids count + counted")
    var = {"iters": args.iters, "method": method, "sets": {}}
    for shape, kind in (("list<string>", "list[str]"), ("map<string,i64>", "strmap[int]")):
        for count in (4, 16, 64):
            for slen in (8, 64):
                var["sets"]["%s x %d, strings of %d" % (shape, count, slen)] = run(args, shape, kind, count, slen, STAGES)
    fixed = {"iters": args.iters, "method": method, "sets": {}}
    for count in (64, 1024):
        fixed["sets"]["map<i32,double> x %d" % count] = run(args, "map<i32,double>", "intmap[float64]", count, 0, (0,))
    for name, res in (("var", var), ("fixed", fixed)):
        with open(os.path.join(args.out, "ents_%s.json" % name), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
