#!/usr/bin/env python3
"""Times the typed column reads (dg_cols_batch_device, dg_cols_list_device).

    python tools/cols_bench.py [--iters 200] [--warmup 20]

1. The cell pass against the lookup, on the t2j-c2 and t2j-c3 batches of
   bench.py (tools/tget_bench.py's setup and paths): 1 and 4 scalar columns,
   alternating in one run with dg_tget_batch_device on the same paths with
   d_val_off / d_val_len on. The walk is the same code; a cell stores 8 + 8
   (+ 4) bytes where a record stores 16 + 8 + 4.
2. The list emit on built batches of list<double> and list<i32> (16 384
   messages of 64, 256 and 1 024 elements each): the scan and the emit of one
   dg_cols_list_device call, the same call with the "cols_full_search" knob, the
   sizing call (the scan alone), and as a yardstick from existing code the kids
   wide emit over the same lists (a DG_KIDS_F_COUNTED call: 32-byte records per
   child), all alternating in one run.

HIP events around every launch. Writes profiles/cols_cells.json and
profiles/cols_lists.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_GBS = 8000.0  # the MI355X's HBM3E peak, the roofline the emit is set against


def stats(ms):
    q = statistics.quantiles(ms, n=10)
    return {"mean": round(statistics.mean(ms), 5), "median": round(statistics.median(ms), 5), "min": round(min(ms), 5),
            "p10": round(q[0], 5), "p90": round(q[-1], 5)}


def timed(stream, iters, warmup, calls):
    """calls alternating on one stream, an event before each and one behind the last -> [ms per launch] per call"""
    import torch
    for _ in range(warmup):
        for f in calls:
            f()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(iters)]
    for row in ev:
        for e, f in zip(row, calls):
            e.record(stream)
            f()
        row[-1].record(stream)
    torch.cuda.synchronize()
    return [[row[j].elapsed_time(row[j + 1]) for row in ev] for j in range(len(calls))]


KIND_OF = {2: "bool", 3: "byte", 6: "int", 8: "int", 10: "int", 4: "float64", 11: "str", 13: "len", 14: "len", 15: "len"}


def cells(args):
    import torch
    import tget_bench as TB
    from dynamicgo_amd import generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"iters": args.iters, "configs": {}}
    mk = {"f": G.PathFieldId, "i": G.PathIndex}
    for cfg in ("t2j-c2", "t2j-c3"):
        ctx, flat, dh, n, d_thrift, d_toff = TB.make_batch(cfg, dev)
        toff = d_toff.cpu().numpy()
        t_max = int(np.diff(toff).max())
        stream = torch.cuda.current_stream()
        shallow, deep, four = TB.PATHS[cfg]
        res = out["configs"][cfg] = {"messages": n, "thrift_bytes": int(toff[-1]), "sets": {}}
        for name, paths in (("p1_shallow", [shallow]), ("p1_deep", [deep]), ("p4", four)):
            steps = [[mk[k](v) for k, v in p] for p in paths]
            ps = G.PathSet(steps, ctx=ctx)
            P = ps.count
            d_rec = torch.zeros((n, P, 4), dtype=torch.int32, device=dev)
            d_voff = torch.zeros(n * P, dtype=torch.int64, device=dev)
            d_vlen = torch.zeros(n * P, dtype=torch.int32, device=dev)

            def tget():
                G.get_by_path_device(ps, d_thrift, d_toff, n, d_rec, d_voff, d_vlen, stream=stream, max_len=t_max)

            tget()
            torch.cuda.synchronize()
            rec = d_rec.cpu().numpy().view(G.REC_DTYPE).reshape(n, P)
            # each column's kind from the wire type the lookup finds most often
            kinds = []
            for k in range(P):
                ok = rec[:, k]["status"] == 0
                t = int(np.bincount(rec[:, k]["type"][ok]).argmax()) if ok.any() else 8
                kinds.append(KIND_OF.get(t, "int"))
            plan = G.ColumnPlan(list(zip(steps, kinds)), ctx=ctx)
            d_val = torch.zeros((P, n), dtype=torch.int64, device=dev)
            d_cell = torch.zeros((P, n), dtype=torch.int64, device=dev)
            d_len = torch.zeros((P, n), dtype=torch.int32, device=dev)

            def cols():
                G.columns_device(plan, d_thrift, d_toff, n, d_val, d_cell, d_len, stream=stream, max_len=t_max)

            tc, tg = timed(stream, args.iters, args.warmup, [cols, tget])
            cell = d_cell.cpu().numpy().view(G.COL_CELL_DTYPE).reshape(P, n)
            if not ((cell["status"] == 0).T == (rec["status"] == 0)).all():
                raise SystemExit("%s %s: cells and records disagree on what was found" % (cfg, name))
            res["sets"][name] = {"paths": [["%s%d" % (k, v) for k, v in p] for p in paths], "kinds": kinds,
                                 "ok_share": round(float((cell["status"] == 0).mean()), 4),
                                 "cols_ms": stats(tc), "tget_ms": stats(tg),
                                 "cols_over_tget": round(statistics.mean(tc) / statistics.mean(tg), 4)}
            plan.close()
            ps.close()
    out["method"] = ("HIP events around every launch, the cell pass and the lookup (with d_val_off / d_val_len) "
                     "alternating on one stream; p10 / p90 over the launches are the spread")
    return out


def list_batch(et, width, n, count, seed):
    """n messages struct{1: list<et> of `count` random elements} as (arena uint8 with 16 spare bytes, in_off int64)"""
    rng = np.random.default_rng(seed)
    ln = 3 + 5 + count * width + 1
    m = np.zeros((n, ln), dtype=np.uint8)
    m[:, 0], m[:, 2], m[:, 3] = 15, 1, et
    m[:, 4:8] = np.frombuffer(int(count).to_bytes(4, "big"), dtype=np.uint8)
    m[:, 8:ln - 1] = rng.integers(0, 256, size=(n, count * width), dtype=np.uint8)
    return np.concatenate([m.ravel(), np.zeros(16, dtype=np.uint8)]), np.arange(n + 1, dtype=np.int64) * ln


def lists(args):
    import torch
    from dynamicgo_amd import conv, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = conv.default_context()
    stream = torch.cuda.current_stream()
    out = {"iters": args.iters, "roofline_gbs": HBM_GBS, "sets": {}}
    n = 16384
    wide_min = ctx.get_knob("kids_wide_min")
    ctx.set_knob("kids_wide_min", 1)  # the yardstick is the record-parallel kernel at every length
    for tname, et, width, kind in (("list<double>", 4, 8, "list[float64]"), ("list<i32>", 8, 4, "list[int]")):
        for count in (64, 256, 1024):
            arena, in_off = list_batch(et, width, n, count, seed=count + et)
            d_thrift, d_off = torch.from_numpy(arena).to(dev), torch.from_numpy(in_off).to(dev)
            path = [G.PathFieldId(1)]
            plan, ps = G.ColumnPlan([(path, kind)], ctx=ctx), G.PathSet([path], ctx=ctx)
            d_val = torch.zeros((1, n), dtype=torch.int64, device=dev)
            d_cell = torch.zeros((1, n), dtype=torch.int64, device=dev)
            d_len = torch.zeros((1, n), dtype=torch.int32, device=dev)
            G.columns_device(plan, d_thrift, d_off, n, d_val, d_cell, d_len, stream=stream)
            total = n * count
            d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_elems = torch.zeros(total, dtype=torch.int64, device=dev)
            head = torch.zeros((n, 4), dtype=torch.int32, device=dev)
            rec_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            recs = torch.zeros((total, 8), dtype=torch.int32, device=dev)
            G.children_device(ps, d_thrift, d_off, n, head, rec_off, None, 0, stream=stream)  # count and scan
            torch.cuda.synchronize()
            if int(rec_off[n].item()) != total:
                raise SystemExit("kids counts %d children, built %d" % (int(rec_off[n].item()), total))

            def emit():
                G.column_list_device(plan, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_eoff, d_elems, total,
                                     stream=stream)

            def emit_full():
                ctx.set_knob("cols_full_search", 1)
                emit()
                ctx.set_knob("cols_full_search", 0)

            def sizing():
                G.column_list_device(plan, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_eoff, None, 0, stream=stream)

            def kids():
                G.children_device(ps, d_thrift, d_off, n, head, rec_off, recs, total, counted=True, stream=stream)

            te, tf, ts, tk = timed(stream, args.iters, args.warmup, [emit, emit_full, sizing, kids])
            if int(d_eoff[n].item()) != total:
                raise SystemExit("the scan counts %d elements, built %d" % (int(d_eoff[n].item()), total))
            # spot check: the first and the last list against numpy
            h = d_elems.cpu().numpy()
            for i in (0, n - 1):
                a = int(in_off[i]) + 8
                raw = arena[a:a + count * width]
                want = raw.view(">u8").astype(np.uint64) if et == 4 else raw.view(">i4").astype(np.int64).view(np.uint64)
                if not (h[i * count:(i + 1) * count].view(np.uint64) == want).all():
                    raise SystemExit("%s x %d: message %d's elements are wrong" % (tname, count, i))
            moved = total * (width + 8)
            em = statistics.mean(te) - statistics.mean(ts)  # the emit kernel alone
            out["sets"]["%s x %d" % (tname, count)] = {
                "messages": n, "elements": total, "bytes_moved": moved,
                "list_call_ms": stats(te), "list_call_full_search_ms": stats(tf), "scan_ms": stats(ts),
                "kids_wide_emit_ms": stats(tk),
                "list_call_gbs": round(moved / (statistics.mean(te) * 1e-3) / 1e9, 1),
                "emit_alone_gbs": round(moved / (em * 1e-3) / 1e9, 1),
                "emit_alone_over_roofline": round(moved / (em * 1e-3) / 1e9 / HBM_GBS, 4),
                "kids_gbs": round(total * (width + 32) / (statistics.mean(tk) * 1e-3) / 1e9, 1),
            }
            plan.close()
            ps.close()
    ctx.set_knob("kids_wide_min", wide_min)
    out["method"] = ("HIP events around every launch; the list call (scan + emit), the same under cols_full_search, the "
                     "sizing call (scan alone) and the kids DG_KIDS_F_COUNTED emit alternate on one stream. bytes_moved = "
                     "elements x (element bytes read + 8 written); emit alone = list call - scan, by the means")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("cells", "lists"))
    args = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for name, fn in (("cells", cells), ("lists", lists)):
        if args.only and args.only != name:
            continue
        res = fn(args)
        with open(os.path.join(ROOT, "profiles", "cols_%s.json" % name), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
