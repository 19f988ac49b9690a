#!/usr/bin/env python3
"""Times the typed column writes (dg_vals_batch_device).

    python tools/vals_bench.py [--iters 200] [--warmup 20] [--only scalars|strings|lists|chain]

HIP events around every launch, the compared launches alternating in one run;
the mean and p10 / p90 over the launches are reported. The bytes counted come
from the shapes, by the code below.

scalars  65 536 x 4 scalar columns (Simple's byte, i64, double and i32 fields of
         the t2j-c2 batch of bench.py) encoded by one values_device call, beside
         columns_device reading the same four columns, which moves the same
         cells the other way.
strings  16 384 x one string of 64 / 1 024 / 16 384 bytes: the call, its sizing
         call (size pass + scan), the call under vals_lane_emit, and
         dg_pack_device_scan moving the same spans.
lists    16 384 x list<double> / list<i32> of 64 / 256 / 1 024 elements, read by
         columns_device + column_list_device from built messages and written
         back: the call, its sizing call, the call under vals_lane_emit, and
         dg_cols_list_device (scan + emit) with its sizing call on the same
         lists. Every written value is compared with the list's bytes in its
         message.
chain    cols + vals + editm on the t2j-c3 batch with one i32 column and one
         string column, timed per step; edit_many_device is also the yardstick:
         fed from an arena it costs the same launch, so the other two steps are
         what reading and encoding add.

Writes profiles/vals_<part>.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import HBM_GBS, list_batch, stats, timed  # noqa: E402

N_BUILT = 16384


def gbs(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def mean(x):
    return statistics.mean(x)


def faster(a, b):
    """whether launch a beats launch b by more than both p10 - p90 spreads"""
    sa, sb = stats(a), stats(b)
    return bool(sa["p90"] < sb["p10"])


def scalars(args):
    import torch
    import tget_bench as TB
    from dynamicgo_amd import generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx, _, _, n, d_thrift, d_toff = TB.make_batch("t2j-c2", dev)
    stream = torch.cuda.current_stream()
    t_max = int(np.diff(d_toff.cpu().numpy()).max())
    fields = [(1, "int", "byte"), (2, "int", "i64"), (3, "float64", "f64"), (4, "int", "i32")]
    cp = G.ColumnPlan([([G.PathFieldId(f)], ck) for f, ck, _ in fields], ctx=ctx)
    vp = G.ValuePlan([vk for _, _, vk in fields], ctx=ctx)
    d_val = torch.zeros((4, n), dtype=torch.int64, device=dev)
    d_cell = torch.zeros((4, n), dtype=torch.int64, device=dev)
    item = 1 + 8 + 8 + 4
    d_out = torch.zeros(n * item + 16, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(4 * n + 1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
    cols_in = [{"val": d_val[k]} for k in range(4)]

    def cols():
        G.columns_device(cp, d_thrift, d_toff, n, d_val, d_cell, None, stream=stream, max_len=t_max)

    def vals():
        G.values_device(vp, cols_in, n, d_out, d_off, d_st, cap=n * item, stream=stream)

    tc, tv = timed(stream, args.iters, args.warmup, [cols, vals])
    h_val, h_out = d_val.cpu().numpy(), d_out.cpu().numpy()[:n * item].reshape(n, item)
    if int(d_off[-1].item()) != n * item or d_st.any().item():
        raise SystemExit("scalars: the arena's end or a status is wrong")
    if not (h_out[:, 1:9].copy().view(">i8").ravel() == h_val[1]).all() or not (h_out[:, 0] == (h_val[0] & 0xFF)).all():
        raise SystemExit("scalars: the bytes written are not the values read")
    moved = n * (4 * 8 + item + 4 * 8 + 4)  # inputs read, bytes, offsets and statuses written
    cp.close()
    vp.close()
    return {"iters": args.iters, "messages": n, "columns": [vk for _, _, vk in fields], "bytes_moved": moved,
            "vals_ms": stats(tv), "cols_ms": stats(tc), "vals_over_cols": round(mean(tv) / mean(tc), 4),
            "vals_gbs": gbs(moved, mean(tv)), "vals_over_roofline": round(gbs(moved, mean(tv)) / HBM_GBS, 4),
            "method": "HIP events around every launch; values_device (closed form: one launch) and columns_device on the "
                      "same four scalar columns of the t2j-c2 batch alternate on one stream"}


def emit_report(res, payload, tcall, tsize, tlane, ctx_note=""):
    em = mean(tcall) - mean(tsize)
    res.update({"call_ms": stats(tcall), "sizing_ms": stats(tsize), "lane_emit_call_ms": stats(tlane),
                "call_gbs": gbs(payload, mean(tcall)), "lane_emit_call_gbs": gbs(payload, mean(tlane)),
                "emit_alone_ms": round(em, 5), "emit_alone_gbs": gbs(payload, em),
                "emit_alone_over_roofline": round(gbs(payload, em) / HBM_GBS, 4),
                "call_over_lane_emit": round(mean(tcall) / mean(tlane), 4),
                "shipped_faster_than_lane_emit_beyond_spread": faster(tcall, tlane)})


def strings(args):
    import torch
    from dynamicgo_amd import _lib, conv, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = conv.default_context()
    stream = torch.cuda.current_stream()
    L = _lib.lib()
    n = N_BUILT
    out = {"iters": args.iters, "roofline_gbs": HBM_GBS, "sets": {}}
    vp = G.ValuePlan(["str"], ctx=ctx)
    for ln in (64, 1024, 16384):
        src = torch.randint(0, 256, (n * ln + 16,), dtype=torch.uint8, device=dev)
        val = torch.arange(n, dtype=torch.int64, device=dev) * ln
        lens = torch.full((n,), ln, dtype=torch.int32, device=dev)
        need = n * (ln + 4)
        d_out = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_dst = torch.zeros(n * ln + 16, dtype=torch.uint8, device=dev)
        d_dst_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        col = [{"val": val, "len": lens, "src": src}]

        def call():
            G.values_device(vp, col, n, d_out, d_off, None, cap=need, stream=stream)

        def sizing():
            G.values_device(vp, col, n, None, d_off, None, cap=0, stream=stream)

        def lane():
            ctx.set_knob("vals_lane_emit", 1)
            call()
            ctx.set_knob("vals_lane_emit", 0)

        def pack():
            _lib.check(L.dg_pack_device_scan(ctx.h, src.data_ptr(), val.data_ptr(), lens.data_ptr(), n, d_dst.data_ptr(),
                                             d_dst_off.data_ptr(), stream.cuda_stream))

        tl, = timed(stream, 3, 1, [lane])  # a result to compare the shipped emit's with
        want = d_out.cpu().numpy().copy()
        d_out.zero_()
        tcall, tsize, tlane, tpack = timed(stream, args.iters, args.warmup, [call, sizing, lane, pack])
        call()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        h = got[:need].reshape(n, ln + 4)
        if not (got == want).all() or not (h[:, 4:].ravel() == src.cpu().numpy()[:n * ln]).all() or \
                not (h[:, :4] == np.frombuffer(ln.to_bytes(4, "big"), dtype=np.uint8)).all():
            raise SystemExit("strings x %d: the bytes written are wrong" % ln)
        payload = 2 * n * ln  # payload read plus written
        res = out["sets"]["string x %d" % ln] = {"messages": n, "payload_bytes_read_plus_written": payload,
                                                 "pack_scan_ms": stats(tpack), "pack_scan_gbs": gbs(payload, mean(tpack)),
                                                 "call_over_pack_scan": round(mean(tcall) / mean(tpack), 4)}
        emit_report(res, payload, tcall, tsize, tlane)
    vp.close()
    out["method"] = ("HIP events around every launch; the call (size pass, scan, head pass, body pass), the sizing call "
                     "(size pass + scan), the call under vals_lane_emit and dg_pack_device_scan over the same spans "
                     "alternate on one stream. emit alone = call - sizing call, by the means: head and body pass together")
    return out


def lists(args):
    import torch
    from dynamicgo_amd import conv, generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = conv.default_context()
    stream = torch.cuda.current_stream()
    n = N_BUILT
    out = {"iters": args.iters, "roofline_gbs": HBM_GBS, "sets": {}}
    for tname, et, width, ckind in (("list<double>", 4, 8, "list[float64]"), ("list<i32>", 8, 4, "list[int]")):
        vp = G.ValuePlan([G.VAL_LIST | et], ctx=ctx)
        for count in (64, 256, 1024):
            arena, in_off = list_batch(et, width, n, count, seed=count + et)
            d_thrift, d_in = torch.from_numpy(arena).to(dev), torch.from_numpy(in_off).to(dev)
            cp = G.ColumnPlan([([G.PathFieldId(1)], ckind)], ctx=ctx)
            d_val = torch.zeros((1, n), dtype=torch.int64, device=dev)
            d_cell = torch.zeros((1, n), dtype=torch.int64, device=dev)
            d_len = torch.zeros((1, n), dtype=torch.int32, device=dev)
            total = n * count
            d_eoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_elems = torch.zeros(total, dtype=torch.int64, device=dev)
            G.columns_device(cp, d_thrift, d_in, n, d_val, d_cell, d_len, stream=stream)
            need = n * (5 + count * width)
            d_out = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            col = [{"elem_off": d_eoff, "elems": d_elems}]

            def read():
                G.column_list_device(cp, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_eoff, d_elems, total, stream=stream)

            def read_sizing():
                G.column_list_device(cp, 0, d_thrift, n, d_val[0], d_cell[0], d_len[0], d_eoff, None, 0, stream=stream)

            def call():
                G.values_device(vp, col, n, d_out, d_off, None, cap=need, stream=stream)

            def sizing():
                G.values_device(vp, col, n, None, d_off, None, cap=0, stream=stream)

            def lane():
                ctx.set_knob("vals_lane_emit", 1)
                call()
                ctx.set_knob("vals_lane_emit", 0)

            read()
            tcall, tsize, tlane, tread, trs = timed(stream, args.iters, args.warmup, [call, sizing, lane, read, read_sizing])
            call()
            torch.cuda.synchronize()
            # every written value is the list's bytes in its message (behind the 3-byte field header, before STOP)
            msg = arena[:int(in_off[n])].reshape(n, -1)
            if not (d_out.cpu().numpy()[:need].reshape(n, -1) == msg[:, 3:-1]).all():
                raise SystemExit("%s x %d: the values written are not the lists read" % (tname, count))
            payload = total * (8 + width)  # 8 bytes read plus the element width written
            res = out["sets"]["%s x %d" % (tname, count)] = {"messages": n, "elements": total, "bytes_moved": payload,
                                                             "cols_list_call_ms": stats(tread), "cols_list_sizing_ms": stats(trs)}
            emit_report(res, payload, tcall, tsize, tlane)
            rd = mean(tread) - mean(trs)
            res["cols_list_emit_alone_gbs"] = gbs(payload, rd)
            res["emit_alone_over_cols_list_emit"] = round(res["emit_alone_ms"] / rd, 4)
            cp.close()
        vp.close()
    out["method"] = ("HIP events around every launch; the call, its sizing call, the call under vals_lane_emit, "
                     "dg_cols_list_device (scan + emit) and its sizing call alternate on one stream. bytes_moved = elements "
                     "x (8 read + element bytes written); emit alone = call - sizing call, by the means")
    return out


def chain(args):
    import torch
    import tget_bench as TB
    from dynamicgo_amd import generic as G
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx, _, _, n, d_thrift, d_toff = TB.make_batch("t2j-c3", dev)
    stream = torch.cuda.current_stream()
    toff = d_toff.cpu().numpy().astype(np.int64)
    t_max, total = int(np.diff(toff).max()), int(toff[-1])
    steps = [G.PathFieldId(4), G.PathFieldId(1)]  # NestingI64.I32, NestingI64.String
    cp = G.ColumnPlan([([steps[0]], "int"), ([steps[1]], "str")], ctx=ctx)
    vp = G.ValuePlan(["i32", "str"], ctx=ctx)
    ep = G.EditManyPlan([], steps, G.EDIT_SET, ctx=ctx)
    d_val = torch.zeros((2, n), dtype=torch.int64, device=dev)
    d_cell = torch.zeros((2, n), dtype=torch.int64, device=dev)
    d_len = torch.zeros((2, n), dtype=torch.int32, device=dev)
    cap = 8 * n + total
    d_v = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_voff = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
    out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((np.diff(toff) + 47) & ~15, out=out_off[1:])
    d_oo = torch.from_numpy(out_off).to(dev)
    d_out = torch.zeros(int(out_off[n]) + 16, dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ret = torch.zeros(n, dtype=torch.int64, device=dev)

    def cols():
        G.columns_device(cp, d_thrift, d_toff, n, d_val, d_cell, d_len, stream=stream, max_len=t_max)

    def vals():
        G.values_device(vp, [{"val": d_val[0]}, {"val": d_val[1], "len": d_len[1], "src": d_thrift}], n, d_v, d_voff, None,
                        cap=cap, stream=stream)

    def editm():
        G.edit_many_device(ep, d_thrift, d_toff, n, vp.wire_types, d_v, d_voff, [0, 0], d_out, d_oo, d_ol, d_ret,
                           stream=stream, max_len=t_max)

    tc, tv, te = timed(stream, args.iters, args.warmup, [cols, vals, editm])
    ret, ol = d_ret.cpu().numpy().view(np.uint64), d_ol.cpu().numpy()
    found = (d_cell.cpu().numpy().view(np.uint8).reshape(2, n, 8)[:, :, 0] == 0).all(axis=0)
    ok = (ret & 0xFF) == 0
    # identity: where both items were found the edited message is the message
    h_out, h_in = d_out.cpu().numpy(), d_thrift.cpu().numpy()
    for i in np.nonzero(found & ok)[0][:2000]:
        a, b, o = int(toff[i]), int(toff[i + 1]), int(out_off[i])
        if ol[i] != b - a or not (h_out[o:o + b - a] == h_in[a:b]).all():
            raise SystemExit("chain: message %d is not what was read" % i)
    for p in (cp, vp, ep):
        p.close()
    return {"iters": args.iters, "messages": n, "thrift_bytes": total, "ok_share": round(float(ok.mean()), 4),
            "both_found_share": round(float(found.mean()), 4), "value_bytes": int(d_voff[-1].item()),
            "cols_ms": stats(tc), "vals_ms": stats(tv), "editm_ms": stats(te),
            "chain_ms": round(mean(tc) + mean(tv) + mean(te), 5),
            "chain_over_editm_alone": round((mean(tc) + mean(tv) + mean(te)) / mean(te), 4),
            "vals_over_editm": round(mean(tv) / mean(te), 4),
            "method": "HIP events around every launch; columns_device, values_device and edit_many_device alternate on one "
                      "stream over the t2j-c3 batch (NestingI64.I32 and .String). edit_many_device reads the arena "
                      "values_device wrote: fed a precomputed arena it is the same launch, so its time is the yardstick"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("scalars", "strings", "lists", "chain"))
    args = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for name, fn in (("scalars", scalars), ("strings", strings), ("lists", lists), ("chain", chain)):
        if args.only and args.only != name:
            continue
        res = fn(args)
        with open(os.path.join(ROOT, "profiles", "vals_%s.json" % name), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
