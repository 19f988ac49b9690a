#!/usr/bin/env python3
"""Times the entry column writes (dg_evals_batch_device).

    python tools/evals_bench.py [--iters 200] [--warmup 20] [--only uniform|skew|long|chain]

HIP events around every launch, the compared launches alternating in one run;
the mean and p10 / p90 over the launches are reported. The bytes counted come
from the shapes, by the code below: the arena written plus the payload bytes
and the 8 + 4 bytes an entry's key and value arrays hold.

uniform  16 384 messages of one container each: list<string> and
         map<string,i64> x 4 / 16 / 64 entries with strings of 8 and 64 bytes,
         map<string,string> and map<i32,string> x 16 with strings of 64,
         map<i32,double> x 64 and 1 024. Beside each: its sizing call, the read
         side (entries_device + entry_emit_device) on the messages the call
         itself built in struct mode, and for the fixed-stride maps
         values_device writing list<i64> of the same count.
skew     one map<string,i64> of 10 000 entries among 16 383 of 4, against an
         even batch of the same entries and bytes: the ratio of the two calls
         shows whether the entry-parallel emit does what it is for.
long     list<string> x 1 with strings of 16 KiB, where one lane writes a whole
         payload, against values_device's STRING column (its wave-parallel body
         pass) on the same payloads: what a payload pass over entries would be
         compared with.
chain    ents -> evals -> editm on map<string,i64> x 16, timed per step;
         edit_many_device alone is the last step.

Writes profiles/evals_<part>.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cols_bench import HBM_GBS, stats, timed  # noqa: E402

N = 16384
LIST_STR = 0x4B


def map_kind(kt, vt):
    return 0x100 | kt << 4 | vt


def gbs(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def mean(x):
    return statistics.mean(x)


def column(kind, counts, slen, rng, dev):
    """(device column, entries, bytes read from it, bytes its containers take) for containers of counts[i] entries"""
    import torch
    kt, vt = ((kind >> 4) & 15, kind & 15) if kind & 0x100 else (0, 11)
    ne = int(counts.sum())
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    col, read, entry = {"ent_off": torch.from_numpy(off).to(dev), "n_ent": ne}, 8 * len(off), 0
    for t, side in ((kt, "key"), (vt, "val")):
        if not t:
            continue
        if t == 11:
            col[side] = torch.arange(ne, dtype=torch.int64, device=dev) * slen
            col[side + "_len"] = torch.full((ne,), slen, dtype=torch.int32, device=dev)
            col[side + "_src"] = torch.from_numpy(rng.integers(1, 255, size=ne * slen + 16, dtype=np.uint8)).to(dev)
            read, entry = read + ne * (12 + slen), entry + 4 + slen
        else:
            col[side] = torch.from_numpy(rng.integers(0, 2 ** 62, size=ne, dtype=np.int64)).to(dev)
            w = {2: 1, 3: 1, 4: 8, 6: 2, 8: 4, 10: 8}[t]
            read, entry = read + ne * 8, entry + w
    return col, ne, read, ne * entry + len(counts) * (6 if kind & 0x100 else 5)


class Batch:
    """one plan of one column with its outputs; .call / .sizing launch it on the stream"""

    def __init__(self, kind, counts, slen, seed, ctx, dev, stream, ids=None):
        import torch
        from dynamicgo_amd import generic as G
        self.G, self.stream, self.n = G, stream, len(counts)
        self.col, self.ne, self.read, body = column(kind, counts, slen, np.random.default_rng(seed), dev)
        self.need = body + (4 * self.n if ids else 0)
        self.plan = G.EntryValuePlan([kind], ids, ctx=ctx)
        self.out = torch.zeros(self.need + 16, dtype=torch.uint8, device=dev)
        self.off = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
        self.st = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.work = torch.zeros(self.plan.work_bytes(self.n, [self.ne]), dtype=torch.uint8, device=dev)
        self.moved = self.read + self.need + 9 * self.n

    def call(self):
        self.G.entry_values_device(self.plan, [self.col], self.n, self.out, self.off, self.work, self.st, cap=self.need,
                                   stream=self.stream)

    def sizing(self):
        self.G.entry_values_device(self.plan, [self.col], self.n, None, self.off, self.work, self.st, cap=0, stream=self.stream)

    def check(self, what):
        if int(self.off[-1].item()) != self.need or self.st.any().item():
            raise SystemExit("%s: the arena's end (%d, %d expected) or a status is wrong" % (what, int(self.off[-1].item()), self.need))


def setup():
    import torch
    from dynamicgo_amd import conv
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev, conv.default_context(), torch.cuda.current_stream()


def reader(b, ent_kind, ctx, dev, stream):
    """entries_device + entry_emit_device over the struct messages batch b (struct mode, field 1) has written"""
    import torch
    G = b.G
    b.call()
    torch.cuda.synchronize()
    plan = G.EntryPlan([([G.PathFieldId(1)], ent_kind)], ctx=ctx)
    val = torch.zeros((1, b.n), dtype=torch.int64, device=dev)
    cell = torch.zeros((1, b.n), dtype=torch.int64, device=dev)
    lens, spans = (torch.zeros((1, b.n), dtype=torch.int32, device=dev) for _ in range(2))
    ent_off = torch.zeros(b.n + 1, dtype=torch.int64, device=dev)
    keys, vals = (torch.zeros(b.ne + 1, dtype=torch.int64, device=dev) for _ in range(2))
    klens, vlens = (torch.zeros(b.ne + 1, dtype=torch.int32, device=dev) for _ in range(2))
    max_len = int(np.diff(b.off.cpu().numpy()).max())

    def read():
        G.entries_device(plan, b.out, b.off, b.n, val, cell, lens, spans, stream=stream, max_len=max_len)
        G.entry_emit_device(plan, 0, b.out, b.n, val[0], cell[0], lens[0], spans[0], ent_off, keys, klens, vals, vlens,
                            ent_cap=b.ne, stream=stream)

    def verify(what):
        if int(ent_off[-1].item()) != b.ne:
            raise SystemExit("%s: the read side found %d entries of %d" % (what, int(ent_off[-1].item()), b.ne))

    return read, verify, (ent_off, keys, klens, vals, vlens)


UNIFORM = [("list<string>", LIST_STR, "list[str]", c, s) for c in (4, 16, 64) for s in (8, 64)] + \
    [("map<string,i64>", map_kind(11, 10), "strmap[int]", c, s) for c in (4, 16, 64) for s in (8, 64)] + \
    [("map<string,string>", map_kind(11, 11), "strmap[str]", 16, 64), ("map<i32,string>", map_kind(8, 11), "intmap[str]", 16, 64),
     ("map<i32,double>", map_kind(8, 4), "intmap[float64]", 64, 0), ("map<i32,double>", map_kind(8, 4), "intmap[float64]", 1024, 0)]


def uniform(args):
    import torch
    dev, ctx, stream = setup()
    out = {"iters": args.iters, "messages": N, "roofline_gbs": HBM_GBS, "sets": {}}
    for name, kind, ent_kind, count, slen in UNIFORM:
        b = Batch(kind, np.full(N, count, dtype=np.int64), slen, count + slen, ctx, dev, stream, ids=[1])
        read, verify, _ = reader(b, ent_kind, ctx, dev, stream)
        calls = [b.call, b.sizing, read]
        fixed = kind == map_kind(8, 4)
        if fixed:  # the same count of i64 elements through vals
            G = b.G
            vp = G.ValuePlan([("list", "i64")], ctx=ctx)
            elems = torch.zeros(N * count, dtype=torch.int64, device=dev)
            v_out = torch.zeros(N * (5 + 8 * count) + 16, dtype=torch.uint8, device=dev)
            v_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            calls.append(lambda: G.values_device(vp, [{"elem_off": b.col["ent_off"], "elems": elems}], N, v_out, v_off,
                                                 cap=N * (5 + 8 * count), stream=stream))
        t = timed(stream, args.iters, args.warmup, calls)
        b.check(name)
        verify(name)
        res = {"entries": b.ne, "string_bytes": slen, "bytes_moved": b.moved, "arena_bytes": b.need, "call_ms": stats(t[0]),
               "sizing_ms": stats(t[1]), "read_side_ms": stats(t[2]), "call_gbs": gbs(b.moved, mean(t[0])),
               "call_over_roofline": round(gbs(b.moved, mean(t[0])) / HBM_GBS, 4),
               "call_over_read_side": round(mean(t[0]) / mean(t[2]), 4)}
        if fixed:
            res.update({"vals_list_i64_ms": stats(t[3]), "call_over_vals_list_i64": round(mean(t[0]) / mean(t[3]), 4)})
        out["sets"]["%s x %d, %d-byte strings" % (name, count, slen)] = res
        print(name, count, slen, res["call_ms"]["mean"], res["read_side_ms"]["mean"], flush=True)
    out["method"] = ("HIP events around every launch; the call, its sizing call, the read side (entries_device + "
                     "entry_emit_device on the struct messages the call wrote) and, for the fixed-stride maps, "
                     "values_device writing list<i64> of the same count alternate on one stream")
    return out


def skew(args):
    dev, ctx, stream = setup()
    kind = map_kind(11, 10)
    counts = np.full(N, 4, dtype=np.int64)
    counts[N // 2] = 10000
    total = int(counts.sum())
    even = np.full(N, total // N, dtype=np.int64)
    even[:total - int(even.sum())] += 1
    bs, be = Batch(kind, counts, 8, 1, ctx, dev, stream), Batch(kind, even, 8, 1, ctx, dev, stream)
    ts, te = timed(stream, args.iters, args.warmup, [bs.call, be.call])
    bs.check("skewed"), be.check("even")
    assert bs.ne == be.ne and bs.need == be.need
    return {"iters": args.iters, "messages": N, "entries": bs.ne, "arena_bytes": bs.need, "skewed_ms": stats(ts),
            "even_ms": stats(te), "skewed_over_even": round(mean(ts) / mean(te), 4),
            "method": "HIP events around every launch; one map<string,i64> of 10 000 entries among 16 383 of 4, and an even "
                      "batch of the same entries and bytes, alternate on one stream"}


def long_strings(args):
    import torch
    dev, ctx, stream = setup()
    slen = 16384
    b = Batch(LIST_STR, np.full(N, 1, dtype=np.int64), slen, 3, ctx, dev, stream)
    G = b.G
    vp = G.ValuePlan(["str"], ctx=ctx)
    v_out = torch.zeros(N * (4 + slen) + 16, dtype=torch.uint8, device=dev)
    v_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    col = {"val": b.col["val"], "len": b.col["val_len"], "src": b.col["val_src"]}
    te, tv = timed(stream, args.iters, args.warmup,
                   [b.call, lambda: G.values_device(vp, [col], N, v_out, v_off, cap=N * (4 + slen), stream=stream)])
    b.check("long")
    if not torch.equal(b.out[9:9 + slen], v_out[4:4 + slen]):
        raise SystemExit("long: the two writers disagree on the first payload")
    return {"iters": args.iters, "messages": N, "string_bytes": slen, "bytes_moved": b.moved, "evals_ms": stats(te),
            "vals_string_ms": stats(tv), "evals_gbs": gbs(b.moved, mean(te)), "vals_gbs": gbs(b.moved, mean(tv)),
            "evals_over_vals_string": round(mean(te) / mean(tv), 4),
            "method": "HIP events around every launch; list<string> x 1 of 16 KiB through entry_values_device (one lane per "
                      "payload) and the same payloads through values_device's STRING column (wave-parallel body pass) "
                      "alternate on one stream"}


def chain(args):
    import torch
    dev, ctx, stream = setup()
    kind, count, slen = map_kind(11, 10), 16, 8
    src = Batch(kind, np.full(N, count, dtype=np.int64), slen, 5, ctx, dev, stream, ids=[1])
    read, verify, (ent_off, keys, klens, vals, _) = reader(src, "strmap[int]", ctx, dev, stream)
    G = src.G
    ep = G.EntryValuePlan([kind], ctx=ctx)
    mp = G.EditManyPlan([], [G.PathFieldId(1)], G.EDIT_SET, ctx=ctx)
    need = src.need - 4 * N
    ev = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    ev_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    work = torch.zeros(ep.work_bytes(N, [src.ne]), dtype=torch.uint8, device=dev)
    msg = src.need // N
    slot = (msg + 79) & ~15
    d_oo = torch.arange(N + 1, dtype=torch.int64, device=dev) * slot
    out = torch.zeros(N * slot + 64, dtype=torch.uint8, device=dev)
    ol = torch.zeros(N, dtype=torch.int32, device=dev)
    ret = torch.zeros(N, dtype=torch.int64, device=dev)
    plus = [vals]

    def torch_op():
        plus[0] = vals + 1

    def evals():
        G.entry_values_device(ep, [{"ent_off": ent_off, "key": keys, "key_len": klens, "val": plus[0], "key_src": src.out,
                                    "n_ent": src.ne}], N, ev, ev_off, work, cap=need, stream=stream)

    def editm():
        G.edit_many_device(mp, src.out, src.off, N, ep.wire_types, ev, ev_off, [0], out, d_oo, ol, ret, stream=stream)

    tr, tt, tv, tm = timed(stream, args.iters, args.warmup, [read, torch_op, evals, editm])
    verify("chain")
    if (ret & 0xFF).any().item() or int(ev_off[-1].item()) != need:  # the low byte is the status
        raise SystemExit("chain: an edit failed or the values' arena is short")
    whole = mean(tr) + mean(tt) + mean(tv) + mean(tm)
    return {"iters": args.iters, "messages": N, "entries": src.ne, "ents_ms": stats(tr), "torch_ms": stats(tt),
            "evals_ms": stats(tv), "editm_ms": stats(tm), "chain_ms": round(whole, 5),
            "chain_over_editm_alone": round(whole / mean(tm), 4),
            "method": "HIP events around every step; ents (cell pass + emit), a torch + 1, entry_values_device and "
                      "edit_many_device on map<string,i64> x 16 in turn on one stream; edit_many_device alone is the last step"}


PARTS = {"uniform": uniform, "skew": skew, "long": long_strings, "chain": chain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=sorted(PARTS))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    for name in [args.only] if args.only else list(PARTS):
        res = PARTS[name](args)
        path = os.path.join(args.out_dir, "evals_%s.json" % name)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({name: {k: v for k, v in res.items() if k != "sets"}}), flush=True)


if __name__ == "__main__":
    main()
