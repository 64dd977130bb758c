#!/usr/bin/env python3
"""Per-pair spread top-K (batch.topk_spread_by_pair / ops.topk_spread_by_pair, csrc/topk_spread.hip) at the bench's headline shapes:
default workload, 48 pairs per step, confidence=True, K = 2048.  One step's regrouped matches, then in one process:

  kernel   ops.topk_spread_by_pair for every --cells size (default 16 and 32 pixels) and ops.topk_by_pair - the yardstick - on the
           SAME tensors, preallocated outputs: device events around every launch, the minimum and median of --launches launches
           after 5, the variants alternating launch by launch
  spread   what the selection buys, on the host after the timed part: per pair the cells of every --cells grid that the plain
           top-K's rows touch, beside `occupied` and `top_count` of the spread selection (min / median / max over the pairs)

Prints ONE JSON line.

usage: bench_spread.py [--workload megadepth] [--pairs 48] [--K 2048] [--cells 16 32] [--side left] [--warmup 2] [--launches 50]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from benchlib.common import ITERS, WORKLOADS  # noqa: E402
from benchlib.nets import BenchNets  # noqa: E402


def spans(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--cells", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--side", choices=("left", "right"), default="left")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spread.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, default_pairs, _ = WORKLOADS[args.workload]
    pairs, K = args.pairs or default_pairs, args.K
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS, confidence=True)
    for _ in range(args.warmup + 1):
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, **kw)
        batch.topk_spread_by_pair(out, cap, K, args.cells[0], side=args.side)
    torch.cuda.synchronize()
    first = tuple(t.clone() for t in out["topk"]) + (out["topk_spread"][0].clone(),)
    ml, mr, off, mc = out["by_pair"]
    offs = out["summary"].cpu().tolist()
    counts = [offs[p + 1] - offs[p] for p in range(pairs)]

    # ---- the kernels alone, alternating ----------------------------------------------------------------------------------------
    grids = {c: (-(-32 * h // c), -(-32 * w // c)) for c in args.cells}
    dest = {c: tuple(torch.empty_like(t) for t in first) for c in args.cells}
    dest["topk"] = tuple(torch.empty_like(t) for t in first[:5])
    launch = {c: (lambda c=c: ops.topk_spread_by_pair(ml, mr, mc, off, K, c, grids[c], side=args.side, out=dest[c])) for c in args.cells}
    launch["topk"] = lambda: ops.topk_by_pair(ml, mr, mc, off, K, out=dest["topk"])
    ms = {v: [] for v in launch}
    for i in range(args.launches + 5):
        for v, fn in launch.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 5:
                ms[v].append(e0.elapsed_time(e1))
    assert all(torch.equal(a, b) for a, b in zip(dest[args.cells[0]], first))

    # ---- what it buys: the cells the plain top-K's rows touch, on the host ---------------------------------------------------------
    rows = dest["topk"][0 if args.side == "left" else 1].cpu()
    plain_count = dest["topk"][4].cpu().tolist()
    touched = {c: [] for c in args.cells}
    for c in args.cells:
        g0, g1 = grids[c]
        for p in range(pairs):
            pts = rows[p, :plain_count[p]]
            q = torch.where(pts > 0, pts.clamp(max=16777216.0), torch.zeros_like(pts)).to(torch.int64) // c
            ids = q[:, 0].clamp(max=g0 - 1) * g1 + q[:, 1].clamp(max=g1 - 1)
            touched[c].append(int(torch.unique(ids).numel()))
    result = {
        "tool": "bench_spread", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "K": K, "side": args.side,
        "max_cells": ops.topk_spread_max_cells(), "warmup": args.warmup, "launches": args.launches, "M": offs[pairs + 1],
        "matches_per_pair": spans(counts),
        "kernel_ms": {"topk_by_pair": {"min": min(ms["topk"]), "median": statistics.median(ms["topk"])}},
        "spread": {},
    }
    for c in args.cells:
        occ, cnt = dest[c][5].cpu().tolist(), dest[c][4].cpu().tolist()
        result["kernel_ms"]["topk_spread_by_pair_cell%d" % c] = {"min": min(ms[c]), "median": statistics.median(ms[c]),
                                                                 "median_over_topk": statistics.median(ms[c]) / statistics.median(ms["topk"])}
        result["spread"]["cell%d" % c] = {"cells": list(grids[c]), "occupied": spans(occ), "top_count": spans(cnt),
                                          "cells_touched_by_plain_topk": spans(touched[c])}
    result["spread"]["plain_top_count"] = spans(plain_count)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
