#!/usr/bin/env python3
"""Per-pair top-K (batch.topk_by_pair / ops.topk_by_pair, csrc/topk.hip) at the bench's headline shapes: default workload, 48 pairs
per step, confidence=True, K = 2048.  Three measurements in one process, after a warm-up:

  kernel   ops.topk_by_pair alone on one step's regrouped matches, preallocated outputs: device events around every launch, the
           minimum and median of --launches launches.  (Kernel times proper - topk_by_pair_kernel beside the bypair_* kernels - come
           from a separate `rocprofv3 --kernel-trace --stats` run of this script; no counters in that run.)
  step     batch.forward_pairs + batch.topk_by_pair (which regroups itself) against the same step that stops at
           batch.group_by_pair, alternating, device events around the whole step
  torch    the selection a caller without the kernel would write, on the SAME tensors: summary.cpu() (the offsets must reach the
           host first), then per pair torch.topk + three index gathers.  Host wall time from a synchronised device to a
           synchronised device, against the device path's wall time over the same span: ops.topk_by_pair + the one copy of the
           counts.  The comparison partner, not the code under test; its ranks among equal confidences are torch's, not the
           definition's (the sizes are checked, the bits are not).

Prints ONE JSON line.

usage: bench_topk.py [--workload megadepth] [--pairs 48] [--K 2048] [--steps 6] [--warmup 2] [--launches 50]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from benchlib.common import ITERS, WORKLOADS  # noqa: E402
from benchlib.nets import BenchNets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, default_pairs, _ = WORKLOADS[args.workload]
    pairs, K = args.pairs or default_pairs, args.K
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS, confidence=True)
    variants = ("group_by_pair", "topk_by_pair")
    times = {v: [] for v in variants}
    last = {}

    def step(v, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, **kw)
        if v == "topk_by_pair":
            batch.topk_by_pair(out, cap, K)
        else:
            batch.group_by_pair(out, cap)
        e1.record()
        torch.cuda.synchronize()
        if record:
            times[v].append(e0.elapsed_time(e1))
        last[v] = out

    for _ in range(args.warmup):
        for v in variants:
            step(v, False)
    for _ in range(args.steps):
        for v in variants:
            step(v, True)
    out = last["topk_by_pair"]
    assert torch.equal(out["summary"], last["group_by_pair"]["summary"])
    ml, mr, off, mc = out["by_pair"]
    offs = out["summary"].cpu().tolist()
    counts = [offs[p + 1] - offs[p] for p in range(pairs)]

    # ---- the kernel alone ------------------------------------------------------------------------------------------------------
    dest = tuple(torch.empty_like(t) for t in out["topk"])
    kernel_ms = []
    for i in range(args.launches + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.topk_by_pair(ml, mr, mc, off, K, out=dest)
        e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            kernel_ms.append(e0.elapsed_time(e1))
    assert all(torch.equal(a, b) for a, b in zip(dest, out["topk"]))

    # ---- the selection, wall time: device path against torch on the same tensors ---------------------------------------------------
    def device_path():
        both = torch.empty((2 * pairs + 4,), dtype=torch.int64, device=dev)
        both[:pairs + 4].copy_(out["summary"])
        d = dest[:4] + (both[pairs + 4:],)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.topk_by_pair(ml, mr, mc, both, K, out=d, pairs=pairs)
        host = both.cpu().tolist()                           # the one copy: offsets, M, P, status, counts
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, host[pairs + 4:]

    def torch_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = out["summary"].cpu().tolist()                    # the offsets must reach the host before anything can be sized
        picked = []
        for p in range(pairs):
            lo, hi = o[p], o[p + 1]
            c, idx = torch.topk(mc[lo:hi], min(K, hi - lo))
            picked.append((ml[lo:hi][idx], mr[lo:hi][idx], c, idx))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, [x[3].shape[0] for x in picked]

    wall = {"device": [], "torch": []}
    for i in range(args.launches + 5):
        td, cd = device_path()
        tt, ct = torch_path()
        assert cd == ct == [min(K, c) for c in counts]
        if i >= 5:
            wall["device"].append(td)
            wall["torch"].append(tt)

    med = {v: statistics.median(times[v]) for v in variants}
    result = {
        "tool": "bench_topk", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "K": K, "max_k": ops.topk_max_k(),
        "steps": args.steps, "warmup": args.warmup, "launches": args.launches, "M": offs[pairs + 1],
        "matches_per_pair": {"min": min(counts), "median": statistics.median(counts), "max": max(counts)},
        "kernel_ms": {"min": min(kernel_ms), "median": statistics.median(kernel_ms)},
        "step_ms": {v: {"median": med[v], "all": times[v]} for v in variants},
        "step_topk_over_group": med["topk_by_pair"] / med["group_by_pair"],
        "selection_wall_ms": {k: {"min": min(x), "median": statistics.median(x)} for k, x in wall.items()},
        "torch_over_device_wall": statistics.median(wall["torch"]) / statistics.median(wall["device"]),
        "torch_launches_per_step": 4 * pairs,
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
