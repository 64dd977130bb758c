#!/usr/bin/env python3
"""The bench's step (batch.forward_pairs on BenchNets, default workload, 16 pairs per step: tools/bench_half_desc.py's size) with
and without confidence=True, including the device-side regroup by pair (batch.group_by_pair) - the whole hand-over.  The two
variants alternate inside one process after a warm-up; every step is timed with device events, and inside it the third-level
launch set (the `third` events of batch.third_stage) and the tail behind it (scatter, compaction, regroup).

Prints ONE JSON line.  Kernel times proper - third_fused3_conf_kernel against third_fused3_kernel, refine_scatter_conf_kernel
against refine_scatter_kernel, match_conf_kernel (an extra launch behind get_result_kernel), bypair_copy_conf_kernel against
bypair_copy_kernel - come from a separate `rocprofv3 --kernel-trace --stats` run of this script (no counters in that run).

usage: bench_confidence.py [--workload megadepth] [--pairs 16] [--steps 6] [--warmup 2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_confidence.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, _, _ = WORKLOADS[args.workload]
    pairs = args.pairs
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS)
    variants = {"plain": False, "confidence": True}
    times = {v: {"step": [], "third": [], "tail": []} for v in variants}
    counts = {}

    def step(v, record):
        ev = {} if record else None
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, events=ev, confidence=variants[v], **kw)
        e1.record()
        batch.group_by_pair(out, cap)
        e2.record()
        torch.cuda.synchronize()
        if record:
            t = times[v]
            t["step"].append(e0.elapsed_time(e2))
            t["third"].append(sum(a.elapsed_time(b) for a, b in ev["third"]))
            t["tail"].append(ev["third"][-1][1].elapsed_time(e2))
        counts[v] = (int(out["rows"].chunk_base[-1].item()), int(out["P"].item()), int(out["M"].item()))
        assert ("match_conf" in out) == variants[v] and len(out["by_pair"]) == (4 if variants[v] else 3)

    for _ in range(args.warmup):
        for v in variants:
            step(v, False)
    for _ in range(args.steps):
        for v in variants:
            step(v, True)
    assert counts["plain"] == counts["confidence"], counts
    result = {"tool": "bench_confidence", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "steps": args.steps,
              "warmup": args.warmup, "variants": {}}
    for v in variants:
        rows, P, M = counts[v]
        med = {k + "_ms": statistics.median(x) for k, x in times[v].items()}
        r = {"rows": rows, "P": P, "M": M, "pairs_per_s": pairs / (med["step_ms"] * 1e-3)}
        r.update(med)
        r["step_ms_all"] = times[v]["step"]
        result["variants"][v] = r
    a, b = result["variants"]["confidence"], result["variants"]["plain"]
    result["confidence_over_plain"] = {k: a[k + "_ms"] / b[k + "_ms"] for k in ("step", "third", "tail")}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
