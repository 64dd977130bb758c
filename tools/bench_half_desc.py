#!/usr/bin/env python3
"""The bench's step (batch.forward_pairs on BenchNets, default workload) with the DESCRIPTORS the three callbacks return -
mdesc0 / mdesc1 of the coarse and fine level, feat_f*_unfold of the third - handed over as fp32, as bf16 and f16 (the typed
cost builds read them as they are), and as bf16 turned .float() inside the callbacks (what a user whose heads run under autocast
had to do before ops.cost_ot / ops.third_level took half descriptors).  The variants alternate inside one process after a
warm-up; every step is timed with device events, and inside it the fine level's cost build and solve, the third level, and
the conversions.

The synthetic nets' gathers emit fp32, so a half variant rounds their output to the half type inside its callback: that cast
("round_*_ms") stands for the network head that would have produced the half tensor and is part of BOTH the typed and the
.float()-in-callback step - their difference is the .float() copies ("convert_*_ms") plus what the kernels gain or lose by
reading 2-byte operands.  bf16 and bf16_float_in_callback run on the same values (the fp32 kernels on them are the half
kernels' twins); fp32 runs on the unrounded ones.

Prints ONE JSON line.  Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

usage: bench_half_desc.py [--workload megadepth] [--pairs 16] [--steps 6] [--warmup 2]"""
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


class DescNets:
    """BenchNets whose callbacks return their descriptors in `dtype` (None: as the gathers emit them, fp32), optionally
    turned back with .float() before they are returned."""

    def __init__(self, nets, dtype=None, float_inside=False):
        self.nets, self.dtype, self.float_inside = nets, dtype, float_inside

    def __getattr__(self, name):
        return getattr(self.nets, name)

    def _pair(self, d0, d1, level):
        n = self.nets
        if self.dtype is None:
            return d0, d1
        e = n._timed("round_" + level)
        d0, d1 = d0.to(self.dtype), d1.to(self.dtype)
        if e is not None:
            e.record()
        if self.float_inside:
            e = n._timed("convert_" + level)
            d0, d1 = d0.float(), d1.float()
            if e is not None:
                e.record()
        return d0, d1

    def coarse(self, lefts, rights):
        r = self.nets.coarse(lefts, rights)
        return self._pair(r[0], r[1], "coarse") + tuple(r[2:])

    def fine(self, rows, new_left, new_right):
        r = self.nets.fine(rows, new_left, new_right)
        return self._pair(r[0], r[1], "fine") + tuple(r[2:])

    def third(self, rows, mk0, mk1, b_ids, P_dev):
        r = self.nets.third(rows, mk0, mk1, b_ids, P_dev)
        return self._pair(r[0], r[1], "third") + tuple(r[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=16, help="pairs per step (tools/bench_half_maps.py's size)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_desc.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, _, _ = WORKLOADS[args.workload]
    pairs = args.pairs
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS)
    variants = {"fp32": DescNets(nets), "bf16": DescNets(nets, torch.bfloat16), "f16": DescNets(nets, torch.float16),
                "bf16_float_in_callback": DescNets(nets, torch.bfloat16, float_inside=True)}
    tags = ("step", "fine_cost", "fine_ot", "third", "round_coarse", "round_fine", "round_third", "convert_coarse", "convert_fine",
            "convert_third")
    times = {v: {t: [] for t in tags} for v in variants}
    counts = {}

    def step(v, record):
        nets.ev = {} if record else None
        ev = {} if record else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = batch.forward_pairs(nets.lefts, nets.rights, variants[v], cap, events=ev, **kw)
        e1.record()
        torch.cuda.synchronize()
        if record:
            t = times[v]
            t["step"].append(e0.elapsed_time(e1))
            (f0, f1), mid = ev["fine"][0], ev["fine_mid"][0]
            t["fine_cost"].append(f0.elapsed_time(mid))
            t["fine_ot"].append(mid.elapsed_time(f1))
            t["third"].append(sum(a.elapsed_time(b) for a, b in ev["third"]))
            for tag, evs in nets.ev.items():
                if tag in t:
                    t[tag].append(sum(a.elapsed_time(b) for a, b in evs))
        counts[v] = (int(out["rows"].chunk_base[-1].item()), int(out["P"].item()), int(out["M"].item()))
        nets.ev = None

    for _ in range(args.warmup):
        for v in variants:
            step(v, False)
    for _ in range(args.steps):
        for v in variants:
            step(v, True)
    # bf16 descriptors and their .float() copies give the same bits, hence the same counts; fp32 / f16 hold other values
    assert counts["bf16"] == counts["bf16_float_in_callback"], counts
    result = {"tool": "bench_half_desc", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "steps": args.steps,
              "warmup": args.warmup, "variants": {}}
    for v in variants:
        rows, P, M = counts[v]
        med = {k + "_ms": statistics.median(x) for k, x in times[v].items() if x}
        r = {"rows": rows, "P": P, "M": M, "pairs_per_s": pairs / (med["step_ms"] * 1e-3)}
        r.update(med)
        r["step_ms_all"] = times[v]["step"]
        result["variants"][v] = r
    a, b = result["variants"]["bf16"], result["variants"]["bf16_float_in_callback"]
    result["bf16_typed_over_float_in_callback"] = {"step": a["step_ms"] / b["step_ms"], "fine_cost": a["fine_cost_ms"] / b["fine_cost_ms"],
                                                   "third": a["third_ms"] / b["third_ms"]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
