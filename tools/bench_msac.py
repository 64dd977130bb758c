#!/usr/bin/env python3
"""Per-pair MSAC scoring (ops.epipolar_score_msac_by_pair / ops.homography_score_msac_by_pair, csrc/epipolar.hip): the MSAC entry
timed against the count entry on identical inputs, and what ranking by gain instead of by count buys in the reference's own
metric, AUC@5/10/20 of max(err_R, err_t).

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_msac.py --measure`  -> profiles/msac_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.  --verify-parent / --verify-this: outputs of `tools/bench_verify.py --measure`
taken in the same session on the parent commit's build and on this one (the tool cannot check out a commit itself); the driver
folds their count-entry times into the JSON line as `count_entry_bench_verify`, which shows whether the count path moved.

--measure, one process:
  times      tools/bench_verify.py's batch shape in the strided form - --pairs pairs x --K matches (its on="topk" list) and x --K-all
             matches (the length of its on="all" lists, 35 063 - 38 749 per pair), --H random unit models per pair, thr 0.05 (every random model keeps a few per cent of the matches: no count is zero, every workgroup issues all
             of its atomics) - on the seeded scenes below.  After three warm-up calls, device events around every call (the fills,
             score, argmax and mask launches), minimum and median of --launches calls in milliseconds, the two entries alternating,
             for both families, moments=True, preallocated outputs.  counts of the two entries are compared bit for bit
  yardstick  tools/bench_pose_error.py's seeded scenes (--steps steps of --pairs scenes, K matches each, 40 % outliers, noise
             5e-4) and its 5-point chain: hypotheses -> verification with moments -> pose -> pose_error_by_pair -> pose_auc, run
             with the count entry and with the MSAC entry on the same scenes, seeds and sample budget (--samples per pair), at
             thr 2e-3 and at 1e-2.  docs/kernels.md 4.7 holds what an MI355X gave

usage: bench_msac.py [--measure] [--pairs 48] [--K 2048] [--K-all 36864] [--H 1024] [--steps 6] [--samples 64] [--launches 30]
                     [--out-dir profiles] [--step-timeout 300] [--verify-parent FILE ...] [--verify-this FILE ...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
THRS = (2e-3, 1e-2)
TIMING_THR = 0.05


def verify_times(paths):
    """The count entry's call times (ms) of bench_verify.py --measure outputs -> [{"all": {...}, "topk": {...}}]."""
    out = []
    for path in paths:
        with open(path) as f:
            d = json.loads([ln for ln in f if ln.startswith("{")][-1])
        out.append({on: r["call_ms"] for on, r in d["on"].items()})
    return out


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_msac: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    result = json.loads(line)
    if args.verify_parent or args.verify_this:
        result["count_entry_bench_verify"] = {"parent": verify_times(args.verify_parent), "this": verify_times(args.verify_this)}
        line = json.dumps(result)
    with open(os.path.join(out_dir, "msac_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def measure(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_msac.py: no GPU - nothing to measure")
    from bench_pose_error import scenes
    from pats_amd import ops
    pairs, K, H, steps, samples = args.pairs, args.K, args.H, args.steps, args.samples
    dev = torch.device("cuda")
    counts = torch.full((pairs,), K, dtype=torch.int64, device=dev)
    seg = dict(stride=K, counts=counts)
    entries = {"epipolar": {"count": ops.epipolar_score_by_pair, "msac": ops.epipolar_score_msac_by_pair},
               "homography": {"count": ops.homography_score_by_pair, "msac": ops.homography_score_msac_by_pair}}

    # ---- the yardstick: the 5-point chain with either ranking ------------------------------------------------------------------------
    yard = {}
    for thr_v in THRS:
        thr = torch.full((pairs,), thr_v, device=dev)
        running = {s: torch.empty(steps * pairs, dtype=torch.float64, device=dev) for s in ("count", "msac")}
        evaluated = {s: torch.zeros((), dtype=torch.int64, device=dev) for s in running}
        differ = torch.zeros((), dtype=torch.int64, device=dev)
        scratch = (torch.empty(pairs, dtype=torch.float64, device=dev), torch.empty(pairs, dtype=torch.float64, device=dev),
                   torch.empty(pairs, dtype=torch.int32, device=dev))
        for step in range(steps):
            ml, mr, T1 = (torch.from_numpy(a).to(dev) for a in scenes(np, pairs, K, 4000 + step))
            seed = torch.arange(pairs, dtype=torch.int64, device=dev) + 1000 * step
            models = ops.epipolar_hypotheses5_by_pair(ml, mr, samples, seed, **seg).view(pairs, 10 * samples, 3, 3)
            best = {}
            for s in running:
                ver = entries["epipolar"][s](ml, mr, models, thr, moments=True, **seg)
                best[s] = ver[1]
                pose = ops.epipolar_pose_by_pair(ml, mr, ver[3], ver[2], moments=ver[4], **seg)
                ops.pose_error_by_pair(pose[1], pose[2], T1, counts=counts, out=scratch[:2] + (running[s][step * pairs:(step + 1) * pairs], scratch[2]))
                evaluated[s] += (scratch[2] == 0).sum()
            differ += (best["count"] != best["msac"]).sum()
        y = {}
        for s in running:
            auc, below = ops.pose_auc(running[s])
            y[s] = {"auc@5": float(auc[0]), "auc@10": float(auc[1]), "auc@20": float(auc[2]), "below": below.tolist(),
                    "evaluated": int(evaluated[s]), "median_err": float(running[s].clamp(max=180.0).median())}
        y["pairs_with_another_winner"] = int(differ)
        yard["%g" % thr_v] = y

    # ---- the two entries on identical inputs, at the top-K list's length and at the full lists' ------------------------------------
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    models = torch.randn((pairs, H, 3, 3), generator=gen, device=dev)
    models = (models / models.reshape(pairs, H, 9).norm(dim=2)[:, :, None, None]).contiguous()
    thr = torch.full((pairs,), TIMING_THR, device=dev)
    times = {}
    for shape, rows in (("topk", K), ("all", args.K_all)):
        ml, mr, _ = (torch.from_numpy(a).to(dev) for a in scenes(np, pairs, rows, 4000))
        tseg = dict(stride=rows, counts=torch.full((pairs,), rows, dtype=torch.int64, device=dev))
        times[shape] = {"rows_per_pair": rows, "cells": pairs * rows * H}
        for fam, e in entries.items():
            dest = {s: tuple(torch.empty_like(t) for t in e[s](ml, mr, models, thr, moments=True, **tseg)) for s in e}
            ms = {s: [] for s in e}
            for i in range(args.launches + 3):
                for s in e:                                                       # alternating: the same clocks and caches for both
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    e[s](ml, mr, models, thr, moments=True, out=dest[s], **tseg)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= 3:
                        ms[s].append(e0.elapsed_time(e1))
            assert torch.equal(dest["count"][0], dest["msac"][0]), "the two entries' counts differ"
            r = {s: {"min": min(v), "median": statistics.median(v)} for s, v in ms.items()}
            r["msac_over_count"] = r["msac"]["median"] / r["count"]["median"]
            r["zero_counts"] = int((dest["count"][0] == 0).sum())
            r["pairs_with_another_winner"] = int((dest["count"][1] != dest["msac"][1]).sum())
            times[shape][fam] = r
    result = {"tool": "bench_msac", "pairs_per_step": pairs, "K": K, "H": H, "launches": args.launches, "timing_thr": TIMING_THR,
              "call_ms": times,
              "yardstick": {"steps": steps, "pairs": steps * pairs, "outliers": 0.4, "samples": samples, "chain": "5-point", "thr": yard}}
    for shape, t in times.items():
        for fam in entries:
            r = t[fam]
            print("%-4s %6d rows per pair %-10s count %.3f ms | msac %.3f ms | ratio %.2f"
                  % (shape, t["rows_per_pair"], fam, r["count"]["median"], r["msac"]["median"], r["msac_over_count"]))
    for t, y in yard.items():
        for s in ("count", "msac"):
            print("thr %-6s %-5s AUC@5/10/20 = %.4f / %.4f / %.4f  (%d of %d evaluated, median error %.3f degrees)"
                  % (t, s, y[s]["auc@5"], y[s]["auc@10"], y[s]["auc@20"], y[s]["evaluated"], steps * pairs, y[s]["median_err"]))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--K-all", type=int, default=36864, help="matches per pair of the second timing shape (bench_verify's on=\"all\" lists)")
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the driver's GPU step may take")
    ap.add_argument("--verify-parent", nargs="*", default=[], help="bench_verify.py --measure outputs of the parent commit's build")
    ap.add_argument("--verify-this", nargs="*", default=[], help="the same of this build, same session")
    args, _ = ap.parse_known_args()
    if args.measure:
        measure(args)
    else:
        driver(args, [a for a in sys.argv[1:] if a != "--measure"])


if __name__ == "__main__":
    main()
