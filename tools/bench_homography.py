#!/usr/bin/env python3
"""Per-pair homographies (ops.homography_{hypotheses,score,refit}_by_pair: csrc/hypotheses.hip, csrc/epipolar.hip, csrc/homography.hip) at the verification bench's shape:
default workload, 48 pairs per step, confidence=True, H = 1024 hypotheses per pair, on="all" (every match) and on="topk" (K = 2048).

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_homography.py --measure`  -> profiles/homography_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process after one matching step that supplies the lists:
  stages   hypotheses, score (two fills + score + argmax + mask, moments on) and refit, each alone on preallocated outputs with
           device events around every call: minimum and median of --launches calls after 3.  The score kernel's arithmetic rate
           from the cells (participating or not) x 21 flop (9 FMA + 3 multiplies per cell, the threshold's included) against the
           fp32 vector peak.  Two calls of every stage give the same bits (asserted)
  torch    the same verification written per pair with torch on the same device and tensors: the offsets to the host, then per
           pair one einsum over [H, M_p, 3], the comparison, sum, argmax and the winner's row.  Wall time from a synchronised device
           to a synchronised device, against the device path's wall time over the same span.  The comparison partner, not the code
           under test: its verdicts may differ on cells within float32 rounding of the threshold
  scale    ops.epipolar_score_by_pair (batch.verify_by_pair's kernel) on the same lists with the same number of random models, the
           same session
The hypotheses come from the lists themselves, the threshold is wide (0.05 in normalised units): no winner is empty.

usage: bench_homography.py [--measure] [--workload megadepth] [--pairs 48] [--K 2048] [--H 1024] [--launches 30]
                           [--torch-launches 3] [--no-torch] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP32_VECTOR_PEAK = 157.3e12       # MI355X, flop/s
FLOP_PER_CELL = 21                # 9 FMA + 3 multiplies


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_homography: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "homography_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def torch_verify(torch, ml, mr, offs, models, thr, norm):
    """The partner: per pair, [H, M_p] tensors."""
    res = []
    for p in range(models.shape[0]):
        lo, hi = offs[p], offs[p + 1]
        n = norm[p]
        xl = torch.cat([(ml[lo:hi] - n[0:2]) * n[2:4], torch.ones((hi - lo, 1), device=ml.device)], 1)
        xr = (mr[lo:hi] - n[4:6]) * n[6:8]
        a = torch.einsum("hij,mj->hmi", models[p], xl)
        d0, d1 = a[..., 0] - xr[None, :, 0] * a[..., 2], a[..., 1] - xr[None, :, 1] * a[..., 2]
        w = a[..., 2] ** 2
        inl = (w > 0) & (d0 * d0 + d1 * d1 <= thr[p] * thr[p] * w)
        counts = inl.sum(1)
        best = torch.argmax(counts)
        res.append((counts, best, inl[best]))
    return res


def timed(torch, fn, launches):
    """-> (min, median) ms of `launches` calls after 3, device events around each."""
    ms = []
    for i in range(launches + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return {"min": min(ms), "median": statistics.median(ms)}


def measure(args):
    import torch
    from benchlib.common import ITERS, WORKLOADS
    from benchlib.nets import BenchNets
    if not torch.cuda.is_available():
        raise SystemExit("bench_homography.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, default_pairs, _ = WORKLOADS[args.workload]
    pairs, K, H = args.pairs or default_pairs, args.K, args.H
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, if_outdoor=outdoor, merge_new=True, iters=ITERS, confidence=True)
    batch.topk_by_pair(out, cap, K)
    torch.cuda.synchronize()
    thr = torch.full((pairs,), 0.05, device=dev)
    Hpx, Wpx = 32 * h, 32 * w
    norm = torch.tensor([Wpx / 2, Hpx / 2, 2.0 / Wpx, 2.0 / Wpx] * 2, device=dev).repeat(pairs, 1).contiguous()
    seed = torch.arange(pairs, dtype=torch.int64, device=dev) + 2024
    e_models = torch.randn((pairs, H, 3, 3), generator=gen, device=dev)
    e_models = (e_models / e_models.reshape(pairs, H, 9).norm(dim=2)[:, :, None, None]).contiguous()
    ml, mr, off, mc = out["by_pair"]
    tl, tr, tc, ti, tn = out["topk"]
    offs = out["summary"].cpu().tolist()
    lens = [offs[p + 1] - offs[p] for p in range(pairs)]
    top_lens = tn.cpu().tolist()
    forms = {"all": (dict(matches_l=ml, matches_r=mr, pair_off=out["summary"], pairs=pairs), sum(lens), False),
             "topk": (dict(matches_l=tl, matches_r=tr, stride=K, counts=tn), sum(top_lens), True)}
    result = {"tool": "bench_homography", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "K": K, "H": H,
              "M": offs[pairs + 1], "launches": args.launches,
              "matches_per_pair": {"min": min(lens), "median": statistics.median(lens), "max": max(lens)},
              "flop_per_cell": FLOP_PER_CELL, "fp32_vector_peak_flops": FP32_VECTOR_PEAK, "on": {}}
    same = lambda x, y: all(torch.equal(a_, b_) for a_, b_ in zip(x, y))       # noqa: E731
    for on, (a, rows, progressive) in forms.items():
        models = ops.homography_hypotheses_by_pair(H=H, seed=seed, norm=norm, progressive=progressive, **a)
        again_m = torch.empty_like(models)
        r = {"rows": rows, "cells": rows * H}
        r["hypotheses_ms"] = timed(torch, lambda: ops.homography_hypotheses_by_pair(H=H, seed=seed, norm=norm, progressive=progressive,
                                                                                    out=again_m, **a), args.launches)
        assert torch.equal(models, again_m)
        dest = ops.homography_score_by_pair(models=models, thr=thr, norm=norm, moments=True, **a)
        again = tuple(torch.empty_like(t) for t in dest)
        r["score_ms"] = timed(torch, lambda: ops.homography_score_by_pair(models=models, thr=thr, norm=norm, moments=True, out=again, **a),
                              args.launches)
        assert same(dest, again)                                              # two calls, the same bits (moments included)
        med = r["score_ms"]["median"]
        r["score_flops"] = r["cells"] * FLOP_PER_CELL / (med * 1e-3)
        r["score_share_of_fp32_vector_peak"] = r["score_flops"] / FP32_VECTOR_PEAK
        r["best_count"] = {"min": int(dest[2].min()), "max": int(dest[2].max())}
        fit = ops.homography_refit_by_pair(dest[2], moments=dest[4], norm=norm, return_pixel=True)
        again_f = tuple(torch.empty_like(t) for t in fit)
        r["refit_ms"] = timed(torch, lambda: ops.homography_refit_by_pair(dest[2], moments=dest[4], norm=norm, return_pixel=True, out=again_f),
                              args.launches)
        assert same(fit, again_f) and bool(torch.isfinite(fit[0]).all())
        e_dest = tuple(torch.empty_like(t) for t in dest)
        r["epipolar_score_ms"] = timed(torch, lambda: ops.epipolar_score_by_pair(models=e_models, thr=thr, norm=norm, moments=True,
                                                                                 out=e_dest, **a), args.launches)
        if not args.no_torch:
            fl, fr = (ml, mr) if on == "all" else (tl.reshape(-1, 2), tr.reshape(-1, 2))
            wall = {"device": [], "torch": []}
            for i in range(args.torch_launches + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.homography_score_by_pair(models=models, thr=thr, norm=norm, out=again[:4], **a)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if on == "all":
                    res = torch_verify(torch, fl, fr, out["summary"].cpu().tolist(), models, thr, norm)     # the offsets reach the host first
                else:
                    c = tn.cpu().tolist()
                    res = [torch_verify(torch, fl[p * K:p * K + c[p]], fr[p * K:p * K + c[p]], [0, c[p]], models[p:p + 1], thr[p:p + 1],
                                        norm[p:p + 1])[0] for p in range(pairs)]
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if i >= 1:
                    wall["device"].append((t1 - t0) * 1e3)
                    wall["torch"].append((t2 - t1) * 1e3)
            r["wall_ms"] = {k: {"min": min(x), "median": statistics.median(x)} for k, x in wall.items()}
            r["torch_over_device_wall"] = statistics.median(wall["torch"]) / statistics.median(wall["device"])
            r["torch_max_count_difference"] = max(int((res[p][0] - again[0][p]).abs().max()) for p in range(pairs))
            r["torch_same_best"] = "%d of %d" % (sum(int(res[p][1]) == int(again[1][p]) for p in range(pairs)), pairs)
        result["on"][on] = r
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--workload", default="megadepth")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--torch-launches", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds the driver's GPU step may take")
    args, _ = ap.parse_known_args()
    if args.measure:
        measure(args)
    else:
        driver(args, [a for a in sys.argv[1:] if a != "--measure"])


if __name__ == "__main__":
    main()
