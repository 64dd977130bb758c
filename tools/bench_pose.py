#!/usr/bin/env python3
"""Per-pair relative pose (batch.pose_by_pair / ops.epipolar_pose_by_pair, csrc/pose.hip) at the verification bench's shape: default
workload, 48 pairs per step, confidence=True, H = 1024 hypotheses per pair verified on the top-K (K = 2048) with moments.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_pose.py --measure`  -> profiles/pose_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process after a warm-up step:
  kernel   ops.epipolar_pose_by_pair alone on one step's verified top-K (strided form, moments as the source), preallocated outputs
           with the front mask, device events around every call (a fill and one kernel), minimum and median of --launches calls
  torch    the same stage written with torch on the same device and tensors: torch.linalg.eigh of the moments, torch.linalg.svd of the
           refits, the four candidates and ONE batched masked count of the sign tests over [pairs, 4, K] in float32.  Wall time from
           a synchronised device to a synchronised device, against the device path's wall time over the same span.  The comparison
           partner, not the code under test; its E must agree with the kernel's and its best count with front_count
  step     batch.forward_pairs + topk_by_pair + hypothesize_by_pair + verify_by_pair + pose_by_pair against the same step without
           pose_by_pair, alternating

usage: bench_pose.py [--measure] [--workload megadepth] [--pairs 48] [--K 2048] [--H 1024] [--steps 4] [--warmup 2]
                     [--launches 30] [--torch-launches 3] [--no-torch] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_pose: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "pose_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def torch_pose(torch, tl, tr, inl, tn, moments, norm):
    """The partner.  tl, tr [pairs,K,2], inl [pairs,K] uint8, tn [pairs], moments [pairs,9,9], norm [pairs,8] on the device
    -> (E [pairs,3,3] float64, best count [pairs])."""
    pairs, K = inl.shape
    dev = tl.device
    e = torch.linalg.eigh(moments).eigenvectors[:, :, 0].reshape(pairs, 3, 3)
    U, _, Vh = torch.linalg.svd(e)
    U = torch.cat([U[:, :, :2], U[:, :, 2:] * torch.linalg.det(U)[:, None, None]], 2)
    Vh = torch.cat([Vh[:, :2, :], Vh[:, 2:, :] * torch.linalg.det(Vh)[:, None, None]], 1)
    D = torch.diag(torch.tensor([0.5 ** 0.5, 0.5 ** 0.5, 0.0], dtype=torch.float64, device=dev))
    W = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev)
    E = U @ D @ Vh
    R = torch.stack([U @ W @ Vh, U @ W.T @ Vh], 1).float()[:, [0, 1, 0, 1]]                  # [pairs,4,3,3]
    u = U[:, :, 2].float()
    t = torch.stack([u, u, -u, -u], 1)                                                        # [pairs,4,3]
    one = torch.ones((pairs, K, 1), device=dev)
    xl = torch.cat([(tl - norm[:, None, 0:2]) * norm[:, None, 2:4], one], 2)
    b = torch.cat([(tr - norm[:, None, 4:6]) * norm[:, None, 6:8], one], 2)[:, None].expand(pairs, 4, K, 3)
    a = torch.einsum("pcij,pkj->pcki", R, xl)
    tt = t[:, :, None, :].expand(pairs, 4, K, 3)
    c = torch.linalg.cross(a, b)
    dl, dr = (c * torch.linalg.cross(b, tt)).sum(3), (c * torch.linalg.cross(a, tt)).sum(3)
    used = (inl != 0) & (torch.arange(K, device=dev)[None, :] < tn[:, None])
    front = ((c * c).sum(3) > 0) & (dl > 0) & (dr > 0) & used[:, None, :]
    return E, front.sum(2).max(1).values


def measure(args):
    import torch
    from benchlib.common import ITERS, WORKLOADS
    from benchlib.nets import BenchNets
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, default_pairs, _ = WORKLOADS[args.workload]
    pairs, K, H = args.pairs or default_pairs, args.K, args.H
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS, confidence=True)
    thr = torch.full((pairs,), 0.01, device=dev)
    Hpx, Wpx = 32 * h, 32 * w
    norm = torch.tensor([Wpx / 2, Hpx / 2, 2.0 / Wpx, 2.0 / Wpx] * 2, device=dev).repeat(pairs, 1).contiguous()
    variants = ("verify", "verify+pose")
    times = {v: [] for v in variants}
    last = {}

    def step(v, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, **kw)
        batch.topk_by_pair(out, cap, K)
        models = batch.hypothesize_by_pair(out, cap, H, seed=7, norm=norm)
        batch.verify_by_pair(out, cap, models, thr, norm=norm, on="topk", moments=True)
        if v != "verify":
            batch.pose_by_pair(out, cap, norm=norm, swapped=True)
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
    out = last[variants[1]]
    tl, tr, _, _, tn = out["topk"]
    _, best, best_count, inl, moments = out["verified"]
    a = dict(matches_l=tl, matches_r=tr, inlier=inl, best_count=best_count, moments=moments, stride=K, counts=tn, norm=norm)
    dest = ops.epipolar_pose_by_pair(return_front=True, **a)
    again = tuple(torch.empty_like(t) for t in dest)
    ms = []
    for i in range(args.launches + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.epipolar_pose_by_pair(return_front=True, out=again, **a)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(dest, again)), "two calls differ"
    lens = tn.cpu().tolist()
    result = {"tool": "bench_pose", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "K": K, "H": H,
              "steps": args.steps, "warmup": args.warmup, "launches": args.launches,
              "matches_per_pair": {"min": min(lens), "median": statistics.median(lens), "max": max(lens)},
              "call_ms": {"min": min(ms), "median": statistics.median(ms)},
              "best_count": {"min": int(best_count.min()), "max": int(best_count.max())},
              "front_count": {"min": int(dest[3].min()), "max": int(dest[3].max())},
              "pairs_with_a_pose": int((dest[0].abs().sum((1, 2)) > 0).sum())}
    if not args.no_torch:
        wall = {"device": [], "torch": []}
        for i in range(args.torch_launches + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.epipolar_pose_by_pair(return_front=True, out=again, **a)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            E, top = torch_pose(torch, tl, tr, inl.view(pairs, K), tn, moments, norm)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= 1:
                wall["device"].append((t1 - t0) * 1e3)
                wall["torch"].append((t2 - t1) * 1e3)
        diff = torch.minimum((E - dest[0]).abs().amax((1, 2)), (E + dest[0]).abs().amax((1, 2)))
        result["wall_ms"] = {k: {"min": min(x), "median": statistics.median(x)} for k, x in wall.items()}
        result["torch_over_device_wall"] = statistics.median(wall["torch"]) / statistics.median(wall["device"])
        result["torch_over_device_call"] = statistics.median(wall["torch"]) / statistics.median(ms)
        result["torch_E_max_abs_difference"] = float(diff.max())
        result["torch_best_count_differences"] = int((top != dest[3]).sum())
    med = {v: statistics.median(times[v]) for v in variants}
    result["step_ms"] = {v: {"median": med[v], "all": times[v]} for v in variants}
    result["step_with_over_without"] = med[variants[1]] / med[variants[0]]
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--workload", default="megadepth")
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
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
