#!/usr/bin/env python3
"""Per-pair pose error and its AUC (ops.pose_error_by_pair / ops.pose_auc, csrc/pose_error.hip): the two entry points timed at the
pose bench's batch shape, and the yardstick itself run on seeded two-view scenes - what a minimal solver or the local optimisation
buys in the reference's own metric, AUC@5/10/20 of max(err_R, err_t).

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_pose_error.py --measure`  -> profiles/pose_error_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process:
  times      after three warm-up calls, device events around every call, minimum and median of --launches calls in microseconds:
             ops.pose_error_by_pair at --pairs pairs with T0 and counts on preallocated outputs (one kernel), ops.pose_auc at
             --n accumulated errors and at pose_auc_max_n() on preallocated outputs (one kernel), and ops.epipolar_pose_by_pair
             at --pairs x --K as the neighbour to compare with
  yardstick  --steps steps of --pairs scenes, K matches each in the strided (top-K) form: tests/pose_cases.make_scene's
             distributions restated here (depth 3..8, |t| = 1, a rotation of 0.05..0.4 rad, noise 5e-4) with 40 % outliers.  Three
             chains on the same scenes, seeds, threshold (2e-3) and sample budget (--samples per pair):
               8-point            hypotheses -> verification with moments -> pose
               5-point            the calibrated sampler (up to ten models per sample) -> the same
               5-point + polish   the same with four local-optimisation rounds on the winner before the pose
             every step writes its `err` into one running device buffer (out= a slice of it), one pose_auc at the end: no host
             read until the three numbers come back.  docs/kernels.md 4.9.2 holds what an MI355X gave

usage: bench_pose_error.py [--measure] [--pairs 48] [--K 2048] [--n 4000] [--steps 6] [--samples 64] [--launches 30]
                           [--out-dir profiles] [--step-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
THR = 2e-3


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_pose_error: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "pose_error_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def scenes(np, pairs, K, seed, outliers=0.4, noise=5e-4):
    """-> (ml, mr [pairs,K,2] float32, T1 [pairs,4,4] float64: the ground truth (R | t))."""
    rng = np.random.default_rng(seed)
    ml, mr, T1 = np.empty((pairs, K, 2), np.float32), np.empty((pairs, K, 2), np.float32), np.zeros((pairs, 4, 4), np.float64)
    for p in range(pairs):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        ang = rng.uniform(0.05, 0.4)
        R = np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        Z = rng.uniform(3.0, 8.0, K)
        X = np.stack([rng.uniform(-0.6, 0.6, K) * Z, rng.uniform(-0.6, 0.6, K) * Z, Z], 1)
        Y = X @ R.T + t[None, :]
        xr = Y[:, :2] / Y[:, 2:3] + rng.normal(scale=noise, size=(K, 2))
        bad = rng.random(K) < outliers
        xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
        ml[p], mr[p] = X[:, :2] / X[:, 2:3], xr
        T1[p, :3, :3], T1[p, :3, 3], T1[p, 3, 3] = R, t, 1.0
    return ml, mr, T1


def timed(torch, call, launches):
    us = []
    for i in range(launches + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            us.append(e0.elapsed_time(e1) * 1e3)
    return {"min": min(us), "median": statistics.median(us)}


def measure(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_error.py: no GPU - nothing to measure")
    from pats_amd import ops
    pairs, K, steps, samples = args.pairs, args.K, args.steps, args.samples
    dev = torch.device("cuda")
    counts = torch.full((pairs,), K, dtype=torch.int64, device=dev)
    thr = torch.full((pairs,), THR, device=dev)
    seg = dict(stride=K, counts=counts)

    def pose_of(ml, mr, models, polish):
        ver = ops.epipolar_score_by_pair(ml, mr, models, thr, moments=True, **seg)
        inlier, best_count, moments = ver[3], ver[2], ver[4]
        if polish:
            pol = ops.epipolar_polish_by_pair(ml, mr, models, thr, best=ver[1], rounds=4, **seg)
            best_count, inlier, moments = pol[1], pol[2], pol[3]
        return ops.epipolar_pose_by_pair(ml, mr, inlier, best_count, moments=moments, **seg)

    chains = {"8-point": (lambda ml, mr, seed: ops.epipolar_hypotheses_by_pair(ml, mr, samples, seed, **seg), False),
              "5-point": (lambda ml, mr, seed: ops.epipolar_hypotheses5_by_pair(ml, mr, samples, seed, **seg).view(pairs, 10 * samples, 3, 3), False),
              "5-point+polish": (lambda ml, mr, seed: ops.epipolar_hypotheses5_by_pair(ml, mr, samples, seed, **seg).view(pairs, 10 * samples, 3, 3), True)}
    running = {name: torch.empty(steps * pairs, dtype=torch.float64, device=dev) for name in chains}
    scratch = {name: tuple(torch.empty(pairs, dtype=dt, device=dev) for dt in (torch.float64, torch.float64)) + (torch.empty(pairs, dtype=torch.int32, device=dev),)
               for name in chains}
    evaluated = {name: torch.zeros((), dtype=torch.int64, device=dev) for name in chains}
    for step in range(steps):
        ml, mr, T1 = (torch.from_numpy(a).to(dev) for a in scenes(np, pairs, K, 4000 + step))
        seed = torch.arange(pairs, dtype=torch.int64, device=dev) + 1000 * step
        for name, (models_of, polish) in chains.items():
            pose = pose_of(ml, mr, models_of(ml, mr, seed), polish)
            eR, eT, st = scratch[name]
            ops.pose_error_by_pair(pose[1], pose[2], T1, counts=counts, out=(eR, eT, running[name][step * pairs:(step + 1) * pairs], st))
            evaluated[name] += (st == 0).sum()
    yard = {}
    for name in chains:
        auc, below = ops.pose_auc(running[name])
        yard[name] = {"auc@5": float(auc[0]), "auc@10": float(auc[1]), "auc@20": float(auc[2]), "below": below.tolist(),
                      "evaluated": int(evaluated[name]), "median_err": float(running[name].clamp(max=180.0).median())}

    # ---- the two entry points, and the pose stage beside them ---------------------------------------------------------------------
    pose = pose_of(ml, mr, chains["8-point"][0](ml, mr, seed), False)
    T0 = torch.eye(4, dtype=torch.float64, device=dev).repeat(pairs, 1, 1)
    dest = tuple(torch.empty(pairs, dtype=dt, device=dev) for dt in (torch.float64,) * 3 + (torch.int32,))
    err_us = timed(torch, lambda: ops.pose_error_by_pair(pose[1], pose[2], T1, T0=T0, counts=counts, out=dest), args.launches)
    rng = np.random.default_rng(9)
    big = ops.pose_auc_max_n()
    errors = torch.from_numpy(np.maximum(rng.gamma(1.2, 6.0, big), rng.gamma(1.0, 8.0, big))).to(dev)
    auc_dest = (torch.empty(3, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.int64, device=dev))
    auc_us = timed(torch, lambda: ops.pose_auc(errors[:args.n], out=auc_dest), args.launches)
    first = tuple(t.clone() for t in auc_dest)
    ops.pose_auc(errors[:args.n], out=auc_dest)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(first, auc_dest)), "two calls differ"
    auc_big_us = timed(torch, lambda: ops.pose_auc(errors, out=auc_dest), args.launches)
    ver = ops.epipolar_score_by_pair(ml, mr, chains["8-point"][0](ml, mr, seed), thr, moments=True, **seg)
    pa = dict(matches_l=ml, matches_r=mr, inlier=ver[3], best_count=ver[2], moments=ver[4], **seg)
    pose_dest = tuple(torch.empty_like(t) for t in ops.epipolar_pose_by_pair(**pa))
    pose_us = timed(torch, lambda: ops.epipolar_pose_by_pair(out=pose_dest, **pa), args.launches)
    result = {"tool": "bench_pose_error", "pairs_per_step": pairs, "K": K, "launches": args.launches, "pose_error_call_us": err_us,
              "pose_auc_n": args.n, "pose_auc_call_us": auc_us, "pose_auc_max_n": big, "pose_auc_max_n_call_us": auc_big_us,
              "pose_call_us": pose_us, "pose_error_over_pose": err_us["median"] / pose_us["median"],
              "yardstick": {"steps": steps, "pairs": steps * pairs, "outliers": 0.4, "thr": THR, "samples": samples, "chains": yard}}
    print("pose_error %.1f us | pose_auc %.1f us at n = %d, %.1f us at n = %d | pose %.1f us"
          % (err_us["median"], auc_us["median"], args.n, auc_big_us["median"], big, pose_us["median"]))
    for name, y in yard.items():
        print("%-16s AUC@5/10/20 = %.4f / %.4f / %.4f  (%d of %d evaluated, median error %.3f degrees)"
              % (name, y["auc@5"], y["auc@10"], y["auc@20"], y["evaluated"], steps * pairs, y["median_err"]))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the driver's GPU step may take")
    args, _ = ap.parse_known_args()
    if args.measure:
        measure(args)
    else:
        driver(args, [a for a in sys.argv[1:] if a != "--measure"])


if __name__ == "__main__":
    main()
