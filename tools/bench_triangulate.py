#!/usr/bin/env python3
"""Per-pair triangulation (batch.triangulate_by_pair / ops.epipolar_triangulate_by_pair, csrc/triangulate.hip) at the pose bench's
batch shape: 48 pairs per step, K = 2048 matches per pair in the strided (top-K) form - here synthetic two-view scenes (depth 3..8,
|t| = 1, a rotation of 0.05..0.4 rad, 30 % outliers, noise 5e-4), verified against the true model with moments and posed on the device.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_triangulate.py --measure`  -> profiles/triangulate_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process after three warm-up calls per stage:
  pose         ops.epipolar_pose_by_pair with the front mask on preallocated outputs, device events around every call (a fill and
               one kernel), minimum and median of --launches calls, in microseconds
  triangulate  ops.epipolar_triangulate_by_pair on the pose's front mask, all three optional outputs, preallocated, the same way
               (five fills and one kernel); and once more without the optional outputs (two fills and one kernel)
  hbm_us       the stage's bytes - 17 read per match (two float2 and the mask byte), 29 zero-filled per row and 29 stored per
               valid match (points, valid, depths, reproj, cos_parallax) - divided by the 8 TB/s of docs/measurement.md: what the
               stage would take at the memory bound.  docs/kernels.md 4.9.1 holds the numbers measured on an MI355X

usage: bench_triangulate.py [--measure] [--pairs 48] [--K 2048] [--launches 30] [--out-dir profiles] [--step-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8e12                                 # docs/measurement.md: the 8 TB/s spec


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_triangulate: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "triangulate_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def scenes(np, pairs, K, seed=1234):
    """-> (ml, mr [pairs,K,2] float32, models [pairs,1,3,3] float32: the true essential matrices)."""
    rng = np.random.default_rng(seed)
    ml, mr, models = np.empty((pairs, K, 2), np.float32), np.empty((pairs, K, 2), np.float32), np.empty((pairs, 1, 3, 3), np.float32)
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
        xr = Y[:, :2] / Y[:, 2:3] + rng.normal(scale=5e-4, size=(K, 2))
        bad = rng.random(K) < 0.3
        xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        ml[p], mr[p], models[p, 0] = X[:, :2] / X[:, 2:3], xr, E / np.linalg.norm(E)
    return ml, mr, models


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
        raise SystemExit("bench_triangulate.py: no GPU - nothing to measure")
    from pats_amd import ops
    pairs, K = args.pairs, args.K
    dev = torch.device("cuda")
    ml, mr, models = (torch.from_numpy(a).to(dev) for a in scenes(np, pairs, K))
    counts = torch.full((pairs,), K, dtype=torch.int64, device=dev)
    seg = dict(stride=K, counts=counts)
    ver = ops.epipolar_score_by_pair(ml, mr, models, torch.full((pairs,), 2e-3, device=dev), moments=True, **seg)
    pa = dict(matches_l=ml, matches_r=mr, inlier=ver[3], best_count=ver[2], moments=ver[4], **seg)
    pose = ops.epipolar_pose_by_pair(return_front=True, **pa)
    pose_again = tuple(torch.empty_like(t) for t in pose)
    ta = dict(matches_l=ml, matches_r=mr, mask=pose[6], R=pose[1], t=pose[2], **seg)
    full = dict(return_depths=True, return_reproj=True, return_cos=True)
    tri = ops.epipolar_triangulate_by_pair(**ta, **full)
    tri_again = tuple(torch.empty_like(t) for t in tri)
    pose_us = timed(torch, lambda: ops.epipolar_pose_by_pair(return_front=True, out=pose_again, **pa), args.launches)
    tri_us = timed(torch, lambda: ops.epipolar_triangulate_by_pair(out=tri_again, **ta, **full), args.launches)
    lean_us = timed(torch, lambda: ops.epipolar_triangulate_by_pair(out=tri_again[:4], **ta), args.launches)
    assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(tri, tri_again)), "two calls differ"
    assert bool(torch.equal(tri[1].view(pairs, K).sum(1), tri[2])), "tri_count != valid.sum()"
    cap, valid = pairs * K, int(tri[2].sum())
    nbytes = 17 * cap + 29 * cap + 29 * valid
    lean_bytes = 17 * cap + 13 * cap + 13 * valid
    result = {"tool": "bench_triangulate", "pairs_per_step": pairs, "K": K, "launches": args.launches,
              "best_count": {"min": int(ver[2].min()), "max": int(ver[2].max())},
              "front_count": {"min": int(pose[3].min()), "max": int(pose[3].max())},
              "tri_count": {"min": int(tri[2].min()), "max": int(tri[2].max())}, "valid_matches": valid,
              "pose_call_us": pose_us, "triangulate_call_us": tri_us, "triangulate_lean_call_us": lean_us,
              "bytes": nbytes, "hbm_us": nbytes / HBM_BYTES_PER_S * 1e6, "lean_bytes": lean_bytes,
              "lean_hbm_us": lean_bytes / HBM_BYTES_PER_S * 1e6,
              "triangulate_over_pose": tri_us["median"] / pose_us["median"],
              "triangulate_over_hbm_bound": tri_us["median"] / (nbytes / HBM_BYTES_PER_S * 1e6)}
    print("pose %.1f us | triangulate %.1f us (%.1f us without the optional outputs) | %d bytes at 8 TB/s: %.2f us"
          % (pose_us["median"], tri_us["median"], lean_us["median"], nbytes, result["hbm_us"]))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
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
