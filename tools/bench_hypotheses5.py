#!/usr/bin/env python3
"""Per-pair 5-point hypotheses (ops.epipolar_hypotheses5_by_pair, csrc/hypotheses5.hip) beside the 8-point generator
(csrc/hypotheses.hip) at EQUAL MODEL COUNT: 48 pairs, each a confidence-ordered top-2048 in the strided layout, 1000 models per pair -
H = 100 five-point samples (ten slots each) against H = 1000 eight-point hypotheses.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_hypotheses5.py --measure`  -> profiles/hypotheses5_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process:
  call     each generator alone on preallocated outputs, device events around every call (one kernel), minimum and median of
           --launches calls after three warm-up calls
  quality  synthetic two-view pairs in the style of the tests' make_case (a seeded rotation and translation, points at depth 3 .. 8,
           noise 5e-4 on the right image, a share of the right points replaced by uniform ones), `outliers` 0.4 and 0.6: both
           generators' models through ops.epipolar_score_by_pair (thr 2e-3), the mean best_count over the pairs, and the mean inlier
           count of the true essential matrix for scale.  Recorded, not asserted

usage: bench_hypotheses5.py [--measure] [--pairs 48] [--K 2048] [--H5 100] [--H8 1000] [--launches 30] [--out-dir profiles]
                            [--step-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_hypotheses5: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "hypotheses5_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def two_view_pairs(np, pairs, n, outliers, seed, noise=5e-4):
    """-> (ml [pairs,n,2], mr [pairs,n,2] float32 in calibrated coordinates, E [pairs,3,3] float32 unit: x_r^T E x_l = 0)."""
    ml, mr, Es = [], [], []
    for p in range(pairs):
        rng = np.random.default_rng(seed + p)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.05, 0.4)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        Z = rng.uniform(3.0, 8.0, n)
        X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.6, 0.6, n) * Z, Z], 1)
        Y = X @ R.T + t[None, :]
        xr = Y[:, :2] / Y[:, 2:3] + rng.normal(scale=noise, size=(n, 2))
        bad = rng.random(n) < outliers
        xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
        ml.append(X[:, :2] / X[:, 2:3])
        mr.append(xr)
        Es.append(E / np.linalg.norm(E))
    return np.stack(ml).astype(np.float32), np.stack(mr).astype(np.float32), np.stack(Es).astype(np.float32)


def measure(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hypotheses5.py: no GPU - nothing to measure")
    from pats_amd import ops
    dev = torch.device("cuda")
    pairs, K, H5, H8 = args.pairs, args.K, args.H5, args.H8
    seeds = torch.arange(pairs, dtype=torch.int64, device=dev) + 7
    counts = torch.full((pairs,), K, dtype=torch.int64, device=dev)
    thr = torch.full((pairs,), 2e-3, device=dev)
    result = {"tool": "bench_hypotheses5", "pairs": pairs, "K": K, "H5": H5, "H8": H8, "models_per_pair": {"5-point": 10 * H5, "8-point": H8},
              "launches": args.launches, "outliers": {}}
    for share in (0.4, 0.6):
        ml, mr, E = two_view_pairs(np, pairs, K, share, seed=9000)
        dl, dr = torch.from_numpy(ml).to(dev), torch.from_numpy(mr).to(dev)
        seg = dict(stride=K, counts=counts)
        gens = {"5-point": lambda out=None: ops.epipolar_hypotheses5_by_pair(dl, dr, H5, seeds, return_counts=True, out=out, **seg),
                "8-point": lambda out=None: ops.epipolar_hypotheses_by_pair(dl, dr, H8, seeds, out=out, **seg)}
        r = {"true_model_inliers_mean": float(ops.epipolar_score_by_pair(dl, dr, torch.from_numpy(E).to(dev)[:, None], thr, **seg)[2].float().mean())}
        for name, gen in gens.items():
            dest = gen()
            ms = []
            for i in range(args.launches + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gen(dest)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            models = dest[0] if isinstance(dest, tuple) else dest
            ver = ops.epipolar_score_by_pair(dl, dr, models.reshape(pairs, -1, 3, 3), thr, **seg)
            r[name] = {"call_ms": {"min": min(ms), "median": statistics.median(ms)}, "best_count_mean": float(ver[2].float().mean()),
                       "best_count_min": int(ver[2].min()), "nonzero_models_per_pair": float(models.reshape(pairs, -1, 9).any(2).sum(1).float().mean())}
        result["outliers"][str(share)] = r
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--H5", type=int, default=100)
    ap.add_argument("--H8", type=int, default=1000)
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
