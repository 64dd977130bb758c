#!/usr/bin/env python3
"""Per-pair pose from a homography and the E-or-H decision (batch.pose_h_by_pair / select_pose_by_pair, csrc/pose_h.hip) on synthetic
pairs: 48 pairs x 2048 matches, half of them looking at a plane (1700 matches on it, 200 off it, 148 outliers), half of them mostly
rotating (|t| / d = 0.01, the same mix) - the two situations in which the epipolar model is degenerate.  The scenes are
tests/pose_h_cases.py's generator; both branches run from seeded hypotheses (8-point and 4-point, H each) through verification with
moments to their poses.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_pose_h.py --measure`  -> profiles/pose_h_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process after a warm-up:
  call    ops.homography_pose_by_pair (thr given, front and candidates written), ops.pose_select_by_pair and, in the same run as the
          comparison, ops.epipolar_pose_by_pair, each alone on the step's verified lists with preallocated outputs, device events
          around every call (the fills and one kernel), minimum and median of --launches calls.  Nothing is promised: all three are
          launch-bound
  auc     AUC@5/10/20 (ops.pose_auc) of batch.pose_error_by_pair on the epipolar pose against the same on
          batch.pose_branch(out, "selected") and batch.pose_branch(out, "planar"), over the 48 pairs and per family, with the number
          of pairs per branch

usage: bench_pose_h.py [--measure] [--pairs 48] [--matches 2048] [--H 256] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_pose_h: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "pose_h_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def timed(torch, call, launches):
    ms = []
    for i in range(launches + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1) * 1e3)
    return {"min": min(ms), "median": statistics.median(ms)}


def measure(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_h.py: no GPU - nothing to measure")
    import pose_h_cases as ph
    from pats_amd import batch, ops
    pairs, n, H = args.pairs, args.matches, args.H
    n_off, n_out = n * 200 // 2048, n * 148 // 2048
    family = ["plane" if i % 2 == 0 else "small" for i in range(pairs)]
    scenes = [ph.make_scene(9000 + i, n - n_off - n_out, n_off, n_out, family=family[i]) for i in range(pairs)]
    dev = torch.device("cuda")
    ml = torch.from_numpy(np.concatenate([s["ml"] for s in scenes])).to(dev)
    mr = torch.from_numpy(np.concatenate([s["mr"] for s in scenes])).to(dev)
    summary = torch.tensor([i * n for i in range(pairs + 1)] + [pairs * n, 0, 0], dtype=torch.int64, device=dev)
    T1 = np.tile(np.eye(4), (pairs, 1, 1))
    for i, s in enumerate(scenes):
        T1[i, :3, :3], T1[i, :3, 3] = s["R"], s["t"]
    T1 = torch.from_numpy(T1).to(dev)
    cap = batch.Capacities(pairs, 5, 6)
    thr = torch.full((pairs,), 2e-3, device=dev)
    out = {"matches_l": ml, "matches_r": mr, "by_pair": (ml, mr, summary[:pairs + 1]), "summary": summary}

    def both_branches():
        batch.verify_by_pair(out, cap, batch.hypothesize_by_pair(out, cap, H, seed=7, on="all"), thr, moments=True)
        batch.pose_by_pair(out, cap, front=True)
        batch.verify_h_by_pair(out, cap, batch.hypothesize_h_by_pair(out, cap, H, seed=7, on="all"), thr, moments=True)
        batch.pose_h_by_pair(out, cap, thr=thr, front=True, candidates=True)
        batch.select_pose_by_pair(out, cap, ratio=args.ratio)

    both_branches()
    both_branches()
    torch.cuda.synchronize()
    ver, ver_h = out["verified"], out["verified_h"]
    seg = {"pair_off": summary, "pairs": pairs}
    a_e = dict(matches_l=ml, matches_r=mr, inlier=ver[3], best_count=ver[2], moments=ver[4], return_front=True, **seg)
    a_h = dict(matches_l=ml, matches_r=mr, inlier=ver_h[3], best_count=ver_h[2], moments=ver_h[4], thr=thr, return_front=True,
               return_candidates=True, **seg)
    dest_e, dest_h = ops.epipolar_pose_by_pair(**a_e), ops.homography_pose_by_pair(**a_h)
    pe, php = out["pose"], out["pose_h"]
    a_s = (pe[:4] + pe[6:7], ver[2], ver[3], php[:4] + php[6:7], out["pose_h_extra"][3], ver_h[2], ver_h[3],
           torch.full((pairs,), args.ratio, device=dev))
    dest_s = ops.pose_select_by_pair(*a_s, **seg)
    call_us = {"epipolar_pose_by_pair": timed(torch, lambda: ops.epipolar_pose_by_pair(out=dest_e, **a_e), args.launches),
               "homography_pose_by_pair": timed(torch, lambda: ops.homography_pose_by_pair(out=dest_h, **a_h), args.launches),
               "pose_select_by_pair": timed(torch, lambda: ops.pose_select_by_pair(*a_s, out=dest_s, **seg), args.launches)}
    auc, fams = {}, {"plane": [i for i in range(pairs) if family[i] == "plane"], "small": [i for i in range(pairs) if family[i] == "small"]}
    for b in ("epipolar", "planar", "selected"):
        err = batch.pose_error_by_pair(batch.pose_branch(out, b), cap, T1)[2]
        auc[b] = {"all": ops.pose_auc(err)[0].cpu().tolist()}
        for name, idx in fams.items():
            auc[b][name] = ops.pose_auc(err[torch.tensor(idx, device=dev)].contiguous())[0].cpu().tolist()
    branch = out["pose_selected_extra"][0].cpu().tolist()
    status = out["pose_h_extra"][3].cpu().tolist()
    result = {"tool": "bench_pose_h", "pairs": pairs, "matches_per_pair": n, "H": H, "ratio": args.ratio, "launches": args.launches,
              "families": {k: len(v) for k, v in fams.items()}, "call_us": call_us,
              "homography_over_epipolar_call": call_us["homography_pose_by_pair"]["median"] / call_us["epipolar_pose_by_pair"]["median"],
              "auc_thresholds_deg": [5.0, 10.0, 20.0], "auc": auc,
              "branch_counts": {str(k): branch.count(k) for k in range(4)}, "status_h_counts": {str(k): status.count(k) for k in range(3)},
              "best_count_e": {"min": int(ver[2].min()), "max": int(ver[2].max())},
              "best_count_h": {"min": int(ver_h[2].min()), "max": int(ver_h[2].max())}}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds the driver's GPU step may take")
    args, _ = ap.parse_known_args()
    if args.measure:
        measure(args)
    else:
        driver(args, [a for a in sys.argv[1:] if a != "--measure"])


if __name__ == "__main__":
    main()
