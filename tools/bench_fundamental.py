#!/usr/bin/env python3
"""The uncalibrated branch (csrc/hypotheses7.hip, csrc/fundamental.hip, polish.hip's Fundamental family) beside what it stands next
to, on the SAME inputs, in the same session:
  hypotheses  ops.epipolar_hypotheses7_by_pair against the 8-point ops.epipolar_hypotheses_by_pair: 48 pairs, a top-2048 each in
              the strided layout, H = 1024 samples (3 H model slots against H)
  polish      ops.fundamental_polish_by_pair, four rounds, against the chain it replaces - per round ops.fundamental_refit_by_pair,
              the cast of its F to a float32 H = 1 model and ops.epipolar_score_by_pair(moments=True) - at 48 x 2048 (strided) and
              48 x 4000 (ragged); the fused call's counts and model must equal the chain's
  refit       ops.fundamental_refit_by_pair alone (with F_px)

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/fundamental_bench.json.  A step that fails or runs out of time ends the driver.

--measure (docs/measurement.md 5.5): after three untimed calls of each the two sides of a comparison alternate, --launches times
each, preallocated outputs, device events around every call (fills and launches) and the host's clock around call + synchronise;
quartiles of both.  Recorded, not asserted: no time is a pass condition.

usage: bench_fundamental.py [--measure] [--pairs 48] [--K 2048] [--H 1024] [--matches 4000] [--rounds 4] [--launches 30]
                            [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_fundamental: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "fundamental_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def alternate(torch, sides, launches):
    """sides: {name: callable}; -> {name: {"device_ms": quartiles, "wall_ms": quartiles}}, the sides alternating call by call."""
    from bench_polish import quartiles
    ms = {k: [] for k in sides}
    wall = {k: [] for k in sides}
    for i in range(launches + 3):
        for name, call in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= 3:
                ms[name].append(e0.elapsed_time(e1))
                wall[name].append((t1 - t0) * 1e3)
    return {k: {"device_ms": quartiles(ms[k]), "wall_ms": quartiles(wall[k])} for k in sides}


def measure(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fundamental.py: no GPU - nothing to measure")
    from bench_hypotheses5 import two_view_pairs
    from bench_polish import planted_batch
    from pats_amd import ops
    dev = torch.device("cuda")
    pairs, K, H, rounds = args.pairs, args.K, args.H, args.rounds
    result = {"tool": "bench_fundamental", "pairs": pairs, "K": K, "H": H, "rounds": rounds, "launches": args.launches}

    # ---- hypotheses: 7-point against 8-point, the same lists, the same seeds, the same number of samples -------------------------
    seeds = torch.arange(pairs, dtype=torch.int64, device=dev) + 7
    seg = {"stride": K, "counts": torch.full((pairs,), K, dtype=torch.int64, device=dev)}
    thr = torch.full((pairs,), 2e-3, device=dev)
    ml, mr, E = two_view_pairs(np, pairs, K, 0.4, seed=9000)
    dl, dr = torch.from_numpy(ml).to(dev), torch.from_numpy(mr).to(dev)
    gen7 = lambda out=None: ops.epipolar_hypotheses7_by_pair(dl, dr, H, seeds, progressive=True, out=out, **seg)      # noqa: E731
    gen8 = lambda out=None: ops.epipolar_hypotheses_by_pair(dl, dr, H, seeds, progressive=True, out=out, **seg)       # noqa: E731
    m7, m8 = gen7(), gen8()
    r = alternate(torch, {"7-point": lambda: gen7(m7), "8-point": lambda: gen8(m8)}, args.launches)
    for name, models in (("7-point", m7), ("8-point", m8)):
        ver = ops.epipolar_score_by_pair(dl, dr, models.reshape(pairs, -1, 3, 3), thr, **seg)
        r[name].update(best_count_mean=float(ver[2].float().mean()), best_count_min=int(ver[2].min()),
                       nonzero_models_per_pair=float(models.reshape(pairs, -1, 9).any(2).sum(1).float().mean()))
        r[name]["us_per_sample"] = r[name]["device_ms"]["median"] * 1e3 / (pairs * H)
    r["true_model_inliers_mean"] = float(ops.epipolar_score_by_pair(dl, dr, torch.from_numpy(E).to(dev)[:, None], thr, **seg)[2].float().mean())
    r["seven_over_eight_device"] = r["7-point"]["device_ms"]["median"] / r["8-point"]["device_ms"]["median"]
    result["hypotheses"] = r

    # ---- polish: the fused walk against the chain it replaces; the refit alone ---------------------------------------------------
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    result["polish"] = {}
    for on, n in (("topk", K), ("all", args.matches)):
        pl, pr, model, pthr = planted_batch(torch, gen, pairs, n)
        if on == "topk":
            pseg = {"stride": n, "counts": torch.full((pairs,), n, dtype=torch.int64, device=dev)}
        else:
            pseg = {"pair_off": torch.arange(pairs + 1, device=dev, dtype=torch.int64) * n}
        first = ops.epipolar_score_by_pair(pl, pr, model, pthr, moments=True, **pseg)   # the verification a caller already has
        last = [None]

        def chain():
            ver = first
            for _ in range(rounds):
                m = ops.fundamental_refit_by_pair(ver[2], moments=ver[4])[0].float().reshape(pairs, 1, 3, 3)
                ver = ops.epipolar_score_by_pair(pl, pr, m, pthr, moments=True, **pseg)
            last[0] = (ver, m)

        dest = ops.fundamental_polish_by_pair(pl, pr, model, pthr, rounds=rounds, **pseg)
        c = alternate(torch, {"chain": chain, "fused": lambda: ops.fundamental_polish_by_pair(pl, pr, model, pthr, rounds=rounds, out=dest, **pseg)},
                      args.launches)
        counts = dest[5].cpu()
        assert torch.equal(counts[:, rounds].long(), last[0][0][2].cpu()), "the fused walk's last count is not the chain's"
        keep = (dest[4].cpu() == rounds).nonzero().flatten()
        assert torch.equal(dest[0].cpu()[keep], last[0][1].cpu()[keep, 0]), "the fused walk's last model is not the chain's"
        c.update(on=on, matches_per_pair=n, chain_over_fused_device=c["chain"]["device_ms"]["median"] / c["fused"]["device_ms"]["median"],
                 chain_over_fused_wall=c["chain"]["wall_ms"]["median"] / c["fused"]["wall_ms"]["median"],
                 mean_best_round=float(dest[4].float().mean()), mean_gain_inliers=float((dest[1].cpu() - counts[:, 0]).float().mean()))
        result["polish"]["on=%s" % on] = c
        if on == "topk":
            fit = ops.fundamental_refit_by_pair(dest[1], moments=dest[3], return_pixel=True)
            result["refit"] = alternate(torch, {"refit": lambda: ops.fundamental_refit_by_pair(dest[1], moments=dest[3], return_pixel=True, out=fit)},
                                        args.launches)["refit"]
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--matches", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=4)
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
