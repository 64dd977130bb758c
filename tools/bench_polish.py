#!/usr/bin/env python3
"""Per-pair local optimisation (ops.epipolar_polish_by_pair, csrc/polish.hip: ONE launch walks the rounds) against the chain of
existing calls it replaces - per round ops.epipolar_pose_by_pair, the cast of its E to a float32 H = 1 model in torch, and
ops.epipolar_score_by_pair(moments=True) - on the SAME inputs, in the same session.

Workload: 48 pairs with a planted epipolar model each (a share of the matches within noise of its epipolar lines, the rest random),
the walk started from a perturbed copy of that model; the lists once as a top-2048 (strided segments, K = 2048 rows per pair, all
filled) and once as on="all" (ragged segments of --matches rows); rounds in 1, 2, 4, 8.  The chain starts from an existing
verification of the start model (a caller has one) and runs `rounds` rounds; the fused call also re-derives round 0 itself.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/polish_bench.json.  A step that fails or runs out of time ends the driver.

--measure (docs/measurement.md 5.5): after three untimed calls of each the two alternate, --launches times each, preallocated
outputs for the fused call, device events around every call (fills and launches) and the host's clock around call + synchronise;
medians, minima and the chain's own spread (its quartiles).  The two results are compared: the fused call's counts and model must
equal the chain's.

usage: bench_polish.py [--measure] [--pairs 48] [--matches 4000] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROUNDS = (1, 2, 4, 8)
TOPK = 2048


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_polish: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "polish_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def planted_batch(torch, gen, pairs, n, ratio=0.6, noise=5e-4, start=0.03):
    """-> (ml, mr [pairs * n, 2] float32, model [pairs,1,3,3] float32 - the planted unit model plus N(0, start) per entry, renormalised -,
    thr [pairs]): round(ratio * n) matches of a pair lie within N(0, noise) of the planted model's epipolar lines."""
    dev = gen.device
    R = torch.linalg.qr(torch.randn((pairs, 3, 3), generator=gen, device=dev, dtype=torch.float64))[0]
    R = R * torch.linalg.det(R)[:, None, None]                                         # proper rotations
    t = torch.randn((pairs, 3), generator=gen, device=dev, dtype=torch.float64)
    z = torch.zeros(pairs, device=dev, dtype=torch.float64)
    tx = torch.stack([z, -t[:, 2], t[:, 1], t[:, 2], z, -t[:, 0], -t[:, 1], t[:, 0], z], 1).reshape(pairs, 3, 3)
    E = tx @ R                                                                         # an essential matrix: the refit projects onto these
    E = E / E.reshape(pairs, 9).norm(dim=1)[:, None, None]
    xl = torch.rand((pairs, n, 2), generator=gen, device=dev, dtype=torch.float64) * 1.2 - 0.6
    u = torch.rand((pairs, n, 2), generator=gen, device=dev, dtype=torch.float64) * 1.2 - 0.6
    a = torch.einsum("pij,pnj->pni", E, torch.cat([xl, torch.ones((pairs, n, 1), device=dev, dtype=torch.float64)], 2))
    d = (a[..., 0] * u[..., 0] + a[..., 1] * u[..., 1] + a[..., 2]) / (a[..., 0] ** 2 + a[..., 1] ** 2)
    on_line = u - d[..., None] * a[..., :2] + noise * torch.randn((pairs, n, 2), generator=gen, device=dev, dtype=torch.float64)
    inlier = torch.rand((pairs, n), generator=gen, device=dev, dtype=torch.float64) < ratio
    xr = torch.where(inlier[..., None], on_line, u * (0.8 / 0.6))
    m = E + start * torch.randn((pairs, 3, 3), generator=gen, device=dev, dtype=torch.float64)
    m = m / m.reshape(pairs, 9).norm(dim=1)[:, None, None]
    thr = torch.full((pairs,), 2e-3, device=dev)
    return xl.float().reshape(-1, 2).contiguous(), xr.float().reshape(-1, 2).contiguous(), m.float().reshape(pairs, 1, 3, 3).contiguous(), thr


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"min": min(v), "q1": q[0], "median": q[1], "q3": q[2], "max": max(v)}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_polish.py: no GPU - nothing to measure")
    from pats_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    pairs = args.pairs
    result = {"tool": "bench_polish", "pairs": pairs, "launches": args.launches, "family": "epipolar", "cases": {}}
    for on, n in (("topk", TOPK), ("all", args.matches)):
        ml, mr, model, thr = planted_batch(torch, gen, pairs, n)
        if on == "topk":
            seg = {"stride": n, "counts": torch.full((pairs,), n, dtype=torch.int64, device=dev)}
        else:
            seg = {"pair_off": torch.arange(pairs + 1, device=dev, dtype=torch.int64) * n}
        first = ops.epipolar_score_by_pair(ml, mr, model, thr, moments=True, **seg)       # the verification a caller already has
        for rounds in ROUNDS:
            def chain():
                ver = first
                for r in range(rounds):
                    E = ops.epipolar_pose_by_pair(ml, mr, ver[3], ver[2], moments=ver[4], **seg)[0]
                    m = E.float().reshape(pairs, 1, 3, 3)
                    ver = ops.epipolar_score_by_pair(ml, mr, m, thr, moments=True, **seg)
                return ver, m

            fused = lambda out=None: ops.epipolar_polish_by_pair(ml, mr, model, thr, rounds=rounds, out=out, **seg)        # noqa: E731
            dest = fused()
            ms = {"chain": [], "fused": []}
            wall = {"chain": [], "fused": []}
            last = None
            for i in range(args.launches + 3):
                for which in ("chain", "fused"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    if which == "chain":
                        last = chain()
                    else:
                        fused(dest)
                    e1.record()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if i >= 3:
                        ms[which].append(e0.elapsed_time(e1))
                        wall[which].append((t1 - t0) * 1e3)
            counts = dest[5].cpu()
            assert torch.equal(counts[:, rounds].long(), last[0][2].cpu()), "the fused walk's last count is not the chain's"
            keep = (dest[4].cpu() == rounds).nonzero().flatten()
            assert torch.equal(dest[0].cpu()[keep], last[1].cpu()[keep, 0]), "the fused walk's last model is not the chain's"
            c, f = quartiles(ms["chain"]), quartiles(ms["fused"])
            wc, wf = quartiles(wall["chain"]), quartiles(wall["fused"])
            result["cases"]["on=%s rounds=%d" % (on, rounds)] = {
                "on": on, "matches_per_pair": n, "rounds": rounds, "chain_device_ms": c, "fused_device_ms": f, "chain_wall_ms": wc,
                "fused_wall_ms": wf, "chain_over_fused_device": c["median"] / f["median"], "chain_over_fused_wall": wc["median"] / wf["median"],
                "device_gain_ms": c["median"] - f["median"], "chain_device_spread_ms": c["q3"] - c["q1"],
                "wall_gain_ms": wc["median"] - wf["median"], "chain_wall_spread_ms": wc["q3"] - wc["q1"],
                "launches_chain": 7 * rounds, "launches_fused": 2, "mean_best_round": float(dest[4].float().mean()),
                "pairs_whose_last_round_is_not_best": int((dest[4].cpu() < rounds).sum()),
                "mean_gain_inliers": float((dest[1].cpu() - counts[:, 0]).float().mean())}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--matches", type=int, default=4000)
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
