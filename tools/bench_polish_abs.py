#!/usr/bin/env python3
"""Per-pair absolute local optimisation (ops.absolute_polish_by_pair, csrc/absolute.hip: ONE launch walks the rounds) against the
chain it replaces, written in torch on the device - per round ops.absolute_score_by_pair with M = 1 for the mask, then `steps`
times masked normal equations in float64 (the header's J, A = sum J^T J, b = sum J^T e over the inliers), torch.linalg.solve and
the Rodrigues update, then the orthonormalising step and the cast to float32 - on the SAME inputs, in the same session.  The parent
commit has no such stage: the chain, measured in the same run, is the yardstick.

Workload: --pairs pairs (the benchmark's 48) of --matches matches (2048) in the strided form of a top-K: points in front of a known
pose, 30 % outliers, 10 % invalid lifts, noise of 1e-3 on the right points; the walk starts from the pose moved by 5e-4; rounds in
1, 2, 4, 8 and steps = 3.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/polish_abs_bench.json.  A step that fails or runs out of time ends the driver.

--measure (docs/measurement.md 5.5): after three untimed calls of each the two alternate, --launches times each, preallocated
outputs for the fused call, device events around every call (fills and launches) and the host's clock around call + synchronise;
medians, minima and the chain's own spread (its quartiles).  The two results are compared: round 0's support must be equal, and the
chain's last model within float32 rounding of the fused walk's where that walk's best round is the last.

usage: bench_polish_abs.py [--measure] [--pairs 48] [--matches 2048] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
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
STEPS = 3


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_polish_abs: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "polish_abs_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def rodrigues(torch, w):
    """w [pairs,3] float64 -> exp([w]x) [pairs,3,3]: the header's formula, the identity for w = 0."""
    th2 = (w * w).sum(1)
    th = th2.sqrt()
    safe = torch.where(th2 > 0, th, torch.ones_like(th))
    a = torch.where(th2 > 0, torch.sin(safe) / safe, torch.ones_like(th))
    b = torch.where(th2 > 0, 2 * torch.sin(0.5 * safe) ** 2 / (safe * safe), torch.full_like(th, 0.5))
    z = torch.zeros_like(th)
    W = torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], 1).view(-1, 3, 3)
    return torch.eye(3, dtype=w.dtype, device=w.device) + a[:, None, None] * W + b[:, None, None] * (W @ W)


def planted_batch(torch, gen, pairs, n, outliers=0.3, holes=0.1, noise=1e-3, start=5e-4):
    """-> (X [pairs * n, 3], xr [pairs * n, 2] float32, model [pairs,1,3,4] float32 = the planted pose moved by N(0, start), thr)."""
    dev = gen.device
    f64 = {"generator": gen, "device": dev, "dtype": torch.float64}
    xl = torch.rand((pairs, n, 2), **f64) * 1.2 - 0.6
    d = torch.rand((pairs, n, 1), **f64) * 7 + 1
    X = torch.cat([xl * d, d], 2)
    R = rodrigues(torch, 0.25 * torch.randn((pairs, 3), **f64))
    t = 0.3 * torch.randn((pairs, 3), **f64)
    Y = X @ R.transpose(1, 2) + t[:, None, :]
    xr = Y[..., :2] / Y[..., 2:3] + noise * torch.randn((pairs, n, 2), **f64)
    bad = torch.rand((pairs, n), **f64) < outliers
    xr = torch.where(bad[..., None], torch.rand((pairs, n, 2), **f64) * 1.6 - 0.8, xr)
    X = torch.where((torch.rand((pairs, n), **f64) < holes)[..., None], torch.full_like(X, float("nan")), X)
    E = rodrigues(torch, start * torch.randn((pairs, 3), **f64))
    m = torch.cat([E @ R, ((E @ t[:, :, None])[:, :, 0] + start * torch.randn((pairs, 3), **f64))[:, :, None]], 2)
    thr = torch.full((pairs,), 3e-3, device=dev)
    return X.float().reshape(-1, 3).contiguous(), xr.float().reshape(-1, 2).contiguous(), m.float().reshape(pairs, 1, 3, 4).contiguous(), thr


def torch_refit(torch, X, xr, mask, m32, steps):
    """The refit of include/pats_amd.h in torch: X [pairs,n,3], xr [pairs,n,2] float64 (NaN rows zeroed), mask [pairs,n] float64,
    m32 [pairs,3,4] float32 -> float32 [pairs,3,4].  (The yardstick skips the "no refit" rules: the workload never trips them.)"""
    m = m32.double()
    for _ in range(steps):
        Y = X @ m[:, :, :3].transpose(1, 2) + m[:, None, :, 3]
        iz = 1.0 / Y[..., 2]
        u, v = Y[..., 0] * iz, Y[..., 1] * iz
        e = torch.stack([u - xr[..., 0], v - xr[..., 1]], 2)
        z = torch.zeros_like(u)
        J = torch.stack([torch.stack([-u * v, 1 + u * u, -v, iz, z, -u * iz], 2), torch.stack([-(1 + v * v), u * v, u, z, iz, -v * iz], 2)], 2)
        Jw = J * mask[:, :, None, None]
        A = torch.einsum("pnki,pnkj->pij", Jw, J)
        b = torch.einsum("pnki,pnk->pi", Jw, e)
        d = torch.linalg.solve(A, -b)
        E = rodrigues(torch, d[:, :3])
        m = torch.cat([E @ m[:, :, :3], ((E @ m[:, :, 3:])[:, :, 0] + d[:, 3:])[:, :, None]], 2)
    R = m[:, :, :3]
    R = R + 0.5 * R @ (torch.eye(3, dtype=R.dtype, device=R.device) - R.transpose(1, 2) @ R)
    return torch.cat([R, m[:, :, 3:]], 2).float()


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"min": min(v), "q1": q[0], "median": q[1], "q3": q[2], "max": max(v)}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_polish_abs.py: no GPU - nothing to measure")
    from pats_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    pairs, n = args.pairs, args.matches
    result = {"tool": "bench_polish_abs", "pairs": pairs, "matches_per_pair": n, "steps": STEPS, "launches": args.launches, "cases": {}}
    X, xr, model, thr = planted_batch(torch, gen, pairs, n)
    seg = {"stride": n, "counts": torch.full((pairs,), n, dtype=torch.int64, device=dev)}
    X64 = torch.nan_to_num(X.double().view(pairs, n, 3), nan=1.0)             # an invalid lift is never an inlier: its row is masked out
    xr64 = xr.double().view(pairs, n, 2)
    for rounds in ROUNDS:
        def chain():
            m = model
            for r in range(rounds):
                ver = ops.absolute_score_by_pair(X, xr, m, thr, **seg)
                m = torch_refit(torch, X64, xr64, ver[3].view(pairs, n).double(), m[:, 0], STEPS)[:, None].contiguous()
            return ops.absolute_score_by_pair(X, xr, m, thr, **seg), m

        fused = lambda out=None: ops.absolute_polish_by_pair(X, xr, model, thr, rounds=rounds, steps=STEPS, out=out, **seg)      # noqa: E731
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
        counts = dest[4].cpu()
        first = ops.absolute_score_by_pair(X, xr, model, thr, **seg)
        assert torch.equal(counts[:, 0].long(), first[2].cpu()), "the fused walk's round 0 is not the verification's"
        keep = (dest[3].cpu() == rounds).nonzero().flatten()
        diff = float((dest[0].cpu()[keep] - last[1].cpu()[keep, 0]).abs().max()) if keep.numel() else 0.0
        assert diff <= 1e-4, "the fused walk's last model is %g from the chain's" % diff
        c, f = quartiles(ms["chain"]), quartiles(ms["fused"])
        wc, wf = quartiles(wall["chain"]), quartiles(wall["fused"])
        result["cases"]["rounds=%d" % rounds] = {
            "rounds": rounds, "chain_device_ms": c, "fused_device_ms": f, "chain_wall_ms": wc, "fused_wall_ms": wf,
            "chain_over_fused_device": c["median"] / f["median"], "chain_over_fused_wall": wc["median"] / wf["median"],
            "chain_device_spread_ms": c["q3"] - c["q1"], "chain_wall_spread_ms": wc["q3"] - wc["q1"],
            "mean_best_round": float(dest[3].float().mean()), "largest_model_difference": diff,
            "mean_support_round0": float(counts[:, 0].float().mean()), "mean_gain_inliers": float((dest[1].cpu() - counts[:, 0]).float().mean())}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--matches", type=int, default=2048)
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
