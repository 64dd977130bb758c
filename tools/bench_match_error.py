#!/usr/bin/env python3
"""Per-pair match error against ground truth (ops.match_error_by_pair, csrc/match_error.hip: two fills and ONE launch for the batch)
against the chain it replaces, written in torch on the device - the ground truth from the extrinsics, the projection in float64, the
status cascade with the gather from the right depth maps, the tallies, the per-threshold counts, the confidence sweep and the confusion
against a mask - on the SAME device inputs, in the same session.  The parent commit has no such stage: the chain, measured in the same
run, is the yardstick.

Workload: --pairs pairs (the benchmark's 48) of --matches matches (2048) in the strided form of a top-K on 480 x 640 images: lifted
points in front of a known pose, 10 % invalid lifts, 3 % lost right points, right points = the projection plus noise of 0 .. 6 px, a
right depth map per pair that agrees with the projection but for 10 % occluded taps and 5 % holes; thresholds 1, 3, 5 px, 16
confidence floors, min_conf 0.1, a random mask.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/match_error_bench.json.  A step that fails or runs out of time ends the driver.

--measure (docs/measurement.md 5.5): after three untimed calls of each the two alternate, --launches times each, preallocated
outputs for the stage, device events around every call (fills and launches) and the host's clock around call + synchronise; medians,
minima and the chain's own spread (its quartiles).  The two results are compared: status, tally, correct, sweep and confusion must
be equal and err within 1e-9 px.

usage: bench_match_error.py [--measure] [--pairs 48] [--matches 2048] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

THR = (1.0, 3.0, 5.0)
EDGES = tuple(0.05 + 0.055 * k for k in range(16))
MIN_CONF, OCCL = 0.1, 0.2
H, W, FOCAL = 480, 640, 520.0


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_match_error: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "match_error_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def rotation(torch, w):
    """w [pairs,3] float64 -> exp([w]x) [pairs,3,3]."""
    th = (w * w).sum(1).sqrt().clamp_min(1e-12)
    z = torch.zeros_like(th)
    Wm = torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=w.dtype, device=w.device)
    return eye + (torch.sin(th) / th)[:, None, None] * Wm + ((1 - torch.cos(th)) / (th * th))[:, None, None] * (Wm @ Wm)


def planted_batch(torch, gen, pairs, n):
    """The device inputs of one call -> dict (everything in the frame of the points: swapped = 0)."""
    dev = gen.device
    f64 = {"generator": gen, "device": dev, "dtype": torch.float64}
    norm = torch.tensor([H / 2, W / 2, 1 / FOCAL, 1 / FOCAL] * 2, device=dev).repeat(pairs, 1).contiguous()
    xl = torch.stack([(torch.rand((pairs, n), **f64) - 0.5) * (H - 40) / FOCAL, (torch.rand((pairs, n), **f64) - 0.5) * (W - 40) / FOCAL], 2)
    d = torch.rand((pairs, n, 1), **f64) * 5 + 2
    X = torch.cat([xl * d, d], 2).float()
    X = torch.where((torch.rand((pairs, n), **f64) < 0.10)[..., None], torch.full_like(X, float("nan")), X)
    R, t = rotation(torch, 0.05 * torch.randn((pairs, 3), **f64)), 0.15 * torch.randn((pairs, 3), **f64)
    R0, t0 = rotation(torch, 0.5 * torch.randn((pairs, 3), **f64)), torch.randn((pairs, 3), **f64)
    T0 = torch.eye(4, dtype=torch.float64, device=dev).repeat(pairs, 1, 1)
    T1 = T0.clone()
    T0[:, :3, :3], T0[:, :3, 3] = R0, t0
    T1[:, :3, :3], T1[:, :3, 3] = R @ R0, (R @ t0[:, :, None])[:, :, 0] + t
    Y = torch.nan_to_num(X.double(), nan=1.0) @ R.transpose(1, 2) + t[:, None, :]
    q = Y[..., :2] / Y[..., 2:3] * FOCAL + torch.tensor([H / 2, W / 2], device=dev, dtype=torch.float64)
    ang, mag = torch.rand((pairs, n), **f64) * 6.283185307179586, torch.rand((pairs, n), **f64) * 6
    mr = (q + mag[..., None] * torch.stack([ang.cos(), ang.sin()], 2)).float()
    mr = torch.where((torch.rand((pairs, n), **f64) < 0.03)[..., None], torch.full_like(mr, float("nan")), mr)
    maps = torch.full((pairs, H, W), 4.0, device=dev)
    i, j = torch.round(q[..., 0]).long().clamp(0, H - 1), torch.round(q[..., 1]).long().clamp(0, W - 1)
    depth = Y[..., 2] * torch.where(torch.rand((pairs, n), **f64) < 0.10, 0.6, 1.0)          # 10 % of the taps lie in front: occluded
    depth = torch.where(torch.rand((pairs, n), **f64) < 0.05, torch.zeros_like(depth), depth)   # 5 % holes
    maps[torch.arange(pairs, device=dev)[:, None].expand(pairs, n), i, j] = depth.float()
    return {"X": X.reshape(-1, 3).contiguous(), "mr": mr.reshape(-1, 2).contiguous(), "T1": T1, "T0": T0, "norm": norm, "maps": maps,
            "conf": torch.rand((pairs * n,), generator=gen, device=dev), "mask": (torch.rand((pairs * n,), generator=gen, device=dev) < 0.5).to(torch.uint8),
            "size_r": torch.tensor([H, W], dtype=torch.float32, device=dev).repeat(pairs, 1).contiguous()}


def torch_chain(torch, b, pairs, n):
    """The stage's seven outputs by torch operations on the device, float64 (the yardstick: what a caller would otherwise write)."""
    dev = b["X"].device
    R1, t1, R0, t0 = b["T1"][:, :3, :3], b["T1"][:, :3, 3], b["T0"][:, :3, :3], b["T0"][:, :3, 3]
    Rg = R1 @ R0.transpose(1, 2)
    tg = t1 - (Rg @ t0[:, :, None])[:, :, 0]
    X, p = b["X"].view(pairs, n, 3), b["mr"].view(pairs, n, 2).double()
    conf, mask = b["conf"].view(pairs, n), b["mask"].view(pairs, n) != 0
    Y = X.double() @ Rg.transpose(1, 2) + tg[:, None, :]
    nr = b["norm"][:, 4:].double()
    q = Y[..., :2] / Y[..., 2:3] / nr[:, None, 2:] + nr[:, None, :2]
    part = torch.isfinite(p).all(2) & (conf >= MIN_CONF)
    no_depth = ~torch.isfinite(X).all(2)
    behind = ~torch.isfinite(Y).all(2) | ~(Y[..., 2] > 0)
    hw = b["size_r"].double()
    outside = ~((q[..., 0] >= 0) & (q[..., 0] <= hw[:, None, 0] - 1) & (q[..., 1] >= 0) & (q[..., 1] <= hw[:, None, 1] - 1))
    ij = torch.round(torch.nan_to_num(q, nan=-1.0, posinf=-1.0, neginf=-1.0))                # half to even
    inb = (ij[..., 0] >= 0) & (ij[..., 0] < H) & (ij[..., 1] >= 0) & (ij[..., 1] < W)
    rows = torch.arange(pairs, device=dev)[:, None].expand(pairs, n)
    d1 = b["maps"][rows, ij[..., 0].long().clamp(0, H - 1), ij[..., 1].long().clamp(0, W - 1)].double()
    no_tap = ~inb | ~torch.isfinite(d1) | ~(d1 > 0)
    hidden = (Y[..., 2] - d1).abs() > OCCL * d1
    status = torch.full((pairs, n), 1, dtype=torch.uint8, device=dev)
    for flag, value in ((hidden, 6), (no_tap, 5), (outside, 4), (behind, 3), (no_depth, 2), (~part, 0)):   # the first rule wins: applied last
        status = torch.where(flag, torch.full_like(status, value), status)
    scored = status == 1
    e = q - p
    err = torch.where(scored, (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]).sqrt(), torch.full_like(e[..., 0], float("nan")))
    tally = torch.stack([(status == v).sum(1) for v in range(7)] + [torch.zeros(pairs, dtype=torch.int64, device=dev)], 1)
    thr = torch.tensor(THR, dtype=torch.float64, device=dev)
    within = scored[..., None] & (err[..., None] <= thr)
    correct = within.sum(1)
    err_sum = torch.where(scored, err, torch.zeros_like(err)).sum(1)
    at = scored[..., None] & (conf[..., None] >= torch.tensor(EDGES, dtype=torch.float32, device=dev))
    sweep = torch.cat([at.sum(1)[..., None], torch.einsum("pnb,pnk->pbk", at.double(), within.double()).round().long()], 2)
    good = within[..., 0]
    confusion = torch.stack([(scored & mask & good).sum(1), (scored & mask & ~good).sum(1), (scored & ~mask & good).sum(1),
                             (scored & ~mask & ~good).sum(1)], 1)
    return err.reshape(-1), status.reshape(-1), tally, correct, err_sum, sweep, confusion


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"min": min(v), "q1": q[0], "median": q[1], "q3": q[2], "max": max(v)}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_error.py: no GPU - nothing to measure")
    from pats_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(8642)
    pairs, n = args.pairs, args.matches
    b = planted_batch(torch, gen, pairs, n)
    seg = {"stride": n, "counts": torch.full((pairs,), n, dtype=torch.int64, device=dev)}
    table = ops.lift_table([b["maps"][k] for k in range(pairs)])

    def stage(out=None):
        return ops.match_error_by_pair(b["X"], b["mr"], b["T1"], T0=b["T0"], thr=THR, norm=b["norm"], swapped=False, table_r=table, occl_rel=OCCL,
                                       size_r=b["size_r"], conf=b["conf"], min_conf=MIN_CONF, edges=EDGES, mask=b["mask"], out=out, **seg)

    dest = stage()
    ms, wall, last = {"chain": [], "stage": []}, {"chain": [], "stage": []}, None
    for i in range(args.launches + 3):
        for which in ("chain", "stage"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            if which == "chain":
                last = torch_chain(torch, b, pairs, n)
            else:
                stage(dest)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= 3:
                ms[which].append(e0.elapsed_time(e1))
                wall[which].append((t1 - t0) * 1e3)
    for k, name in ((1, "status"), (2, "tally"), (3, "correct"), (5, "sweep"), (6, "confusion")):
        assert torch.equal(dest[k], last[k]), "the stage's %s is not the chain's" % name
    sc = dest[1] == 1
    diff = float((dest[0][sc] - last[0][sc]).abs().max())
    assert diff <= 1e-9 and torch.equal(torch.isnan(dest[0]), torch.isnan(last[0])), "err differs from the chain's by %g px" % diff
    c, f = quartiles(ms["chain"]), quartiles(ms["stage"])
    wc, wf = quartiles(wall["chain"]), quartiles(wall["stage"])
    tally = dest[2].sum(0).tolist()
    print(json.dumps({"tool": "bench_match_error", "pairs": pairs, "matches_per_pair": n, "launches": args.launches, "n_thr": len(THR),
                      "bins": len(EDGES), "chain_device_ms": c, "stage_device_ms": f, "chain_wall_ms": wc, "stage_wall_ms": wf,
                      "chain_over_stage_device": c["median"] / f["median"], "chain_over_stage_wall": wc["median"] / wf["median"],
                      "chain_device_spread_ms": c["q3"] - c["q1"], "largest_err_difference_px": diff, "rows_per_status": tally[:7],
                      "precision_at_thr": [float(v) / max(tally[1], 1) for v in dest[3].sum(0).tolist()]}))


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
