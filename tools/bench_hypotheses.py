#!/usr/bin/env python3
"""Per-pair 8-point hypotheses (batch.hypothesize_by_pair / ops.epipolar_hypotheses_by_pair, csrc/hypotheses.hip) at the verification
bench's shape: default workload, 48 pairs per step, confidence=True, H = 1024 hypotheses per pair, on="topk" (K = 2048,
progressive) and on="all" (every match).

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_hypotheses.py --measure`  -> profiles/hypotheses_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process after a warm-up step:
  kernel   ops.epipolar_hypotheses_by_pair alone on one step's top-K and on its regrouped matches, preallocated outputs (models and
           sample_idx), device events around every call (one kernel), minimum and median of --launches calls
  torch    the same stage written with torch on the same device and tensors: the header's sampler over [pairs, H] in int64
           arithmetic (masked to 32 bits), a gather of the samples, the [pairs*H, 8, 9] constraint matrices and ONE
           torch.linalg.svd over them, the last right singular vector.  For on="all" the offsets must reach the host first
           (summary.cpu()).  Wall time from a synchronised device to a synchronised device, against the device path's wall time
           over the same span.  The comparison partner, not the code under test; its samples must equal the kernel's, and both
           solvers' backward errors |A e| / (eps32 |A|_F) are reported
  step     batch.forward_pairs + topk_by_pair + hypothesize_by_pair + verify_by_pair (on="topk") against the same step that stops
           at topk_by_pair, alternating

usage: bench_hypotheses.py [--measure] [--workload megadepth] [--pairs 48] [--K 2048] [--H 1024] [--steps 4] [--warmup 2]
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

M32 = 0xFFFFFFFF


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_hypotheses: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "hypotheses_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def torch_mix(x):
    x = x & M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def torch_hypotheses(torch, ml, mr, lo, n, seeds, H, norm, progressive):
    """The partner.  ml, mr [cap,2]; lo, n, seeds int64 [pairs] on the device (every n >= 8) -> (models [pairs,H,9], idx [pairs,H,8])."""
    pairs, dev = n.numel(), ml.device
    h = torch.arange(H, dtype=torch.int64, device=dev)[None, :]
    m = n[:, None].expand(pairs, H)
    if progressive:
        m = torch.clamp((n[:, None] * (h + 1) + H - 1) // H, min=8)
    s_lo, s_hi = seeds & M32, (seeds >> 32) & M32
    k = torch_mix((torch_mix(torch_mix(s_lo) ^ s_hi)[:, None] + h) & M32)
    idx = torch.empty((pairs, H, 8), dtype=torch.int64, device=dev)
    for t in range(8):
        u = torch_mix((k + ((0x9E3779B9 * (t + 1)) & M32)) & M32)
        j = (u * (m - t)) >> 32
        if t:
            prev = torch.sort(idx[:, :, :t], dim=2).values
            for i in range(t):
                j = j + (prev[:, :, i] <= j)
        idx[:, :, t] = j
    rows = (lo[:, None, None] + idx).reshape(-1)
    xl = ((ml[rows].view(pairs, H, 8, 2) - norm[:, None, None, 0:2]) * norm[:, None, None, 2:4])
    xr = ((mr[rows].view(pairs, H, 8, 2) - norm[:, None, None, 4:6]) * norm[:, None, None, 6:8])
    one = torch.ones((pairs, H, 8, 1), device=dev)
    A = (torch.cat([xr, one], 3)[..., :, None] * torch.cat([xl, one], 3)[..., None, :]).reshape(pairs * H, 8, 9)
    e = torch.linalg.svd(A).Vh[:, 8, :]
    return e.view(pairs, H, 9), idx


def backward_error(torch, ml, mr, lo, idx, norm, models):
    """max |A e| / (eps32 |A|_F) in float64 over the nonzero models."""
    pairs, H = idx.shape[:2]
    rows = (lo[:, None, None] + idx.long()).reshape(-1)
    xl = ((ml[rows].view(pairs, H, 8, 2) - norm[:, None, None, 0:2]) * norm[:, None, None, 2:4]).double()
    xr = ((mr[rows].view(pairs, H, 8, 2) - norm[:, None, None, 4:6]) * norm[:, None, None, 6:8]).double()
    one = torch.ones((pairs, H, 8, 1), dtype=torch.float64, device=ml.device)
    A = (torch.cat([xr, one], 3)[..., :, None] * torch.cat([xl, one], 3)[..., None, :]).reshape(pairs, H, 8, 9)
    e = models.reshape(pairs, H, 9).double()
    q = torch.einsum("phtk,phk->pht", A, e).norm(dim=2) / (2.0 ** -23 * A.reshape(pairs, H, 72).norm(dim=2))
    return float(q[e.abs().sum(2) > 0].max())


def measure(args):
    import torch
    from benchlib.common import ITERS, WORKLOADS
    from benchlib.nets import BenchNets
    if not torch.cuda.is_available():
        raise SystemExit("bench_hypotheses.py: no GPU - nothing to measure")
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
    variants = ("topk", "topk+hypothesize+verify")
    times = {v: [] for v in variants}
    last = {}

    def step(v, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, **kw)
        batch.topk_by_pair(out, cap, K)
        if v != "topk":
            models = batch.hypothesize_by_pair(out, cap, H, seed=7, norm=norm)
            batch.verify_by_pair(out, cap, models, thr, norm=norm, on="topk", moments=True)
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
    ml, mr = out["by_pair"][:2]
    tl, tr, _, _, tn = out["topk"]
    offs = out["summary"].cpu().tolist()
    lens = [offs[p + 1] - offs[p] for p in range(pairs)]
    seeds = torch.arange(pairs, dtype=torch.int64, device=dev) + 7
    forms = {"topk": (dict(matches_l=tl, matches_r=tr, stride=K, counts=tn), True),
             "all": (dict(matches_l=ml, matches_r=mr, pair_off=out["summary"], pairs=pairs), False)}
    result = {"tool": "bench_hypotheses", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w], "K": K, "H": H,
              "M": offs[pairs + 1], "steps": args.steps, "warmup": args.warmup, "launches": args.launches,
              "matches_per_pair": {"min": min(lens), "median": statistics.median(lens), "max": max(lens)}, "on": {}}
    for on, (a, progressive) in forms.items():
        dest = ops.epipolar_hypotheses_by_pair(H=H, seed=seeds, norm=norm, progressive=progressive, return_samples=True, **a)
        again = tuple(torch.empty_like(t) for t in dest)
        ms = []
        for i in range(args.launches + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.epipolar_hypotheses_by_pair(H=H, seed=seeds, norm=norm, progressive=progressive, return_samples=True, out=again, **a)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        assert torch.equal(dest[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(dest[1], again[1])
        fl, fr = (ml, mr) if on == "all" else (tl.reshape(-1, 2), tr.reshape(-1, 2))
        if on == "all":
            lo_d, n_d = out["summary"][:pairs], out["summary"][1:pairs + 1] - out["summary"][:pairs]
        else:
            lo_d, n_d = torch.arange(pairs, dtype=torch.int64, device=dev) * K, tn
        r = {"hypotheses": pairs * H, "call_ms": {"min": min(ms), "median": statistics.median(ms)},
             "zero_models": int((dest[0].reshape(pairs * H, 9).abs().sum(1) == 0).sum()),
             "device_backward_error": backward_error(torch, fl, fr, lo_d, dest[1], norm, dest[0])}
        if not args.no_torch:
            assert int(n_d.min()) >= 8
            wall = {"device": [], "torch": []}
            for i in range(args.torch_launches + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.epipolar_hypotheses_by_pair(H=H, seed=seeds, norm=norm, progressive=progressive, return_samples=True, out=again, **a)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if on == "all":                                               # the offsets must reach the host before anything is sized
                    o = out["summary"].cpu()
                    lo_t, n_t = o[:pairs].to(dev), (o[1:pairs + 1] - o[:pairs]).to(dev)
                else:
                    lo_t, n_t = lo_d, tn
                e, idx = torch_hypotheses(torch, fl, fr, lo_t, n_t, seeds, H, norm, progressive)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if i >= 1:
                    wall["device"].append((t1 - t0) * 1e3)
                    wall["torch"].append((t2 - t1) * 1e3)
            assert torch.equal(idx.int(), again[1]), "the torch sampler and the kernel disagree"
            r["wall_ms"] = {k: {"min": min(x), "median": statistics.median(x)} for k, x in wall.items()}
            r["torch_over_device_wall"] = statistics.median(wall["torch"]) / statistics.median(wall["device"])
            r["torch_over_device_call"] = statistics.median(wall["torch"]) / statistics.median(ms)
            r["torch_backward_error"] = backward_error(torch, fl, fr, lo_d, idx, norm, e)
        result["on"][on] = r
    med = {v: statistics.median(times[v]) for v in variants}
    result["step_ms"] = {v: {"median": med[v], "all": times[v]} for v in variants}
    result["step_with_over_without"] = med[variants[1]] / med[variants[0]]
    result["best_count_on_topk"] = {"min": int(out["verified"][2].min()), "max": int(out["verified"][2].max())}
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
