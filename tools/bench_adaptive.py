#!/usr/bin/env python3
"""Per-pair adaptive verification (ops.epipolar_score_adaptive_by_pair, csrc/adaptive.hip + csrc/epipolar.hip) against the
fixed-budget entry (ops.epipolar_score_by_pair, whose kernels this feature leaves as they were) on the SAME inputs.

Workload: a YFCC-like batch - 48 pairs of 4000 matches each in normalised coordinates, on="all" (ragged segments) - with PLANTED
inlier ratios: a share of a pair's matches lies on the epipolar lines of one model, which sits at a random index of the pair's H
unit models; the rest of the matches and of the models is random.  Ratios 0.8, 0.5 and 0.2 alone, and mixed within one batch (a
third of the pairs each); H = 1024 and 4096 at confidence = 1 - 1e-5 with 8-point samples (sample_size 8, round_models 256), then
a sweep over small H at ratio 0.8 for the budget below which the extra launches do not pay.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/adaptive_bench.json.  A step that fails or runs out of time ends the driver.

--measure: after three untimed calls of each entry the two alternate, --launches times each, preallocated outputs, device events
around every call (the fills and every launch of the call), minimum and median.  Per case also: the models actually tested (the sum
of used against pairs * H) and the pairs that stopped early.  The two entries' outputs are compared where the definition makes them
equal (counts below used).

usage: bench_adaptive.py [--measure] [--pairs 48] [--matches 4000] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIDENCE = 1 - 1e-5
SAMPLE_SIZE, ROUND_MODELS = 8, 256


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_adaptive: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "adaptive_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def planted_batch(torch, gen, pairs, n, H, ratios):
    """-> (ml, mr [pairs * n, 2], pair_off, models [pairs,H,3,3], thr): pair p has round(ratios[p % len] * n) matches on the epipolar
    lines of models[p, true[p]]."""
    dev = gen.device
    models = torch.randn((pairs, H, 3, 3), generator=gen, device=dev, dtype=torch.float64)
    models = models / models.reshape(pairs, H, 9).norm(dim=2)[:, :, None, None]
    true = torch.randint(0, H, (pairs,), generator=gen, device=dev)
    E = models[torch.arange(pairs, device=dev), true]                                  # [pairs,3,3]
    xl = torch.rand((pairs, n, 2), generator=gen, device=dev, dtype=torch.float64) * 1.2 - 0.6
    u = torch.rand((pairs, n, 2), generator=gen, device=dev, dtype=torch.float64) * 1.2 - 0.6
    a = torch.einsum("pij,pnj->pni", E, torch.cat([xl, torch.ones((pairs, n, 1), device=dev, dtype=torch.float64)], 2))
    d = (a[..., 0] * u[..., 0] + a[..., 1] * u[..., 1] + a[..., 2]) / (a[..., 0] ** 2 + a[..., 1] ** 2)
    on_line = u - d[..., None] * a[..., :2]                                            # the foot of u on the line E x_l
    share = torch.tensor([ratios[p % len(ratios)] for p in range(pairs)], device=dev, dtype=torch.float64)
    inlier = torch.rand((pairs, n), generator=gen, device=dev, dtype=torch.float64) < share[:, None]
    xr = torch.where(inlier[..., None], on_line, u * (0.8 / 0.6))
    off = torch.arange(pairs + 1, device=dev, dtype=torch.int64) * n
    thr = torch.full((pairs,), 2e-3, device=dev)
    return xl.float().reshape(-1, 2).contiguous(), xr.float().reshape(-1, 2).contiguous(), off, models.float().contiguous(), thr


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaptive.py: no GPU - nothing to measure")
    from pats_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    pairs, n = args.pairs, args.matches
    cases = [("H=%d ratio=%s" % (H, "mixed" if len(r) > 1 else r[0]), H, r) for H in (1024, 4096) for r in ((0.8,), (0.5,), (0.2,), (0.8, 0.5, 0.2))]
    cases += [("H=%d ratio=0.8 (small-budget sweep)" % H, H, (0.8,)) for H in (64, 128, 256, 512)]
    result = {"tool": "bench_adaptive", "pairs": pairs, "matches_per_pair": n, "confidence": CONFIDENCE, "sample_size": SAMPLE_SIZE,
              "round_models": ROUND_MODELS, "launches": args.launches, "cases": {}}
    for name, H, ratios in cases:
        ml, mr, off, models, thr = planted_batch(torch, gen, pairs, n, H, ratios)
        fixed = lambda out=None: ops.epipolar_score_by_pair(ml, mr, models, thr, pair_off=off, moments=True, out=out)          # noqa: E731
        adaptive = lambda out=None: ops.epipolar_score_adaptive_by_pair(ml, mr, models, thr, CONFIDENCE, SAMPLE_SIZE,          # noqa: E731
                                                                        round_models=ROUND_MODELS, pair_off=off, moments=True, out=out)
        dest = {"fixed": fixed(), "adaptive": adaptive()}
        ms = {"fixed": [], "adaptive": []}
        for i in range(args.launches + 3):
            for which, fn in (("fixed", fixed), ("adaptive", adaptive)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(dest[which])
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms[which].append(e0.elapsed_time(e1))
        used = dest["adaptive"][-2].cpu()
        cf, ca = dest["fixed"][0].cpu(), dest["adaptive"][0].cpu()
        assert all(torch.equal(ca[p, :int(used[p])], cf[p, :int(used[p])]) and not ca[p, int(used[p]):].any() for p in range(pairs))
        med = {k: statistics.median(v) for k, v in ms.items()}
        result["cases"][name] = {"H": H, "ratios": list(ratios), "fixed_ms": {"min": min(ms["fixed"]), "median": med["fixed"]},
                                 "adaptive_ms": {"min": min(ms["adaptive"]), "median": med["adaptive"]},
                                 "fixed_over_adaptive": med["fixed"] / med["adaptive"],
                                 "models_tested_share": float(used.sum()) / (pairs * H), "pairs_stopped_early": int((used < H).sum()),
                                 "launches_adaptive": 2 * -(-H // ROUND_MODELS) + 1}
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
