#!/usr/bin/env python3
"""The plane-and-parallax (DEGENSAC) stage (csrc/plane_parallax.hip) beside the torch chain it replaces, on the SAME inputs, in the
same session: --pairs pairs, a top-K each in the strided layout, 80 % of every pair's matches on one plane, H hypotheses.
  stage       ops.plane_parallax_hypotheses_by_pair -> ops.epipolar_score_by_pair -> ops.plane_parallax_select_by_pair
  torch       the plane's transfer test as a mask, ONE nonzero over the batch (a host read: the pool sizes), two random draws per
              hypothesis gathered from it, the cross products x' x Hp x, l_1 x l_2 and e x Hp in float64, the normalisation and the
              cast -> the same ops.epipolar_score_by_pair -> torch.where over count, mask, moments and model
  hypotheses  the two generators alone
The two sides draw different samples (the device's generator is counter-based, torch's is its own): the support they reach is
recorded beside the times, not compared bit for bit.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`, whose JSON line goes to
profiles/degensac_bench.json.  A step that fails or runs out of time ends the driver.

--measure (docs/measurement.md 5.5): after three untimed calls of each the two sides of a comparison alternate, --launches times
each, device events around every call (fills and launches) and the host's clock around call + synchronise; quartiles of both.
Recorded, not asserted: no time is a pass condition.

usage: bench_degensac.py [--measure] [--pairs 48] [--K 2048] [--H 256] [--launches 30] [--out-dir profiles] [--step-timeout 600]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_degensac: the measurement step ended with status %d; nothing else was started" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "degensac_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def planar_batch(torch, gen, pairs, K, on_plane=0.8, off_true=0.12):
    """[pairs,K,2] lists around a translating camera: on_plane of the matches on the plane's homography, off_true true matches off it
    (they move along the same epipole), the rest uniform -> (ml, mr, Hp [pairs,1,3,3])."""
    dev = gen.device
    ml = torch.rand((pairs, K, 2), generator=gen, device=dev) - 0.5
    Hp = torch.eye(3, device=dev).repeat(pairs, 1, 1) + 0.05 * (torch.rand((pairs, 3, 3), generator=gen, device=dev) - 0.5)
    a = torch.cat([ml, torch.ones((pairs, K, 1), device=dev)], 2) @ Hp.transpose(1, 2)
    on = a[..., :2] / a[..., 2:]
    epipole = torch.tensor([2.0, 0.3], device=dev)
    depth = 0.02 + 0.1 * torch.rand((pairs, K, 1), generator=gen, device=dev)
    off = on + depth * (on - epipole)                                      # parallax along the line to the epipole
    noise = torch.rand((pairs, K, 2), generator=gen, device=dev) - 0.5
    u = torch.rand((pairs, K, 1), generator=gen, device=dev)
    mr = torch.where(u < on_plane, on, torch.where(u < on_plane + off_true, off, noise))
    return ml.contiguous(), mr.contiguous(), Hp[:, None].contiguous()


def torch_hypotheses(torch, ml, mr, Hp, thr, parallax, H, gen):
    """The chain a caller without the stage writes: mask, nonzero, gather, cross products -> models [pairs,H,3,3] float32."""
    pairs, K = ml.shape[:2]
    Hd = Hp[:, 0].double()
    x = torch.cat([ml.double(), torch.ones((pairs, K, 1), dtype=torch.float64, device=ml.device)], 2)
    y = torch.cat([mr.double(), torch.ones((pairs, K, 1), dtype=torch.float64, device=ml.device)], 2)
    a = x @ Hd.transpose(1, 2)
    d = a[..., :2] - y[..., :2] * a[..., 2:]
    off = (d * d).sum(2) > ((parallax * thr.double()) ** 2)[:, None] * a[..., 2] ** 2
    where = off.nonzero()                                                  # the host read: the size of the result
    counts = off.sum(1)
    base = torch.cumsum(counts, 0) - counts
    j = (torch.rand((pairs, H, 2), generator=gen, device=ml.device) * counts[:, None, None]).long().clamp_(max=where.shape[0] - 1)
    at = where[(base[:, None, None] + j).clamp_(max=where.shape[0] - 1), 1]           # [pairs,H,2] positions inside the pair's list
    pick = lambda t: torch.gather(t[:, :, None].expand(-1, -1, 2, -1), 1, at[..., None].expand(-1, -1, -1, 3))      # noqa: E731
    ls = torch.linalg.cross(pick(y), pick(a))
    e = torch.linalg.cross(ls[:, :, 0], ls[:, :, 1])
    F = torch.linalg.cross(e[:, :, None, :].expand(-1, -1, 3, -1), Hd.transpose(1, 2)[:, None].expand(-1, H, -1, -1)).transpose(2, 3)
    F = F / F.flatten(2).norm(dim=2)[..., None, None]
    return torch.nan_to_num(F, nan=0.0, posinf=0.0, neginf=0.0).float().contiguous()


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_degensac.py: no GPU - nothing to measure")
    from bench_fundamental import alternate
    from pats_amd import ops
    dev = torch.device("cuda")
    pairs, K, H, parallax = args.pairs, args.K, args.H, 2.0
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    ml, mr, Hp = planar_batch(torch, gen, pairs, K)
    seg = {"stride": K, "counts": torch.full((pairs,), K, dtype=torch.int64, device=dev)}
    thr = torch.full((pairs,), 2e-3, device=dev)
    seeds = torch.arange(pairs, dtype=torch.int64, device=dev) + 11
    best_h = torch.zeros(pairs, dtype=torch.int32, device=dev)
    # the standing verification: the 7-point winner of a short budget, as a caller has it when the stage runs
    h7 = ops.epipolar_hypotheses7_by_pair(ml, mr, 16, seeds, **seg).reshape(pairs, -1, 3, 3)
    ver = ops.epipolar_score_by_pair(ml, mr, h7, thr, moments=True, **seg)
    standing = (h7, ver[1], ver[2], ver[3], ver[4])
    hyp_dest = ops.plane_parallax_hypotheses_by_pair(ml, mr, H, seeds, Hp, best_h, thr, parallax=parallax, **seg)
    score_dest = ops.epipolar_score_by_pair(ml, mr, hyp_dest[0], thr, moments=True, **seg)
    sel_dest = ops.plane_parallax_select_by_pair(ml, mr, thr, Hp, best_h, standing, (hyp_dest[0],) + tuple(score_dest[1:]), **seg)
    kept = {}

    def device_hypotheses():
        return ops.plane_parallax_hypotheses_by_pair(ml, mr, H, seeds, Hp, best_h, thr, parallax=parallax, out=hyp_dest, **seg)

    def stage():
        models = device_hypotheses()[0]
        new = ops.epipolar_score_by_pair(ml, mr, models, thr, moments=True, out=score_dest, **seg)
        kept["stage"] = ops.plane_parallax_select_by_pair(ml, mr, thr, Hp, best_h, standing, (models,) + tuple(new[1:]), out=sel_dest, **seg)

    def chain():
        models = torch_hypotheses(torch, ml, mr, Hp, thr, parallax, H, gen)
        new = ops.epipolar_score_by_pair(ml, mr, models, thr, moments=True, **seg)
        take = new[2] > standing[2]
        win = models[torch.arange(pairs, device=dev), new[1].long()]
        old = standing[0][torch.arange(pairs, device=dev), standing[1].long()]
        kept["torch"] = (torch.where(take[:, None, None], win, old), torch.where(take, new[2], standing[2]),
                         torch.where(take.repeat_interleave(K), new[3], standing[3]), torch.where(take[:, None, None], new[4], standing[4]))

    result = {"tool": "bench_degensac", "pairs": pairs, "K": K, "H": H, "parallax": parallax, "launches": args.launches,
              "pool_max": ops.plane_parallax_pool_max()}
    result["stage"] = alternate(torch, {"stage": stage, "torch": chain}, args.launches)
    result["hypotheses"] = alternate(torch, {"device": device_hypotheses,
                                             "torch": lambda: torch_hypotheses(torch, ml, mr, Hp, thr, parallax, H, gen)}, args.launches)
    for part in ("stage", "hypotheses"):
        a, b = result[part].keys()
        result[part]["torch_over_device"] = result[part][b]["device_ms"]["median"] / result[part][a]["device_ms"]["median"]
        result[part]["torch_over_device_wall"] = result[part][b]["wall_ms"]["median"] / result[part][a]["wall_ms"]["median"]
    result["support"] = {"standing_mean": float(standing[2].float().mean()), "stage_mean": float(kept["stage"][1].float().mean()),
                         "torch_mean": float(kept["torch"][1].float().mean()), "replaced": int(kept["stage"][-2].sum()),
                         "pool_mean": float(hyp_dest[1].float().mean())}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--H", type=int, default=256)
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
