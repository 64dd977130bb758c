#!/usr/bin/env python3
"""The subdivision gather's crops (Compute_imgs, a13 / a14) at the bench's workload shapes, and the glue between them and the fine
backbone.  Images and coarse matches are the bench's (BenchNets, 48 pairs of 480x640 on the 15x20 grid); the crops run over
the capacity with the count on the device, as batch.coarse_stage runs them.  Variants, alternated inside one process after a
warm-up, each timed with device events:
  a_fp32_plus_glue   fp32 images -> fp32 HWC crops, then the reference's glue in torch (second_layer.py:66-68):
                     normalize(x.permute(0,3,1,2).float().contiguous()) per side, torch.cat, then .to(bfloat16)
  b_fused_bf16       uint8 images -> CropFormat.backbone(bfloat16) crops written into buf[0] / buf[1] of ONE [2,cap,3,96,96]
                     buffer (the backbone reads buf.view(2 cap, 3, 96, 96): no glue)
  c_fp32_from_u8     uint8 images -> fp32 HWC crops (against a_crops_only_fp32: the same crops from fp32 images, no glue)
  d_bf16_hwc_from_fp32  fp32 images -> bf16 HWC crops, not normalised: the fp32 kernels' direct bf16 twins
Prints ONE JSON line with the median wall times.  Kernel times proper come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

usage: bench_crop_formats.py [--workload megadepth] [--pairs 48] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from benchlib.common import ITERS, WORKLOADS  # noqa: E402
from benchlib.nets import BenchNets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=None, help="pairs per step (default: the workload's, 48 for megadepth)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop_formats.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, _, default_pairs, _ = WORKLOADS[args.workload]
    pairs = args.pairs or default_pairs
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch)
    lefts, rights = nets.lefts, nets.rights
    H, W = int(lefts.shape[1]), int(lefts.shape[2])
    # the coarse level's matches, as batch.coarse_stage forms them
    mdesc0, mdesc1, scale, alpha = nets.coarse(lefts, rights)
    Z = ops.cost_ot(mdesc0, mdesc1, 1, alpha, scale, ITERS)
    scales, cflag = ops.colmass_sqrt(Z, return_flags=True)
    _, pts, xs, ys, ifn1, _ = ops.est_position_first(Z, scales, (H, W), 32, col_nomatch=cflag)
    del mdesc0, mdesc1, scale, Z
    # uint8 images holding the same values (the bench's images are integers 0..255 stored as float32 when they are; the
    # variants are timed on their own values either way)
    lefts_u8 = lefts.clamp(0, 255).round().to(torch.uint8)
    rights_u8 = rights.clamp(0, 255).round().to(torch.uint8)
    lefts_f, rights_f = lefts_u8.float(), rights_u8.float()
    n_cap = pairs * h * w
    fmt = ops.CropFormat.backbone(torch.bfloat16)
    mean = torch.tensor(fmt.mean, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(fmt.std, device=dev).view(1, 3, 1, 1)
    buf = torch.empty((2, n_cap, 3, 96, 96), dtype=torch.bfloat16, device=dev)

    def crops(l, r, **kw):
        return ops.Compute_imgs_ex(xs, ys, pts, ifn1, l, r, width=w, height=h, known_count="device", **kw)

    def a_fp32_plus_glue():
        o = crops(lefts_f, rights_f)
        sides = [(x.permute(0, 3, 1, 2).float().contiguous() - mean) / std for x in o[:2]]
        return torch.cat(sides).to(torch.bfloat16), o[7]

    def b_fused_bf16():
        o = crops(lefts_u8, rights_u8, crop_format=fmt, out=(buf[0], buf[1]))
        return buf.view(2 * n_cap, 3, 96, 96), o[7]

    def c_fp32_from_u8():
        o = crops(lefts_u8, rights_u8)
        return o[0], o[7]

    def d_bf16_hwc_from_fp32():
        o = crops(lefts_f, rights_f, crop_format=ops.CropFormat(torch.bfloat16))
        return o[0], o[7]

    def a_crops_only():
        o = crops(lefts_f, rights_f)
        return o[0], o[7]

    variants = {"a_fp32_plus_glue": a_fp32_plus_glue, "b_fused_bf16": b_fused_bf16, "c_fp32_from_u8": c_fp32_from_u8,
                "d_bf16_hwc_from_fp32": d_bf16_hwc_from_fp32, "a_crops_only_fp32": a_crops_only}
    times = {v: [] for v in variants}
    for it in range(args.warmup + args.steps):
        for v, fn in variants.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, K = fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[v].append(e0.elapsed_time(e1))
            del out
    K = int(K.item())
    # the fused output equals the glue's, bit for bit, on the crops in use
    ga, _ = a_fp32_plus_glue()
    gb, _ = b_fused_bf16()
    same = bool(torch.equal(ga[:K], gb[:K]) and torch.equal(ga[n_cap:n_cap + K], gb[n_cap:n_cap + K]))
    med = {v: statistics.median(t) for v, t in times.items()}
    res = {"tool": "bench_crop_formats", "workload": args.workload, "pairs": pairs, "grid": [h, w], "image": [H, W],
           "crops_in_use": K, "crop_capacity": n_cap, "steps": args.steps, "warmup": args.warmup,
           "median_wall_ms": med, "b_over_a": med["b_fused_bf16"] / med["a_fp32_plus_glue"],
           "c_over_a_crops_only": med["c_fp32_from_u8"] / med["a_crops_only_fp32"],
           "d_over_a_crops_only": med["d_bf16_hwc_from_fp32"] / med["a_crops_only_fp32"], "fused_equals_glue": same}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
