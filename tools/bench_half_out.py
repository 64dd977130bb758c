#!/usr/bin/env python3
"""The two descriptor gathers and the fine level's cost build + solve at the bench's row counts, for {fp32, bf16} maps x
{fp32, bf16} OUTPUT of the gathers, in both memory orders of the maps.  Each kernel is timed on its own with device events
(median of --reps launches after --warmup), and next to the milliseconds stands the achieved rate over the bytes the kernel
must move - arithmetic, not counters:

  fine gather, per stacked crop    145 nodes x (4 x 64 + 4 x 64 + 128) taps x element = 368 640 B (fp32 maps; half: 184 320 B)
                                   + 1 088 B title / dustbin features + 264 x 145 outputs x element (153 120 B / 76 560 B)
  third gather, per point          2 sides x 64 cells x 128 channels x element + 512 B dustbin features
                                   + 2 x 128 x 65 outputs x element
  fine cost_ot, per row            the two descriptor reads, 2 x 264 x 145 x element (306 240 B / 153 120 B); the solver's
                                   traffic is not counted, so this leg reports milliseconds only

"to_bf16_ms" is a separate .to(torch.bfloat16) pass over the float32 output: what a caller pays today for half descriptors
on top of the fp32-output gather.  On a checkout whose ops lack out_dtype (the parent of the change that added it) only the
fp32-output legs run, which is how the two commits are compared.

Prints ONE JSON line.

usage: bench_half_out.py [--rows 20208] [--points 111057] [--reps 7] [--warmup 2]"""
import argparse
import inspect
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

PEAK = 8.0e12       # bytes / s, MI355X HBM3E


def fill(shape, channels_last, chunk=512):
    """float32 standard-normal [n, C, H, W] in the given memory order, drawn in row chunks (no big temporaries)"""
    n, c, hh, ww = shape
    t = torch.empty((n, hh, ww, c), device="cuda").permute(0, 3, 1, 2) if channels_last else torch.empty(shape, device="cuda")
    for r in range(0, n, chunk):
        t[r:r + chunk].normal_()
    return t


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20208, help="fine-level rows (bench.py's default step: 48 pairs)")
    ap.add_argument("--points", type=int, default=111057, help="third-level problems of that step")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_out.py: no GPU - nothing to measure")
    from pats_amd import ops
    has_out = "out_dtype" in inspect.signature(ops.fine_descriptors).parameters
    R, P = args.rows, args.points
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4321)
    title = 0.5 * torch.randn((R, 8), device="cuda", generator=gen)
    rub = 1.5 * torch.randn((R, 264), device="cuda", generator=gen)
    kenc = 0.1 * torch.randn((128, 64), device="cuda", generator=gen)
    rub3 = 1.5 * torch.randn((R, 128, 144), device="cuda", generator=gen)
    mk0 = (torch.randint(1, 11, (P, 2), device="cuda", generator=gen) * 8 + 4).float()
    mk1 = torch.randint(8, 185, (P, 2), device="cuda", generator=gen).float() * 0.5
    b_ids = torch.sort(torch.randint(0, R, (P,), device="cuda", generator=gen))[0]      # a fine row's points are consecutive
    ns = (torch.rand((R, 1, 144), device="cuda", generator=gen) + 0.5).contiguous()
    one = torch.ones(1, device="cuda")
    result = {"tool": "bench_half_out", "rows": R, "points": P, "reps": args.reps, "warmup": args.warmup, "out_dtype_supported": has_out,
              "peak_bytes_per_s": PEAK, "legs": {}}
    outs = [torch.float32] + ([torch.bfloat16] if has_out else [])
    for layout in ("nchw", "channels_last"):
        cl = layout == "channels_last"
        for mdt in (torch.float32, torch.bfloat16):
            esz = 4 if mdt == torch.float32 else 2
            maps = [fill(s, cl).to(mdt) for s in ((2 * R, 64, 48, 48), (2 * R, 64, 24, 24), (2 * R, 128, 12, 12))]
            fmt = torch.channels_last if cl else torch.contiguous_format
            assert all(m.is_contiguous(memory_format=fmt) for m in maps)
            for odt in outs:
                osz = 4 if odt == torch.float32 else 2
                leg = {}
                desc = torch.empty((2, R, 264, 145), dtype=odt, device="cuda")
                ms, _ = timed(lambda: ops.fine_descriptors(maps, title, rub, out=desc), args.reps, args.warmup)
                nbytes = 2 * R * (368640 // 4 * esz + 1088 + 264 * 145 * osz)
                leg["fine_gather"] = {"ms": ms, "bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3), "of_peak": nbytes / (ms * 1e-3) / PEAK}
                if odt == torch.float32:
                    leg["fine_to_bf16_ms"] = timed(lambda: desc.to(torch.bfloat16), args.reps, args.warmup)[0]
                if mdt == torch.float32 or odt != torch.float32:      # the cost build reads the gather's output whatever the maps were
                    ms, _ = timed(lambda: ops.cost_ot(desc[0], desc[1], 2, one, ns, 100, bias_k=2.0, return_flags=True), args.reps,
                                  args.warmup)
                    leg["fine_cost_ot"] = {"ms": ms, "descriptor_bytes": R * 2 * 264 * 145 * osz}
                del desc
                result["legs"]["%s/maps_%s/out_%s" % (layout, str(mdt)[6:], str(odt)[6:])] = leg
            del maps
            torch.cuda.empty_cache()
            ff = [fill((R, 128, 52, 52), cl).to(mdt) for _ in range(2)]
            for odt in outs:
                osz = 4 if odt == torch.float32 else 2
                leg = result["legs"]["%s/maps_%s/out_%s" % (layout, str(mdt)[6:], str(odt)[6:])]
                t = (torch.empty((P, 128, 65), dtype=odt, device="cuda"), torch.empty((P, 128, 65), dtype=odt, device="cuda"))
                ms, _ = timed(lambda: ops.third_descriptors(ff[0], ff[1], mk0, mk1, b_ids, kenc, rub3, out=t), args.reps, args.warmup)
                nbytes = P * (2 * 64 * 128 * esz + 512 + 2 * 128 * 65 * osz)
                leg["third_gather"] = {"ms": ms, "bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3), "of_peak": nbytes / (ms * 1e-3) / PEAK}
                if odt == torch.float32:
                    leg["third_to_bf16_ms"] = timed(lambda: (t[0].to(torch.bfloat16), t[1].to(torch.bfloat16)), args.reps, args.warmup)[0]
                del t
            del ff
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
