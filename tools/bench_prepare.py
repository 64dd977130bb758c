#!/usr/bin/env python3
"""The image front end (ops.prepare_images, csrc/prepare.hip) at a YFCC-sized batch: --pairs pairs (96 images) of 1600 x 1200 uint8,
prepared the YFCC way at size = 1024 - against the same batch done with what a caller had before on the GPU.

Without --measure this is the driver: ONE GPU step, a child process under its own `timeout -k 10`:
  `bench_prepare.py --measure`  -> profiles/prepare_bench.json (the JSON line below)
A step that fails or runs out of time ends the driver.

--measure, one process:
  kernel     ops.prepare_images with a table made once (no allocation, no upload in the timed call) into preallocated stores, uint8
             and float32: after --warmup calls, device events around each of --launches calls (minimum and median, ms), and one
             window of --launches back-to-back calls between two events (ms per launch).  The bytes are the algorithm's: the crop
             windows read once plus the canvases written once; bytes/s = those over the window's time per launch
  torch      per image the window sliced, permuted to CHW, .float(), F.interpolate(mode="bilinear", align_corners=False) to the
             target, permuted back, F.pad to the pair's canvas; then batch.pack_pairs(keep_dtype=True) (its torch.cat into float32
             stores) - the plan (windows, targets, canvases) given, host work of the plan not timed.  Float bilinear: its values
             are within a grey level of the kernel's, not its bits
  ratio      torch over kernel (float32 stores), on the windows' ms
docs/kernels.md 4.20 holds what an MI355X gave.

usage: bench_prepare.py [--measure] [--pairs 48] [--h0 1200] [--w0 1600] [--size 1024] [--launches 50] [--warmup 5]
                        [--out-dir profiles] [--step-timeout 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def driver(args, passthrough):
    out_dir = os.path.join(REPO, args.out_dir)
    os.makedirs(out_dir, exist_ok=True)
    step = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--measure"] + passthrough
    p = subprocess.run(step, stdout=subprocess.PIPE, text=True, cwd=REPO)
    if p.returncode != 0:
        raise SystemExit("bench_prepare: the measurement step ended with status %d" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(out_dir, "prepare_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def timed(torch, call, launches, warmup):
    """-> per-call events (min, median) and one window of back-to-back calls, all in ms per call."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    torch.cuda.synchronize()
    return {"min": min(ms), "median": statistics.median(ms), "window": e0.elapsed_time(e1) / launches}


def measure(args):
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    dev = torch.device("cuda")
    pairs, h0, w0 = args.pairs, args.h0, args.w0
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    srcs = [tuple(torch.randint(0, 256, (h0, w0, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(2)) for _ in range(pairs)]
    plan = ops.prepare_plan([((h0, w0), (h0, w0))] * pairs, size=args.size)
    table = ops.prepare_table(srcs, plan)
    window_bytes = int((plan.h_c * plan.w_c).sum()) * 3
    result = {"tool": "bench_prepare", "images": 2 * pairs, "source": [h0, w0], "size": args.size,
              "target": [int(plan.h_t[0, 0]), int(plan.w_t[0, 0])], "canvas": [int(v) for v in plan.canvas[0]], "launches": args.launches,
              "window_bytes": window_bytes}
    for name, dt in (("uint8", torch.uint8), ("float32", torch.float32)):
        left, right = torch.empty(plan.elems, dtype=dt, device=dev), torch.empty(plan.elems, dtype=dt, device=dev)
        t = timed(torch, lambda: ops.prepare_images(srcs, plan, left, right, table=table), args.launches, args.warmup)
        nbytes = window_bytes + 2 * plan.elems * left.element_size()
        result["kernel_" + name] = dict(t, bytes=nbytes, tb_per_s=nbytes / (t["window"] * 1e-3) / 1e12)
        print("prepare_images %-7s %.3f ms per launch (events: min %.3f, median %.3f), %.2f TB/s of %d algorithmic bytes"
              % (name, t["window"], t["min"], t["median"], result["kernel_" + name]["tb_per_s"], nbytes))

    def torch_way():
        prepared = []
        for p, pr in enumerate(srcs):
            H, W = int(plan.canvas[p, 0]), int(plan.canvas[p, 1])
            out = []
            for s, img in enumerate(pr):
                y0, x0, h_c, w_c, h_t, w_t = (int(getattr(plan, k)[p, s]) for k in ("y0", "x0", "h_c", "w_c", "h_t", "w_t"))
                x = img[y0:y0 + h_c, x0:x0 + w_c].permute(2, 0, 1)[None].float()
                x = F.interpolate(x, size=(h_t, w_t), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
                out.append(F.pad(x, (0, 0, 0, W - w_t, 0, H - h_t)))
            prepared.append(tuple(out))
        return batch.pack_pairs(prepared, keep_dtype=True)

    pk = torch_way()
    ours = torch.empty(plan.elems, dtype=torch.float32, device=dev)
    ops.prepare_images(srcs, plan, ours, torch.empty_like(ours), table=table)
    result["max_abs_diff_to_torch"] = float((pk.left - ours).abs().max())
    t = timed(torch, torch_way, max(5, args.launches // 5), 2)
    result["torch_float32"] = t
    result["torch_over_kernel"] = t["window"] / result["kernel_float32"]["window"]
    print("torch composition      %.3f ms per batch (events: min %.3f, median %.3f): %.1f x the kernel's float32 time; values within %.3f"
          % (t["window"], t["min"], t["median"], result["torch_over_kernel"], result["max_abs_diff_to_torch"]))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--pairs", type=int, default=48)
    ap.add_argument("--h0", type=int, default=1200)
    ap.add_argument("--w0", type=int, default=1600)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds the driver's GPU step may take")
    args, _ = ap.parse_known_args()
    if args.measure:
        measure(args)
    else:
        driver(args, [a for a in sys.argv[1:] if a != "--measure"])


if __name__ == "__main__":
    main()
