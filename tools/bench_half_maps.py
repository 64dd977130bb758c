#!/usr/bin/env python3
"""The bench's step (batch.forward_pairs on BenchNets, default workload) with the five backbone maps m0 / m1 / m2 / ff0 / ff1
handed over as fp32, bf16, f16, and bf16 converted with .float() inside the callbacks (what a user with a bf16 backbone had to
do before the gathers took half maps), on NCHW and channels-last maps.  The variants alternate inside one process after a
warm-up; every step is timed with device events, the two gathers (and the .float() conversions) inside it as well.
Prints ONE JSON line: per layout and variant pairs/s, median event times of the fine / third gathers per step, and their
algorithmic HBM bytes (from the shapes) with the share of 8 TB/s those times give.
Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

The bench's workload shapes with 16 pairs per step (--pairs) and the row capacity of a dry run: fp32 + bf16 + f16 maps and the
.float() copies of the last variant live side by side in HBM.

usage: bench_half_maps.py [--workload megadepth] [--pairs 16] [--steps 6] [--warmup 2] [--layouts nchw,channels_last]"""
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

MAPS = ("m0", "m1", "m2", "ff0", "ff1")
HBM = 8.0e12                      # MI355X peak HBM bandwidth, bytes/s


def fine_bytes_per_crop(el):
    """a15 per stacked crop: 4 taps x 64 ch x 144 points of maps 0 and 1, 128 ch x 144 of map 2 in `el`-byte elements; desc
    [264,145] fp32 out, title + dustbin feature in."""
    return (2 * 4 * 64 * 144 + 128 * 144) * el + 264 * 145 * 4 + (8 + 264) * 4


def third_bytes_per_point(el):
    """a16 per point: two 8x8x128 windows in `el`-byte elements; two [128,65] fp32 out, the dustbin feature column, the
    points in and the rounded points out."""
    return 2 * 64 * 128 * el + 2 * 128 * 65 * 4 + 128 * 4 + 32


class FloatInside:
    """BenchNets whose callbacks get bf16 maps and call .float() on them before the gathers (timed as 'convert')."""

    def __init__(self, nets):
        self.nets = nets

    def __getattr__(self, name):
        return getattr(self.nets, name)

    def _widened(self, names, tag):
        n = self.nets
        e = n._timed(tag)
        saved = {k: getattr(n, k) for k in names}
        for k in names:
            setattr(n, k, saved[k].float())
        if e is not None:
            e.record()
        return saved

    def fine(self, rows, new_left, new_right):
        saved = self._widened(("m0", "m1", "m2"), "convert_fine")
        try:
            return self.nets.fine(rows, new_left, new_right)
        finally:
            for k, t in saved.items():
                setattr(self.nets, k, t)

    def third(self, rows, mk0, mk1, b_ids, P_dev):
        saved = self._widened(("ff0", "ff1"), "convert_third")
        try:
            return self.nets.third(rows, mk0, mk1, b_ids, P_dev)
        finally:
            for k, t in saved.items():
                setattr(self.nets, k, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="megadepth")
    ap.add_argument("--pairs", type=int, default=16,
                    help="pairs per step (the bench's 48 do not fit four copies of the maps in HBM)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layouts", default="nchw,channels_last")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_maps.py: no GPU - nothing to measure")
    from pats_amd import batch, ops
    h, w, if_local, outdoor, _, _ = WORKLOADS[args.workload]
    pairs = args.pairs
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    layouts = args.layouts.split(",")
    # the row capacity from a dry run of the coarse stage (bench.py --rows-cap dry-run): the maps exist for rows in use only
    nets = BenchNets(ops, dev, gen, cap, h, w, batch=batch, channels_last=layouts[0] == "channels_last", rows_cap_policy="dry-run")
    kw = dict(if_outdoor=outdoor, merge_new=True, iters=ITERS)
    result = {"tool": "bench_half_maps", "workload": args.workload, "pairs_per_step": pairs, "grid": [h, w],
              "steps": args.steps, "warmup": args.warmup, "layouts": {}}
    for layout in layouts:
        nets.set_layout(layout == "channels_last")
        fp32 = {k: getattr(nets, k) for k in MAPS}
        bf16 = {k: t.to(torch.bfloat16) for k, t in fp32.items()}
        f16 = {k: t.to(torch.float16) for k, t in fp32.items()}
        variants = {"fp32": (fp32, nets, 4), "bf16": (bf16, nets, 2), "f16": (f16, nets, 2),
                    "bf16_float_in_callback": (bf16, FloatInside(nets), 2)}
        times = {v: {"step": [], "fine_desc": [], "third_desc": [], "convert_fine": [], "convert_third": []} for v in variants}
        counts = {}

        def step(v, record):
            maps, n, _ = variants[v]
            for k, t in maps.items():
                setattr(nets, k, t)
            nets.ev = {} if record else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = batch.forward_pairs(nets.lefts, nets.rights, n, cap, **kw)
            e1.record()
            torch.cuda.synchronize()
            if record:
                times[v]["step"].append(e0.elapsed_time(e1))
                for tag, evs in nets.ev.items():
                    times[v][tag].append(sum(a.elapsed_time(b) for a, b in evs))
            counts[v] = (int(out["rows"].chunk_base[-1].item()), int(out["P"].item()), int(out["M"].item()))
            nets.ev = None

        for _ in range(args.warmup):
            for v in variants:
                step(v, False)
        for _ in range(args.steps):
            for v in variants:
                step(v, True)
        # bf16 maps and their .float() copies give the same bits, hence the same counts; fp32 / f16 maps hold other values
        assert counts["bf16"] == counts["bf16_float_in_callback"], counts
        res = {}
        for v, (maps, _, el) in variants.items():
            rows, P, M = counts[v]
            t = times[v]
            med = {k: statistics.median(x) for k, x in t.items() if x}
            fb, tb = 2 * rows * fine_bytes_per_crop(el), P * third_bytes_per_point(el)
            r = {"rows": rows, "P": P, "M": M, "pairs_per_s": pairs / (med["step"] * 1e-3), "step_ms": med["step"],
                 "fine_desc_ms": med["fine_desc"], "third_desc_ms": med["third_desc"],
                 "fine_desc_alg_bytes": fb, "third_desc_alg_bytes": tb,
                 "fine_desc_share_of_8TBps": fb / (med["fine_desc"] * 1e-3) / HBM,
                 "third_desc_share_of_8TBps": tb / (med["third_desc"] * 1e-3) / HBM}
            if "convert_fine" in med:
                r["convert_fine_ms"], r["convert_third_ms"] = med["convert_fine"], med["convert_third"]
            res[v] = r
        result["layouts"][layout] = res
        for k, t in fp32.items():
            setattr(nets, k, t)
        for d in (variants, bf16, f16, fp32):         # the half copies go before the maps are re-laid (HBM: the maps are large)
            d.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
