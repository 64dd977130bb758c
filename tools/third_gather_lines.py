#!/usr/bin/env python3
"""How many 128-byte lines the NCHW third-level gather (a16) has to fetch, at the bench's workload: the headroom of a gather that
shares lines between neighbouring points.

Runs ONE bench-shaped step (bench.py's default workload, seed and pairs, NCHW maps) through benchlib.nets.run_steps with a
BenchNets whose third() callback also keeps mkpts0_c, mkpts1_c, b_ids and the live count.  From those arrays, with the index
arithmetic of third_point_at (pats_amd/csrc/gather.hip: the rounding to the 4-px lattice, the clamp of mkpts1_c to [0, 96],
python floor division, the clamp of a cell's NHWC-view row to [0, B*52*52 - 1]), it counts the lines the 8x8 windows touch in
the [B, 128, 52, 52] fp32 maps:

  per point        lines touched per (point, side, channel), summed: what a gather without any reuse fetches
  per row          distinct lines per (fine row, side, channel) plane: the floor of a row-local kernel
  per tile of T    distinct lines per (tile of T consecutive points, side, channel), T = 4, 8, 16: the floor of a kernel that
                   shares lines among the T points of one workgroup (tiles start at multiples of T, as third_desc_kernel's)

A plane is 52 * 52 * 4 = 10 816 bytes, 84.5 lines: even channels start on a line boundary, odd ones half-way into a line, and
the count is taken for each parity (64 channels each).  Lines of two planes that share a line at the boundary are counted
once per plane.  Also printed: the algorithmic window bytes and the points-per-row histogram.

usage: third_gather_lines.py [--pairs N] [--out FILE]     (needs a GPU: the step runs on cuda:0)"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchlib.common import ITERS, WORKLOADS  # noqa: E402,F401
from benchlib.nets import BenchNets, run_steps  # noqa: E402

M, C, W, LINE = 52, 128, 8, 128
PLANE = M * M * 4


class KeepThird(BenchNets):
    """BenchNets whose third() callback also keeps its inputs (clones; the step's tensors are reused)."""

    def third(self, rows, mk0, mk1, b_ids, P_dev):
        self.kept = (mk0.detach().clone(), mk1.detach().clone(), b_ids.detach().clone(), P_dev.detach().clone())
        return super().third(rows, mk0, mk1, b_ids, P_dev)


def rint4(x):
    """round(x / 4) * 4 in fp32, half to even (torch.round / rintf)."""
    return (np.rint(x.astype(np.float32) / np.float32(4.0)).astype(np.int64)) * 4


def cell_rows(mk0, mk1, b, B):
    """[P, 2, 64] rows of the NHWC view each window cell reads, clamped as the kernel does (third_point_at + the cell loop)."""
    s0, s1 = rint4(mk0[:, 0]), rint4(mk0[:, 1])
    t = np.clip(mk1.astype(np.float32), np.float32(0.0), np.float32(96.0))
    q0, q1 = rint4(t[:, 0]), rint4(t[:, 1])
    i00 = np.stack([b * M * M + (s1 // 2 - W // 2 + 2) * M + (s0 // 2 - W // 2 + 2),
                    b * M * M + (q1 // 2 - W // 2 + 2) * M + (q0 // 2 - W // 2 + 2)], axis=1)       # python floor division
    lane = np.arange(64)
    i = i00[:, :, None] + (lane >> 3)[None, None, :] * M + (lane & 7)[None, None, :]
    return np.clip(i, 0, B * M * M - 1)


def line_keys(rows, parity):
    """Line of each cell within channel c's plane family: (bb * C + c) * PLANE + 4 r over 128, less the part every point of
    channel c shares (84 c + c // 2), so that keys of one channel compare across points; parity = c & 1."""
    bb = rows // (M * M)
    r = rows - bb * (M * M)
    return bb * (C * PLANE // LINE) + (64 * parity + 4 * r) // LINE


def distinct(groups, keys):
    """number of distinct (group, key) pairs: groups [P, 2] per (point, side), keys [P, 2, 64]."""
    g = np.broadcast_to(groups[:, :, None], keys.shape).reshape(-1).astype(np.int64)
    k = keys.reshape(-1).astype(np.int64)
    k = k - k.min()
    span = int(k.max()) + 1
    return int(np.unique(g * span + k).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--workload", default="megadepth", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pats_amd import batch, ops, synth
    dev = torch.device("cuda:0")
    h, w, if_local, outdoor, default_pairs, label = WORKLOADS[args.workload]
    pairs = args.pairs or default_pairs
    wl = {"outdoor": outdoor, "merge_new": outdoor, "bias_k": 2.0 if outdoor else 3.0}
    gen = torch.Generator(device=dev)
    gen.manual_seed(synth.SEED)                                   # bench.py's seed of rank 0
    cap = batch.Capacities(pairs, h, w, if_local=if_local)
    nets = KeepThird(ops, dev, gen, cap, h, w, batch=batch, channels_last=False)
    run_steps(batch, nets, cap, wl, None, 1, None)
    torch.cuda.synchronize()
    mk0, mk1, b_ids, P_dev = nets.kept
    B = nets.ff0.shape[0]
    P = int(P_dev.reshape(-1)[0].item())
    mk0 = mk0.reshape(-1, 2)[:P].cpu().numpy()
    mk1 = mk1.reshape(-1, 2)[:P].cpu().numpy()
    b = b_ids.reshape(-1)[:P].cpu().numpy().astype(np.int64)
    rows = cell_rows(mk0, mk1, b, B)
    side = np.arange(2)[None, :]
    out = []
    out.append("# NCHW third-level gather: 128-byte lines the windows touch (tools/third_gather_lines.py)")
    out.append("")
    out.append("workload %s, %d pairs per step (one step, seed of bench.py's rank 0): P = %d live points, %d fine rows with points, "
               "map tensor [%d, 128, 52, 52] fp32 per side" % (args.workload, pairs, P, np.unique(b).size, B))
    algo = P * 2 * C * 64 * 4
    out.append("algorithmic window bytes (2 sides x 128 ch x 64 cells x 4 B per point): %.3f GB" % (algo / 1e9))
    out.append("")
    out.append("| grouping | lines (even ch) | lines (odd ch) | lines per (group, side, channel) | GB per step | x algorithmic |")
    out.append("|---|---|---|---|---|---|")
    groupings = [("per point (no reuse)", np.arange(P)[:, None] * 2 + side, P)]
    groupings.append(("per fine row (row floor)", b[:, None] * 2 + side, np.unique(b).size))
    for T in (4, 8, 16):
        groupings.append(("per tile of %d points" % T, (np.arange(P) // T)[:, None] * 2 + side, (P + T - 1) // T))
    res = {}
    for name, groups, ngroups in groupings:
        n = [distinct(groups, line_keys(rows, par)) for par in (0, 1)]
        lines = 64 * (n[0] + n[1])
        res[name] = lines * LINE
        out.append("| %s | %d | %d | %.2f | %.3f | %.2f |" % (name, n[0], n[1], lines / (ngroups * 2 * C), lines * LINE / 1e9,
                                                            lines * LINE / algo))
    out.append("")
    out.append("(lines per (group, side, channel) = all lines / (groups x 2 sides x 128 channels); GB = lines x 128 B, both sides,"
               " all 128 channels)")
    out.append("")
    counts = np.bincount(np.unique(b, return_counts=True)[1])
    out.append("points per fine row: mean %.2f, median %d, max %d" % (P / np.unique(b).size,
                                                                      int(np.median(np.unique(b, return_counts=True)[1])),
                                                                      counts.size - 1))
    out.append("")
    out.append("| points in the row | rows |")
    out.append("|---|---|")
    for k in range(1, counts.size):
        if counts[k]:
            out.append("| %d | %d |" % (k, counts[k]))
    sorted_rows = bool(np.all(np.diff(b) >= 0))
    out.append("")
    out.append("b_ids non-decreasing in p (points of a row consecutive): %s" % sorted_rows)
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
