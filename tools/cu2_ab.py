#!/usr/bin/env python3
"""The one-CU coarse Sinkhorn solver (csrc/sinkhorn.hip) held to itself, two ways.

  (no argument)         sinkhorn_cu2_kernel against sinkhorn_cu_kernel (diagnostic library: PATS_CU_V1=1 selects the first version):
                        the coarse level's log-plans of 48 + 1 problems at 301x301, a ragged 251x291 case and the solver shapes
                        (304, 320), (289, 257), (160, 64), (29, 320) and (304, 31) must be BIT-IDENTICAL (the packed row pass and the
                        once-formed column sums keep every operand and every summation order), and the time per solve is printed.
                        Needs `python -m pats_amd.build --diag`; the script re-runs itself as two child processes (the switch is
                        read once per process).
  dump OUT.npz          calls the PRODUCTION library of THIS checkout on the cases of tests/coarse_cases.py, in solver modes "kernel"
                        and "log", and writes every output array and the fallback count behind every guard case
  compare A.npz B.npz   the two dumps hold the same names, dtypes and shapes, and numpy.array_equal on the raw bytes (-inf included)
  time                  one JSON line: event-timed medians of log_optimal_transport at 48 and at 1 coarse problem

`dump` and `compare` check a build of the parent commit against the tree after a change to the solver: run `dump` once in a
checkout of the parent (copy this file there) and once in the tree, each a fresh process under its own time limit; `compare` needs
no GPU.  The cases are the edge suite's (tests/test_coarse_solver_edges_gpu.py): the smallest shapes that reach every row slot,
column slice and padding branch of the kernel and its dispatch neighbours."""
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ab_child(path):
    import torch
    sys.path.insert(0, REPO)
    from pats_amd import ops
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    outs = {}
    # (b, m, n) of the descriptors; the solver sees [m + 1, n + 1].  The last five are shape edges of tests/coarse_cases.py: every
    # row slot and column slice full, slot 18 / slice 4 held by one wave / lane, every pair's second half padding, fewer rows
    # than two per wave, fewer columns than lanes
    shapes = {"coarse48": (48, 300, 300), "one": (1, 300, 300), "ragged": (3, 250, 290), "full": (3, 303, 319),
              "one_wave_one_lane": (3, 288, 256), "half_pairs": (3, 159, 63), "few_rows": (3, 28, 319), "few_columns": (3, 303, 30)}
    for name, (b, M, N) in shapes.items():
        base = torch.randn((b, 448, max(M, N)), device="cuda", generator=g)
        d0 = 3.0 * (base[:, :, :M] + 0.3 * torch.randn((b, 448, M), device="cuda", generator=g))
        d1 = 3.0 * (base[:, :, :N] + 0.3 * torch.randn((b, 448, N), device="cuda", generator=g))
        ns = torch.exp(torch.randn((b, 1, N), device="cuda", generator=g) * 0.5)
        Z = ops.cost_ot(d0.contiguous(), d1.contiguous(), 1, 0.25, ns, 100)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            Z = ops.cost_ot(d0, d1, 1, 0.25, ns, 100)
        torch.cuda.synchronize()
        outs[name] = Z.cpu().numpy()
        print("%s %s: %.1f us per call (cost build + solve), fallbacks %d" % (os.environ.get("PATS_CU_V1", "0"), name, (time.perf_counter() - t0) / 20 * 1e6, ops.sinkhorn_fallbacks()))
    np.savez(path, **outs)


def ab():
    files = []
    for v1 in ("1", "0"):
        f = "/tmp/cu2_ab_%s.npz" % v1
        env = dict(os.environ, PATS_AMD_DIAG_LIB="1", PATS_CU_V1=v1)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "ab-child", f], env=env, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:
            sys.exit(r.stderr[-2000:])
        files.append(np.load(f))
    for k in files[0].files:
        same = np.array_equal(files[0][k], files[1][k])
        print("%s: bit-identical %s (finite %s)" % (k, same, bool(np.isfinite(files[1][k]).all())))
        assert same


def dump(path):
    assert os.environ.get("PATS_AMD_DIAG_LIB", "") in ("", "0"), "dump is for the production library: unset PATS_AMD_DIAG_LIB"
    import torch
    sys.path.insert(0, REPO)
    from pats_amd import ops
    spec = importlib.util.spec_from_file_location("coarse_cases", os.path.join(REPO, "tests", "coarse_cases.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    arrays = {}

    def keep(tag, a):
        arrays["%04d_%s" % (len(arrays), tag)] = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    for mode in ("kernel", "log"):
        prev = ops.set_sinkhorn_mode(mode)
        for M, N in cc.SINKHORN_SHAPES:
            c = cc.sinkhorn_case(M, N)
            Z, log_mu, log_nu = cc.cu(c["Z"]), cc.cu(c["log_mu"]), cc.cu(c["log_nu"])
            for it in (0,) + tuple(cc.SWEEPS_SINKHORN):
                keep("%s_sinkhorn_%dx%d_it%d" % (mode, M, N, it), ops.log_sinkhorn_iterations(Z, log_mu, log_nu, it))
        for M, N in cc.OT_SHAPES:
            c = cc.ot_case(M, N)
            S, ns = cc.cu(c["scores"]), cc.cu(c["ns"])
            for it in cc.SWEEPS_OT:
                keep("%s_ot_%dx%d_it%d" % (mode, M, N, it), ops.log_optimal_transport(S, c["alpha"], ns, it))
        for M, N in cc.COST_OT_SHAPES:
            c = cc.cost_ot_case(M, N)
            d0, d1, ns = cc.cu(c["d0"]), cc.cu(c["d1"]), cc.cu(c["ns"])
            for it in cc.SWEEPS_OT:
                keep("%s_cost_ot_%dx%d_it%d" % (mode, M, N, it), ops.cost_ot(d0, d1, 1, c["alpha"], ns, it))
        for (M, N), entry in ((s, e) for s in cc.GUARD_SHAPES for e in "so"):
            g = cc.guard_case(M, N, entry)
            for name in ("Z", "Z_inf"):                          # the guard-tripping batch, then the tame one with its -inf blocks
                ops.sinkhorn_fallbacks(reset=True)
                if entry == "s":
                    out = ops.log_sinkhorn_iterations(cc.cu(g[name]), cc.cu(g["log_mu"]), cc.cu(g["log_nu"]), cc.GUARD_SWEEPS)
                else:
                    out = ops.log_optimal_transport(cc.cu(g[name]), g["alpha"], cc.cu(g["ns"]), cc.GUARD_SWEEPS)
                tag = "%s_guard_%s_%dx%d_%s" % (mode, entry, M, N, name)
                keep(tag, out)
                keep(tag + "_fallbacks", np.int64(ops.sinkhorn_fallbacks(reset=True)))
        c = cc.many_case()
        keep("%s_many_%dx%d_b%d" % ((mode,) + cc.MANY_MN + (cc.MANY_B,)),
             ops.log_sinkhorn_iterations(cc.cu(c["Z"]), cc.cu(c["log_mu"]), cc.cu(c["log_nu"]), cc.MANY_SWEEPS))
        ops.set_sinkhorn_mode(prev)
    torch.cuda.synchronize()
    np.savez_compressed(path, **arrays)
    print("cu2_ab: %d arrays (%d of them fallback counts), %d bytes -> %s" % (
        len(arrays), sum(k.endswith("_fallbacks") for k in arrays), sum(a.nbytes for a in arrays.values()), path))


def timed():
    """One JSON line: the event-timed median of 30 calls after 3 of log_optimal_transport, 100 sweeps, on [48, 300, 300] and
    [1, 300, 300] scores (docs/measurement.md 5.7)."""
    import json
    import torch
    sys.path.insert(0, REPO)
    from pats_amd import ops
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    res = {}
    for b in (48, 1):
        S = torch.randn((b, 300, 300), device="cuda", generator=g)
        ns = torch.exp(torch.randn((b, 1, 300), device="cuda", generator=g) * 0.5)
        ms = []
        for k in range(33):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.log_optimal_transport(S, 0.25, ns, 100)
            e1.record()
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
        res["ot_%dx300x300_ms" % b] = float(np.median(ms))
    res["fallbacks"] = ops.sinkhorn_fallbacks()
    print(json.dumps(res))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the dumps hold different arrays"
    total, differ = 0, []
    for k in sorted(a.files):
        x, y = a[k], b[k]
        same = x.dtype == y.dtype and x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).reshape(-1).view(np.uint8),
                                                                            np.ascontiguousarray(y).reshape(-1).view(np.uint8))
        total += x.nbytes
        if not same:
            differ.append(k)
    counts = [k for k in a.files if k.endswith("_fallbacks")]
    print("cu2_ab: %d arrays, %d bytes compared, %d differ%s; %d fallback counts (sum %d), %d of them differ" % (
        len(a.files), total, len(differ), ": " + ", ".join(differ[:20]) if differ else "", len(counts),
        sum(int(a[k]) for k in counts), sum(k in differ for k in counts)))
    assert not differ, "%d arrays differ" % len(differ)


if __name__ == "__main__":
    if len(sys.argv) == 1:
        ab()
    elif len(sys.argv) == 3 and sys.argv[1] == "ab-child":
        ab_child(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "time":
        timed()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
