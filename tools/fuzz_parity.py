#!/usr/bin/env python3
"""Randomised HIP-vs-oracle cross-check (GPU box).  TEST INFRASTRUCTURE: the oracle is only the checker.

Draws random shapes / seeds for every op of the path and compares the C-ABI result with
oracle/pats_oracle.c under the gates of tests/test_gpu_parity.py.  Prints one line per failing case
(op, seed, shape) and a summary; exit code 1 if anything failed.
usage: fuzz_parity.py [--seconds 120] [--seed 0] [--ops gnn,gnn_fine,scale,conv,attention,sinkhorn,ot,ot2,cost,expand,resize,merge,result,third,third_wild]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import pats_oracle as oracle  # noqa: E402
from pats_amd import ops  # noqa: E402

MASS_TOL = 1e-4
NEAR_TIES = 0        # expand rows whose bounds hinge on a strip-sum tie within an ulp (see op_expand)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def mass_close(got, want):
    # 1e-4 absolute on transport mass.  The relative term only matters where masses exceed 1 (dustbin entries under a bias of
    # 2 or 3 with large ns: log-plan entries of 7..9): two fp32 evaluations of ((Z + u) + v) - norm + log k + log k differ by
    # up to ~4 ulp of such a Z (five roundings and the two duals), i.e. 4e-6 relative in exp(Z); seed 101000676 of the
    # round-2 campaign needed 3.2e-6 on one corner entry of mass 3.7e3 (oracle 0.5e-6, HIP 1.5e-6 from float64)
    eg, ew = np.exp(got.astype(np.float64)), np.exp(want.astype(np.float64))
    np.testing.assert_allclose(eg, ew, atol=MASS_TOL, rtol=5e-6)
    np.testing.assert_allclose(eg.sum(-1), ew.sum(-1), atol=MASS_TOL, rtol=5e-6)
    np.testing.assert_allclose(eg.sum(-2), ew.sum(-2), atol=MASS_TOL, rtol=5e-6)


def rand_shape(rng):
    """OT shapes: the resident ones, their neighbours, ragged ones, a few large."""
    pick = rng.integers(0, 11)
    if pick == 10:
        # the dispatch edges of the coarse solvers (csrc/sinkhorn.hip: cu_shape, stream_shape, the wg kernel's thread switch),
        # redrawn until M + N fits the general kernel's LDS bound (launch_wg: (M + N) floats in 64 KiB)
        while True:
            M = int(rng.choice([29, 30, 31, 95, 96, 97, 303, 304, 305]))
            N = int(rng.choice([30, 31, 32, 319, 320, 321]))
            if (M + N) * 4 <= 64 * 1024:
                return M, N
    if pick == 0:
        return 65, 65
    if pick == 1:
        return 145, 145
    if pick == 2:
        return int(rng.integers(2, 12)), int(rng.integers(2, 12))
    if pick == 3:
        n = int(rng.choice([64, 66, 144, 146, 301, 302]))
        return n, n
    if pick == 4:
        return int(rng.integers(280, 321)), int(rng.integers(280, 321))
    if pick == 5:
        return int(rng.integers(330, 700)), int(rng.integers(330, 700))
    return int(rng.integers(2, 200)), int(rng.integers(2, 200))


def op_sinkhorn(rng):
    M, N = rand_shape(rng)
    b = int(rng.integers(1, 5))
    it = int(rng.choice([1, 2, 7, 30, 100]))
    Z = (rng.standard_normal((b, M, N)) * rng.choice([0.3, 2.0, 6.0])).astype(np.float32)
    mu = rng.uniform(0.2, 3.0, (b, M))
    nu = rng.uniform(0.2, 3.0, (b, N))
    nu *= (mu.sum(1) / nu.sum(1))[:, None]
    lm, ln = np.log(mu).astype(np.float32), np.log(nu).astype(np.float32)
    got = ops.log_sinkhorn_iterations(cu(Z), cu(lm), cu(ln), it).cpu().numpy()
    mass_close(got, oracle.log_sinkhorn_iterations(Z, lm, ln, it))
    return "b=%d %dx%d it=%d" % (b, M, N, it)


def op_ot(rng):
    m, n = rand_shape(rng)
    b = int(rng.integers(1, 4))
    S = (rng.standard_normal((b, m, n)) * rng.choice([0.5, 3.0])).astype(np.float32)
    ns = np.exp(rng.uniform(-2.7, 2.7, (b, 1, n))).astype(np.float32)
    alpha = float(rng.choice([0.0, 0.5, 1.3]))
    got = ops.log_optimal_transport(cu(S), alpha, cu(ns), 100).cpu().numpy()
    mass_close(got, oracle.log_optimal_transport(S, alpha, ns, 100))
    return "b=%d %dx%d alpha=%g" % (b, m, n, alpha)


def op_ot2(rng):
    m, n = rand_shape(rng)
    m, n = max(m, 3), max(n, 3)
    b = int(rng.integers(1, 6))
    # now and then a WILD problem (round 4): score ranges of tens to hundreds of nats send the scalings out of the guard band
    # and the problem through its re-solve (145 x 145: stabilised linear sweeps with absorption; else log-sum-exp sweeps)
    wild = rng.random() < 0.25
    amp = float(rng.choice([15.0, 40.0, 90.0])) if wild else float(rng.choice([0.5, 3.0]))
    S = (rng.standard_normal((b, m, n)) * amp).astype(np.float32)
    ns = np.exp(rng.uniform(-2.7, 2.7, (b, 1, n - 1))).astype(np.float32)
    k = float(rng.choice([0.0, 2.0, 3.0]))
    got = ops.log_optimal_transport2(cu(S), 1.0, cu(ns), 100, bias_k=k).cpu().numpy()
    want = oracle.log_optimal_transport2(S, 1.0, ns, 100)
    if k:
        want = oracle.dustbin_bias(want, k)
    if wild:          # the gate of tests/test_gpu_parity.py::test_wide_dynamic_range...: log-plan entries to fp32 resolution of |Z|
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want, atol=2e-5 * max(50.0, 5.0 * amp), rtol=2e-5)
    else:
        mass_close(got, want)
    return "b=%d %dx%d bias=%g amp=%g" % (b, m, n, k, amp)


def op_cost(rng):
    b = int(rng.integers(1, 4))
    D = int(rng.choice([7, 32, 66, 128, 264, 448, int(rng.integers(1, 300))]))
    n, m = int(rng.integers(1, 400)), int(rng.integers(1, 400))
    if rng.random() < 0.3:
        n = m = int(rng.choice([65, 145, 300, 160, 161, 320]))
    d0 = rng.standard_normal((b, D, n)).astype(np.float32)
    d1 = rng.standard_normal((b, D, m)).astype(np.float32)
    got = ops.cost(cu(d0), cu(d1)).cpu().numpy()
    np.testing.assert_allclose(got, oracle.cost(d0, d1), atol=3e-5, rtol=1e-5)
    return "b=%d D=%d %dx%d" % (b, D, n, m)


def op_expand(rng):
    h, w = int(rng.integers(2, 26)), int(rng.integers(2, 34))
    N = h * w
    b = int(rng.integers(1, 4))
    it = int(rng.choice([1, 8, 15]))
    lb = float(rng.choice([1e-5, 1e-3]))
    # a plan-like positive matrix with peaked rows (so rectangles grow) and a dustbin
    base = rng.standard_normal((b, N + 1, N + 1)) * 2.0
    for bi in range(b):
        tgt = rng.integers(0, N, N)
        base[bi, np.arange(N), tgt] += rng.uniform(3, 9, N)
        # a share of rows whose dustbin entry dominates: the `if_nomatching` branch (whole_cost / core_cost zeroed)
        dusty = np.nonzero(rng.random(N) < 0.15)[0]
        base[bi, dusty, N] = base[bi, dusty, :].max(1) + rng.uniform(0.5, 4.0, len(dusty))
    P = np.exp(base - base.max(2, keepdims=True)).astype(np.float32)
    P /= P.sum(2, keepdims=True).astype(np.float32)
    sc = np.exp(rng.uniform(-1.0, 1.0, (b, N))).astype(np.float32)
    scy = np.exp(rng.uniform(-1.0, 1.0, (b, N))).astype(np.float32)                    # drawn independently of scalex
    want = oracle.iterative_expand(P, sc, scy, w, h, w, lb, it)                       # lim3 = limitation[3] = w
    positions, ranges = ops.Compute_positions_and_ranges(h, w, "cuda")
    got = ops.Iterative_expand_matrix(cu(P), cu(sc).reshape(b, -1, 1), cu(scy).reshape(b, -1, 1), [0, h, 0, w], ranges,
                                      positions, lower_bound=lb, iter_num=it, width=w, height=h)
    gb = got[5].cpu().numpy()
    bad_rows = np.argwhere((gb != want[5]).any(-1))
    if len(bad_rows):
        # A growth step compares four strip sums; two of them within an ulp of each other are decided by the summation
        # order (the reference's own torch.sum differs between CPU and GPU there).  Accept a differing row only if the
        # oracle itself changes its answer for that row under 1e-7 relative noise on the plan.
        assert len(bad_rows) <= 2, "bounds differ in %d rows" % len(bad_rows)
        flips = set()
        for _ in range(6):
            Pn = (P * (1.0 + 1e-7 * rng.standard_normal(P.shape))).astype(np.float32)
            wn = oracle.iterative_expand(Pn, sc, scy, w, h, w, lb, it)[5]
            flips |= {tuple(r) for r in np.argwhere((wn != want[5]).any(-1))}
        assert all(tuple(r) in flips for r in bad_rows), "bounds differ (no near-tie)"
        global NEAR_TIES
        NEAR_TIES += len(bad_rows)
        return "near tie"
    np.testing.assert_allclose(got[0].cpu().numpy(), want[0], atol=3e-6, rtol=5e-5)
    np.testing.assert_allclose(got[1].cpu().numpy(), want[1], atol=3e-6, rtol=5e-4)     # core_cost: test_coarse_level's gate
    np.testing.assert_allclose(got[2].cpu().numpy(), want[2], atol=2e-4, rtol=2e-5)
    np.testing.assert_allclose(got[3].cpu().numpy(), want[3], atol=1e-5, rtol=5e-5)
    np.testing.assert_allclose(got[4].cpu().numpy(), want[4], atol=1e-5, rtol=5e-5)
    return "b=%d grid %dx%d it=%d lb=%g" % (b, h, w, it, lb)


def op_resize(rng):
    n_img, C = int(rng.integers(1, 3)), int(rng.choice([1, 3, 5]))
    Hp, Wp = int(rng.integers(40, 300)), int(rng.integers(40, 300))
    K = int(rng.integers(0, 40))
    src = (rng.random((n_img, C, Hp, Wp)) * 255).astype(np.float32)
    y0 = rng.integers(0, Hp - 2, K)
    x0 = rng.integers(0, Wp - 2, K)
    y1 = np.minimum(Hp, y0 + 1 + rng.integers(0, Hp, K))
    x1 = np.minimum(Wp - 1, x0 + rng.integers(0, Wp, K))
    seq = rng.integers(0, n_img, K) * 10000 + rng.integers(0, 9999, K)
    bound = np.stack([y0, y1, x0, x1, seq], 1).astype(np.int64).reshape(K, 5)
    got = ops.tensor_resize(cu(src), cu(bound)).cpu().numpy()
    np.testing.assert_allclose(got, oracle.tensor_resize(src, bound), atol=1e-4)
    return "n=%d C=%d %dx%d K=%d" % (n_img, C, Hp, Wp, K)


def op_merge(rng):
    new = bool(rng.integers(0, 2))
    h, w, bt = int(rng.integers(1, 26)), int(rng.integers(1, 34)), int(rng.integers(1, 3))
    l1 = rng.random((bt, h * w)) < rng.choice([0.0, 0.3, 0.9])
    B = int((~l1).sum())
    if B == 0:
        l1[0, 0] = False
        B = 1
    trust = rng.lognormal(-1.0, 0.9, (B, 144)).astype(np.float32)
    if rng.random() < 0.5:
        trust = (np.round(trust * 4) / 4).astype(np.float32)          # tie-heavy
    f2 = rng.random((B, 144)) < rng.choice([0.1, 0.5, 0.95])
    sb0 = np.where(rng.random((bt, h * w, 16, 9)) < 0.5, 0.0,
                   np.round(rng.normal(0, 1, (bt, h * w, 16, 9)), 1) - rng.choice([0.0, 10000.0]))
    want, wt, wf2, wsb = oracle.merge_patches(new, trust, (h * 32, w * 32), l1, f2, sb0)
    tr, ff, sb = cu(trust), cu(f2), cu(sb0)
    fn = ops.merge_patches_new if new else ops.merge_patches_old
    out, _ = fn(B, tr, (h * 32, w * 32), cu(l1), ff, sb)
    assert np.array_equal(out.cpu().numpy(), want), "%d flags differ" % int((out.cpu().numpy() != want).sum())
    assert np.array_equal(tr.cpu().numpy(), wt) and np.array_equal(ff.cpu().numpy(), wf2)
    assert np.array_equal(sb.cpu().numpy(), wsb)
    return "%s grid %dx%d bt=%d B=%d" % ("new" if new else "old", h, w, bt, B)


def op_result(rng):
    h, w, bs = int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(1, 3))
    N = h * w
    ifn0 = rng.random((bs, N)) < rng.choice([0.0, 0.3, 0.8])
    if ifn0.all():
        ifn0[0, 0] = False
    K = int((~ifn0).sum())
    ap0 = rng.uniform(0, [h, w], (bs, N, 2)).astype(np.float32)
    sc0 = np.exp(rng.uniform(-1.2, 1.2, (bs, N, 2))).astype(np.float32)
    ifn2 = rng.random((K, 144)) < rng.choice([0.2, 0.6, 1.0])
    pts = (rng.integers(0, 97, (K, 144, 2)) / 8.0).astype(np.float32)          # many exact .5 cases for round-half-even
    P = int((~ifn2).sum())
    mk = rng.uniform(0, 96, (P, 16, 2)).astype(np.float32)
    lab = np.where(rng.random((P * 16,)) < 0.3, -10.0, 1e8).astype(np.float32)
    g0, g1, gb = ops.third_inputs(cu(ifn2), cu(pts))
    w0, w1, wb = oracle.third_inputs(ifn2, pts)
    assert np.array_equal(g0.cpu().numpy(), w0) and np.array_equal(g1.cpu().numpy(), w1) and np.array_equal(gb.cpu().numpy(), wb)
    f16, p16 = ops.refine_scatter(cu(ifn2), cu(pts), cu(mk), cu(lab))
    wf, wp = oracle.refine_scatter(ifn2, pts, mk, lab)
    assert np.array_equal(f16.cpu().numpy(), wf) and np.array_equal(p16.cpu().numpy(), wp)
    ch0, ch1 = rng.random((bs,)) < 0.7, rng.random((K,)) < 0.7
    sc_rows = sc0[~ifn0]
    ml, mr = ops.get_result(bs, [cu(ifn0), f16], [cu(ap0), p16.flip(dims=[2]) / 2.0], [cu(sc0), cu(sc_rows)],
                            [[32, h, w], [2, 48, 48]], [cu(ch0), cu(ch1)])
    wl, wr = oracle.get_result(bs, [ifn0, wf], [ap0, wp[:, :, ::-1] / np.float32(2.0)],
                               [sc0, np.repeat(sc_rows.reshape(-1, 1, 2), 2304, 1)], [[32, h, w], [2, 48, 48]], [ch0, ch1])
    assert np.array_equal(ml.cpu().numpy(), wl) and np.array_equal(mr.cpu().numpy(), wr)
    return "grid %dx%d bs=%d K=%d P=%d M=%d" % (h, w, bs, K, P, wl.shape[0])


def op_third(rng):
    P = int(rng.integers(1, 200))
    D = int(rng.choice([32, 64, 128, 256]))
    outdoor = bool(rng.integers(0, 2))
    base = rng.standard_normal((P, D, 65)).astype(np.float32)
    amp = float(rng.choice([1.0, 3.0]))
    d0 = (amp * (base + 0.3 * rng.standard_normal((P, D, 65)))).astype(np.float32)
    d1 = (amp * (base + 0.3 * rng.standard_normal((P, D, 65)))).astype(np.float32)
    scale = np.exp(rng.uniform(-2.7, 2.7, (P, 1, 64))).astype(np.float32)
    ps = (rng.integers(1, 23, (P, 2)) * 4).astype(np.int64)
    pt = (rng.integers(0, 25, (P, 2)) * 4).astype(np.int64)
    m0, m1, label, ifm = ops.third_level(cu(d0), cu(d1), cu(scale), cu(ps), cu(pt), outdoor=outdoor)
    Zr = oracle.log_optimal_transport2(oracle.cost(d0, d1), 1.0, scale, 100)
    sq = np.sqrt(scale + np.float32(1e-8)).astype(np.float32)
    r0, r1, rwl, rlabel, rifm = oracle.compute_result(np.exp(Zr), sq, sq, ps, pt, outdoor)
    assert np.array_equal(m0.cpu().numpy(), r0)
    # argmax ties between near-equal plan entries may legitimately flip under 1e-6 relative noise: compare
    # positions only where the oracle's top two entries of a centre row are separated
    S = np.exp(Zr)[:, :-1, :].reshape(P, 8, 8, 65)[:, 2:6, 2:6, :].reshape(P, 16, 65)
    top2 = np.sort(S[:, :, :64], axis=2)[:, :, -2:]
    clear = (top2[:, :, 1] - top2[:, :, 0]) > 1e-4 * top2[:, :, 1]
    d = np.abs(m1.cpu().numpy() - r1).max(2)
    assert (d[clear] <= 2e-3).all(), "mkpts1 differs by %g" % d[clear].max()
    topd = np.sort(S, axis=2)[:, :, -2:]
    cleard = (topd[:, :, 1] - topd[:, :, 0]) > 1e-4 * topd[:, :, 1]
    assert np.array_equal(ifm.cpu().numpy().astype(bool)[cleard], rifm[cleard])
    return "P=%d D=%d outdoor=%d" % (P, D, outdoor)


def op_third_wild(rng):
    """The third level with about a quarter of the problems beyond the guard band, on both sides of the 6144 workgroups of
    the redo walk (tests/test_third_redo_walk_gpu.py), with and without a device-side count.  The launch is an index vector
    into 48 base problems, so the oracle solves 48 problems whatever P is."""
    from pats_amd import synth
    K, REDO, NAN_BITS = 48, 0xEE, 0x7FC00000
    P = int(rng.integers(6145, 13001)) if rng.integers(0, 2) else int(rng.integers(1, 201))
    inp = synth.third_inputs(seed=int(rng.integers(0, 1 << 30)), P=K)
    wild = np.sort(rng.permutation(K)[:K // 4])
    amp = rng.choice([5.0, 9.0, 14.0], size=len(wild)).astype(np.float32)
    d0, d1 = inp["d0"].copy(), inp["d1"].copy()
    d0[wild] *= amp[:, None, None]
    d1[wild] *= amp[:, None, None]
    idx = rng.permutation(K)[:P] if P <= K else rng.integers(0, K, P)
    count = int(rng.integers(0, P + 2)) if rng.integers(0, 2) else None
    live = P if count is None else min(count, P)
    # reference for the base set; the near-tie mask may leave out 2 % of the wild centre rows at most
    Zr = oracle.log_optimal_transport2(oracle.cost(d0, d1), 1.0, inp["scale"], 100)
    sq = np.sqrt(inp["scale"] + np.float32(1e-8)).astype(np.float32)
    r0, r1, rwl, rlabel, rifm = oracle.compute_result(np.exp(Zr), sq, sq, inp["p_s"], inp["p_t"], True)
    S = np.exp(Zr)[wild][:, :-1, :].reshape(len(wild), 8, 8, 65)[:, 2:6, 2:6, :].reshape(len(wild), 16, 65)
    top = np.sort(S, axis=2)[:, :, -2:]
    clear = (top[:, :, 1] - top[:, :, 0]) > 1e-3 * top[:, :, 1]
    assert 1.0 - clear.mean() <= 0.02, "near-tie mask leaves out %.1f %% of the wild centre rows" % (100 * (1 - clear.mean()))
    sel = cu(idx)
    nan = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)     # noqa: E731
    out = (nan(P, 16, 2), nan(P, 16, 2), nan(P * 16, 2), torch.full((P, 16), REDO, dtype=torch.uint8, device="cuda"))
    ops.third_level(*(torch.index_select(cu(a), 0, sel) for a in (d0, d1, inp["scale"], inp["p_s"], inp["p_t"])), outdoor=True,
                    out=out, count=None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda"))
    m0, m1, label, ifm = (t.cpu().numpy() for t in out)
    label = label.reshape(P, 16, 2)
    for name, a in (("mkpts0_f", m0), ("mkpts1_f", m1), ("label", label)):
        assert (a[live:].view(np.uint32) == NAN_BITS).all(), "%s: a row at or past the count was written" % name
    assert (ifm[live:] == REDO).all(), "if_matching1: a row at or past the count was written"
    m0, m1, label, ifm, idx = m0[:live], m1[:live], label[:live], ifm[:live], idx[:live]
    assert set(np.unique(ifm)) <= {0, 1}, "if_matching1 holds %s" % np.unique(ifm)
    assert np.array_equal(m0, r0[idx])
    is_wild = np.isin(idx, wild)
    tame = ~is_wild
    assert np.array_equal(label[tame], rlabel.reshape(K, 16, 2)[idx[tame]])
    assert np.array_equal(ifm.astype(bool)[tame], rifm.astype(bool)[idx[tame]])
    if tame.any():
        d = np.abs(m1[tame] - r1[idx[tame]]).max()
        assert d <= 3e-4 * 8, "mkpts1 of a tame problem differs by %g" % d
    clear_all = np.ones((K, 16), bool)
    clear_all[wild] = clear
    ok = clear_all[idx[is_wild]]
    assert np.array_equal(ifm.astype(bool)[is_wild][ok], rifm.astype(bool)[idx[is_wild]][ok])
    assert np.isfinite(m1).all() and np.isfinite(label).all()
    return "P=%d count=%s wild=%d" % (P, count, int(is_wild.sum()))


def op_attention(rng):
    pick = rng.integers(0, 4)
    if pick == 0:
        b, dim, heads, n, m = int(rng.integers(1, 40)), 32, int(rng.integers(1, 5)), 65, 65       # one-wave kernel
    elif pick == 1:
        b, dim, heads = int(rng.integers(1, 4)), int(rng.choice([66, 112, 32, 7])), int(rng.integers(1, 5))
        n = m = int(rng.choice([145, 300, 65, 64, 33]))
    else:
        b, dim, heads = int(rng.integers(1, 4)), int(rng.integers(1, 130)), int(rng.integers(1, 5))
        n, m = int(rng.integers(1, 200)), int(rng.integers(1, 641))
    amp = float(rng.choice([0.3, 1.0, 3.0]))
    q = (amp * rng.standard_normal((b, dim, heads, n))).astype(np.float32)
    k = (amp * rng.standard_normal((b, dim, heads, m))).astype(np.float32)
    v = rng.standard_normal((b, dim, heads, m)).astype(np.float32)
    want_prob = bool(rng.integers(0, 2))
    x, prob = ops.attention(cu(q), cu(k), cu(v), return_prob=want_prob)
    wx, wp = oracle.attention(q, k, v)
    # scores grow like amp^2 sqrt(dim); fp32 rounding of a score (any fp32 evaluation, the reference's
    # included: torch-CPU fp32 misses the double-accumulating oracle by 3.9e-5 on seed 3000809) is
    # amplified one-to-one into the probabilities
    np.testing.assert_allclose(x.cpu().numpy(), wx, atol=3e-5 * max(1.0, amp * amp), rtol=2e-5)
    if want_prob:
        np.testing.assert_allclose(prob.cpu().numpy(), wp, atol=3e-6, rtol=2e-5)
    return "b=%d dim=%d heads=%d n=%d m=%d prob=%d" % (b, dim, heads, n, m, want_prob)


def op_conv(rng):
    """Conv1d(k=1) with every optional of pats_conv1x1_f32, and the folded batch statistics (pats_bn_fold_f32)."""
    b, n = int(rng.integers(1, 6)), int(rng.integers(1, 400))
    K, M = int(rng.integers(1, 300)), int(rng.integers(1, 300))
    amp = float(rng.choice([0.1, 1.0, 10.0]))
    x = (amp * rng.standard_normal((b, K, n))).astype(np.float32)
    w = (rng.standard_normal((M, K, 1)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(M).astype(np.float32) if rng.integers(0, 2) else None
    res = rng.standard_normal((b, M, n)).astype(np.float32) if rng.integers(0, 2) else None
    # batch statistics over fewer than 8 samples per channel are not a case (one sample: variance 0, scale = gamma / sqrt(eps) = 316 gamma,
    # and x * scale + shift cancels to beta with an error of an ulp of 316 |x|; torch's BatchNorm1d refuses to train on one value per channel)
    fold = bool(rng.integers(0, 2)) and b * n >= 8
    xa = x
    sc = sh = None
    if fold:
        gam = rng.uniform(0.5, 1.5, K).astype(np.float32); bet = rng.standard_normal(K).astype(np.float32)
        sc, sh = ops.bn_fold(cu(x), cu(gam), cu(bet), 1e-5)
        mean = x.astype(np.float64).mean((0, 2)); var = x.astype(np.float64).var((0, 2))
        s64 = gam / np.sqrt(var + 1e-5)
        np.testing.assert_allclose(sc.cpu().numpy(), s64, rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(sh.cpu().numpy(), bet - mean * s64, rtol=2e-4, atol=2e-5 * max(1.0, amp))
        xa = np.maximum(x * sc.cpu().numpy()[None, :, None] + sh.cpu().numpy()[None, :, None], 0).astype(np.float32)
    y = ops.conv1d(cu(x), cu(w), None if bias is None else cu(bias), sc, sh, None if res is None else cu(res)).cpu().numpy()
    want = oracle.conv1d(xa, w, bias)
    if res is not None:
        want = want + res
    scale = max(1.0, float(np.abs(xa).max()))
    np.testing.assert_allclose(y, want, atol=3e-6 * scale * np.sqrt(K) + 1e-6, rtol=2e-5)
    return "b=%d K=%d M=%d n=%d amp=%g bias=%d res=%d fold=%d" % (b, K, M, n, amp, bias is not None, res is not None, fold)


def op_scale(rng):
    """The scale head (pats_scale_head_f32) on random grids, channel counts, one or two heads, with / without the dustbin column."""
    h, w = int(rng.integers(1, 23)), int(rng.integers(1, 23))
    b, C, heads = int(rng.integers(1, 9)), int(rng.integers(1, 300)), int(rng.integers(1, 3))
    ld = h * w + int(rng.integers(0, 3))
    amp = float(rng.choice([0.3, 1.0, 4.0]))
    x = (amp * rng.standard_normal((b, C, ld))).astype(np.float32)
    ws = [(rng.standard_normal((1, C, 3, 3)) / np.sqrt(9.0 * C)).astype(np.float32) for _ in range(heads)]
    bs = [rng.standard_normal(1).astype(np.float32) for _ in range(heads)]
    y = ops.scale_head(cu(x), h, w, [cu(v) for v in ws], [cu(v) for v in bs]).cpu().numpy()
    # d(out)/out = ln256 * sigmoid' * dv <= 1.4 dv; dv ~ a few ulp of the stencil sum
    np.testing.assert_allclose(y, oracle.scale_head(x, h, w, ws, bs), rtol=2e-5 * max(1.0, amp))
    return "b=%d C=%d %dx%d ld=%d heads=%d amp=%g" % (b, C, h, w, ld, heads, amp)


def op_gnn(rng):
    """AttentionalPropagation (modules.py:107-117): the fused kernel at the third level's shape (C = 128, 65 tokens: eval /
    batch-statistics BatchNorm, with / without the residual, weight and activation magnitudes over three decades, now and then
    an activation beyond the fp16 range -> the gated composition) and, at other shapes, the packed-weights convolutions around
    attention145_kernel / the general attention kernel (spikes there too: their redo flags)."""
    from pats_amd import synth
    kind = int(rng.integers(0, 4))
    fused = kind < 2
    if fused:
        C, n, m, b = 128, 65, 65, int(rng.integers(1, 24))
    elif kind == 2:                                        # attention145_kernel's box (97..160 tokens, 33..80 channels per head)
        C = int(rng.choice([136, 160, 200, 264, 296, 320]))
        n, m, b = int(rng.integers(97, 161)), int(rng.integers(97, 161)), int(rng.integers(1, 4))
    else:                                                  # conv_pk_kernel at any width, the general attention kernel
        C = int(rng.choice([8, 32, 64, 72, 128, 136, 264, 448]))
        n, m, b = int(rng.integers(1, 171)), int(rng.integers(1, 171)), int(rng.integers(1, 5))
    params = synth.gnn_params(seed=int(rng.integers(0, 1 << 30)), C=C)
    wamp = float(rng.choice([0.1, 1.0, 3.0]))
    for k in list(params):
        if k.endswith("weight") and params[k].ndim == 3:
            params[k] = (params[k] * wamp).astype(np.float32)
    amp = float(rng.choice([0.1, 1.0, 5.0]))
    x = (amp * rng.standard_normal((b, C, n))).astype(np.float32)
    src = (amp * rng.standard_normal((b, C, m))).astype(np.float32)
    spike = rng.integers(0, 12) == 0
    if spike:
        x[int(rng.integers(0, b)), int(rng.integers(0, C)), int(rng.integers(0, n))] = 2500.0 if fused else float(rng.choice([2500.0, 70000.0]))
    train = bool(rng.integers(0, 2)) and b * n >= 8
    res = bool(rng.integers(0, 2))
    y = ops.attentional_propagation(cu(x), cu(src), ops.PropagationParams(params), bn_train=train, residual=cu(x) if res else None).cpu().numpy()
    want = oracle.attentional_propagation(x, src, params, bn_train=train, residual=x if res else None)
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(y, want, atol=(3e-5 if not spike else 2e-3) * scale, rtol=3e-4 if not spike else 1e-3)
    return "C=%d b=%d n=%d m=%d train=%d res=%d wamp=%g amp=%g spike=%d" % (C, b, n, m, train, res, wamp, amp, spike)


def op_gnn_fine(rng):
    """The fine level's three-kernel layer (csrc/gnn_fine.hip) at ITS shape - [b, 264, 145], eval-mode BatchNorm: a single layer
    (self or cross, with / without the residual) for b across the tile classes (full tiles, tile 8 of four problems, token 144 of 64),
    or an AttentionalGNN stack of 2-4 layers kept in the kernels' own form between the layers, against the oracle layer by layer;
    weight and activation magnitudes over three decades, now and then an activation beyond the fp16 range (the gated redo)."""
    from pats_amd import synth
    C, n = 264, 145
    stack = rng.integers(0, 3) == 0
    b = int(rng.choice([1, 2, 3, 4, 5, 7, 9, 16, 33, 65, 70])) if not stack else int(rng.choice([1, 3, 5, 17]))
    wamp = float(rng.choice([0.3, 1.0, 2.0]))
    amp = float(rng.choice([0.1, 1.0, 4.0]))

    def pars(seed):
        q = synth.gnn_params(seed=seed, C=C)
        for k in list(q):
            if k.endswith("weight") and q[k].ndim == 3:
                q[k] = (q[k] * wamp).astype(np.float32)
        return q
    x = (amp * rng.standard_normal((b, C, n))).astype(np.float32)
    src = (amp * rng.standard_normal((b, C, n))).astype(np.float32)
    spike = rng.integers(0, 16) == 0
    if spike:
        x[int(rng.integers(0, b)), int(rng.integers(0, C)), int(rng.integers(0, n))] = 2500.0
    if not stack:
        params = pars(int(rng.integers(0, 1 << 30)))
        self_ = bool(rng.integers(0, 2))
        res = bool(rng.integers(0, 2))
        s_ = x if self_ else src
        y = ops.attentional_propagation(cu(x), cu(s_), ops.PropagationParams(params), residual=cu(x) if res else None).cpu().numpy()
        want = oracle.attentional_propagation(x, s_, params, residual=x if res else None)
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(y, want, atol=(3e-5 if not spike else 2e-3) * scale, rtol=3e-4 if not spike else 1e-3)
        return "fine layer b=%d self=%d res=%d wamp=%g amp=%g spike=%d" % (b, self_, res, wamp, amp, spike)
    L = int(rng.integers(2, 5))
    plist = [pars(int(rng.integers(0, 1 << 30))) for _ in range(L)]
    names = [str(rng.choice(["self", "cross"])) for _ in range(L)]
    y0, y1 = ops.attentional_gnn(cu(x), cu(src), [ops.PropagationParams(q) for q in plist], names)
    def reference(a0, a1):                                    # AttentionalGNN.forward, modules.py:127-134
        for q, nm in zip(plist, names):
            s0, s1 = (a1, a0) if nm == "cross" else (a0, a1)
            a0, a1 = oracle.attentional_propagation(a0, s0, q, residual=a0), oracle.attentional_propagation(a1, s1, q, residual=a1)
        return a0, a1
    d0, d1 = reference(x, src)
    # A stack of these layers is not well-conditioned everywhere: at weights x 2 and activations x 4 the ORACLE ITSELF turns a
    # 1e-7 relative perturbation of its inputs into 0.03-0.07 absolute after four layers (x 10 a layer: saturated softmax rows).
    # The gate is therefore the larger of the usual one and 8 x the oracle's own response to such a perturbation.
    pr = np.random.default_rng(1)
    p0, p1 = reference((x * (1 + 1e-7 * pr.standard_normal(x.shape))).astype(np.float32), (src * (1 + 1e-7 * pr.standard_normal(src.shape))).astype(np.float32))
    sens = max(float(np.abs(p0 - d0).max()), float(np.abs(p1 - d1).max()))
    for got, want in ((y0.cpu().numpy(), d0), (y1.cpu().numpy(), d1)):
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, atol=max((1e-4 if not spike else 4e-3) * scale, 8.0 * sens), rtol=1e-3)
    return "fine stack L=%d b=%d %s wamp=%g amp=%g spike=%d" % (L, b, "".join(nm[0] for nm in names), wamp, amp, spike)


OPS = {"gnn": op_gnn, "gnn_fine": op_gnn_fine, "scale": op_scale, "conv": op_conv, "attention": op_attention, "sinkhorn": op_sinkhorn, "ot": op_ot, "ot2": op_ot2, "cost": op_cost, "expand": op_expand,
       "resize": op_resize, "merge": op_merge, "result": op_result, "third": op_third, "third_wild": op_third_wild}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--mode", default="auto", choices=["auto", "log", "kernel"])
    args = ap.parse_args()
    ops.set_sinkhorn_mode(args.mode)
    names = args.ops.split(",")
    t_end = time.time() + args.seconds
    fails, runs = 0, {n: 0 for n in names}
    case = 0
    while time.time() < t_end:
        for n in names:
            seed = args.seed * 1000003 + case
            rng = np.random.default_rng(seed)
            try:
                OPS[n](rng)
            except Exception as e:   # noqa: BLE001
                fails += 1
                desc = str(e).strip().split("\n")
                print("FAIL %-8s seed=%d : %s" % (n, seed, " | ".join(x.strip() for x in desc[:4])[:300]), flush=True)
            runs[n] += 1
            case += 1
    print("fuzz: %d cases, %d failures; per op %s; guard fallbacks %d; expand near-tie rows %d"
          % (case, fails, runs, ops.sinkhorn_fallbacks(), NEAR_TIES))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
