"""CPU-only: the restatements of tests/absolute_cases.py hold on their own - the lift's tie and border cases against hand-worked
values, the K = 3 sampler against the existing one, the float64 P3P's truth recovery on the generator (so that the GPU test's
completeness cap can never be met by weakening the cases), the exact FMA emulation against rational arithmetic, the float32
emulation against the float64 classification outside the undecided band - and the new entry points exist in every layer and refuse
bad arguments before any launch."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import absolute_cases as ac
import hypotheses_cases as hc

F32 = np.float32
NAN = float("nan")


def ulp_below(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ---- the lift ---------------------------------------------------------------------------------------------------------------------
def test_nearest_rounds_half_to_even_and_stops_at_the_border():
    depth = (np.arange(12, dtype=F32).reshape(3, 4) + 1)                     # depth[i, j] = 4 i + j + 1
    h, w = depth.shape
    pts = np.array([[0, 0], [2, 3], [0.5, 0], [1.5, 0], [0, 2.5], [-0.5, 0], [ulp_below(-0.5), 0], [h - 0.5, 0],
                    [ulp_below(h - 0.5), 0], [0, w - 0.5], [NAN, 0], [0, np.inf], [1e30, 0]], F32)
    X, ok = ac.lift32(pts, depth)
    want = [1, 12, 1, 9, 3, 1, None, 9, 9, None, None, None, None]          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0 = 0; h - 0.5 = 2.5 -> 2 (even: inside), w - 0.5 = 3.5 -> 4 (outside)
    for k, d in enumerate(want):
        assert ok[k] == (d is not None), k
        if d is not None:
            assert X[k, 2] == d and X[k, 0] == pts[k, 0] * F32(d) and X[k, 1] == pts[k, 1] * F32(d)
        else:
            assert np.isnan(X[k]).all()


def test_bilinear_taps_weights_and_the_upper_edge():
    depth = np.array([[1, 2, 4], [3, 5, 9]], F32)
    pts = np.array([[0, 0], [1, 2], [0.5, 0.5], [0.25, 1.75], [1, 1.5], [1.5, 0], [0, 2.25], [-0.25, 0], [0.5, -1e-3]], F32)
    X, ok = ac.lift32(pts, depth, interp=1)
    assert ok.tolist() == [True, True, True, True, True, False, False, False, False]
    assert X[0, 2] == 1 and X[1, 2] == 9                                     # integer centres, the last one on both upper edges (h - 1, w - 1)
    assert X[2, 2] == F32(0.25) * 1 + F32(0.25) * 2 + F32(0.25) * 3 + F32(0.25) * 5
    a, b = F32(0.25), F32(0.75)
    assert X[3, 2] == (((1 - a) * (1 - b)) * F32(2) + ((1 - a) * b) * F32(4)) + (a * (1 - b)) * F32(5) + (a * b) * F32(9)
    assert X[4, 2] == F32(0.5) * 5 + F32(0.5) * 9                            # a = 0: row 2 does not exist and is not used
    # a tap that is not used may hold anything
    bad = depth.copy()
    bad[1, :] = NAN
    X2, ok2 = ac.lift32(np.array([[0, 0.5], [0.5, 0.5]], F32), bad, interp=1)
    assert ok2.tolist() == [True, False] and X2[0, 2] == F32(1.5)


def test_lift_depth_rules_and_normalisation():
    depth = np.array([[0, -1, NAN, np.inf, 2, 2.5]], F32)
    pts = np.array([[0, j] for j in range(6)], F32)
    X, ok = ac.lift32(pts, depth, max_depth=2.0)
    assert ok.tolist() == [False, False, False, False, True, False]          # exactly at max_depth passes, just above does not
    X, ok = ac.lift32(pts, depth, max_depth=NAN)
    assert ok.tolist() == [False, False, False, False, True, True]           # a NaN limit does not limit
    # the jump: taps 2 and 2.5, (max - min) = 0.5 against max_jump * min
    mid = np.array([[0, 4.5]], F32)
    assert ac.lift32(mid, depth, interp=1, max_jump=0.25)[1].tolist() == [True]         # at: 0.5 > 0.5 is false
    assert ac.lift32(mid, depth, interp=1, max_jump=float(ulp_below(0.25)))[1].tolist() == [False]
    assert ac.lift32(mid, depth, interp=1, max_jump=0.26)[1].tolist() == [True]
    # the point: one subtract, one multiply, then one product each
    nl = np.array([0.5, -1.0, 0.125, 0.3], F32)
    X, ok = ac.lift32(np.array([[0, 4]], F32), depth, norm_left=nl)
    x0, x1 = (F32(0) - nl[0]) * nl[2], (F32(4) - nl[1]) * nl[3]
    assert ok[0] and X[0].tolist() == [x0 * F32(2), x1 * F32(2), 2.0]
    # no map, an empty map
    for d in (None, np.zeros((0, 5), F32), np.zeros((5, 0), F32)):
        X, ok = ac.lift32(pts, d)
        assert not ok.any() and np.isnan(X).all()
    Xr, vr, cr = ac.lift_reference(pts, [(1, 4), (5, 0)], [depth, None])
    assert cr.tolist() == [1, 0] and not Xr[0].any() and not Xr[5].any() and vr.tolist() == [0, 0, 0, 0, 1, 0]


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
def test_three_draws_are_the_existing_samplers_first_three():
    for seed, n, H in ((5, 8, 33), (-7, 600, 64), (2 ** 40 + 3, 65, 257)):
        assert np.array_equal(ac.sample_idx3(seed, n, H), hc.sample_idx(seed, n, H)[:, :3])          # the same pool: n
        got = ac.sample_idx3(seed, n, H, progressive=True)
        pool = ac.pool3(n, H, True)
        assert pool.min() >= 3 and pool[-1] == n and (np.diff(pool) >= 0).all()
        for h in range(0, H, 7):
            m = int(pool[h])
            if m >= 8:
                assert got[h].tolist() == hc.sample_idx_slow(seed, h, m)[:3]
            assert len(set(got[h].tolist())) == 3 and got[h].max() < m and got[h].min() >= 0
    assert (ac.sample_idx3(1, 2, 5) == -1).all()
    assert (np.sort(ac.sample_idx3(9, 3, 40), 1) == [0, 1, 2]).all()


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def test_float64_p3p_recovers_the_true_pose():
    total = hit = 0
    for k in range(6):
        c = ac.make_pair(900 + k, 300)
        idx = ac.sample_idx3(77 + k, 300, 250)
        for h in range(250):
            X, r = c["X"][idx[h]], c["xr"][idx[h]]
            sols = ac.p3p64(X, r)
            assert len(sols) <= 4
            for R, t in sols:
                assert abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R.T @ R - np.eye(3)).max() < 1e-9
                assert ac.residual3(R, t, X, r) <= 1e-8
            total += 1
            hit += min([ac.pose_distance(R, t, c["R"], c["t"]) for R, t in sols] or [np.inf]) <= ac.POSE_TOL
    share = hit / total
    print("float64 P3P: the true pose within %g in %.2f %% of %d samples" % (ac.POSE_TOL, 100 * share, total))
    assert share >= 0.995
    assert ac.p3p64(np.full((3, 3), NAN), np.zeros((3, 2))) == []


# ---- the test ---------------------------------------------------------------------------------------------------------------------
def test_fma_emulation_is_correctly_rounded():
    rng = np.random.default_rng(3)
    n = 3000
    a, b, c = (rng.normal(size=n).astype(F32) * rng.choice([1e-3, 1, 1e3], n).astype(F32) for _ in range(3))
    c[:n // 3] = -(a[:n // 3] * b[:n // 3])                                  # cancellation: the product's low bits decide
    got = ac.fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = F32(float(exact))
        cands = [near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(F32(x).view(np.uint32)) & 1))
        assert got[i] == best, (a[i], b[i], c[i])


def _models(c, rng, M):
    Rt = np.concatenate([c["R"], c["t"][:, None]], 1)
    models = np.stack([Rt + (0 if k % 4 == 0 else rng.normal(scale=10.0 ** -rng.integers(1, 5), size=(3, 4))) for k in range(M)])
    models[1] = 0                                                            # the zero model
    models[2] = Rt * np.array([[1], [1], [-1]])                              # every point behind the camera
    return models.astype(F32)


def test_emulation_and_classification_agree_outside_the_band():
    rng = np.random.default_rng(11)
    undecided = cells = 0
    for k in range(4):
        c = ac.make_pair(300 + k, 500, outliers=0.3, holes=0.15)
        X, xr = c["X"], c["xr"] + rng.normal(scale=1e-3, size=c["xr"].shape).astype(F32)
        conf = rng.random(500).astype(F32)
        conf[::17] = NAN
        models = _models(c, rng, 24)
        for thr, min_conf in ((2e-3, None), (5e-3, 0.3), (NAN, None), (-1.0, None)):
            part = ac.participates(X, xr, conf, min_conf)
            emu = ac.emulate32(X, xr, part, models, thr)
            inl, dec = ac.classify(X, xr, part, models, thr)
            assert np.array_equal(emu[dec], inl[dec])
            assert not emu[1].any() and not emu[2].any() and not emu[:, ~part].any()
            undecided += (~dec).sum()
            cells += dec.size
            if thr == 2e-3:
                assert emu[0].sum() > 150                                    # the true pose has its inliers
    assert undecided < 0.01 * cells


# ---- the layers -------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_exist_in_every_layer_and_refuse_bad_arguments():
    from pats_amd import _lib, batch, build, ops
    build.build()
    lib = _lib.lib()
    names = ["pats_lift_by_pair_f32", "pats_absolute_hypotheses_by_pair_f32", "pats_absolute_score_by_pair_f32"]
    assert all(n in _lib.SIGNATURES and hasattr(lib, n) for n in names)
    assert "absolute.hip" in build.SOURCES
    assert all(hasattr(ops, n) for n in ("lift_by_pair", "lift_table", "absolute_hypotheses_by_pair", "absolute_score_by_pair"))
    assert all(hasattr(batch, n) for n in ("lift_by_pair", "hypothesize_p3p_by_pair", "verify_abs_by_pair", "pose_abs_by_pair"))
    assert batch._BRANCHES["absolute"][:3] == ("pose_abs", "verified_abs", "pose_abs_by_pair")
    # refused before any launch: no GPU is touched
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    assert lib.pats_lift_by_pair_f32(None, a, 0, None, 1, 0, None, a, None, 0, 0, 0.0, a, a, a, None) == 1
    assert b"lift_by_pair: null matches" in lib.pats_last_error()
    assert lib.pats_lift_by_pair_f32(a, a, 0, None, 1, 0, None, a, None, 2, 0, 0.0, a, a, a, None) == 1
    assert b"interp" in lib.pats_last_error()
    assert lib.pats_lift_by_pair_f32(a, a, 4, a, 1, 8, None, a, None, 0, 0, 0.0, a, a, a, None) == 1
    assert b"exactly one" in lib.pats_last_error()
    assert lib.pats_lift_by_pair_f32(a, a, 0, None, 0, 0, None, a, None, 0, 0, 0.0, a, a, a, None) == 1
    assert b"pairs" in lib.pats_last_error()
    assert lib.pats_lift_by_pair_f32(a + 4, a, 0, None, 1, 0, None, a, None, 0, 0, 0.0, a, a, a, None) == 1
    assert b"aligned" in lib.pats_last_error()
    assert lib.pats_absolute_hypotheses_by_pair_f32(a, a, a, 0, None, 1, 0, 0, a, None, 0, a, None, None, None) == 1
    assert b"absolute_hypotheses_by_pair: H" in lib.pats_last_error()
    assert lib.pats_absolute_hypotheses_by_pair_f32(a, a, a, 0, None, 1, 0, lib.pats_epipolar_max_h() // 4 + 1, a, None, 0, a, None, None, None) == 1
    assert lib.pats_absolute_hypotheses_by_pair_f32(a, a, a, 0, None, 1, 0, 4, a, None, 2, a, None, None, None) == 1
    assert b"progressive" in lib.pats_last_error()
    assert lib.pats_absolute_hypotheses_by_pair_f32(a, None, a, 0, None, 1, 0, 4, a, None, 0, a, None, None, None) == 1
    assert b"null matches_r" in lib.pats_last_error()
    assert lib.pats_absolute_score_by_pair_f32(a, a, None, a, 0, None, 1, 0, a, 0, a, None, 0, 0.0, a, a, a, a, None) == 1
    assert b"absolute_score_by_pair" in lib.pats_last_error()
    assert lib.pats_absolute_score_by_pair_f32(a, a, None, a, 0, None, 1, 0, a, 4, a, None, 1, 0.5, a, a, a, a, None) == 1
    assert b"min_conf needs conf" in lib.pats_last_error()
    assert lib.pats_absolute_score_by_pair_f32(a, a, None, a, 0, None, 1, 2 ** 31, a, 4, a, None, 0, 0.0, a, a, a, a, None) == 1
    assert b"cap" in lib.pats_last_error()
    assert lib.pats_absolute_score_by_pair_f32(a, a, None, a, 0, None, 1, 0, a, 4, None, None, 0, 0.0, a, a, a, a, None) == 1
    assert b"null thr" in lib.pats_last_error()
    cap = batch.Capacities(2, 15, 20)
    with pytest.raises(ValueError, match="pose_branch.*run pose_abs_by_pair first"):
        batch.pose_branch({"pose": ()}, "absolute")
    with pytest.raises(ValueError, match="hypothesize_p3p_by_pair: run lift_by_pair first"):
        batch.hypothesize_p3p_by_pair({}, cap, 8)
    with pytest.raises(ValueError, match="verify_abs_by_pair: run lift_by_pair first"):
        batch.verify_abs_by_pair({}, cap, None, None)
    with pytest.raises(ValueError, match="pose_abs_by_pair: run verify_abs_by_pair first"):
        batch.pose_abs_by_pair({}, cap)
    full = {"pose": 0, "pose_abs": "pa", "verified_abs": "va", "verified_abs_on": "topk", "points": 1}
    view = batch.pose_branch(full, "absolute")
    assert view["pose"] == "pa" and view["verified"] == "va" and view["verified_on"] == "topk" and view["verified_models"] is None
    assert "points" not in view and full["pose"] == 0
