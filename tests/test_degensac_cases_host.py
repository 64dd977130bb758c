"""CPU-only: the numpy restatement of the plane-and-parallax stage (tests/degensac_cases.py) checked against itself and its scenes -
what tests/test_degensac_gpu.py then holds the device to.
    sampler   draw2 equals the definition's first form (Python integers) and the first two draws of the 7-point sampler
    solver    x'^T F x vanishes on the two sampled matches and on the plane; the zero rules
    scenes    (a) no match of any scene lies within a relative 1e-3 of the pool boundary parallax * thr: membership is exact in float32
              (b) with the fixed seed and H = 64 the numpy chain finds an all-true sample on every scene-A pair, and its best model
                  has at least the true inliers as support - the count rule of the GPU end-to-end test, met by the restatement
              (c) the 7-point chain's numpy winner at (SEED7, H7) has less than 0.9 of the true inliers on every scene-A pair"""
import numpy as np

import degensac_cases as dc
import fundamental_cases as fc


def test_draw2_is_the_definition_and_the_head_of_the_seven_point_draws():
    for seed, m in ((0, 2), (1, 3), (-5, 7), (2 ** 63 - 1, 60), (4242, 8192), (99, 2 ** 31 - 2)):
        got = dc.draw2(seed, 65, m)
        assert got.shape == (65, 2) and (got >= 0).all() and (got < m).all() and (got[:, 0] != got[:, 1]).all()
        if m <= 8192:
            for h in (0, 1, 31, 64):
                assert got[h].tolist() == dc.draw2_slow(seed, h, m)
        if m >= 7:
            assert np.array_equal(got, fc.sample_idx(seed, m, 65)[:, :2])


def test_the_solver_puts_the_sampled_and_the_planar_matches_on_their_epipolar_lines():
    for s in dc.scenes("A"):
        ref, counts, all_true = dc.chain_pp(s, 7)
        live = ref["F"].any(1)
        assert live.all() and ref["pool"] == int((s["label"] != dc.LABEL_PLANE).sum())
        assert np.abs(np.linalg.norm(ref["F"], axis=1) - 1).max() <= 1e-12
        assert np.array_equal(fc.sign_rule(ref["F"].astype(np.float32)), ref["F"].astype(np.float32))
        alg = dc.algebraic(ref["F"], s["xl"], s["xr"])
        for h in range(ref["F"].shape[0]):
            assert np.abs(alg[h, ref["idx"][h]]).max() <= 1e-12
        assert np.abs(alg[:, s["label"] == dc.LABEL_PLANE]).max() <= 1e-5      # the plane is the true one to float32 rounding
        # an all-true sample is the scene's geometry
        assert (counts[all_true] >= s["true"].sum()).all()


def test_the_zero_rules():
    s = dc.scenes("A")[0]
    n = len(s["ml"])
    Hp = s["H"].astype(np.float32).reshape(1, 1, 3, 3)
    args = (s["ml"], s["mr"], [(0, n)], [5], 16)
    ref = dc.reference(*args, np.zeros_like(Hp), [0], [dc.THR], norm=s["norm"][None])[0]
    assert not ref["plane"] and (ref["idx"] == -1).all() and not ref["F"].any()
    off = np.flatnonzero(s["label"] != dc.LABEL_PLANE)
    keep = np.concatenate([np.flatnonzero(s["label"] == dc.LABEL_PLANE), off[:1]])
    one = dc.reference(s["ml"][keep], s["mr"][keep], [(0, len(keep))], [5], 16, Hp, [0], [dc.THR], norm=s["norm"][None])[0]
    assert one["pool"] == 1 and (one["idx"] == -1).all() and not one["F"].any()
    twice = np.concatenate([keep, off[:1]])                                # the same match twice: the two lines coincide
    two = dc.reference(s["ml"][twice], s["mr"][twice], [(0, len(twice))], [5], 16, Hp, [0], [dc.THR], norm=s["norm"][None])[0]
    assert two["pool"] == 2 and (two["idx"] >= 0).all() and not two["F"].any() and not two["cond"].any()
    nan = dc.reference(*args, np.full_like(Hp, np.nan), [0], [dc.THR], norm=s["norm"][None])[0]
    assert nan["plane"] and nan["pool"] == 0 and not nan["F"].any()


def test_a_no_match_lies_near_the_pool_boundary():
    for which in "AB":
        for s in dc.scenes(which):
            margin = dc.margin64(s["xl"], s["xr"], s["H"].astype(np.float32), dc.THR, dc.PARALLAX)
            assert margin.min() > 1e-3, (which, margin.min())
            pool = dc.pool_test32(s["xl"], s["xr"], s["H"].astype(np.float32), dc.THR, dc.PARALLAX)
            if which == "A":
                assert np.array_equal(pool, s["label"] != dc.LABEL_PLANE)
                assert abs((s["label"] == dc.LABEL_PLANE).mean() - 0.80) < 0.01 and abs((s["label"] == dc.LABEL_OFF).mean() - 0.12) < 0.01


def test_b_the_numpy_chain_finds_an_all_true_sample_and_meets_the_count_rule():
    for i, s in enumerate(dc.scenes("A")):
        ref, counts, all_true = dc.chain_pp(s, dc.SEED_PP + i, dc.H_PP)
        assert all_true.any() and counts.max() >= s["true"].sum()
        best = ref["F"][int(np.argmax(counts))]
        assert dc.sampson64(best.reshape(1, 9), s["xl"], s["xr"])[0][s["true"]].max() <= float(dc.THR)


def test_c_the_seven_point_winner_of_scene_a_is_the_degenerate_one():
    for i, s in enumerate(dc.scenes("A")):
        support, true = dc.chain7(s, dc.SEED7 + i)
        assert 7 <= support < 0.9 * true, (i, support, true)
        assert support >= 0.8 * len(s["ml"]) - 1                           # it explains the plane
    for i, s in enumerate(dc.scenes("B")):                                 # scene B's chain finds the scene: nothing is left to gain
        support, true = dc.chain7(s, dc.SEED7 + i, dc.H7_B)
        assert support == true
