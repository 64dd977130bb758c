"""CPU-only: tests/pose_cases.py against itself - the float64 restatement of the pose stage recovers the ground truth of its own
scenes, the undecided band of the cheirality test is thin, and a float32 evaluation of the test agrees with the float64 one
everywhere outside that band.  The GPU test leans on all three."""
import numpy as np
import pytest

import epipolar_cases as ec
import pose_cases as pc

# the share of (match, candidate) cells the band may hold: a cap, not a measurement (the committed scenes stay near 1e-4)
UNDECIDED_CAP = 1e-3
# Ground truth: what this bound must catch is a transposed R - an error of twice the scene's rotation, at least 2 * 0.05 rad = 5.7
# degrees with make_scene's distribution - and a wrong sign of t (asserted on its own below).  What it must let pass is the noise:
# 5e-4 rad = 0.03 degrees per coordinate, amplified by the plain 8-point fit's conditioning when a scene has barely more inliers
# than unknowns (a dozen at n = 20).  Five degrees lies below the smallest transposition error of any scene and two orders above
# the noise itself.
POSE_DEG = 5.0


@pytest.fixture(scope="module")
def scenes():
    out = []
    for seed, n in pc.HOST_CASES:
        s = pc.make_scene(seed, n)
        s["xl"], s["xr"] = ec.points32(s["ml"], s["mr"])
        s["M"] = ec.moments64(s["xl"], s["xr"], s["good"])[0]
        s["n"] = n
        out.append(s)
    return out


def test_the_scenes_are_what_the_stage_needs(scenes):
    for s in scenes:
        assert int(s["good"].sum()) >= pc.MIN_INLIERS, "a scene with fewer than eight inliers: change the seed"
        assert np.allclose(s["R"] @ s["R"].T, np.eye(3), atol=1e-14) and abs(np.linalg.det(s["R"]) - 1) < 1e-14
        assert abs(np.linalg.norm(s["t"]) - 1) < 1e-14


def test_the_refit_over_the_true_inliers_recovers_the_ground_truth(scenes):
    for s in scenes:
        if s["n"] not in [n for _, n in pc.REFIT_CASES]:
            continue
        ref = pc.reference(s["xl"], s["xr"], s["good"], M=s["M"])
        assert ref["ok"]
        good = int(s["good"].sum())
        others = [int(c) for k, c in enumerate(ref["counts"]) if k != ref["choice"]]
        print("n = %d: %d inliers, counts %s, R error %.4f deg, t error %.4f deg"
              % (s["n"], good, ref["counts"].tolist(), pc.angle_R(ref["R"], s["R"]), pc.angle_t(ref["t"], s["t"])))
        assert int(ref["counts"][ref["choice"]]) == good and others == [0, 0, 0]
        assert pc.angle_R(ref["R"], s["R"]) < POSE_DEG and pc.angle_t(ref["t"], s["t"]) < POSE_DEG
        assert float(np.dot(ref["t"], s["t"])) > 0                              # the sign of t, which angle_t forgives
        E = pc.project64(ref["e"])
        sv = np.linalg.svd(E, compute_uv=False)
        assert np.allclose(sv, [np.sqrt(0.5), np.sqrt(0.5), 0.0], atol=1e-15) and E.reshape(-1)[np.argmax(np.abs(E))] > 0
        tx = pc.cross_matrix(ref["t"]) @ ref["R"]
        tx /= np.linalg.norm(tx)
        assert min(np.abs(tx - E).max(), np.abs(tx + E).max()) < 1e-14


def test_the_band_is_thin_and_float32_agrees_outside_it(scenes):
    cells = undecided = 0
    for s in scenes:
        used = np.ones(s["n"], bool)                                            # every match: all four candidates are non-trivial
        cands = pc.candidates64(pc.refit64(s["M"])[0])
        f64, und = pc.fronts(s["xl"], s["xr"], used, cands)
        f32, _ = pc.fronts(s["xl"], s["xr"], used, cands, dtype=np.float32)
        assert np.array_equal(f32[~und], f64[~und]), "a float32 verdict differs outside the band (n = %d)" % s["n"]
        cells += und.size
        undecided += int(und.sum())
    print("undecided: %d of %d cells (%.2e)" % (undecided, cells, undecided / cells))
    assert cells == 4 * sum(n for _, n in pc.HOST_CASES) and undecided <= UNDECIDED_CAP * cells


def test_no_pose_cases_of_the_restatement():
    s = pc.make_scene(301, 100)
    xl, xr = ec.points32(s["ml"], s["mr"])
    M = ec.moments64(xl, xr, s["good"])[0]
    assert not pc.reference(xl, xr, s["good"], M=M, best_count=7)["ok"]
    assert not pc.reference(xl, xr, s["good"], M=np.zeros((9, 9)))["ok"]
    nan = M.copy()
    nan[3, 4] = np.nan
    assert not pc.reference(xl, xr, s["good"], M=nan)["ok"]
    assert pc.reference(xl, xr, s["good"], model=pc.true_model(s))["ok"]
    assert not pc.reference(xl, xr, s["good"], model=np.zeros((3, 3), np.float32))["ok"]
