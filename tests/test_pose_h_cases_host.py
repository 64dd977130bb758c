"""CPU-only: the numpy restatement of the per-pair pose from a homography and of the E-or-H decision (tests/pose_h_cases.py) and the
C-ABI surface of the feature.  The figures the GPU test leans on are recomputed and asserted here:
    the float64 constant   the largest difference between the restatement (eigh of the moments, eigh of G^T G, the eigenvector form)
                           and an independent route (SVD of the moments, SVD of G', the cosine / sine form) over the committed scenes;
                           printed, recorded in docs/parity.md; the GPU test holds the kernel to MARGIN = 16 times it
    the dropped share      of generated scenes below the gap min(l1 - 1, 1 - l3) >= 1e-3: at most 5 %
    the band shares        of the float32 decisions on the committed seeds: at most 1 % of a scene's compared matches
TRUTH_TOL = 2^20 eps64 (2.3e-10) bounds a float64 decomposition of an exact homography against the ground truth: the candidates divide
by sqrt(l1 - l3) and take sqrt(l1 - 1), sqrt(1 - l3) of values known to a few eps, so the error is a few eps / sqrt(GAP) = 32 times a
few eps on top of the conditioning of the 3x3 eigenvectors, 1 / GAP = 1000 - 2^20 eps leaves two bits above their product."""
import ctypes
import os
import re

import numpy as np
import pytest

import epipolar_cases as ec
import pose_h_cases as ph
from conftest import REPO

TRUTH_TOL = 2.0 ** 20 * ph.EPS64
SYMBOLS = {"pats_homography_pose_workspace_bytes": (ctypes.c_size_t, 2), "pats_homography_pose_by_pair_f64": (ctypes.c_int, 34),
           "pats_pose_select_workspace_bytes": (ctypes.c_size_t, 2), "pats_pose_select_by_pair": (ctypes.c_int, 31)}
CTYPE_OF = (("*", ctypes.c_void_p), ("pats_stream_t", ctypes.c_void_p), ("int64_t", ctypes.c_int64), ("size_t", ctypes.c_size_t),
            ("double", ctypes.c_double), ("float", ctypes.c_float), ("int", ctypes.c_int))
EXACT_SEEDS = list(range(1000, 1040))


def exact_scenes():
    return [s for s in (ph.make_scene(seed, 60, 20, 10, exact=True) for seed in EXACT_SEEDS) if ph.gap_of(s["H"]) >= ph.GAP]


# ---- the decomposition ----------------------------------------------------------------------------------------------------------------
def test_on_exact_scenes_the_chosen_candidate_is_the_ground_truth_and_every_candidate_reconstructs_the_homography():
    scenes = exact_scenes()
    assert len(scenes) >= 0.95 * len(EXACT_SEEDS)
    for i, s in enumerate(scenes):
        scale = (-1.0) ** i * (0.3 + 0.1 * i)                                 # any scale, either sign: the vote fixes the sign
        r = ph.restate(s["ml"], s["mr"], s["kind"] == 0, G=scale * s["H"], thr=2e-3)
        assert r["status"] == 1 and r["sign_sure"]
        for R, t, n in r["cands"]:
            assert np.abs(r["Gp"] - R - np.outer(t, n)).max() <= 64 * ph.EPS64 * np.linalg.norm(r["Gp"])
            assert np.abs(R.T @ R - np.eye(3)).max() <= TRUTH_TOL and abs(np.linalg.det(R) - 1) <= TRUTH_TOL
            assert abs(np.linalg.norm(t) - r["baseline"]) <= TRUTH_TOL and abs(np.linalg.norm(n) - 1) <= TRUTH_TOL
        assert np.abs(r["R"] - s["R"]).max() <= TRUTH_TOL and np.abs(r["n"] - s["n"]).max() <= TRUTH_TOL
        assert np.abs(r["t"] - s["t"] / np.linalg.norm(s["t"])).max() <= TRUTH_TOL
        assert abs(r["baseline"] - np.linalg.norm(s["t"]) / s["d"]) <= TRUTH_TOL
        E = ph.essential(s["R"], s["t"])
        assert np.abs(r["E"] - E).max() <= TRUTH_TOL and abs(np.linalg.norm(r["E"]) - 1) <= TRUTH_TOL


def test_the_eigenvector_form_and_the_svd_form_agree_and_their_difference_is_the_float64_constant():
    scenes, made = ph.comparison_scenes()
    assert len(scenes) >= (1 - ph.MAX_DROPPED) * made
    const = ph.float64_constant(scenes)
    print("the float64 constant over %d scenes: %.3e (the GPU bound is %g times it: %.3e)" % (len(scenes), const, ph.MARGIN, ph.MARGIN * const))
    assert 0 < const <= TRUTH_TOL
    for s in exact_scenes()[:10]:                                             # and on exact homographies, candidate for candidate
        r = ph.restate(s["ml"], s["mr"], s["kind"] == 0, G=s["H"])
        other = ph.candidates_svd(r["Gp"])
        assert sorted(ph.nearest(other, *c)[0] for c in r["cands"]) == [0, 1, 2, 3]
        assert max(ph.nearest(other, *c)[1] for c in r["cands"]) <= TRUTH_TOL


def test_at_most_five_percent_of_the_family_is_dropped_by_the_gap_condition():
    dropped = sum(ph.gap_of(ph.make_scene(5000 + i, 4)["H"]) < ph.GAP for i in range(2000))
    print("dropped by the gap condition: %d of 2000" % dropped)
    assert dropped <= ph.MAX_DROPPED * 2000
    kept, made = ph.comparison_scenes()
    assert made == len(ph.HOST_CASES) + len(ph.SMALL_BASELINE_CASES) and len(kept) >= (1 - ph.MAX_DROPPED) * made


def test_visibility_then_support_pick_the_true_candidate_when_matches_lie_off_the_plane():
    twofold = 0
    for c in ph.HOST_CASES:
        s = ph.make_scene(*c)
        xl, xr, used, M = ph.plane_moments(s)
        r = ph.restate(xl, xr, used, M=M, thr=2e-3)
        assert r["status"] == 1 and r["choice_sure"] and r["sign_sure"]
        assert ph.angle_R(r["R"], s["R"]) < 0.5 and ph.angle_t(r["t"], s["t"]) < 2.0 and float(r["t"] @ s["t"]) > 0
        assert float(r["n"] @ s["n"]) > 0.99 and r["front_count"] == int(used.sum())
        assert (r["sup"][:2] == r["sup"][2:]).all() and r["sup"][r["choice"]] == r["sup"].max()
        twofold += int((r["vis"] == r["vis"].max()).sum() >= 2)
        blind = ph.restate(xl, xr, used, M=M)                                 # without thr: visibility alone, sup = 0
        assert not blind["sup"].any() and (blind["vis"] == r["vis"]).all()
    assert twofold >= 1                                                       # the two-fold ambiguity occurs: sup is what decides there


def test_the_undecided_bands_of_the_committed_seeds_stay_below_one_percent():
    worst = 0.0
    for c, fam in [(c, "plane") for c in ph.HOST_CASES] + [(c, "small") for c in ph.SMALL_BASELINE_CASES]:
        s = ph.make_scene(*c, family=fam)
        xl, xr, used, M = ph.plane_moments(s)
        r = ph.restate(xl, xr, used, M=M, thr=2e-3)
        n_used, n_all = int(used.sum()), xl.shape[0]
        vis_band = int((r["vis_hi"] - r["vis_lo"]).max())
        sup_band = int((r["sup_hi"] - r["sup_lo"]).max())
        worst = max(worst, vis_band / n_used, sup_band / n_all)
        assert vis_band <= ph.BAND_CAP * n_used and sup_band <= ph.BAND_CAP * n_all, (c, vis_band, sup_band)
        assert r["sign_sure"]
    print("largest band share: %.4f" % worst)


def test_rotation_and_small_baseline_scenes():
    for i, c in enumerate(ph.ROTATION_CASES):
        s = ph.make_scene(*c, family="rotation")
        xl, xr, used, M = ph.plane_moments(s)
        r = ph.restate(xl, xr, used, M=M, thr=2e-3, min_baseline=5e-3)
        assert r["status"] == 2 and not r["t"].any() and not r["n"].any() and not r["E"].any() and not r["sup"].any()
        assert (r["vis"] == int(used.sum())).all() and r["choice"] == 0 and np.array_equal(r["front"], used)
        assert ph.angle_R(r["R"], s["R"]) < 0.1 and np.abs(r["R"].T @ r["R"] - np.eye(3)).max() < 1e-2
        ex = ph.make_scene(*c, family="rotation", exact=True)
        for scale in (1.0, -2.5):
            e = ph.restate(ex["ml"], ex["mr"], ex["kind"] == 0, G=scale * ex["H"], min_baseline=1e-9)
            assert e["status"] == 2 and np.abs(e["R"] - ex["R"]).max() <= TRUTH_TOL and e["baseline"] <= 1e-9
    for c in ph.SMALL_BASELINE_CASES:
        s = ph.make_scene(*c, family="small")
        xl, xr, used, M = ph.plane_moments(s)
        assert ph.restate(xl, xr, used, M=M, min_baseline=5e-3)["status"] == 1
        assert abs(ph.restate(xl, xr, used, M=M)["baseline"] - 0.01) < 2e-3
        assert ph.restate(xl, xr, used, M=M, min_baseline=2e-2)["status"] == 2


def test_no_pose_cases_of_the_restatement():
    s = ph.make_scene(*ph.HOST_CASES[0])
    xl, xr, used, M = ph.plane_moments(s)
    bad = M.copy()
    bad[2, 5] = np.nan
    rank1 = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0])
    for kw in ({"M": M, "best_count": 3}, {"M": bad}, {"model": np.zeros((3, 3), np.float32)}, {"G": rank1}):
        r = ph.restate(xl, xr, used, **kw)
        assert r["status"] == 0 and np.array_equal(r["R"], np.eye(3)) and not r["t"].any() and not r["vis"].any() and not r["front"].any()
    sing = ph.restate(xl, xr, used, G=np.diag([1.0, 1.0, 0.0]))               # lambda3 = 0 with a baseline: still a pose, and finite
    assert sing["status"] == 1 and all(np.isfinite(x).all() for c in sing["cands"] for x in c)
    assert ph.restate(xl, xr, used, G=np.diag([1.0, 1.0, 0.0]), min_baseline=10.0)["status"] == 0     # rotation only and l3 <= 0


def test_swapped_points_give_the_permuted_candidates():
    for s in exact_scenes()[:8]:
        used = s["kind"] == 0
        a = ph.restate(s["ml"], s["mr"], used, G=s["H"], thr=2e-3)
        b = ph.restate(s["ml"][:, ::-1], s["mr"][:, ::-1], used, G=ph.P_SWAP @ s["H"] @ ph.P_SWAP, thr=2e-3)
        sw = ph.swap(a)
        assert np.abs(b["R"] - sw["R"]).max() <= TRUTH_TOL and np.abs(b["t"] - sw["t"]).max() <= TRUTH_TOL
        assert np.abs(b["n"] - sw["n"]).max() <= TRUTH_TOL and np.abs(b["E"] - sw["E"]).max() <= TRUTH_TOL
        assert sorted(b["vis"].tolist()) == sorted(a["vis"].tolist()) and b["front_count"] == a["front_count"]
        assert np.array_equal(ph.swap(sw)["R"], a["R"]) and np.array_equal(ph.swap(sw)["cand_t"], a["cand_t"])      # an involution, exactly


def test_the_select_rules_truth_table():
    nan = float("nan")
    table = [  # best_count_e, best_count_h, status_h, ratio -> branch
        (100, 90, 1, 0.8, 2), (100, 79, 1, 0.8, 1), (100, 81, 1, 0.8, 2), (100, 90, 2, 0.8, 3), (100, 90, 0, 0.8, 1),
        (7, 5, 1, 0.8, 2), (7, 5, 2, 0.8, 3), (7, 500, 0, 0.8, 0), (0, 0, 0, 0.8, 0), (8, 4, 1, 0.5, 2), (8, 3, 1, 0.5, 1),
        (100, 10 ** 6, 1, nan, 1), (7, 10, 1, nan, 2), (7, 10, 0, nan, 0), (100, 0, 1, 0.0, 2), (100, 1, 1, -1.0, 2),
        (100, 10 ** 6, 1, float("inf"), 1), (0, 4, 1, float("inf"), 2), (2 ** 40, 2 ** 40, 1, 1.0, 2), (10, 8, 1, 0.8, 1)]
    for ce, chh, st, ratio, want in table:
        assert ph.select(ce, chh, st, ratio) == want, (ce, chh, st, ratio)
    # float32(0.8) is above 0.8: 8 >= float32(0.8) * 10 is false - the product is the rule's one rounding


# ---- the C-ABI surface ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_library_exports_the_four_symbols_with_the_headers_prototypes(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in SYMBOLS.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and len(got_args) == nargs, name
        for p, a in zip(params, got_args):                                    # the prototype's types against the ctypes table's
            want = next(ct for word, ct in CTYPE_OF if (word == "*" and "*" in p) or re.search(r"\b%s\b" % re.escape(word), p))
            assert a is want, (name, p, a)
    assert "pose_h.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.pats_homography_pose_workspace_bytes(48, 2048) == 0 and lib.pats_pose_select_workspace_bytes(48, 2048) == 0


@pytest.mark.parametrize("which", sorted(ph.ENTRY))
def test_every_bad_argument_is_refused_by_name_before_any_launch(lib, which):
    """Fake device addresses: validation refuses them before anything touches them (tests/test_pose_h_gpu.py repeats this with a real
    allocation behind the pointers, where a launch would be possible)."""
    assert ph.check_refusals(lib, which, 0x7f0000001000) > 60


def test_ops_and_batch_signatures_and_refusals_without_a_gpu():
    import inspect
    import torch
    from pats_amd import batch, ops
    assert str(inspect.signature(batch.pose_h_by_pair)) == \
        "(out, cap, thr=None, norm=None, swapped=False, front=False, candidates=False, min_baseline=0.0)"
    assert str(inspect.signature(batch.select_pose_by_pair)) == "(out, cap, ratio=0.8)"
    assert str(inspect.signature(batch.pose_branch)) == "(out, branch)"
    ml, off = torch.zeros(20, 2), torch.tensor([0, 10, 20])
    inl, bc, mom = torch.zeros(20, dtype=torch.uint8), torch.tensor([10, 10]), torch.zeros(2, 9, 9, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.homography_pose_by_pair(ml, ml, inl, bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="matches_l must be contiguous"):
        ops.homography_pose_by_pair(torch.zeros(20, 4)[:, ::2], ml, inl, bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="inlier must be uint8"):
        ops.homography_pose_by_pair(ml, ml, inl.int(), bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="thr must be float32"):
        ops.homography_pose_by_pair(ml, ml, inl, bc, moments=mom, pair_off=off, thr=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="give moments, or models and best"):
        ops.homography_pose_by_pair(ml, ml, inl, bc, pair_off=off)
    with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
        ops.homography_pose_by_pair(ml, ml, inl, bc, moments=mom)
    for bad in (float("nan"), -1.0):
        with pytest.raises(RuntimeError, match="min_baseline"):
            ops.homography_pose_by_pair(ml, ml, inl, bc, moments=mom, pair_off=off, min_baseline=bad)
    f64 = torch.float64
    pose = (torch.zeros(2, 3, 3, dtype=f64), torch.zeros(2, 3, 3, dtype=f64), torch.zeros(2, 3, dtype=f64), torch.zeros(2, dtype=torch.int64))
    st, ratio = torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_select_by_pair(pose, bc, inl, pose, st, bc, inl, ratio, pair_off=off)
    with pytest.raises(RuntimeError, match="ratio must be float32"):
        ops.pose_select_by_pair(pose, bc, inl, pose, st, bc, inl, ratio.double(), pair_off=off)
    with pytest.raises(RuntimeError, match="status_h must be int32"):
        ops.pose_select_by_pair(pose, bc, inl, pose, st.long(), bc, inl, ratio, pair_off=off)
    with pytest.raises(RuntimeError, match=r"\(E, R, t, front_count"):
        ops.pose_select_by_pair(pose[:3], bc, inl, pose, st, bc, inl, ratio, pair_off=off)
    cap = batch.Capacities(2, 5, 6)
    with pytest.raises(ValueError, match="run verify_h_by_pair first"):
        batch.pose_h_by_pair({}, cap)
    with pytest.raises(ValueError, match="pose_by_pair and pose_h_by_pair"):
        batch.select_pose_by_pair({"pose": pose}, cap)
    with pytest.raises(ValueError, match="verified_on"):
        batch.select_pose_by_pair({"pose": pose, "pose_h": pose, "verified_on": "all", "verified_h_on": "topk"}, cap)
    with pytest.raises(ValueError, match="branch must be"):
        batch.pose_branch({"pose": pose}, "affine")
    with pytest.raises(ValueError, match="run pose_by_pair first"):
        batch.pose_branch({}, "epipolar")
    with pytest.raises(ValueError, match="run pose_h_by_pair first"):
        batch.pose_branch({"pose": pose}, "planar")
    with pytest.raises(ValueError, match="run select_pose_by_pair first"):
        batch.pose_branch({"pose": pose, "pose_h": pose}, "selected")
    full = {"pose": pose, "verified": ("c", "b", "bc", "i"), "verified_on": "all", "verified_models": "m", "points": 1, "pose_error": 2,
            "pose_h": pose[:3], "verified_h": ("ch", "bh", "bch", "ih"), "verified_h_on": "all", "verified_h_models": "mh", "summary": 3}
    view = batch.pose_branch(full, "planar")
    assert view["pose"] is full["pose_h"] and view["verified"] is full["verified_h"] and view["verified_models"] == "mh"
    assert "points" not in view and "pose_error" not in view and view["summary"] == 3
    same = batch.pose_branch(full, "epipolar")
    assert same["pose"] is pose and same["verified"] is full["verified"] and "points" not in same
    assert full["pose"] is pose and full["points"] == 1 and full["pose_error"] == 2 and len(full) == 11      # the result is never touched
