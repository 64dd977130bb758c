"""CPU-only: the numpy restatement of the pose-error stage and its AUC (tests/pose_error_cases.py) against the reference's recorded
outputs (tests/golden/pose_metrics.npz, written by tools/make_pose_metrics_golden.py from utils/metrics.py itself):
    AUC      `below` exactly, auc within n 2^-50 relative (both sides add at most n + 1 non-negative float64 terms)
    angles   within the angle's conditioning: the cosine moved by 16 * 2^-53 * sum|terms| in both directions, clipped, the spread of
             acos over that interval, plus 8 ulps of the result (the reference's np.dot / np.trace / np.linalg.norm fix no
             summation order, so near c = +-1 a bare ulp bound would be wrong)
    T0       the rigid R1 R0^T, t1 - R_gt t0 against numpy's T1 inv(T0) (the reference's general inverse): the same bound
and the entry points exist: the symbols are exported with the header's argument counts, ops refuses CPU tensors, and the batch
function needs a pose.  No kernel runs here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import pose_error_cases as pe
from conftest import REPO, golden

SYMBOLS = {"pats_pose_error_by_pair_f64": (ctypes.c_int, 13), "pats_pose_auc_max_n": (ctypes.c_int64, 0), "pats_pose_auc_f64": (ctypes.c_int, 8)}
MOVES_REFERENCE = 16


@pytest.fixture(scope="module")
def gold():
    return golden("pose_metrics.npz")


def _reference_angles(R, t, R_gt, t_gt):
    """angle_error_mat and the folded angle_error_vec as the reference writes them (np.trace, np.dot, np.linalg.norm): for ground
    truths the golden file could not hold, since compute_pose_error itself needs OpenCV."""
    with np.errstate(all="ignore"):
        eR = np.array([np.rad2deg(np.abs(np.arccos(np.clip((np.trace(np.dot(a.T, b)) - 1) / 2, -1.0, 1.0)))) for a, b in zip(R, R_gt)])
        e = np.array([np.rad2deg(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))) for a, b in zip(t, t_gt)])
    return eR, np.minimum(e, 180 - e)


def _within(ref, want_R, want_t, moves):
    worst = 0.0
    for k, c, a, want in (("err_R", "cos_R", "abs_R", want_R), ("err_t", "cos_t", "abs_t", want_t)):
        bound = pe.angle_bound(ref[c], ref[a], ref[k], moves)
        diff = np.abs(ref[k] - want)
        print("%s: largest difference %.3g degrees, %.3g of its bound" % (k, diff.max(), (diff / bound).max()))
        assert (diff <= bound).all(), (k, int(np.argmax(diff / bound)))
        worst = max(worst, float((diff / bound).max()))
    return worst


def test_the_angles_are_the_references_within_their_conditioning(gold):
    R, t, Rg, tg = gold["pose_R"], gold["pose_t"], gold["pose_R_gt"], gold["pose_t_gt"]
    assert len(R) >= len(pe.ANGLES) * len(pe.T_KINDS)
    ref = pe.pose_error64(R, t, pe.as_T(Rg, tg))
    assert not ref["status"].any() and np.isfinite(ref["err"]).all()
    _within(ref, gold["pose_err_R"], gold["pose_err_t"], MOVES_REFERENCE)
    assert np.array_equal(ref["err"], np.maximum(ref["err_R"], ref["err_t"]))
    # the set reaches what it was built for: identical and opposite rotations, the fold, parallel and orthogonal translations
    assert (gold["pose_err_R"] < 1e-4).sum() >= 24 and gold["pose_err_R"].max() > 180.0 - 1e-4
    assert gold["pose_err_t"].min() < 1e-6 and gold["pose_err_t"].max() > 90 - 1e-6 and (ref["e_t"] > 179.0).any()


def test_the_rigid_ground_truth_is_numpys_t1_inv_t0_within_the_same_bound(gold):
    R, t, T0, T1 = gold["pose_R"], gold["pose_t"], gold["pose_T0"], gold["pose_T1"]
    ref = pe.pose_error64(R, t, T1, T0)
    rel = T1 @ np.linalg.inv(T0)
    _within(ref, *_reference_angles(R, t, rel[:, :3, :3], rel[:, :3, 3]), MOVES_REFERENCE)
    # and the product is the ground truth the extrinsics were made from
    plain = pe.pose_error64(R, t, pe.as_T(gold["pose_R_gt"], gold["pose_t_gt"]))
    _within(ref, plain["err_R"], plain["err_t"], MOVES_REFERENCE)


def test_auc_and_below_are_the_references(gold):
    lists = pe.error_lists(0)
    assert {int(k.split("_")[1]) for k in lists} == set(pe.AUC_SIZES) | {200}
    worst = 0.0
    for name in lists:
        eR, eT = gold["auc_%s_err_R" % name], gold["auc_%s_err_t" % name]
        errors = np.maximum(eR, eT)
        auc, below, srt = pe.auc64(errors)
        want = gold["auc_%s_ref" % name]
        assert np.array_equal(below, gold["auc_%s_below" % name]), name
        assert (np.abs(auc - want) <= pe.auc_bound(errors.size, want)).all(), (name, auc, want)
        if want.any():
            worst = max(worst, float((np.abs(auc - want) / want.clip(1e-300)).max()))
        assert np.array_equal(srt, np.sort(errors))
    print("largest relative AUC difference %.3g" % worst)
    ties = np.maximum(gold["auc_ties_200_err_R"], gold["auc_ties_200_err_t"])
    for j, thr in enumerate(pe.THRESHOLDS):                               # an error equal to the threshold is out
        assert (ties == thr).sum() >= 1 and gold["auc_ties_200_below"][j] == (ties < thr).sum()
    assert np.isinf(np.maximum(gold["auc_inf_4000_err_R"], gold["auc_inf_4000_err_t"])).mean() > 0.15


def test_statuses_and_the_stated_departures_of_the_restatement():
    R, t, Rg, tg = pe.pose_sets(5, 12)
    T1 = pe.as_T(Rg, tg)
    counts = np.array([14, 15] * 6)
    ref = pe.pose_error64(R, t, T1, counts=counts)
    assert ref["status"].tolist() == [1, 0] * 6 and np.isinf(ref["err"][::2]).all() and np.isfinite(ref["err"][1::2]).all()
    R2, t2, T2 = R.copy(), t.copy(), T1.copy()
    R2[0], t2[0] = np.eye(3), 0.0                                          # pose_by_pair's "no pose"
    R2[1, 2, 1], t2[2, 0], T2[3, 1, 3], T2[4, 3, 0] = np.nan, np.inf, np.nan, np.nan      # the last one is in the row that is not read
    T2[0, 0, 0] = np.inf                                                   # two apply: the lower number wins
    ref = pe.pose_error64(R2, t2, T2, counts=np.array([20, 20, 20, 20, 20, 3] + [20] * 6))
    assert ref["status"].tolist() == [2, 2, 2, 3, 0, 1] + [0] * 6
    for k in ("err_R", "err_t", "err"):
        assert not np.isnan(ref[k]).any() and np.isinf(ref[k][[0, 1, 2, 3, 5]]).all() and np.isfinite(ref[k][4])
    T3 = T1.copy()
    T3[0, :3, 3] = 0.0
    T3[1, :3, 3] = [3e-4, 0.0, 4e-4]                                       # |t_gt| = 5e-4
    assert pe.pose_error64(R, t, T3)["err_t"][0] == 0.0
    assert pe.pose_error64(R, t, T3, min_gt_t=6e-4)["err_t"][1] == 0.0 and pe.pose_error64(R, t, T3, min_gt_t=4e-4)["err_t"][1] > 0.0
    big = pe.pose_error64(R * 1e200, t, T1 * 1e200)                         # an overflow inside an evaluated pair: +inf, never a NaN
    assert not big["status"].any() and not np.isnan(big["err"]).any() and np.isinf(big["err"]).any()


# ---- the feature exists: these fail without it ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    assert "Per-pair pose error and AUC (ABI 8, symbols added)" in header
    for name, (res, nargs) in SYMBOLS.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "pose_error.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.pats_pose_auc_max_n() == pe.MAX_N


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
ERR_REQUIRED = ("R", "t", "T1", "err_R", "err_t", "err", "status")
ERR_OPTIONAL = ("T0", "counts")
ERR_ALIGN = {"R": 8, "t": 8, "T1": 8, "T0": 8, "counts": 8, "err_R": 8, "err_t": 8, "err": 8, "status": 4}
ERR_ORDER = ("R", "t", "T1", "T0", "counts", "pairs", "min_matches", "min_gt_t", "err_R", "err_t", "err", "status")


def call_error(lib, pairs=2, min_matches=15, min_gt_t=0.0, **ptrs):
    a = {n: A16 for n in ERR_REQUIRED + ERR_OPTIONAL}
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    p.update(pairs=pairs, min_matches=min_matches, min_gt_t=min_gt_t)
    return lib.pats_pose_error_by_pair_f64(*[p[n] for n in ERR_ORDER], None)


def error_refusals(base=A16):
    """Every refusal of the header's list for the per-pair entry -> [(keyword arguments of call_error(), the message's words)]."""
    out = [({name: 0}, (b"null", name.encode())) for name in ERR_REQUIRED]
    for name in sorted(ERR_ALIGN):
        out += [({name: base + off}, (b"%d-byte aligned" % ERR_ALIGN[name], name.encode())) for off in ((1, 2, 3) if ERR_ALIGN[name] == 4 else (1, 2, 4))]
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -2}, b"pairs"), ({"pairs": 2 ** 31}, b"pairs"),
                                           ({"min_matches": -1}, b"min_matches"), ({"min_gt_t": -1e-300}, b"min_gt_t"),
                                           ({"min_gt_t": float("nan")}, b"min_gt_t"))]
    return out


AUC_ORDER = ("errors", "n", "thresholds", "n_thr", "auc", "below", "sorted")


def call_auc(lib, n=100, thresholds=(5.0, 10.0, 20.0), n_thr=None, null_thresholds=False, **ptrs):
    a = {"errors": A16, "auc": A16, "below": A16, "sorted": A16}
    a.update(ptrs)
    p = {k: (ctypes.c_void_p(v) if v else None) for k, v in a.items()}
    thr = (ctypes.c_double * max(len(thresholds), 1))(*thresholds)
    p.update(n=n, thresholds=None if null_thresholds else thr, n_thr=len(thresholds) if n_thr is None else n_thr)
    return lib.pats_pose_auc_f64(*[p[k] for k in AUC_ORDER], None)


def auc_refusals(base=A16):
    out = [({name: 0}, (b"null", name.encode())) for name in ("errors", "auc", "below")] + [({"null_thresholds": True}, (b"null", b"thresholds"))]
    for name in ("errors", "auc", "below", "sorted"):
        out += [({name: base + off}, (b"8-byte aligned", name.encode())) for off in (1, 2, 4)]
    out += [({"n": v}, (b"n =",)) for v in (pe.MAX_N + 1, -1, 2 ** 40)]
    out += [({"n_thr": 0}, (b"n_thr",)), ({"thresholds": (1.0,) * 9}, (b"n_thr",)), ({"n_thr": -1}, (b"n_thr",))]
    out += [({"thresholds": (5.0, v, 20.0)}, (b"thresholds[1]",)) for v in (0.0, -0.0, -5.0, float("inf"), float("-inf"), float("nan"))]
    return out


def refused(lib, call, who, kw, words):
    assert call(lib, **kw) != 0, kw
    msg = lib.pats_last_error()
    assert who in msg and all(w in msg for w in words), (kw, msg)


def test_every_bad_argument_is_refused_by_name(lib):
    cases = error_refusals()
    assert len(cases) > 35
    for kw, words in cases:
        refused(lib, call_error, b"pose_error_by_pair", kw, words)
    cases = auc_refusals()
    assert len(cases) > 25
    for kw, words in cases:
        refused(lib, call_auc, b"pose_auc", kw, words)


def test_ops_refuse_cpu_tensors_bad_layouts_and_bad_types():
    import torch
    from pats_amd import ops
    f64 = torch.float64
    R, t, T1 = torch.zeros(2, 3, 3, dtype=f64), torch.zeros(2, 3, dtype=f64), torch.zeros(2, 4, 4, dtype=f64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_error_by_pair(R, t, T1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_auc(torch.zeros(10, dtype=f64))
    with pytest.raises(RuntimeError, match="R must be contiguous"):
        ops.pose_error_by_pair(R.transpose(1, 2), t, T1)
    with pytest.raises(RuntimeError, match="T0 must be contiguous"):
        ops.pose_error_by_pair(R, t, T1, T0=T1.transpose(1, 2))
    for kw, word in (({"R": R.float()}, "R must be float64"), ({"t": t.float()}, "t must be float64"), ({"T1": T1.float()}, "T1 must be float64"),
                     ({"T0": T1.float()}, "T0 must be float64"), ({"counts": torch.zeros(2, dtype=torch.int32)}, "counts must be int64")):
        args = dict(R=R, t=t, T1=T1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.pose_error_by_pair(**args)
    with pytest.raises(RuntimeError, match="errors must be float64"):
        ops.pose_auc(torch.zeros(10))
    with pytest.raises(RuntimeError, match="errors must be contiguous"):
        ops.pose_auc(torch.zeros(20, dtype=f64)[::2])
    assert str(inspect.signature(ops.pose_error_by_pair)) == "(R, t, T1, T0=None, counts=None, min_matches=15, min_gt_t=0.0, out=None)"
    assert str(inspect.signature(ops.pose_auc)) == "(errors, thresholds=(5.0, 10.0, 20.0), return_sorted=False, out=None)"
    assert ops.pose_auc_max_n() == pe.MAX_N


def test_batch_pose_error_by_pair_needs_a_pose():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    with pytest.raises(ValueError, match="pose_by_pair"):
        batch.pose_error_by_pair({"matches_l": None, "matches_r": None, "verified": (None,) * 4, "verified_on": "all"}, cap, None)
    import torch
    f64 = torch.float64
    posed = {"pose": (None, torch.zeros(2, 3, 3, dtype=f64), torch.zeros(2, 3, dtype=f64)), "summary": torch.zeros(6, dtype=torch.int64)}
    for into in ((torch.zeros(8, dtype=f64), 0), (torch.zeros(8), 0), (torch.zeros(8, dtype=f64), 7), (torch.zeros(8, dtype=f64), -1), (None, 0)):
        with pytest.raises(ValueError, match="into must be"):                 # a running buffer on the CPU among them: named, before any call
            batch.pose_error_by_pair(dict(posed), cap, torch.zeros(2, 4, 4, dtype=f64), into=into)
    assert str(inspect.signature(batch.pose_error_by_pair)) == "(out, cap, T1, T0=None, min_matches=15, min_gt_t=0.0, into=None)"
