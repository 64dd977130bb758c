"""GPU: ops.epipolar_pose_by_pair / batch.pose_by_pair against the definition of include/pats_amd.h restated in numpy float64
(tests/pose_cases.py):
    e_refit      residual r(e) = |M e - (e^T M e) e| / (eps64 |M|_F) <= 8 b64, b64 = what numpy's eigh reaches on the same moments in
                 the same run; Rayleigh quotient and angle to numpy's vector by the residual bounds of a symmetric matrix
    E, R, t      against a host float64 SVD of the device's OWN outputs, within TOL = 2^12 eps64: a condition (the conditioning is
                 s1 / (s2 - s3) ~ 1.4: a float64 implementation lands within a few eps), five orders below any float32 step
    counts       equal to the float64 counts outside the undecided band (cell for cell for the chosen candidate's mask), the band's
                 share capped at 1e-3; choice and front consistent with the device's own counts exactly
    ground truth the device's angular errors within 1e-6 degrees of the host pipeline's on the same inliers
Measured on an MI355X: b64 = 0.45, the device's worst r = 0.67; docs/parity.md records them with the band shares.
Every output lies inside a larger sentinel-filled buffer and every input list in a larger NaN-filled one."""
import os
import re

import numpy as np
import pytest
import torch

import epipolar_cases as ec
import pose_cases as pc
from conftest import REPO

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0xAB
TOL = 2.0 ** 12 * pc.EPS64
MARGIN = 8.0
UNDECIDED_CAP = 1e-3
POSE_DEG = 5.0          # tests/test_pose_cases_host.py derives it: below any transposition error, far above the noise


def _kernel_constant(name):
    src = open(os.path.join(REPO, "pats_amd", "csrc", "pose.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


T = _kernel_constant("POSE_THREADS")                   # threads per workgroup = matches per step of a segment's walk


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a, fill):
    """a as a view of a longer buffer whose rows beyond it hold `fill`."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.shape[0] + PAD,) + a.shape[1:], fill, dtype=cu(a[:0]).dtype, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


NAMES = ("E", "R", "t", "front_count", "front_counts", "choice", "front", "e_refit")


def run(ops, ml, mr, inl, bc, **kw):
    """One call on fresh sentinel buffers -> dict of numpy arrays (the surroundings checked)."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs, cap = len(bc), ml.shape[0]
    shapes = [((pairs, 3, 3), torch.float64, SENT_F), ((pairs, 3, 3), torch.float64, SENT_F), ((pairs, 3), torch.float64, SENT_F),
              ((pairs,), torch.int64, SENT_I), ((pairs, 4), torch.int32, SENT_I), ((pairs,), torch.int32, SENT_I),
              ((cap,), torch.uint8, SENT_B), ((pairs, 9), torch.float64, SENT_F)]
    bufs, views = [], []
    for shape, dt, sent in shapes:
        b = torch.full((int(np.prod(shape)) + 2 * PAD,), sent, dtype=dt, device="cuda")
        bufs.append((b, sent))
        views.append(b[PAD:b.numel() - PAD].view(shape))
    got = ops.epipolar_pose_by_pair(guarded(ml, float("nan")), guarded(mr, float("nan")), guarded(inl.astype(np.uint8), 1),
                                    cu(np.asarray(bc, np.int64)), return_front=True, return_refit=True, out=tuple(views), **d)
    torch.cuda.synchronize()
    assert len(got) == 8 and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    for b, sent in bufs:
        assert bool((torch.cat([b[:PAD], b[b.numel() - PAD:]]) == sent).all()), "bytes around an output view changed"
    out = {n: v.cpu().numpy() for n, v in zip(NAMES, views)}
    for n in ("E", "R", "t", "e_refit"):
        assert np.isfinite(out[n]).all() and not (out[n] == SENT_F).any(), n
    assert not (out["front_counts"] == SENT_I).any() and not (out["choice"] == SENT_I).any() and not (out["front_count"] == SENT_I).any()
    assert set(np.unique(out["front"]).tolist()) <= {0, 1}
    return out


def pack(scenes):
    """Scenes -> (ml, mr [cap,2], pair_off, segs)."""
    lens = [s["ml"].shape[0] for s in scenes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ml = np.concatenate([s["ml"] for s in scenes]).reshape(-1, 2).astype(np.float32)
    mr = np.concatenate([s["mr"] for s in scenes]).reshape(-1, 2).astype(np.float32)
    return ml, mr, off, [(int(off[i]), lens[i]) for i in range(len(lens))]


def no_pose(out, p):
    return (not out["E"][p].any() and np.array_equal(out["R"][p], np.eye(3)) and not out["t"][p].any() and not out["front_counts"][p].any()
            and out["choice"][p] == 0 and out["front_count"][p] == 0)


def check_pair(out, p, xl, xr, used, front_seg, M=None, stats=None, unit=True):
    """Everything the definition says about pair p with a pose, from the device's own e_refit on."""
    e, E, R, t = out["e_refit"][p], out["E"][p], out["R"][p], out["t"][p]
    assert not unit or abs(np.linalg.norm(e) - 1) <= TOL
    if M is not None:
        assert pc.residual(M, e) <= MARGIN * stats["b64"]
    # projection and decomposition against a host SVD of the device's outputs
    assert np.abs(np.linalg.svd(E, compute_uv=False) - [np.sqrt(0.5), np.sqrt(0.5), 0.0]).max() <= TOL
    assert np.abs(E - pc.project64(e)).max() <= TOL
    assert E.reshape(-1)[int(np.argmax(np.abs(E)))] > 0
    assert np.abs(R.T @ R - np.eye(3)).max() <= TOL and abs(np.linalg.det(R) - 1) <= TOL and abs(np.linalg.norm(t) - 1) <= TOL
    tx = pc.cross_matrix(t) @ R
    tx /= np.linalg.norm(tx)
    assert min(np.abs(tx - E).max(), np.abs(tx + E).max()) <= TOL
    # the device's candidate d is the host's candidate d ^ m (which member is R1, and the sign of u, are the SVD's freedom)
    cands = pc.candidates64(E.reshape(9))
    ch = int(out["choice"][p])
    j = pc.match_candidates(cands, R, t)
    assert np.abs(cands[j][0] - R).max() <= TOL and np.abs(cands[j][1] - t).max() <= TOL
    m = ch ^ j
    f64, und = pc.fronts(xl, xr, used, cands)
    counts = out["front_counts"][p]
    for d in range(4):
        strict, loose = int((f64[d ^ m] & ~und[d ^ m]).sum()), int((f64[d ^ m] | und[d ^ m]).sum())
        assert strict <= counts[d] <= loose, (p, d, strict, int(counts[d]), loose)
    assert ch == int(np.argmax(counts)) and out["front_count"][p] == counts[ch]
    assert int(front_seg.sum()) == out["front_count"][p]
    keep = ~und[j]
    assert np.array_equal(front_seg[keep].astype(bool), f64[j][keep])
    if stats is not None:
        stats["cells"] += und.size
        stats["undecided"] += int(und.sum())


# ---- 1. accuracy on the committed scenes ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_scenes():
    out = []
    for seed, n in pc.HOST_CASES:
        s = pc.make_scene(seed, n)
        s["xl"], s["xr"] = ec.points32(s["ml"], s["mr"])
        s["M"] = ec.moments64(s["xl"], s["xr"], s["good"])[0]
        out.append(s)
    return out


def test_refit_projection_and_decomposition_on_the_host_cases(ops, host_scenes):
    ml, mr, off, segs = pack(host_scenes)
    M = np.stack([s["M"] for s in host_scenes])
    good = np.concatenate([s["good"] for s in host_scenes])
    out = run(ops, ml, mr, good, [int(s["good"].sum()) for s in host_scenes], moments=M, pair_off=off)
    stats = {"b64": max(pc.residual(s["M"], pc.refit64(s["M"])[0]) for s in host_scenes), "cells": 0, "undecided": 0}
    worst = 0.0
    for p, (s, (lo, n)) in enumerate(zip(host_scenes, segs)):
        e = out["e_refit"][p]
        e0, w = pc.refit64(s["M"])
        r_dev, r_np, fro = pc.residual(s["M"], e), pc.residual(s["M"], e0), np.linalg.norm(s["M"])
        worst = max(worst, r_dev)
        assert e @ s["M"] @ e <= w[0] + MARGIN * stats["b64"] * pc.EPS64 * fro
        sin = np.linalg.norm(e - (e @ e0) * e0) / np.linalg.norm(e)            # the part of e across numpy's vector
        assert sin <= (r_dev + r_np) * pc.EPS64 * fro / (w[1] - w[0])
        check_pair(out, p, s["xl"], s["xr"], s["good"], out["front"][lo:lo + n], M=s["M"], stats=stats)
        # ground truth: the device against the host pipeline on the same inliers
        ref = pc.reference(s["xl"], s["xr"], s["good"], M=s["M"])
        assert abs(pc.angle_R(out["R"][p], s["R"]) - pc.angle_R(ref["R"], s["R"])) <= 1e-6
        assert abs(pc.angle_t(out["t"][p], s["t"]) - pc.angle_t(ref["t"], s["t"])) <= 1e-6
        assert pc.angle_R(out["R"][p], s["R"]) < POSE_DEG and float(out["t"][p] @ s["t"]) > 0
    print("b64 = %.3f, device worst r = %.3f; undecided %d of %d cells" % (stats["b64"], worst, stats["undecided"], stats["cells"]))
    assert worst <= MARGIN * stats["b64"]


@pytest.mark.parametrize("used", ["verified", "all"])
def test_counts_choice_and_mask_against_float64(ops, host_scenes, used):
    """Once with the verification's own mask and moments (the true model as the only hypothesis), once with every match used:
    then the outliers vote too and several candidates hold matches."""
    ml, mr, off, segs = pack(host_scenes)
    pairs = len(host_scenes)
    models = np.stack([pc.true_model(s) for s in host_scenes]).reshape(pairs, 1, 3, 3)
    ver = ops.epipolar_score_by_pair(cu(ml), cu(mr), cu(models), cu(np.full(pairs, 2e-3, np.float32)), pair_off=cu(off), moments=True)
    inl, bc, M = ver[3].cpu().numpy().astype(bool), ver[2].cpu().numpy(), ver[4].cpu().numpy()
    if used == "all":
        inl = np.ones_like(inl)
    out = run(ops, ml, mr, inl, bc, moments=M, pair_off=off)
    stats = {"b64": max(pc.residual(m, pc.refit64(m)[0]) for m in M), "cells": 0, "undecided": 0}
    for p, (s, (lo, n)) in enumerate(zip(host_scenes, segs)):
        check_pair(out, p, s["xl"], s["xr"], inl[lo:lo + n], out["front"][lo:lo + n], M=M[p], stats=stats)
        if used == "all" and n >= 500:
            assert (out["front_counts"][p] > 0).sum() >= 2                      # the vote is a contest here, not a formality
        else:
            assert out["front_count"][p] >= 0.9 * bc[p]
    print("%s: undecided %d of %d cells (%.2e)" % (used, stats["undecided"], stats["cells"], stats["undecided"] / stats["cells"]))
    assert stats["undecided"] <= UNDECIDED_CAP * stats["cells"]


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------
NORM = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)


def edge_case(lengths, seed0, norm):
    scenes = [pc.make_scene(seed0 + i, n, outliers=0.0) for i, n in enumerate(lengths)]
    ml, mr, off, segs = pack(scenes)
    nm = None if not norm else np.tile(NORM, (len(lengths), 1)) + np.arange(len(lengths), dtype=np.float32)[:, None] * np.float32(0.01)
    pts = [ec.points32(s["ml"], s["mr"], None if nm is None else nm[i]) for i, s in enumerate(scenes)]
    M = np.stack([ec.moments64(xl, xr, s["good"])[0] for (xl, xr), s in zip(pts, scenes)])
    good = np.concatenate([s["good"] for s in scenes]) if sum(lengths) else np.zeros(0, bool)
    return scenes, ml, mr, off, segs, nm, pts, M, good


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("lengths", [[0], [7], [8], [1, 0, 63], [64, 0, 65], [T - 1, 0, T], [T + 1, 0, 2 * T + 1]])
def test_segment_lengths_around_eight_the_wave_and_the_workgroup_in_both_forms(ops, lengths, norm):
    scenes, ml, mr, off, segs, nm, pts, M, good = edge_case(lengths, 400 + sum(lengths), norm)
    pairs = len(lengths)
    bc = [int(s["good"].sum()) for s in scenes]
    kw = {} if nm is None else {"norm": nm}
    out = run(ops, ml, mr, good, bc, moments=M, pair_off=off, **kw)
    stats = {"b64": 1.0, "cells": 0, "undecided": 0}
    for p, (lo, n) in enumerate(segs):
        if bc[p] < pc.MIN_INLIERS:
            assert no_pose(out, p) and not out["e_refit"][p].any() and not out["front"][lo:lo + n].any()
        else:
            check_pair(out, p, pts[p][0], pts[p][1], scenes[p]["good"], out["front"][lo:lo + n], stats=stats)
    # the strided form: the same segments in rows of `stride`, the slack filled with NaN rows marked as inliers
    stride = max(lengths) + 3
    sl, sr = np.full((pairs, stride, 2), np.nan, np.float32), np.full((pairs, stride, 2), np.nan, np.float32)
    si = np.ones((pairs, stride), bool)
    for p, (lo, n) in enumerate(segs):
        sl[p, :n], sr[p, :n], si[p, :n] = ml[lo:lo + n], mr[lo:lo + n], good[lo:lo + n]
    two = run(ops, sl.reshape(-1, 2), sr.reshape(-1, 2), si.reshape(-1), bc, moments=M, stride=stride,
              counts=np.asarray(lengths, np.int64), **kw)
    for n_ in ("E", "R", "t", "e_refit", "front_count", "front_counts", "choice"):
        assert out[n_].tobytes() == two[n_].tobytes(), n_
    f2 = two["front"].reshape(pairs, stride)
    for p, (lo, n) in enumerate(segs):
        assert np.array_equal(f2[p, :n], out["front"][lo:lo + n]) and not f2[p, n:].any()


def test_corrupt_offsets_and_counts_stay_inside_the_arrays(ops):
    scenes, ml, mr, off, segs, _, pts, M, good = edge_case([300, 200, 100], 77, False)
    bc = [int(s["good"].sum()) for s in scenes]
    bad_off = np.array([-5, 250, 2 ** 40, 100], np.int64)                    # clamped: [0,250), [250,600), empty
    out = run(ops, ml, mr, good, bc, moments=M, pair_off=bad_off)
    segs2 = ec.segments(3, 600, pair_off=bad_off)
    assert segs2 == [(0, 250), (250, 350), (600, 0)]
    assert out["front_counts"][2].sum() == 0 and not out["front"][600:].any()
    for p, (lo, n) in enumerate(segs2[:2]):
        assert int(out["front"][lo:lo + n].sum()) == out["front_count"][p]
    two = run(ops, ml, mr, good, bc, moments=M, stride=200, counts=np.array([-3, 2 ** 50, 150], np.int64))
    for p, (lo, n) in enumerate(ec.segments(3, 600, stride=200, counts=[-3, 2 ** 50, 150])):
        assert int(two["front"][lo:lo + n].sum()) == two["front_count"][p] and not two["front"][lo + n:(p + 1) * 200].any()
    assert two["front_count"][0] == 0


def test_empty_arrays_define_every_per_pair_output(ops):
    s = pc.make_scene(5, 50, outliers=0.0)
    xl, xr = ec.points32(s["ml"], s["mr"])
    M = np.stack([ec.moments64(xl, xr, s["good"])[0], np.zeros((9, 9))])
    out = run(ops, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, bool), [50, 0], moments=M,
              pair_off=np.zeros(3, np.int64))
    assert no_pose(out, 1) and not out["front_counts"].any() and out["front"].size == 0
    assert np.abs(out["E"][0] - pc.project64(pc.refit64(M[0])[0])).max() <= TOL          # a pose without a vote: candidate 0
    assert out["choice"][0] == 0 and abs(np.linalg.det(out["R"][0]) - 1) <= TOL


def test_no_pose_cases_disturb_no_other_pair(ops):
    lengths = [120, 120, 120, 120, 120, 120]
    scenes, ml, mr, off, segs, _, pts, M, good = edge_case(lengths, 900, False)
    bc = [int(s["good"].sum()) for s in scenes]
    clean = run(ops, ml, mr, good, bc, moments=M, pair_off=off)
    assert not any(no_pose(clean, p) for p in range(6))
    M2, bc2, ml2 = M.copy(), list(bc), ml.copy()
    bc2[0] = 7                                                                # too few inliers
    M2[1] = 0.0                                                               # zero moments: a refit of rank 1
    M2[2][4, 7] = np.nan                                                      # read through the upper triangle
    M2[3][0, 0] = np.inf
    first = segs[4][0] + int(np.flatnonzero(scenes[4]["good"])[0])
    ml2[first, 1] = np.inf                                                    # a used match that is not finite: not used
    out = run(ops, ml2, mr, good, bc2, moments=M2, pair_off=off)
    for p in range(4):
        lo, n = segs[p]
        assert no_pose(out, p) and not out["front"][lo:lo + n].any(), p
    assert not out["e_refit"][0].any() and not out["e_refit"][2].any() and not out["e_refit"][3].any()
    for n_ in ("E", "R", "t", "e_refit", "front_count", "front_counts", "choice"):
        assert out[n_][5].tobytes() == clean[n_][5].tobytes(), n_
    lo, n = segs[5]
    assert np.array_equal(out["front"][lo:lo + n], clean["front"][lo:lo + n])
    # pair 4 keeps its pose (the moments are the caller's), the match is out of the vote
    lo, n = segs[4]
    assert out["E"][4].tobytes() == clean["E"][4].tobytes() and out["front"][first] == 0
    assert out["front_count"][4] == clean["front_count"][4] - int(clean["front"][first])
    # NaN moments as a whole
    M3 = M.copy()
    M3[0] = np.nan
    out = run(ops, ml, mr, good, bc, moments=M3, pair_off=off)
    assert no_pose(out, 0) and out["E"][1].tobytes() == clean["E"][1].tobytes()


def test_the_winning_model_as_the_source_equals_its_projector_as_moments(ops):
    lengths = [200, 90]
    scenes, ml, mr, off, segs, _, pts, M, good = edge_case(lengths, 50, False)
    bc = [int(s["good"].sum()) for s in scenes]
    H = 3
    models = np.zeros((2, H, 3, 3), np.float32)
    best = np.array([2, 1], np.int32)
    for p, s in enumerate(scenes):
        models[p, best[p]] = pc.true_model(s)
    a = run(ops, ml, mr, good, bc, models=models, best=best, pair_off=off)
    proj = []
    for p in range(2):
        e = models[p, best[p]].astype(np.float64).reshape(9)
        assert np.array_equal(a["e_refit"][p], e)                             # promoted, nothing else
        proj.append(np.eye(9) - np.outer(e, e) / (e @ e))
    b = run(ops, ml, mr, good, bc, moments=np.stack(proj), pair_off=off)
    for p, (lo, n) in enumerate(segs):
        check_pair(a, p, pts[p][0], pts[p][1], scenes[p]["good"], a["front"][lo:lo + n], unit=False)
        assert np.abs(a["E"][p] - b["E"][p]).max() <= TOL and np.abs(a["R"][p] - b["R"][p]).max() <= TOL
        assert np.abs(a["t"][p] - b["t"][p]).max() <= TOL
        und = pc.fronts(pts[p][0], pts[p][1], scenes[p]["good"], [(a["R"][p], a["t"][p])])[1]
        assert abs(int(a["front_count"][p]) - int(b["front_count"][p])) <= int(und.sum())
    zero = run(ops, ml, mr, good, bc, models=np.zeros((2, 1, 3, 3), np.float32), best=np.array([5, -2], np.int32), pair_off=off)
    assert no_pose(zero, 0) and no_pose(zero, 1)                              # a zero model; best is clamped, never followed outside


def test_swapped_is_an_exact_permutation(ops, host_scenes):
    ml, mr, off, segs = pack(host_scenes[:4])
    M = np.stack([s["M"] for s in host_scenes[:4]])
    good = np.concatenate([s["good"] for s in host_scenes[:4]])
    bc = [int(s["good"].sum()) for s in host_scenes[:4]]
    a = run(ops, ml, mr, good, bc, moments=M, pair_off=off)
    b = run(ops, ml, mr, good, bc, moments=M, pair_off=off, swapped=True)
    P = pc.P_SWAP
    for p in range(4):
        assert np.array_equal(b["R"][p], P @ a["R"][p] @ P) and np.array_equal(b["t"][p], P @ a["t"][p])
        assert np.array_equal(b["E"][p], pc.sign_rule(P @ a["E"][p] @ P))
    for n_ in ("front_count", "front_counts", "choice", "front", "e_refit"):
        assert a[n_].tobytes() == b[n_].tobytes(), n_


# ---- 3. through the batch path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_verify_then_pose_through_batch_and_the_local_optimisation_round(ops, mixed):
    from pats_amd import batch
    pairs, n, thr = 4, 600, np.float32(2e-3)
    scenes = [pc.make_scene(seed, n, outliers=0.3) for seed in (21, 22, 23, 24)]          # the CALLER's order
    caller_of = [2, 0, 3, 1] if mixed else [0, 1, 2, 3]                                     # slot s holds the caller's pair caller_of[s]
    ml, mr, off, _ = pack([scenes[i] for i in caller_of])
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([off, [pairs * n, 0, 0]]).astype(np.int64)                    # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if mixed:
        out["caller_of"] = caller_of
    models = cu(np.stack([pc.true_model(s) for s in scenes]).reshape(pairs, 1, 3, 3))
    dthr = cu(np.full(pairs, thr, np.float32))
    ver = batch.verify_by_pair(out, cap, models, dthr, moments=True)
    res = batch.pose_by_pair(out, cap, front=True)
    assert out["pose"] is res and len(res) == 7 and tuple(res[6].shape) == (pairs * n,)
    E, R, t, front_count = (x.cpu().numpy() for x in res[:4])
    first_count = ver[2].cpu().numpy()
    for i, s in enumerate(scenes):
        slot = caller_of.index(i)
        assert pc.angle_R(R[i], s["R"]) < POSE_DEG and pc.angle_t(t[i], s["t"]) < POSE_DEG and float(t[i] @ s["t"]) > 0
        lo = slot * n
        hand = ops.epipolar_pose_by_pair(dl[lo:lo + n], dr[lo:lo + n], ver[3][lo:lo + n], ver[2][slot:slot + 1], moments=ver[4][slot:slot + 1],
                                         pair_off=cu(np.array([0, n], np.int64)))
        assert torch.equal(hand[0][0], res[0][i]) and torch.equal(hand[1][0], res[1][i]) and torch.equal(hand[2][0], res[2][i])
        assert int(hand[3][0]) == front_count[i] == int(res[6][lo:lo + n].sum()) and front_count[i] >= 0.9 * first_count[slot]
    split = batch.split_pose_by_pair(out, cap)
    assert len(split) == pairs and all(torch.equal(split[i][0], res[1][i]) and torch.equal(split[i][1], res[2][i]) and
                                       torch.equal(split[i][2], res[0][i]) and int(split[i][3]) == front_count[i] for i in range(pairs))
    # without moments the winning model is the source
    batch.verify_by_pair(out, cap, models, dthr)
    plain = batch.pose_by_pair(out, cap)
    assert len(plain) == 6
    for i, s in enumerate(scenes):
        assert pc.angle_R(plain[1][i].cpu().numpy(), s["R"]) < 1e-3 and torch.equal(plain[3][i].cpu(), plain[4][i].max().long().cpu())
    # the local-optimisation round: E as the one model of the next verification
    ver2 = batch.verify_by_pair(out, cap, res[0].float().reshape(pairs, 1, 3, 3), dthr, moments=True)
    again = batch.pose_by_pair(out, cap)
    second = ver2[2].cpu().numpy()
    print("inliers of the true model %s, of the refit %s" % (first_count.tolist(), second.tolist()))
    assert (second >= 0.9 * first_count).all() and bool(torch.isfinite(again[1]).all())
    for i, s in enumerate(scenes):
        assert pc.angle_R(again[1][i].cpu().numpy(), s["R"]) < POSE_DEG
    overflow = dict(out, summary=cu(np.concatenate([off, [pairs * n, 0, 1]]).astype(np.int64)))
    with pytest.raises(RuntimeError, match="Cmax"):
        batch.split_pose_by_pair(overflow, cap)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    import test_pose_host as th
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.zeros(4096, dtype=torch.float32, device="cuda")                        # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    th.A16 = base
    try:
        for kw, words in th.refusals(lib, base=base):
            th.refused(lib, kw, words)
    finally:
        th.A16 = 0x7f0000001000
    torch.cuda.synchronize()
    assert not live.any()                                                               # nothing ran: nothing was written
    ml = torch.zeros((20, 2), device="cuda")
    inl, bc = torch.zeros(20, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    mom, off = torch.zeros((2, 9, 9), dtype=torch.float64, device="cuda"), torch.tensor([0, 10, 20], device="cuda")
    for kw, word in (({"norm": torch.zeros((3, 8), device="cuda")}, "norm"), ({"moments": mom[:1]}, "moments must be"),
                     ({"out": (mom,)}, "out must be"), ({"inlier": inl[:5]}, "inlier must be")):
        args = dict(inlier=inl, moments=mom)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.epipolar_pose_by_pair(ml, ml, args.pop("inlier"), bc, pair_off=off, **args)
    with pytest.raises(RuntimeError, match="best_count must hold one int64 per pair"):
        ops.epipolar_pose_by_pair(ml, ml, inl, bc[:1], moments=mom, pair_off=off)
