"""GPU: ops.homography_pose_by_pair / ops.pose_select_by_pair and batch.pose_h_by_pair / select_pose_by_pair / pose_branch (the view
through which the consumers of a pose read either new result) against the definition of include/pats_amd.h restated in numpy float64 (tests/pose_h_cases.py):
    R, t, n, E, baseline, cand_*   within BOUND = 16 x the measured float64 constant of the restatement - what numpy's eigh route and an
                 independent SVD route differ by on the committed scenes, recomputed in this run (tests/test_pose_h_cases_host.py prints
                 and bounds it; docs/parity.md records it).  The device's candidates are the restatement's up to k -> k ^ m (the signs
                 of the eigenvectors): one candidate is matched, the rest follow
    vis, sup     between the restatement's sure count and its sure-plus-band count; choice where the band cannot change it; the mask
                 cell for cell outside the band; front.sum() == front_count == vis[choice] exactly
    select       exactly the restatement's branch, the chosen branch's values and mask bytes
Measured on an MI355X: the float64 constant 2.8e-13, the bound 4.5e-12, the device's worst difference 3.4e-13 from the moments and
1.2e-13 from a float32 model; 2 of 6392 visibility cells undecided.  docs/parity.md records them.
Every output lies inside a larger sentinel-filled buffer and every input list in a larger NaN-filled one."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import homography_cases as hmc
import pose_h_cases as ph

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0xAB
THR = np.float32(2e-3)
ORTHO = 1e-9            # |R^T R - I| of any written rotation: far above float64 rounding, far below any float32 step
NAMES = ("E", "R", "t", "front_count", "vis", "choice", "n", "baseline", "sup", "status", "cand_R", "cand_t", "cand_n", "front")


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bound():
    """MARGIN x the float64 constant, from the reference's own two routes - never from the kernel's output."""
    scenes, made = ph.comparison_scenes()
    assert len(scenes) >= (1 - ph.MAX_DROPPED) * made
    const = ph.float64_constant(scenes)
    print("float64 constant %.3e, bound %.3e" % (const, ph.MARGIN * const))
    return ph.MARGIN * const


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a, fill):
    """a as a view of a longer buffer whose rows beyond it hold `fill`."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.shape[0] + PAD,) + a.shape[1:], fill, dtype=cu(a[:0]).dtype, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


def run(ops, ml, mr, inl, bc, **kw):
    """One call on fresh sentinel buffers -> dict of numpy arrays (the surroundings checked; nothing written is a NaN, an infinity or
    a sentinel)."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs, cap = len(bc), ml.shape[0]
    f64, i32 = torch.float64, torch.int32
    shapes = [((pairs, 3, 3), f64, SENT_F), ((pairs, 3, 3), f64, SENT_F), ((pairs, 3), f64, SENT_F), ((pairs,), torch.int64, SENT_I),
              ((pairs, 4), i32, SENT_I), ((pairs,), i32, SENT_I), ((pairs, 3), f64, SENT_F), ((pairs,), f64, SENT_F),
              ((pairs, 4), i32, SENT_I), ((pairs,), i32, SENT_I), ((pairs, 2, 3, 3), f64, SENT_F), ((pairs, 2, 3), f64, SENT_F),
              ((pairs, 2, 3), f64, SENT_F), ((cap,), torch.uint8, SENT_B)]
    bufs, views = [], []
    for shape, dt, sent in shapes:
        b = torch.full((int(np.prod(shape)) + 2 * PAD,), sent, dtype=dt, device="cuda")
        bufs.append((b, sent))
        views.append(b[PAD:b.numel() - PAD].view(shape))
    got = ops.homography_pose_by_pair(guarded(ml, float("nan")), guarded(mr, float("nan")), guarded(np.asarray(inl).astype(np.uint8), 1),
                                      cu(np.asarray(bc, np.int64)), return_candidates=True, return_front=True, out=tuple(views), **d)
    torch.cuda.synchronize()
    assert len(got) == 14 and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    for b, sent in bufs:
        assert bool((torch.cat([b[:PAD], b[b.numel() - PAD:]]) == sent).all()), "bytes around an output view changed"
    out = {n: v.cpu().numpy() for n, v in zip(NAMES, views)}
    for n in ("E", "R", "t", "n", "baseline", "cand_R", "cand_t", "cand_n"):
        assert np.isfinite(out[n]).all() and not (out[n] == SENT_F).any(), n
    for n in ("front_count", "vis", "choice", "sup", "status"):
        assert not (out[n] == SENT_I).any(), n
    assert set(np.unique(out["front"]).tolist()) <= {0, 1}
    return out


def pack(scenes):
    """Scenes -> (ml, mr [cap,2], pair_off, segs)."""
    lens = [s["ml"].shape[0] for s in scenes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ml = np.concatenate([s["ml"] for s in scenes] + [np.zeros((0, 2), np.float32)]).reshape(-1, 2).astype(np.float32)
    mr = np.concatenate([s["mr"] for s in scenes] + [np.zeros((0, 2), np.float32)]).reshape(-1, 2).astype(np.float32)
    return ml, mr, off, [(int(off[i]), lens[i]) for i in range(len(lens))]


def is_no_pose(out, p):
    return (out["status"][p] == 0 and not out["E"][p].any() and np.array_equal(out["R"][p], np.eye(3)) and not out["t"][p].any()
            and not out["n"][p].any() and out["baseline"][p] == 0 and not out["vis"][p].any() and not out["sup"][p].any()
            and out["choice"][p] == 0 and out["front_count"][p] == 0 and np.array_equal(out["cand_R"][p], np.stack([np.eye(3)] * 2))
            and not out["cand_t"][p].any() and not out["cand_n"][p].any())


def consistent(out, p, front_seg, values=True):
    """What one call guarantees of pair p whatever the scene: the counts, the choice and the mask agree, the rotations are rotations.
    values=False (a G of rank 1, where lambda2 is a rounding of zero): only the integers."""
    st, ch = int(out["status"][p]), int(out["choice"][p])
    assert st in (0, 1, 2) and 0 <= ch < 4
    assert int(front_seg.sum()) == out["front_count"][p] == out["vis"][p][ch]
    if not values:
        return
    for R in (out["R"][p], out["cand_R"][p][0], out["cand_R"][p][1]):
        assert np.abs(R.T @ R - np.eye(3)).max() <= ORTHO and abs(np.linalg.det(R) - 1) <= ORTHO
    if st == 0:
        assert is_no_pose(out, p) and not front_seg.any()
    if st == 1:
        vis, sup = out["vis"][p], out["sup"][p]
        assert ch == max(range(4), key=lambda k: (vis[k], sup[k], -k)) and sup[0] == sup[2] and sup[1] == sup[3]
        assert abs(np.linalg.norm(out["t"][p]) - 1) <= ORTHO and abs(np.linalg.norm(out["n"][p]) - 1) <= ORTHO
        assert abs(np.linalg.norm(out["E"][p]) - 1) <= ORTHO and out["E"][p].reshape(-1)[int(np.argmax(np.abs(out["E"][p])))] > 0
        assert np.abs(np.linalg.norm(out["cand_t"][p], axis=1) - out["baseline"][p]).max() <= ORTHO
    if st == 2:
        assert not out["t"][p].any() and not out["n"][p].any() and not out["E"][p].any() and not out["sup"][p].any() and ch == 0
        assert (out["vis"][p] == out["vis"][p][0]).all()


def check_pair(out, p, ref, front_seg, bound, stats=None):
    """Pair p against the restatement `ref` (a comparison scene: its gap is at least GAP)."""
    consistent(out, p, front_seg)
    assert out["status"][p] == ref["status"]
    if ref["status"] == 0:
        return
    assert abs(out["baseline"][p] - ref["baseline"]) <= bound
    if ref["status"] == 2:
        assert np.abs(out["R"][p] - ref["R"]).max() <= bound and (out["vis"][p] == ref["used"]).all()
        assert np.array_equal(front_seg.astype(bool), ref["front"])
        return
    assert ref["sign_sure"]
    cands = ref["cands"]
    m = ph.match_xor(cands, out["cand_R"][p][0], out["cand_t"][p][0], out["cand_n"][p][0])
    assert m in (0, 1, 2, 3)
    worst = 0.0
    for c in range(2):
        R, t, n = cands[c ^ m]
        worst = max(worst, np.abs(out["cand_R"][p][c] - R).max(), np.abs(out["cand_t"][p][c] - t).max(), np.abs(out["cand_n"][p][c] - n).max())
    ch = int(out["choice"][p])
    R, t, n = cands[ch ^ m]
    worst = max(worst, np.abs(out["R"][p] - R).max(), np.abs(out["t"][p] - t / np.linalg.norm(t)).max(), np.abs(out["n"][p] - n).max(),
                np.abs(out["E"][p] - ph.essential(R, t)).max())
    if stats is not None:
        stats["worst"] = max(stats["worst"], float(worst))
    assert worst <= bound, (p, worst, bound)
    for k in range(4):
        j = k ^ m
        assert ref["vis_lo"][j] <= out["vis"][p][k] <= ref["vis_hi"][j], (p, k, ref["vis_lo"][j], out["vis"][p][k], ref["vis_hi"][j])
        assert ref["sup_lo"][j] <= out["sup"][p][k] <= ref["sup_hi"][j], (p, k, ref["sup_lo"][j], out["sup"][p][k], ref["sup_hi"][j])
    if ref["choice_sure"]:
        assert ch ^ m == ref["choice"]
    keep = ~ref["side_und"][ch ^ m]
    assert np.array_equal(front_seg.astype(bool)[keep], ref["side"][ch ^ m][keep])
    if stats is not None:
        stats["cells"] += ref["side_und"][:2].size
        stats["undecided"] += int(ref["side_und"][:2].sum())


# ---- 1. accuracy on the committed scenes ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_scenes():
    out, made = ph.comparison_scenes()
    assert len(out) >= (1 - ph.MAX_DROPPED) * made
    for s in out:
        s["xl"], s["xr"], s["used"], s["M"] = ph.plane_moments(s)
    return out


@pytest.mark.parametrize("source", ["moments", "models"])
def test_float64_outputs_and_float32_decisions_on_the_host_scenes(ops, host_scenes, bound, source):
    """Measured on an MI355X (bound = 16 x the float64 constant = 4.5e-12): worst difference 3.4e-13 (moments), 1.2e-13 (models)."""
    ml, mr, off, segs = pack(host_scenes)
    pairs = len(host_scenes)
    used = np.concatenate([s["used"] for s in host_scenes])
    bc = [int(s["used"].sum()) for s in host_scenes]
    thr = np.full(pairs, THR, np.float32)
    if source == "moments":
        src = {"moments": np.stack([s["M"] for s in host_scenes])}
    else:
        models = np.zeros((pairs, 3, 3, 3), np.float32)
        best = np.array([p % 3 for p in range(pairs)], np.int32)
        for p, s in enumerate(host_scenes):
            models[p, best[p]] = hmc.sign_rule(s["H"] / np.linalg.norm(s["H"])).astype(np.float32)
        src = {"models": models, "best": best}
    out = run(ops, ml, mr, used, bc, pair_off=off, thr=thr, **src)
    stats = {"worst": 0.0, "cells": 0, "undecided": 0}
    for p, (s, (lo, n)) in enumerate(zip(host_scenes, segs)):
        kw = {"M": s["M"]} if source == "moments" else {"model": src["models"][p, src["best"][p]]}
        ref = ph.restate(s["xl"], s["xr"], s["used"], thr=THR, **kw)
        check_pair(out, p, ref, out["front"][lo:lo + n], bound, stats)
        assert out["status"][p] == 1 and ph.angle_R(out["R"][p], s["R"]) < 1.0 and float(out["n"][p] @ s["n"]) > 0.99
    print("%s: worst difference %.3e (bound %.3e); undecided %d of %d visibility cells" % (source, stats["worst"], bound, stats["undecided"],
                                                                                      stats["cells"]))
    assert stats["undecided"] <= ph.BAND_CAP * stats["cells"]
    # without thr the support is 0 and the visibility stands alone
    blind = run(ops, ml, mr, used, bc, pair_off=off, **src)
    assert not blind["sup"].any() and np.array_equal(blind["vis"], out["vis"]) and blind["R"].shape == out["R"].shape
    for p, (lo, n) in enumerate(segs):
        consistent(blind, p, blind["front"][lo:lo + n])


def test_rotation_scenes_and_min_baseline(ops, bound):
    scenes = [ph.make_scene(*c, family="rotation") for c in ph.ROTATION_CASES] + [ph.make_scene(*c, family="small") for c in ph.SMALL_BASELINE_CASES]
    ml, mr, off, segs = pack(scenes)
    pts = [ph.plane_moments(s) for s in scenes]
    M = np.stack([q[3] for q in pts])
    used = np.concatenate([q[2] for q in pts])
    bc = [int(q[2].sum()) for q in pts]
    thr = np.full(len(scenes), THR, np.float32)
    for mb, want in ((5e-3, [2, 2, 1, 1]), (2e-2, [2, 2, 2, 2])):
        out = run(ops, ml, mr, used, bc, pair_off=off, moments=M, thr=thr, min_baseline=mb)
        assert out["status"].tolist() == want
        for p, (s, (lo, n)) in enumerate(zip(scenes, segs)):
            ref = ph.restate(pts[p][0], pts[p][1], pts[p][2], M=M[p], thr=THR, min_baseline=mb)
            if want[p] == 2:                             # the rotation: no square root of a gap, compared on every scene
                check_pair(out, p, ref, out["front"][lo:lo + n], bound)
                assert ph.angle_R(out["R"][p], s["R"]) < 0.1 + (1.0 if p >= 2 else 0.0) and out["front_count"][p] == bc[p]
                assert np.array_equal(out["cand_R"][p][0], out["R"][p]) and np.array_equal(out["cand_R"][p][1], out["R"][p])
            else:
                consistent(out, p, out["front"][lo:lo + n])
                assert abs(out["baseline"][p] - ref["baseline"]) <= bound


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------
NORM = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)
LENGTHS = [0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513]
PER_PAIR = ("E", "R", "t", "front_count", "vis", "choice", "n", "baseline", "sup", "status", "cand_R", "cand_t", "cand_n")


def edge_case(lengths, seed0, norm):
    scenes = [ph.make_scene(seed0 + i, max(n - n // 4, min(n, 4)), n - max(n - n // 4, min(n, 4))) for i, n in enumerate(lengths)]
    ml, mr, off, segs = pack(scenes)
    nm = None if not norm else np.tile(NORM, (len(lengths), 1)) + np.arange(len(lengths), dtype=np.float32)[:, None] * np.float32(0.01)
    pts = [ph.plane_moments(s, None if nm is None else nm[i]) for i, s in enumerate(scenes)]
    M = np.stack([q[3] for q in pts])
    used = np.concatenate([q[2] for q in pts] + [np.zeros(0, bool)])
    return scenes, ml, mr, off, segs, nm, M, used, [int(q[2].sum()) for q in pts]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("groups", [[[n] for n in LENGTHS], [[0, 3, 4, 5, 63], [64, 65, 255, 256, 257], [513, 0, 3, 257, 4]]],
                         ids=["pairs1", "pairs5"])
def test_segment_lengths_in_both_forms_and_pairs_below_four_inliers(ops, groups, norm):
    for lengths in groups:
        scenes, ml, mr, off, segs, nm, M, used, bc = edge_case(lengths, 700 + sum(lengths), norm)
        pairs = len(lengths)
        kw = {"thr": np.full(pairs, THR, np.float32)}
        if nm is not None:
            kw["norm"] = nm
        out = run(ops, ml, mr, used, bc, moments=M, pair_off=off, **kw)
        for p, (lo, n) in enumerate(segs):
            consistent(out, p, out["front"][lo:lo + n])
            assert (out["status"][p] == 0) == (bc[p] < ph.MIN_INLIERS), (lengths, p)
            if bc[p] < ph.MIN_INLIERS:
                assert is_no_pose(out, p)
            if pairs > 1 and n:                          # the neighbours disturb nothing: the pair on its own gives the same bits
                alone = run(ops, ml[lo:lo + n], mr[lo:lo + n], used[lo:lo + n], bc[p:p + 1], moments=M[p:p + 1],
                            pair_off=np.array([0, n], np.int64), **{k: v[p:p + 1] for k, v in kw.items()})
                for name in PER_PAIR:
                    assert alone[name][0].tobytes() == out[name][p].tobytes(), (lengths, p, name)
                assert np.array_equal(alone["front"], out["front"][lo:lo + n])
        # the strided form: the same segments in rows of `stride`, the slack filled with NaN rows marked as inliers
        stride = max(lengths) + 3
        sl, sr = np.full((pairs, stride, 2), np.nan, np.float32), np.full((pairs, stride, 2), np.nan, np.float32)
        si = np.ones((pairs, stride), bool)
        for p, (lo, n) in enumerate(segs):
            sl[p, :n], sr[p, :n], si[p, :n] = ml[lo:lo + n], mr[lo:lo + n], used[lo:lo + n]
        two = run(ops, sl.reshape(-1, 2), sr.reshape(-1, 2), si.reshape(-1), bc, moments=M, stride=stride,
                  counts=np.asarray(lengths, np.int64), **kw)
        for name in PER_PAIR:
            assert out[name].tobytes() == two[name].tobytes(), (lengths, name)
        f2 = two["front"].reshape(pairs, stride)
        for p, (lo, n) in enumerate(segs):
            assert np.array_equal(f2[p, :n], out["front"][lo:lo + n]) and not f2[p, n:].any()


def test_empty_arrays_and_clamped_offsets_and_counts(ops):
    scenes, ml, mr, off, segs, _, M, used, bc = edge_case([300, 200, 100], 77, False)
    empty = run(ops, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, bool), bc, moments=M,
                pair_off=np.zeros(4, np.int64), thr=np.full(3, THR, np.float32))
    assert empty["front"].size == 0 and not empty["vis"].any() and not empty["sup"].any() and not empty["front_count"].any()
    for p in range(3):                                   # a pose without a vote: its sign is the eigenvector's, its rotation a rotation
        consistent(empty, p, np.zeros(0, np.uint8))
        assert empty["status"][p] == 1 and empty["choice"][p] == 0
    none = run(ops, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, bool), [0, 3, 0], moments=M,
               pair_off=np.zeros(4, np.int64))
    assert all(is_no_pose(none, p) for p in range(3))
    bad_off = np.array([-5, 250, 2 ** 40, 100], np.int64)                    # clamped: [0,250), [250,600), empty
    out = run(ops, ml, mr, used, bc, moments=M, pair_off=bad_off)
    segs2 = ec.segments(3, 600, pair_off=bad_off)
    assert segs2 == [(0, 250), (250, 350), (600, 0)]
    assert not out["vis"][2].any() and not out["front"][600:].any()
    for p, (lo, n) in enumerate(segs2):
        consistent(out, p, out["front"][lo:lo + n])
    assert out["front_count"][0] == int(used[:250].sum())
    two = run(ops, ml, mr, used, bc, moments=M, stride=200, counts=np.array([-3, 2 ** 50, 150], np.int64))
    for p, (lo, n) in enumerate(ec.segments(3, 600, stride=200, counts=[-3, 2 ** 50, 150])):
        consistent(two, p, two["front"][lo:lo + n])
        assert not two["front"][lo + n:(p + 1) * 200].any()
    assert two["front_count"][0] == 0 and two["front_count"][1] == int(used[200:400].sum())


def test_degenerate_inputs_give_no_nan_and_disturb_no_other_pair(ops):
    lengths = [120] * 7
    scenes, ml, mr, off, segs, _, M, used, bc = edge_case(lengths, 900, False)
    thr = np.full(7, THR, np.float32)
    clean = run(ops, ml, mr, used, bc, moments=M, pair_off=off, thr=thr)
    assert (clean["status"] == 1).all()
    M2, thr2 = M.copy(), thr.copy()
    M2[0][4, 7] = np.nan                                                      # read through the upper triangle
    M2[1][0, 0] = np.inf
    r1 = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]).reshape(9)              # a rank-1 G as the null vector of the moments
    M2[2] = np.eye(9) - np.outer(r1, r1) / (r1 @ r1)
    g = np.diag([1.0, 1.0, 0.0]).reshape(9)                                   # lambda3 = 0
    M2[3] = np.eye(9) - np.outer(g, g) / (g @ g)
    thr2[4] = np.nan
    thr2[5] = -1.0
    out = run(ops, ml, mr, used, bc, moments=M2, pair_off=off, thr=thr2)      # run() asserts: nothing written is a NaN or an infinity
    assert is_no_pose(out, 0) and is_no_pose(out, 1) and out["status"][2] in (0, 1) and out["status"][3] in (0, 1)
    for p, (lo, n) in enumerate(segs):
        consistent(out, p, out["front"][lo:lo + n], values=p != 2)
    for p in (4, 5):                                                          # a NaN or negative thr: no support, everything else as before
        assert not out["sup"][p].any() and np.array_equal(out["vis"][p], clean["vis"][p])
        assert out["cand_R"][p].tobytes() == clean["cand_R"][p].tobytes()
    for name in PER_PAIR:
        assert out[name][6].tobytes() == clean[name][6].tobytes(), name
    assert np.array_equal(out["front"][segs[6][0]:], clean["front"][segs[6][0]:])
    zero = run(ops, ml, mr, used, bc, models=np.zeros((7, 1, 3, 3), np.float32), best=np.array([5, -2, 0, 0, 0, 0, 0], np.int32),
               pair_off=off, thr=thr)                                         # an all-zero model; best is clamped, never followed outside
    assert all(is_no_pose(zero, p) for p in range(7)) and not zero["front"].any()
    sing = run(ops, ml, mr, used, bc, moments=np.stack([M2[3]] * 7), pair_off=off, thr=thr, min_baseline=10.0)
    assert all(is_no_pose(sing, p) for p in range(7))                         # rotation only and lambda3 = 0


def test_swapped_is_an_exact_permutation(ops, host_scenes):
    ml, mr, off, segs = pack(host_scenes[:4])
    M = np.stack([s["M"] for s in host_scenes[:4]])
    used = np.concatenate([s["used"] for s in host_scenes[:4]])
    bc = [int(s["used"].sum()) for s in host_scenes[:4]]
    thr = np.full(4, THR, np.float32)
    a = run(ops, ml, mr, used, bc, moments=M, pair_off=off, thr=thr)
    b = run(ops, ml, mr, used, bc, moments=M, pair_off=off, thr=thr, swapped=True)
    for p in range(4):
        sw = ph.swap({k: a[k][p] for k in ("R", "t", "n", "E", "cand_R", "cand_t", "cand_n")})
        for k in ("R", "t", "n", "E", "cand_R", "cand_t", "cand_n"):
            assert np.array_equal(b[k][p], sw[k]), (p, k)
    for name in ("front_count", "vis", "choice", "sup", "status", "baseline", "front"):
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- 3. the E-or-H decision ---------------------------------------------------------------------------------------------------------
def test_select_matches_the_rule_and_hands_on_the_chosen_masks(ops):
    rng = np.random.default_rng(5)
    bce = [100, 100, 100, 7, 7, 0, 100, 100, 8, 10, 100, 2 ** 40]
    bch = [90, 79, 90, 5, 500, 0, 10 ** 6, 90, 4, 8, 81, 2 ** 40]
    sth = [1, 1, 2, 2, 0, 0, 1, 0, 1, 1, 1, 1]
    rat = [0.8, 0.8, 0.8, 0.8, 0.8, 0.8, float("nan"), 0.8, 0.5, 0.8, 0.8, 1.0]
    pairs = len(bce)
    lens = [(37 * p) % 90 for p in range(pairs)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cap = int(off[-1]) + 13                                                   # rows behind the last segment: 0 in both outputs
    f = lambda *shape: rng.normal(size=shape)                                 # noqa: E731
    pe = (f(pairs, 3, 3), f(pairs, 3, 3), f(pairs, 3), rng.integers(0, 99, pairs), rng.integers(0, 2, cap).astype(np.uint8))
    phh = (f(pairs, 3, 3), f(pairs, 3, 3), f(pairs, 3), rng.integers(0, 99, pairs), rng.integers(0, 2, cap).astype(np.uint8))
    ie, ih = rng.integers(0, 2, cap).astype(np.uint8), rng.integers(0, 2, cap).astype(np.uint8)
    args = (cu(np.asarray(bce, np.int64)), cu(ie), tuple(cu(x) for x in phh), cu(np.asarray(sth, np.int32)), cu(np.asarray(bch, np.int64)),
            cu(ih), cu(np.asarray(rat, np.float32)))
    got = ops.pose_select_by_pair(tuple(cu(x) for x in pe), *args, pair_off=cu(off))
    assert len(got) == 7
    E, R, t, fc, branch, isel, fsel = (g.cpu().numpy() for g in got)
    want = [ph.select(*q) for q in zip(bce, bch, sth, rat)]
    assert branch.tolist() == want and set(want) == {0, 1, 2, 3}
    wi, wf = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    for p, br in enumerate(want):
        src = None if br == 0 else (pe if br == 1 else phh)
        assert np.array_equal(E[p], src[0][p] if src else np.zeros((3, 3))) and np.array_equal(R[p], src[1][p] if src else np.eye(3))
        assert np.array_equal(t[p], src[2][p] if src else np.zeros(3)) and fc[p] == (src[3][p] if src else 0)
        if src:
            wi[off[p]:off[p + 1]] = (ie if br == 1 else ih)[off[p]:off[p + 1]]
            wf[off[p]:off[p + 1]] = src[4][off[p]:off[p + 1]]
    assert np.array_equal(isel, wi) and np.array_equal(fsel, wf)
    # the strided form and poses without a front
    stride = 90
    cnt = np.asarray(lens, np.int64)
    ie2, ih2 = rng.integers(0, 2, pairs * stride).astype(np.uint8), rng.integers(0, 2, pairs * stride).astype(np.uint8)
    got2 = ops.pose_select_by_pair(tuple(cu(x) for x in pe[:4]), args[0], cu(ie2), args[2][:4], args[3], args[4], cu(ih2), args[6],
                                   stride=stride, counts=cu(cnt))
    assert len(got2) == 6 and got2[4].cpu().tolist() == want
    s2 = got2[5].cpu().numpy().reshape(pairs, stride)
    for p, br in enumerate(want):
        src = np.zeros(stride, np.uint8) if br == 0 else (ie2 if br == 1 else ih2).reshape(pairs, stride)[p]
        assert np.array_equal(s2[p, :lens[p]], src[:lens[p]]) and not s2[p, lens[p]:].any()
    # cap == 0 defines every per-pair output
    got3 = ops.pose_select_by_pair(tuple(cu(x) for x in pe[:4]), args[0], cu(np.zeros(0, np.uint8)), args[2][:4], args[3], args[4],
                                   cu(np.zeros(0, np.uint8)), args[6], pair_off=cu(np.zeros(pairs + 1, np.int64)))
    assert got3[4].cpu().tolist() == want and got3[5].numel() == 0 and torch.equal(got3[1], got[1])


# ---- 4. through the batch path ------------------------------------------------------------------------------------------------
def _essential32(s):
    if not s["t"].any():
        return np.zeros((3, 3), np.float32)
    return ph.essential(s["R"], s["t"]).astype(np.float32)


@pytest.mark.parametrize("mixed", [False, True])
def test_both_branches_through_batch_and_the_consumers_on_a_branch_view(ops, bound, mixed):
    from pats_amd import batch
    pairs, n = 4, 400
    # the CALLER's order: planar with few matches off the plane, planar with many, rotation only, planar with few
    scenes = [ph.make_scene(41, 340, 40, 20), ph.make_scene(42, 200, 170, 30), ph.make_scene(43, 360, 0, 40, family="rotation"),
              ph.make_scene(44, 330, 50, 20)]
    assert all(s["ml"].shape[0] == n for s in scenes) and all(ph.gap_of(scenes[i]["H"]) >= ph.GAP for i in (0, 1, 3))
    caller_of = [2, 0, 3, 1] if mixed else [0, 1, 2, 3]                       # slot s holds the caller's pair caller_of[s]
    ml, mr, off, _ = pack([scenes[i] for i in caller_of])
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([off, [pairs * n, 0, 0]]).astype(np.int64)       # offsets, M, P, status
    models_e = cu(np.stack([_essential32(s) for s in scenes]).reshape(pairs, 1, 3, 3))
    models_h = cu(np.stack([hmc.sign_rule(s["H"] / np.linalg.norm(s["H"])).astype(np.float32) for s in scenes]).reshape(pairs, 1, 3, 3))
    dthr = cu(np.full(pairs, THR, np.float32))
    T1 = np.tile(np.eye(4), (pairs, 1, 1))
    for i, s in enumerate(scenes):
        T1[i, :3, :3], T1[i, :3, 3] = s["R"], s["t"]
    dT1 = cu(T1)

    def fresh():
        dl, dr, ds = cu(ml), cu(mr), cu(summary)
        o = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
        if mixed:
            o["caller_of"] = caller_of
        return o

    def default_path(o):
        batch.verify_by_pair(o, cap, models_e, dthr, moments=True)
        batch.pose_by_pair(o, cap, front=True)
        batch.triangulate_by_pair(o, cap)
        batch.pose_error_by_pair(o, cap, dT1)
        return batch.split_pose_by_pair(o, cap)

    plain = fresh()
    split_plain = default_path(plain)
    out = fresh()
    batch.verify_by_pair(out, cap, models_e, dthr, moments=True)
    batch.pose_by_pair(out, cap, front=True)
    with pytest.raises(ValueError, match="run verify_h_by_pair first"):
        batch.pose_h_by_pair(out, cap)
    with pytest.raises(ValueError, match="pose_h_by_pair first"):
        batch.pose_branch(out, "planar")
    ver_h = batch.verify_h_by_pair(out, cap, models_h, dthr, moments=True)
    res = batch.pose_h_by_pair(out, cap, thr=dthr, front=True, candidates=True, min_baseline=5e-3)
    assert out["pose_h"] is res and len(res) == 7 and len(out["pose_h_extra"]) == 7 and tuple(res[6].shape) == (pairs * n,)
    with pytest.raises(ValueError, match="select_pose_by_pair first"):
        batch.pose_branch(out, "selected")
    with pytest.raises(ValueError, match="branch must be"):
        batch.pose_branch(out, "affine")
    sel = batch.select_pose_by_pair(out, cap, ratio=0.8)
    assert out["pose_selected"] is sel and len(sel) == 7
    branch, inlier_sel = out["pose_selected_extra"]
    assert branch.cpu().tolist() == [2, 1, 3, 2]                              # the caller's order
    bad = dict(out, verified_h_on="topk")
    with pytest.raises(ValueError, match="verified_on"):
        batch.select_pose_by_pair(bad, cap)
    # the planar pose against the restatement, in the caller's order, and by hand on the pair's own slice
    n_, base, sup, status = (x.cpu().numpy() for x in out["pose_h_extra"][:4])
    assert status.tolist() == [1, 1, 2, 1]
    E, R, t, front_count, vis, choice = (x.cpu().numpy() for x in res[:6])
    inl_h, bc_h, mom_h = ver_h[3].cpu().numpy().astype(bool), ver_h[2].cpu().numpy(), ver_h[4].cpu().numpy()
    views = {b: batch.pose_branch(out, b) for b in ("planar", "selected")}
    err = {b: [x.cpu().numpy() for x in batch.pose_error_by_pair(views[b], cap, dT1)] for b in ("planar", "selected")}
    assert "pose_error" not in out and all("pose_error" in v for v in views.values())
    for i, s in enumerate(scenes):
        slot, lo = caller_of.index(i), caller_of.index(i) * n
        xl, xr = ec.points32(s["ml"], s["mr"])
        ref = ph.restate(xl, xr, inl_h[lo:lo + n], M=mom_h[slot], best_count=bc_h[slot], thr=THR, min_baseline=5e-3)
        one = {"E": E, "R": R, "t": t, "front_count": front_count, "vis": vis, "choice": choice, "n": n_, "baseline": base, "sup": sup,
               "status": status, "cand_R": out["pose_h_extra"][4].cpu().numpy(), "cand_t": out["pose_h_extra"][5].cpu().numpy(),
               "cand_n": out["pose_h_extra"][6].cpu().numpy()}
        check_pair(one, i, ref, res[6][lo:lo + n].cpu().numpy(), bound)
        if ref["status"] == 1:                 # the error against the ground truth: the restatement's, moved by at most the bound
            assert ref["choice_sure"]          # through acos - nine (three) products in the cosine, each off by at most the bound
            aR, at = np.deg2rad(ph.angle_R(ref["R"], s["R"])), np.deg2rad(ph.angle_t(ref["t"], s["t"]))
            assert abs(err["planar"][0][i] - np.rad2deg(aR)) <= np.rad2deg(5 * bound / np.sin(aR))
            assert abs(err["planar"][1][i] - np.rad2deg(at)) <= np.rad2deg(5 * bound / np.sin(at))
            assert err["planar"][3][i] == 0 and err["planar"][2][i] < 5.0
        else:
            assert err["planar"][3][i] == 2                                   # t = 0: not scored
        src = out["pose"] if branch[i] == 1 else res                          # the selected pose is the chosen branch's, bit for bit
        for k in range(6):
            assert torch.equal(sel[k][i], src[k][i]), (i, k)
        chosen_inl, chosen_front = (out["verified"][3], out["pose"][6]) if branch[i] == 1 else (ver_h[3], res[6])
        assert torch.equal(inlier_sel[lo:lo + n], chosen_inl[lo:lo + n]) and torch.equal(sel[6][lo:lo + n], chosen_front[lo:lo + n])
        want = plain["pose_error"] if branch[i] == 1 else views["planar"]["pose_error"]
        assert all(torch.equal(views["selected"]["pose_error"][k][i], want[k][i]) for k in range(4))
    # triangulation under either new branch, with either mask
    for b in ("planar", "selected"):
        for mask in ("front", "inlier"):
            pts = batch.triangulate_by_pair(views[b], cap, mask=mask, depths=True)
            assert views[b]["points"] is pts and "points" not in out
            assert bool(torch.isfinite(pts[0]).all()) and bool(torch.isfinite(pts[3]).all())
            X, valid, tri_count = pts[0].cpu().numpy(), pts[1].cpu().numpy(), pts[2].cpu().numpy()
            for i, s in enumerate(scenes):
                lo = caller_of.index(i) * n
                assert int(valid[lo:lo + n].sum()) == tri_count[i]
                if i == 2:                               # rotation only, t = 0: the header's "no pose" of the triangulation - nothing valid,
                    assert not valid[lo:lo + n].any() and tri_count[i] == 0 and not X[lo:lo + n].any()      # every row exact zeros
                else:
                    assert tri_count[i] >= 0.9 * int(sel[3][i] if b == "selected" else front_count[i]) * (0.9 if mask == "front" else 0.5)
    planar_split = batch.split_pose_by_pair(views["planar"], cap)
    assert all(torch.equal(planar_split[i][0], res[1][i]) and torch.equal(planar_split[i][2], res[0][i]) for i in range(pairs))
    sel_split = batch.split_pose_by_pair(views["selected"], cap)
    assert all(torch.equal(sel_split[i][1], sel[2][i]) and int(sel_split[i][3]) == int(sel[3][i]) for i in range(pairs))
    pts_split = batch.split_points_by_pair(views["selected"], cap)                # the caller's order, the chosen branch's inliers
    ver_split = batch.split_verified_by_pair(views["selected"], cap)
    for i in range(pairs):
        lo = caller_of.index(i) * n
        assert torch.equal(pts_split[i][1], views["selected"]["points"][1][lo:lo + n].bool())
        assert torch.equal(ver_split[i][2], inlier_sel[lo:lo + n].bool())
        assert int(ver_split[i][4]) == int((bc_h if branch[i] >= 2 else out["verified"][2].cpu().numpy())[caller_of.index(i)])
    # the default branch: the same bits as a run without any of the new calls
    batch.triangulate_by_pair(out, cap)
    batch.pose_error_by_pair(out, cap, dT1)
    split_out = batch.split_pose_by_pair(out, cap)
    for key in ("verified", "pose", "points", "pose_error"):
        assert len(out[key]) == len(plain[key]) and all(torch.equal(a, b) for a, b in zip(out[key], plain[key])), key
    assert all(torch.equal(a, b) for x, y in zip(split_out, split_plain) for a, b in zip(x, y))
    assert all(torch.equal(a, b) for a, b in zip(out["verified_h"], ver_h))
    # the planar branch on its own: no pose_by_pair, no verify_by_pair
    alone = fresh()
    batch.verify_h_by_pair(alone, cap, models_h, dthr, moments=True)
    res_alone = batch.pose_h_by_pair(alone, cap, thr=dthr, front=True, candidates=True, min_baseline=5e-3)
    assert all(torch.equal(a, b) for a, b in zip(res_alone, res))
    view_alone = batch.pose_branch(alone, "planar")
    pts_alone = batch.triangulate_by_pair(view_alone, cap)
    assert all(torch.equal(a, b) for a, b in zip(pts_alone, batch.triangulate_by_pair(batch.pose_branch(out, "planar"), cap)))
    assert all(torch.equal(a, b) for a, b in zip(batch.pose_error_by_pair(view_alone, cap, dT1), views["planar"]["pose_error"]))
    assert all(torch.equal(a[0], b[0]) for a, b in zip(batch.split_pose_by_pair(view_alone, cap), planar_split))
    assert "pose" not in alone and "points" not in alone and "verified" not in alone
    with pytest.raises(ValueError, match="run pose_by_pair first"):
        batch.triangulate_by_pair(alone, cap)
    # a ratio tensor in the caller's order; without moments the winning model is the source
    sel2 = batch.select_pose_by_pair(out, cap, ratio=cu(np.array([2.0, 0.1, 0.8, float("nan")], np.float32)))
    assert out["pose_selected_extra"][0].cpu().tolist() == [1, 2, 3, 1] and len(sel2) == 7
    batch.verify_h_by_pair(out, cap, models_h, dthr)
    plain_h = batch.pose_h_by_pair(out, cap)
    st = out["pose_h_extra"][3].cpu().tolist()
    assert len(plain_h) == 6 and len(out["pose_h_extra"]) == 4 and [st[0], st[1], st[3]] == [1, 1, 1] and st[2] in (1, 2)
    assert not out["pose_h_extra"][2].any()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.zeros(4096, dtype=torch.float32, device="cuda")             # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    for which in sorted(ph.ENTRY):
        assert ph.check_refusals(lib, which, base) > 60
    torch.cuda.synchronize()
    assert not live.any()                                                     # nothing ran: nothing was written
    ml = torch.zeros((20, 2), device="cuda")
    inl, bc = torch.zeros(20, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    mom, off = torch.zeros((2, 9, 9), dtype=torch.float64, device="cuda"), torch.tensor([0, 10, 20], device="cuda")
    for kw, word in (({"norm": torch.zeros((3, 8), device="cuda")}, "norm"), ({"moments": mom[:1]}, "moments must be"),
                     ({"out": (mom,)}, "out must be"), ({"inlier": inl[:5]}, "inlier must be"),
                     ({"thr": torch.zeros(3, device="cuda")}, "thr must hold"), ({"min_baseline": -1.0}, "min_baseline")):
        args = dict(inlier=inl, moments=mom)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.homography_pose_by_pair(ml, ml, args.pop("inlier"), bc, pair_off=off, **args)
    with pytest.raises(RuntimeError, match="best_count must hold one int64 per pair"):
        ops.homography_pose_by_pair(ml, ml, inl, bc[:1], moments=mom, pair_off=off)
    f64 = dict(dtype=torch.float64, device="cuda")
    pose = (torch.zeros(2, 3, 3, **f64), torch.zeros(2, 3, 3, **f64), torch.zeros(2, 3, **f64), bc)
    st, ratio = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="t_h must be"):
        ops.pose_select_by_pair(pose, bc, inl, pose[:2] + (pose[2][:1],) + pose[3:], st, bc, inl, ratio, pair_off=off)
    with pytest.raises(RuntimeError, match="ratio must hold one value per pair"):
        ops.pose_select_by_pair(pose, bc, inl, pose, st, bc, inl, ratio[:1], pair_off=off)
    with pytest.raises(RuntimeError, match="inlier_e and inlier_h"):
        ops.pose_select_by_pair(pose, bc, inl, pose, st, bc, inl[:5], ratio, pair_off=off)
