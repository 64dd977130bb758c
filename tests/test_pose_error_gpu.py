"""GPU: ops.pose_error_by_pair / ops.pose_auc / batch.pose_error_by_pair against the definitions of include/pats_amd.h restated in
numpy float64 (tests/pose_error_cases.py) and against the reference's recorded outputs (tests/golden/pose_metrics.npz):
    status       equal to the restatement's; +inf exactly where the restatement has it; no NaN anywhere
    angles       finite errors within the angle's conditioning - the cosine moved by 4 * 2^-53 * sum|terms| (with contraction off
                 and the header's order the cosines match bit for bit and only acos differs: 4 ulps by OpenCL's bound), the spread
                 of acos over that interval, plus 8 ulps of the result
    auc          `below` and `sorted` exact, auc within n 2^-50 relative, the same bits in two calls
Every output lies inside a larger sentinel-filled buffer whose surroundings must not change; every float input in a NaN-padded one."""
import os
import re

import numpy as np
import pytest
import torch

import pose_cases as pc
import pose_error_cases as pe
import triangulate_cases as tc
from conftest import REPO, golden

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I = -777.25, -123456
MOVES_DEVICE = 16 // 4                                  # 4: the cosines are the restatement's; acos within 4 ulps
STATS = {"ulps": 0.0, "pairs": 0}


def _kernel_constant(name):
    src = open(os.path.join(REPO, "pats_amd", "csrc", "pose_error.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


T = _kernel_constant("PERR_THREADS")                   # pairs per workgroup: one thread each


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def gold():
    return golden("pose_metrics.npz")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a):
    """a float array as a view of a longer buffer whose rows beyond it hold NaN."""
    a = np.ascontiguousarray(a, np.float64)
    buf = torch.full((a.shape[0] + PAD,) + a.shape[1:], float("nan"), dtype=torch.float64, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


def sentinel_views(specs):
    """[(length, dtype, sentinel)] -> (buffers, views): every view PAD elements inside its own sentinel-filled buffer."""
    bufs, views = [], []
    for length, dt, sent in specs:
        b = torch.full((length + 2 * PAD,), sent, dtype=dt, device="cuda")
        bufs.append((b, sent, length))
        views.append(b[PAD:PAD + length])
    return bufs, views


def surroundings_unchanged(bufs):
    for b, sent, length in bufs:
        assert bool((torch.cat([b[:PAD], b[PAD + length:]]) == sent).all()), "bytes around an output view changed"


NAMES = ("err_R", "err_t", "err", "status")


def run_error(ops, R, t, T1, T0=None, counts=None, **kw):
    """One call on fresh sentinel buffers -> dict of numpy arrays (the surroundings and the absence of NaN checked)."""
    pairs = len(R)
    bufs, views = sentinel_views([(pairs, torch.float64, SENT_F)] * 3 + [(pairs, torch.int32, SENT_I)])
    got = ops.pose_error_by_pair(guarded(R), guarded(t), guarded(T1), T0=None if T0 is None else guarded(T0),
                                 counts=None if counts is None else cu(np.asarray(counts, np.int64)), out=tuple(views), **kw)
    torch.cuda.synchronize()
    assert len(got) == 4 and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    surroundings_unchanged(bufs)
    out = {n: v.cpu().numpy() for n, v in zip(NAMES, views)}
    for n in NAMES[:3]:
        assert not np.isnan(out[n]).any() and not (out[n] == SENT_F).any() and (out[n] >= 0).all(), n
    assert set(np.unique(out["status"]).tolist()) <= {0, 1, 2, 3}
    return out


def check_error(out, ref):
    """Everything the definition says: ref = pose_error_cases.pose_error64's dict for the same inputs."""
    assert np.array_equal(out["status"], ref["status"])
    bound = {}
    for k, c, a in (("err_R", "cos_R", "abs_R"), ("err_t", "cos_t", "abs_t")):
        assert np.array_equal(np.isinf(out[k]), np.isinf(ref[k])), k
        fin = np.isfinite(ref[k])
        exact = fin & np.isnan(ref[c])                  # evaluated without a cosine: err_t = 0 by min_gt_t
        assert np.array_equal(out[k][exact], ref[k][exact]), k
        with np.errstate(invalid="ignore"):
            bound[k] = np.where(fin & ~exact, pe.angle_bound(ref[c], ref[a], ref[k], MOVES_DEVICE), 0.0)
        assert (np.abs(out[k][fin] - ref[k][fin]) <= bound[k][fin]).all(), (k, int(np.argmax(np.abs(out[k] - ref[k]) * fin)))
        STATS["ulps"] = max(STATS["ulps"], float(pe.ulps(out[k][fin], ref[k][fin]).max()) if fin.any() else 0.0)
    assert np.array_equal(np.isinf(out["err"]), np.isinf(ref["err"]))
    fin = np.isfinite(ref["err"])
    assert (np.abs(out["err"][fin] - ref["err"][fin]) <= np.maximum(bound["err_R"], bound["err_t"])[fin]).all()
    assert np.array_equal(out["err"], np.maximum(out["err_R"], out["err_t"]))
    assert np.isinf(out["err"][out["status"] != 0]).all() and np.isinf(out["err_R"][out["status"] != 0]).all()
    STATS["pairs"] += len(out["status"])


# ---- 1. values ------------------------------------------------------------------------------------------------------------------
def test_errors_on_the_golden_and_on_seeded_sets(ops, gold):
    R, t, Rg, tg = gold["pose_R"], gold["pose_t"], gold["pose_R_gt"], gold["pose_t_gt"]
    T1 = pe.as_T(Rg, tg)
    out = run_error(ops, R, t, T1)
    check_error(out, pe.pose_error64(R, t, T1))
    # against the reference's own recorded angles: the host file's bound (16 moves) plus the device's (4)
    ref = pe.pose_error64(R, t, T1)
    for k, c, a in (("err_R", "cos_R", "abs_R"), ("err_t", "cos_t", "abs_t")):
        assert (np.abs(out[k] - gold["pose_" + k]) <= pe.angle_bound(ref[c], ref[a], ref[k], 16 + MOVES_DEVICE)).all(), k
    out = run_error(ops, R, t, gold["pose_T1"], T0=gold["pose_T0"])
    check_error(out, pe.pose_error64(R, t, gold["pose_T1"], gold["pose_T0"]))
    for seed, n in ((71, 200), (72, 77)):
        R, t, Rg, tg = pe.pose_sets(seed, n)
        T0, T1 = pe.extrinsic_sets(seed + 100, Rg, tg)
        counts = np.random.default_rng(seed).integers(0, 40, n)
        check_error(run_error(ops, R, t, pe.as_T(Rg, tg), counts=counts), pe.pose_error64(R, t, pe.as_T(Rg, tg), counts=counts))
        check_error(run_error(ops, R, t, T1, T0=T0), pe.pose_error64(R, t, T1, T0))
    again = run_error(ops, R, t, T1, T0=T0)
    first = run_error(ops, R, t, T1, T0=T0)
    for n_ in NAMES:
        assert again[n_].tobytes() == first[n_].tobytes(), n_
    print("largest difference to the restatement over %d pairs: %.1f ulps" % (STATS["pairs"], STATS["ulps"]))


# ---- 2. the pair-to-thread mapping --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [1, T - 1, T, T + 1, 2 * T + 1])
def test_pair_counts_around_the_workgroup(ops, pairs):
    R, t, Rg, tg = pe.pose_sets(900 + pairs, pairs)
    T0, T1 = pe.extrinsic_sets(800 + pairs, Rg, tg)
    counts = np.arange(pairs) % 31
    check_error(run_error(ops, R, t, T1, T0=T0, counts=counts), pe.pose_error64(R, t, T1, T0, counts=counts))
    check_error(run_error(ops, R, t, pe.as_T(Rg, tg)), pe.pose_error64(R, t, pe.as_T(Rg, tg)))


# ---- 3. every status ------------------------------------------------------------------------------------------------------------
def test_every_status_and_their_precedence(ops):
    n = 24
    R, t, Rg, tg = pe.pose_sets(33, n)
    T0, T1 = pe.extrinsic_sets(34, Rg, tg)
    counts = np.array([14, 15] * (n // 2))
    out = run_error(ops, R, t, T1, T0=T0, counts=counts)
    check_error(out, pe.pose_error64(R, t, T1, T0, counts=counts))
    assert out["status"].tolist() == [1, 0] * (n // 2)
    out = run_error(ops, R, t, T1, T0=T0, counts=counts, min_matches=14)
    assert not out["status"].any()
    out = run_error(ops, R, t, T1, T0=T0)                                 # counts = None: nothing is too short
    check_error(out, pe.pose_error64(R, t, T1, T0))
    assert not out["status"].any() and np.isfinite(out["err"]).all()
    # one bad entry at a time: a NaN and an infinity in R, t, T1 and T0; the row of T that is not read does not count
    R2, t2, A, B = R.copy(), t.copy(), T1.copy(), T0.copy()
    R2[0], t2[0] = np.eye(3), 0.0                                         # pose_by_pair's "no pose"
    R2[1, 2, 1], R2[2, 0, 0], t2[3, 1], t2[4, 2] = np.nan, np.inf, np.nan, -np.inf
    A[5, 1, 3], A[6, 0, 0], B[7, 2, 2], B[8, 0, 3] = np.nan, np.inf, np.nan, -np.inf
    A[9, 3, 1], B[10, 3, 3] = np.nan, np.inf                               # not read
    want = [2, 2, 2, 2, 2, 3, 3, 3, 3, 0, 0] + [0] * (n - 11)
    out = run_error(ops, R2, t2, A, T0=B)
    check_error(out, pe.pose_error64(R2, t2, A, B))
    assert out["status"].tolist() == want
    # two apply: the lowest number wins
    A[0, 0, 0], A[1, 0, 0], counts2 = np.nan, np.nan, np.full(n, 20)
    counts2[[0, 5, 11]] = 3
    out = run_error(ops, R2, t2, A, T0=B, counts=counts2)
    check_error(out, pe.pose_error64(R2, t2, A, B, counts=counts2))
    want2 = list(want)
    want2[0], want2[5], want2[11] = 1, 1, 1
    assert out["status"].tolist() == want2 and out["status"][1] == 2
    # T0 = None reads T1 alone: a bad T0-like entry cannot matter, a bad T1 does
    out = run_error(ops, R, t, A)
    assert out["status"].tolist() == [3, 3, 0, 0, 0, 3, 3] + [0] * (n - 7)
    # an overflow inside an evaluated pair: +inf, not a NaN
    out = run_error(ops, R * 1e200, t, pe.as_T(Rg * 1e200, tg))
    ref = pe.pose_error64(R * 1e200, t, pe.as_T(Rg * 1e200, tg))
    assert not out["status"].any() and np.array_equal(np.isinf(out["err_R"]), np.isinf(ref["err_R"])) and np.isinf(out["err_R"]).any()


def test_a_ground_truth_translation_without_a_direction(ops):
    n = 12
    R, t, Rg, tg = pe.pose_sets(44, n)
    tg[0] = 0.0
    tg[1], tg[2] = [3e-4, 0.0, 4e-4], [0.0, -3e-4, 4e-4]                   # |t_gt| = 5e-4 up to rounding
    T1 = pe.as_T(Rg, tg)
    out = run_error(ops, R, t, T1)                                        # min_gt_t = 0: only t_gt = 0 is caught
    check_error(out, pe.pose_error64(R, t, T1))
    assert out["err_t"][0] == 0.0 and out["status"][0] == 0 and out["err"][0] == out["err_R"][0] and (out["err_t"][1:3] > 0).all()
    for lim, hit in ((6e-4, True), (4e-4, False)):
        out = run_error(ops, R, t, T1, min_gt_t=lim)
        check_error(out, pe.pose_error64(R, t, T1, min_gt_t=lim))
        assert (out["err_t"][:3] == 0.0).tolist() == [True, hit, hit]


def test_t0_given_is_the_relative_pose_precomputed(ops):
    R, t, Rg, tg = pe.pose_sets(55, 100)
    T0, T1 = pe.extrinsic_sets(56, Rg, tg)
    rel = [pe.ground_truth64(T1[p], T0[p]) for p in range(len(R))]
    pre = pe.as_T(np.stack([g[0] for g in rel]), np.stack([g[1] for g in rel]))
    a, b = run_error(ops, R, t, T1, T0=T0), run_error(ops, R, t, pre)
    check_error(a, pe.pose_error64(R, t, T1, T0))
    check_error(b, pe.pose_error64(R, t, pre))
    same = sum(a[k].tobytes() == b[k].tobytes() for k in NAMES)
    print("%d of 4 outputs bit-identical between T0 given and the precomputed relative pose" % same)
    assert np.array_equal(a["status"], b["status"])
    ref = pe.pose_error64(R, t, pre)
    for k, c, a_ in (("err_R", "cos_R", "abs_R"), ("err_t", "cos_t", "abs_t")):
        assert (np.abs(a[k] - b[k]) <= pe.angle_bound(ref[c], ref[a_], ref[k], MOVES_DEVICE)).all(), k
    # and against numpy's general inverse: the reference's route, rounding only
    num = T1 @ np.linalg.inv(T0)
    c = run_error(ops, R, t, num)
    for k, cc, a_ in (("err_R", "cos_R", "abs_R"), ("err_t", "cos_t", "abs_t")):
        assert (np.abs(a[k] - c[k]) <= pe.angle_bound(ref[cc], ref[a_], ref[k], 16 + MOVES_DEVICE)).all(), k


# ---- 4. the AUC -----------------------------------------------------------------------------------------------------------------
def run_auc(ops, errors, thresholds=pe.THRESHOLDS):
    errors = np.asarray(errors, np.float64)
    n, n_thr = errors.size, len(thresholds)
    bufs, views = sentinel_views([(n_thr, torch.float64, SENT_F), (n_thr, torch.int64, SENT_I), (n, torch.float64, SENT_F)])
    src = guarded(errors)
    got = ops.pose_auc(src, thresholds=thresholds, return_sorted=True, out=tuple(views))
    torch.cuda.synchronize()
    assert len(got) == 3 and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    surroundings_unchanged(bufs)
    auc, below, srt = (v.cpu().numpy() for v in views)
    assert src.cpu().numpy().tobytes() == errors.tobytes()                 # the input is not sorted in place
    assert not np.isnan(auc).any() and not np.isnan(srt).any() and not (auc == SENT_F).any() and not (below == SENT_I).any()
    lean = ops.pose_auc(src, thresholds=thresholds)
    assert len(lean) == 2 and lean[0].cpu().numpy().tobytes() == auc.tobytes() and lean[1].cpu().numpy().tobytes() == below.tobytes()
    return auc, below, srt


def check_auc(ops, errors, thresholds=pe.THRESHOLDS):
    errors = np.asarray(errors, np.float64)
    auc, below, srt = run_auc(ops, errors, thresholds)
    want, want_below, want_sorted = pe.auc64(errors, thresholds)
    assert np.array_equal(below, want_below), (errors.size, below, want_below)
    assert srt.tobytes() == want_sorted.tobytes(), errors.size
    assert (np.abs(auc - want) <= pe.auc_bound(errors.size, want)).all(), (errors.size, auc, want)
    assert ((auc >= 0) & (auc <= 1 + 2.0 ** -50)).all()
    return auc, below


# 4096 / 4097 and 8191 / 8192: the sort width S = 8192, where static + dynamic LDS first passes the 64 KiB a launch gets unasked
AUC_N = [0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4000, 4096, 4097, 8191, 8192, 16383, 16384]


@pytest.mark.parametrize("n", AUC_N)
def test_auc_sizes_around_the_waves_the_workgroup_and_the_capacity(ops, n):
    rng = np.random.default_rng(1000 + n)
    errors = np.maximum(rng.gamma(1.2, 6.0, n), rng.gamma(1.0, 8.0, n))
    auc, below = check_auc(ops, errors)
    if n >= 63:
        assert 0 < below[0] < below[1] < below[2] < n and 0 < auc[0] < auc[1] < auc[2] < 1
    lost = errors.copy()
    lost[rng.random(n) < 0.2] = np.inf
    lost[rng.random(n) < 0.05] = np.nan                                   # a NaN counts as +inf
    check_auc(ops, lost)
    a, b = run_auc(ops, lost), run_auc(ops, lost)                          # two calls: the same bits
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    if n:
        auc, below = check_auc(ops, np.full(n, np.inf))                   # nothing was scored
        assert not auc.any() and not below.any()
        auc, below = check_auc(ops, np.full(n, np.nan))
        assert not auc.any() and not below.any()


def test_auc_on_the_references_lists(ops, gold):
    for name in pe.error_lists(0):
        errors = np.maximum(gold["auc_%s_err_R" % name], gold["auc_%s_err_t" % name])
        auc, below = check_auc(ops, errors)
        want = gold["auc_%s_ref" % name]
        assert np.array_equal(below, gold["auc_%s_below" % name]), name
        assert (np.abs(auc - want) <= pe.auc_bound(errors.size, want)).all(), (name, auc, want)


def test_auc_ties_thresholds_and_their_number(ops):
    rng = np.random.default_rng(7)
    errors = np.round(rng.gamma(1.5, 5.0, 700) * 4) / 4                  # quarters: many ties, at the thresholds too
    errors[:9] = [5, 5, 10, 10, 10, 20, 20, 20, 20]
    auc, below = check_auc(ops, errors)
    assert below.tolist() == [int((errors < v).sum()) for v in pe.THRESHOLDS] and (errors == 5).sum() >= 2
    check_auc(ops, errors, thresholds=(7.25,))                            # one threshold
    eight = (0.25, 1.0, 2.5, 5.0, 7.25, 10.0, 20.0, 1e6)
    auc8, below8 = check_auc(ops, errors, thresholds=eight)               # and eight
    assert auc8[3] == auc[0] and auc8[5] == auc[1] and auc8[6] == auc[2] and below8[-1] == errors.size
    lost = errors.copy() + 1.0
    lost[::5] = np.inf
    low, high = 0.5, 1e9                                                   # below every error; above every finite one
    auc, below = check_auc(ops, lost, thresholds=(low, high))
    assert auc[0] == 0.0 and below.tolist() == [0, int(np.isfinite(lost).sum())] and 0.79 < auc[1] < 0.81
    auc, below = check_auc(ops, [3.0], thresholds=(3.0, np.nextafter(3.0, 4.0)))      # strict: an error equal to the threshold is out
    assert below.tolist() == [0, 1] and auc[0] == 0.0
    zeros = np.array([0.0, -0.0, 2.0, -0.0, 0.0, 1.0, -0.0])                            # both zeros are one value: +0.0 in `sorted`
    auc, below, srt = run_auc(ops, zeros)
    check_auc(ops, zeros)
    assert not np.signbit(srt).any() and srt.tolist() == [0.0] * 5 + [1.0, 2.0] and below.tolist() == [7, 7, 7]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_c_level_refusals_return_the_error_code_and_launch_nothing(ops):
    import test_pose_error_cases_host as th
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.full((4096,), SENT_F, dtype=torch.float64, device="cuda")               # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    th.A16 = base
    try:
        for kw, words in th.error_refusals(base=base):
            th.refused(lib, th.call_error, b"pose_error_by_pair", kw, words)
        for kw, words in th.auc_refusals(base=base):
            th.refused(lib, th.call_auc, b"pose_auc", kw, words)
    finally:
        th.A16 = 0x7f0000001000
    torch.cuda.synchronize()
    assert bool((live == SENT_F).all())                                                  # nothing ran: nothing was written
    f64 = dict(dtype=torch.float64, device="cuda")
    R, t, T1 = torch.zeros((2, 3, 3), **f64), torch.zeros((2, 3), **f64), torch.zeros((2, 4, 4), **f64)
    for kw, word in (({"t": t[:1]}, "t must be"), ({"T1": T1[:1]}, "T1 must be"), ({"T0": T1[:1]}, "T0 must be"), ({"R": R[:0]}, "R must be"),
                     ({"counts": torch.zeros(3, dtype=torch.int64, device="cuda")}, "counts must hold"), ({"out": (t,)}, "out must be"),
                     ({"min_matches": -1}, "min_matches"), ({"min_gt_t": float("nan")}, "min_gt_t")):
        args = dict(R=R, t=t, T1=T1)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.pose_error_by_pair(**args)
    for kw, word in (({"errors": torch.zeros(ops.pose_auc_max_n() + 1, **f64)}, "n ="), ({"thresholds": ()}, "thresholds"),
                     ({"thresholds": (1.0,) * 9}, "n_thr"), ({"thresholds": (5.0, 0.0)}, "thresholds"), ({"errors": torch.zeros((4, 2), **f64)}, "vector")):
        args = dict(errors=torch.zeros(10, **f64))
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.pose_auc(**args)


# ---- 6. through the batch path ----------------------------------------------------------------------------------------------------
def _bytes(v):
    return v.contiguous().view(torch.uint8).clone()


@pytest.mark.parametrize("mixed", [False, True])
def test_verify_pose_error_through_batch(ops, mixed):
    from pats_amd import batch
    import test_triangulate_gpu as tg
    pairs, lens, thr = 4, (600, 14, 15, 300), np.float32(2e-3)             # the CALLER's order; 14 and 15 around min_matches
    scenes = [tc.make_scene(seed, n) for seed, n in zip((21, 22, 23, 24), lens)]
    caller_of = [2, 0, 3, 1] if mixed else [0, 1, 2, 3]                    # slot s holds the caller's pair caller_of[s]
    ml, mr, off, segs = tg.pack([scenes[i] for i in caller_of])
    norm = np.array([[0.01, -0.02, 1.0, 1.0, 0.0, 0.015, 1.0, 1.0]], np.float32).repeat(pairs, 0)      # the CALLER's order
    norm[:, 0] += np.arange(pairs, dtype=np.float32) * np.float32(0.005)
    for s_, i in enumerate(caller_of):                                     # stored so that the norm takes it back
        lo, n = segs[s_]
        ml[lo:lo + n] += norm[i, 0:2]
        mr[lo:lo + n] += norm[i, 4:6]
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([off, [int(off[-1]), 0, 0]]).astype(np.int64)                 # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if mixed:
        out["caller_of"] = caller_of
    models = cu(np.stack([pc.true_model(s) for s in scenes]).reshape(pairs, 1, 3, 3))
    dnorm, dthr = cu(norm), cu(np.full(pairs, thr, np.float32))
    P = tc.P_SWAP
    Rg, tgt = np.stack([P @ s["R"] @ P for s in scenes]), np.stack([P @ s["t"] for s in scenes])       # the CALLER's order
    T0, T1 = pe.extrinsic_sets(61, Rg, tgt)
    with pytest.raises(ValueError, match="pose_by_pair"):
        batch.pose_error_by_pair(out, cap, cu(T1))
    batch.verify_by_pair(out, cap, models, dthr, norm=dnorm, on="all", moments=True)
    pose = batch.pose_by_pair(out, cap, norm=dnorm, swapped=True, front=True)
    batch.triangulate_by_pair(out, cap, norm=dnorm, swapped=True)
    watched = ("verified", "pose", "points")
    kept = {k: out[k] for k in watched + ("by_pair", "summary")}
    before = {k: [_bytes(v) for v in out[k]] for k in watched}
    lengths = [int(l[0].shape[0]) for l in batch.split_by_pair(out, cap)]                   # the caller's order
    assert lengths == list(lens)
    R, t = pose[1].cpu().numpy(), pose[2].cpu().numpy()

    res = batch.pose_error_by_pair(out, cap, cu(T1), T0=cu(T0))
    assert out["pose_error"] is res and len(res) == 4
    got = {n: v.cpu().numpy() for n, v in zip(NAMES, res)}
    check_error(got, pe.pose_error64(R, t, T1, T0, counts=lengths))
    print("statuses %s, errors %s" % (got["status"].tolist(), got["err"].tolist()))
    assert got["status"].tolist()[1] == 1 and got["status"].tolist()[0] == 0 and got["status"].tolist()[3] == 0
    assert got["err"][0] < 5.0 and got["err"][3] < 5.0                      # the true models, 600 and 300 matches: the pose is the ground truth's
    res = batch.pose_error_by_pair(out, cap, cu(T1), T0=cu(T0), min_matches=301)
    got = {n: v.cpu().numpy() for n, v in zip(NAMES, res)}
    check_error(got, pe.pose_error64(R, t, T1, T0, counts=lengths, min_matches=301))
    assert got["status"].tolist() == [0, 1, 1, 1]

    for bad in ((torch.zeros(2 * pairs, dtype=torch.float64), 0), (torch.zeros(4 * pairs, dtype=torch.float64, device="cuda")[::2], 0),
                (torch.zeros(2 * pairs, device="cuda"), 0), (torch.zeros(2 * pairs, dtype=torch.float64, device="cuda"), pairs + 1)):
        with pytest.raises(ValueError, match="into must be"):             # on the CPU, strided, float32, too short
            batch.pose_error_by_pair(out, cap, cu(T1), into=bad)
    # two steps into one running buffer, then the one aggregate
    buf = torch.full((2 * pairs + 2 * PAD,), SENT_F, dtype=torch.float64, device="cuda")
    T1b = pe.as_T(np.stack([pe.rotation([1.0, 2.0, 3.0], 0.05 * (i + 1)) @ Rg[i] for i in range(pairs)]), tgt)
    for step, (A, B) in enumerate(((T1, T0), (T1b, None))):
        res = batch.pose_error_by_pair(out, cap, cu(A), T0=None if B is None else cu(B), min_matches=10, into=(buf, PAD + step * pairs))
        assert res[2].data_ptr() == buf[PAD + step * pairs:].data_ptr()
        got = {n: v.cpu().numpy() for n, v in zip(NAMES, res)}
        check_error(got, pe.pose_error64(R, t, A, B, counts=lengths, min_matches=10))
        filled = buf.cpu().numpy()
        assert (filled[:PAD] == SENT_F).all() and (filled[PAD + (step + 1) * pairs:] == SENT_F).all()
        assert filled[PAD + step * pairs:PAD + (step + 1) * pairs].tobytes() == got["err"].tobytes()
    total = buf[PAD:PAD + 2 * pairs]
    auc, below = ops.pose_auc(total, thresholds=(5.0, 10.0, 20.0, 90.0))
    want, want_below, _ = pe.auc64(total.cpu().numpy(), (5.0, 10.0, 20.0, 90.0))
    assert np.array_equal(below.cpu().numpy(), want_below) and (np.abs(auc.cpu().numpy() - want) <= pe.auc_bound(2 * pairs, want)).all()

    assert all(out[k] is v for k, v in kept.items())
    for k in watched:
        assert all(torch.equal(_bytes(v), b) for v, b in zip(out[k], before[k])), k
