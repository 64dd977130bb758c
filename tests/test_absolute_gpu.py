"""GPU: the absolute-pose branch - ops.lift_by_pair / absolute_hypotheses_by_pair / absolute_score_by_pair and batch.lift_by_pair /
hypothesize_p3p_by_pair / verify_abs_by_pair / pose_abs_by_pair / pose_branch(out, "absolute") - against the definition of
include/pats_amd.h restated in numpy (tests/absolute_cases.py):
    lift         points, valid and lift_count equal the float32 restatement bit for bit (NaN rows compared as NaN rows)
    hypotheses   sample_idx equals the restatement; all four slots exactly zero where the definition says so; the non-zero slots first,
                 ordered, rotations, positive depths, and - the accuracy contract - the largest reprojection residual on the sample
                 <= MARGIN * b * eps32, b = what the float64 restatement's solutions, rounded to float32, reach in the same run;
                 completeness against the truth and against the restatement on the generator of the solver cases
    score        counts equal the float32 emulation exactly and lie between the float64 classification's sure and sure + undecided;
                 the lowest index wins a tie; inlier is the winner's mask and sums to best_count; a second run has the same bits
    chain        through batch on a mixed pack and on a top-K: the metric translation has the ground truth's length
docs/parity.md records the measured ratios and shares.  Every output lies inside a larger sentinel-filled buffer and every input list
in a larger NaN-filled one: a call must define every byte of its views, none around them, and read no row beyond cap."""
import numpy as np
import pytest
import torch

import absolute_cases as ac
import epipolar_cases as ec

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0xAB
F32 = np.float32
NAN = float("nan")
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 600]
TAIL = 23                                                                     # rows inside cap behind the last segment


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bound():
    """MARGIN * b: b = the float64 restatement's solutions rounded to float32, measured in this run (shared, computed once)."""
    b = ac.baseline()
    assert np.isfinite(b) and b > 0
    return ac.MARGIN * b


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a):
    """A list as the view of a longer buffer whose rows beyond cap are NaN."""
    buf = torch.full((a.shape[0] + PAD,) + tuple(a.shape[1:]), NAN, dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


class Sentinel:
    """Output views inside sentinel-filled buffers; check() asserts that nothing around them changed."""

    def __init__(self):
        self.bufs = []

    def view(self, shape, dtype):
        sent = {torch.float32: SENT_F, torch.int32: SENT_I, torch.int64: SENT_I, torch.uint8: SENT_B}[dtype]
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device="cuda")
        self.bufs.append((buf, sent))
        return buf[PAD:PAD + n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, sent in self.bufs:
            assert bool((torch.cat([buf[:PAD], buf[-PAD:]]) == sent).all()), "bytes around an output view changed"


def same_rows(got, want):
    """Float arrays equal bit for bit, a NaN row matching a NaN row."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.int32), want[~wn].view(np.int32))


NORM = np.array([[18.0, 26.0, 1 / 40.0, 1 / 41.0, -0.03, 0.015, 1.1, 1.3]], F32)


def norm_for(pairs):
    return np.ascontiguousarray(NORM * np.linspace(0.9, 1.1, pairs, dtype=F32)[:, None])


# ---- 1. the lift -----------------------------------------------------------------------------------------------------------------
MAX_DEPTH, MAX_JUMP = F32(6.0), 0.25


def make_maps():
    """The maps of the lift cases on the device and as numpy arrays: 1x1, 2x3, 37x53 as a view with a longer row stride (special
    values at fixed pixels), none, empty."""
    rng = np.random.default_rng(7)
    big = rng.uniform(1.0, 5.0, (37, 53)).astype(F32)
    big[3, 4:10] = [0, -1, NAN, np.inf, MAX_DEPTH, np.nextafter(MAX_DEPTH, F32(np.inf))]
    big[5, 4:6] = [2.0, 2.5]                                                  # a jump exactly at max_jump
    big[6, 4:6] = [2.0, np.nextafter(F32(2.5), F32(0))]                       # just below
    big[7, 4:6] = [2.0, np.nextafter(F32(2.5), F32(9))]                       # just above
    store = torch.full((37, 64), NAN, dtype=torch.float32, device="cuda")
    store[:, :53] = cu(big)
    small = np.array([[1.5, 2.0, 2.25], [3.0, 2.5, 4.0]], F32)
    one = np.array([[2.0]], F32)
    host = {"1x1": one, "2x3": small, "37x53": big, "none": None, "empty": np.zeros((0, 5), F32)}
    dev = {"1x1": cu(one), "2x3": cu(small), "37x53": store[:, :53], "none": None,
           "empty": torch.zeros((0, 5), dtype=torch.float32, device="cuda")}
    assert dev["37x53"].stride(0) == 64 and not dev["37x53"].is_contiguous()
    return host, dev


def lift_points(h, w, n, seed):
    """n points for an h x w map: the special coordinates first, random ones behind."""
    rng = np.random.default_rng(seed)
    ub = lambda x: np.nextafter(F32(x), F32(-np.inf))                         # noqa: E731
    pts = []
    for axis, size in ((0, h), (1, w)):
        vals = [0, size - 1, 0.5, 1.5, 2.5, 3.5, -0.5, ub(-0.5), size - 0.5, ub(size - 0.5), size - 1 + 0.25, NAN, np.inf, -np.inf]
        for v in vals:
            p = [0.0, 0.0]
            p[axis] = v
            pts.append(p)
    if h == 37:
        pts += [[3, j] for j in range(4, 10)] + [[3, j + 0.5] for j in range(3, 10)] + [[3.5, 8], [2.25, 8]]
        pts += [[5, 4.5], [6, 4.5], [7, 4.5], [5.5, 4.5], [5, 4.25], [7, 4.75]]
    rnd = np.stack([rng.uniform(-1.0, h, max(n, 1)), rng.uniform(-1.0, w, max(n, 1))], 1)
    rnd[::3] = np.floor(rnd[::3]) + rng.choice([0.0, 0.5], (rnd[::3].shape[0], 2))     # centres and ties
    return np.concatenate([np.array(pts, F32), rnd.astype(F32)])[:n]


def run_lift(ops, pts, dev_maps, pairs, **kw):
    """dev_maps: the list of maps, or None with table= among the keywords."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    cap = pts.shape[0]
    s = Sentinel()
    dest = (s.view((cap, 3), torch.float32), s.view((cap,), torch.uint8), s.view((pairs,), torch.int64))
    got = ops.lift_by_pair(guarded(pts), dev_maps, out=dest, **d)
    s.check()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    return tuple(t.cpu().numpy() for t in dest)


@pytest.mark.parametrize("interp", [0, 1])
def test_lift_matches_the_restatement_bit_for_bit(ops, interp):
    host, dev = make_maps()
    kinds = ["1x1", "2x3", "none", "empty", "2x3", "1x1", "2x3", "37x53", "37x53"]
    shape = {"1x1": (1, 1), "2x3": (2, 3), "37x53": (37, 53), "none": (4, 4), "empty": (4, 4)}
    pts = np.concatenate([lift_points(*shape[k], n, 50 + p) for p, (k, n) in enumerate(zip(kinds, LENGTHS))] +
                         [lift_points(37, 53, TAIL, 99)])
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    segs = ec.segments(len(LENGTHS), pts.shape[0], pair_off=off)
    hm, dm = [host[k] for k in kinds], [dev[k] for k in kinds]
    md = np.full(len(kinds), MAX_DEPTH, F32)
    seen = 0
    for norm in (None, norm_for(len(kinds))):
        for max_depth in (None, md):
            for max_jump in ((None, MAX_JUMP) if interp else (None,)):
                got = run_lift(ops, pts, dm, len(kinds), pair_off=off, norm=norm, max_depth=max_depth, interp=interp, max_jump=max_jump)
                want = ac.lift_reference(pts, segs, hm, norm, max_depth, interp, max_jump)
                assert same_rows(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
                assert not got[0][off[-1]:].any() and not got[1][off[-1]:].any()          # behind the last segment: zeros
                seen += int(want[2].sum())
    assert seen > 1000
    full = ac.lift_reference(pts, segs, hm, None, md, interp, MAX_JUMP if interp else None)
    assert 0 < full[2][8] < LENGTHS[8] and full[2][2] == 0 and full[2][3] == 0 and full[2][5] > 0
    # the special pixels did what they are there for
    lo = int(off[8])
    row = {tuple(p): k for k, p in enumerate(pts[lo:lo + LENGTHS[8]].tolist()) if not np.isnan(p).any()}
    if interp == 0:
        assert [int(full[1][lo + row[(3.0, float(j))]]) for j in range(4, 10)] == [0, 0, 0, 0, 1, 0]
    else:
        assert [int(full[1][lo + row[(float(i), 4.5)]]) for i in (5, 6, 7)] == [1, 1, 0]
    # the table form, and the strided form with counts [0, 3, stride]
    stride, counts = 16, np.array([0, 3, 16], np.int64)
    sp = np.concatenate([lift_points(2, 3, 16, 1), lift_points(37, 53, 16, 2), lift_points(37, 53, 16, 3), lift_points(2, 3, 5, 4)])
    sk = ["2x3", "37x53", "37x53"]
    ssegs = ec.segments(3, sp.shape[0], stride=stride, counts=counts)
    tab = ops.lift_table([dev[k] for k in sk])
    for maps, extra in (([dev[k] for k in sk], {}), (None, {"table": tab}), (None, {"table": tab.dev})):
        got = run_lift(ops, sp, maps, 3, stride=stride, counts=counts, interp=interp, **extra)
        want = ac.lift_reference(sp, ssegs, [host[k] for k in sk], None, None, interp, None)
        assert same_rows(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert want[2].tolist()[0] == 0 and want[2][2] > 0


# ---- 2. the hypotheses -----------------------------------------------------------------------------------------------------------
def run_hyp(ops, X, mr, H, seeds, samples=True, counts_out=True, **kw):
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs = len(seeds)
    s = Sentinel()
    vm, vi, vn = s.view((pairs, H, 4, 3, 4), torch.float32), s.view((pairs, H, 3), torch.int32), s.view((pairs, H), torch.int32)
    dest = (vm,) + ((vi,) if samples else ()) + ((vn,) if counts_out else ())
    got = ops.absolute_hypotheses_by_pair(guarded(X), guarded(mr), H, cu(np.asarray(seeds, np.int64)), return_samples=samples,
                                          return_counts=counts_out, out=dest if len(dest) > 1 else vm, **d)
    s.check()
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(dest) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    assert samples or bool((vi == SENT_I).all())
    assert counts_out or bool((vn == SENT_I).all())
    return vm.cpu().numpy(), vi.cpu().numpy() if samples else None, vn.cpu().numpy() if counts_out else None


def check_hyp(got, ref, B=None):
    """The pointwise rules -> the largest residual / eps32 over the non-zero models."""
    models, idx, nm = got
    assert models.dtype == F32 and np.isfinite(models).all()
    worst = 0.0
    for p, r in enumerate(ref):
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        nz = models[p].reshape(models.shape[1], 4, 12).any(2)                 # [H,4]
        assert np.array_equal(nz.sum(1), nm[p]), "pair %d: n_models is not the number of non-zero slots" % p
        assert (nz[:, :-1] >= nz[:, 1:]).all(), "pair %d: a zero slot in front of a model" % p
        assert not nz[~r["finite"]].any(), "pair %d: a model where the definition says none" % p
        if r["n"] < 3:
            assert not nz.any() and (idx[p] == -1).all()
            continue
        for h in np.nonzero(nz.any(1))[0]:
            X, xr = r["X"][r["idx"][h]], r["xr"][r["idx"][h]]
            dist = []
            for s_ in range(int(nm[p][h])):
                Rt = models[p, h, s_].astype(np.float64)
                R, t = Rt[:, :3], Rt[:, 3]
                assert np.linalg.norm(R.T @ R - np.eye(3)) <= 1e-5 and np.linalg.det(R) > 0
                Y = X.astype(np.float64) @ R.T + t
                assert (Y[:, 2] > 0).all(), "pair %d sample %d: a sample point behind the camera" % (p, h)
                q = ac.residual3(R, t, X, xr) / ac.EPS32
                worst = max(worst, q)
                if B is not None:
                    assert q <= B, "pair %d sample %d: residual %g eps32 > %g" % (p, h, q, B)
                dist.append(np.linalg.norm(Y[0]))
            assert all(a <= b * (1 + 1e-6) for a, b in zip(dist, dist[1:])), "pair %d sample %d: the order" % (p, h)
    return worst


@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_hypotheses_rules_at_ragged_lengths_and_sample_counts(ops, bound, H):
    X, mr, off, _ = ac.make_pairs(LENGTHS, seed=100 + H, holes=0.1)
    mr[off[8] + 5] = [NAN, 0.1]                                               # right points that are not finite
    mr[off[8] + 11] = [0.2, np.inf]
    X, mr = np.concatenate([X, X[:TAIL]]), np.concatenate([mr, mr[:TAIL]])
    segs = ec.segments(len(LENGTHS), X.shape[0], pair_off=off)
    seeds = [7000 + H + 3 * p for p in range(len(LENGTHS))]
    models_seen = 0
    for norm in (None, norm_for(len(LENGTHS))):
        for progressive in (False, True):
            got = run_hyp(ops, X, mr, H, seeds, pair_off=off, norm=norm, progressive=progressive)
            ref = ac.hypotheses_reference(X, mr, segs, seeds, H, progressive, norm, solve=False)
            check_hyp(got, ref, bound)
            models_seen += int(got[2].sum())
            if H >= 63:
                fin = ref[8]["finite"]
                assert 0 < (~fin).sum() < H
                if norm is None:                                              # consistent data: the true pose solves every finite sample
                    assert (got[2][8][fin] > 0).mean() > 0.9
    assert models_seen > 0 or H == 1
    both = run_hyp(ops, X, mr, H, seeds, pair_off=off)
    for samples, counts_out in ((False, False), (True, False), (False, True)):         # sample_idx and n_models are optional
        only = run_hyp(ops, X, mr, H, seeds, samples=samples, counts_out=counts_out, pair_off=off)
        assert same_rows(only[0], both[0])
        assert (only[1] is None or np.array_equal(only[1], both[1])) and (only[2] is None or np.array_equal(only[2], both[2]))


def test_hypotheses_strided_form(ops, bound):
    stride, counts = 16, np.array([0, 3, 16], np.int64)
    X, mr, _, _ = ac.make_pairs([stride] * 3 + [9], seed=200)
    segs = ec.segments(3, X.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 0), (16, 3), (32, 16)]
    seeds = [1, 2, 3]
    for progressive in (False, True):
        got = run_hyp(ops, X, mr, 65, seeds, stride=stride, counts=counts, progressive=progressive)
        check_hyp(got, ac.hypotheses_reference(X, mr, segs, seeds, 65, progressive, solve=False), bound)
    a = run_hyp(ops, X[32:], mr[32:], 65, seeds[2:], pair_off=np.array([0, 16], np.int64))
    b = run_hyp(ops, X, mr, 65, seeds, stride=stride, counts=counts)
    c = run_hyp(ops, X, mr, 65, seeds, stride=stride, counts=counts)
    assert same_rows(a[0][0], b[0][2]) and np.array_equal(a[1][0], b[1][2]) and np.array_equal(a[2][0], b[2][2])
    assert same_rows(b[0], c[0]) and np.array_equal(b[1], c[1]) and np.array_equal(b[2], c[2])
    assert not b[0][0].any() and b[2][1].max() >= 1 and b[2][2].max() >= 2


def test_hypotheses_completeness_on_the_solver_cases(ops, bound):
    lengths, H = [300] * 4, 250
    X, mr, off, truth = ac.make_pairs(lengths, seed=900)
    segs = ec.segments(4, X.shape[0], pair_off=off)
    seeds = [77, 78, 79, 80]
    got = run_hyp(ops, X, mr, H, seeds, pair_off=off)
    ref = ac.hypotheses_reference(X, mr, segs, seeds, H)
    worst = check_hyp(got, ref, bound)
    samples = hit = sols = missed = 0
    for p, r in enumerate(ref):
        Rg, tg = truth[p]
        for h in range(H):
            dev = [(m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)) for m in got[0][p, h][:got[2][p, h]]]
            samples += 1
            hit += min([ac.pose_distance(R, t, Rg, tg) for R, t in dev] or [np.inf]) <= ac.POSE_TOL
            for R64, t64 in r["sols"][h]:
                sols += 1
                missed += min([ac.pose_distance(R, t, R64, t64) for R, t in dev] or [np.inf]) > ac.POSE_TOL
    print("P3P: largest residual %.1f eps32 (bound %.1f); the truth among the models in %.2f %% of %d samples; %.2f %% of the float64 "
          "solver's %d solutions without a device model" % (worst, bound, 100 * hit / samples, samples, 100 * missed / sols, sols))
    assert hit >= 0.99 * samples
    assert missed <= 0.01 * sols


# ---- 3. the score ----------------------------------------------------------------------------------------------------------------
def score_models(truth, M, seed):
    rng = np.random.default_rng(seed)
    out = []
    for R, t in truth:
        Rt = np.concatenate([R, t[:, None]], 1)
        m = np.stack([Rt + rng.normal(scale=10.0 ** -rng.integers(2, 6), size=(3, 4)) for _ in range(M)])
        if M >= 4:
            m[0] = rng.normal(size=(3, 4))
            m[1] = 0                                                          # the zero model among real ones
            m[2] = Rt * np.array([[1], [1], [-1]])                            # every point behind the camera
            m[3] = Rt
        if M >= 8:
            m[5] = m[4] = Rt + 1e-6                                           # a tie: the lower index wins
            m[7] = Rt
        out.append(m)
    return np.stack(out).astype(F32)


def run_score(ops, X, mr, models, thr, **kw):
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs, M = models.shape[:2]
    cap = X.shape[0]
    s = Sentinel()
    dest = (s.view((pairs, M), torch.int32), s.view((pairs,), torch.int32), s.view((pairs,), torch.int64), s.view((cap,), torch.uint8))
    if "conf" in d:
        d["conf"] = guarded(kw["conf"])
    got = ops.absolute_score_by_pair(guarded(X), guarded(mr), cu(models), cu(thr), out=dest, **d)
    s.check()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    return tuple(t.cpu().numpy() for t in dest)


def check_score(got, ref, cap):
    counts, best, best_count, inlier = got
    covered = np.zeros(cap, bool)
    for p, r in enumerate(ref):
        assert np.array_equal(counts[p], r["counts"]), "pair %d: counts differ from the float32 emulation" % p
        assert (counts[p] >= r["strict"]).all() and (counts[p] <= r["loose"]).all()
        assert best[p] == r["best"] and best_count[p] == r["best_count"]
        seg = slice(r["lo"], r["lo"] + r["n"])
        assert np.array_equal(inlier[seg].astype(bool), r["mask"]) and inlier[seg].sum() == best_count[p]
        covered[seg] = True
    assert not inlier[~covered].any()


@pytest.mark.parametrize("M", [1, 4, 1024])
def test_score_counts_equal_the_emulation_at_ragged_lengths(ops, M):
    X, mr, off, truth = ac.make_pairs(LENGTHS, seed=300 + M, outliers=0.3, holes=0.15)
    rng = np.random.default_rng(M)
    mr = (mr + rng.normal(scale=5e-4, size=mr.shape)).astype(F32)
    mr[off[8] + 3] = [NAN, 0.0]
    lo5 = int(off[5])
    mr[lo5:lo5 + LENGTHS[5]] = rng.uniform(5.0, 6.0, (LENGTHS[5], 2))          # a pair with no inlier at all
    X, mr = np.concatenate([X, X[:TAIL]]), np.concatenate([mr, mr[:TAIL]])
    cap = X.shape[0]
    segs = ec.segments(len(LENGTHS), cap, pair_off=off)
    models = score_models(truth, M, 40 + M)
    thr = np.full(len(LENGTHS), 2e-3, F32)
    thr[6], thr[7] = NAN, -1.0
    conf = rng.random(cap).astype(F32)
    conf[::13] = NAN
    for norm in (None, norm_for(len(LENGTHS))):
        for min_conf in (None, 0.3):
            kw = {} if min_conf is None else {"conf": conf, "min_conf": min_conf}
            got = run_score(ops, X, mr, models, thr, pair_off=off, norm=norm, **kw)
            ref = ac.score_reference(X, mr, segs, models, thr, norm, conf if min_conf is not None else None, min_conf)
            check_score(got, ref, cap)
            again = run_score(ops, X, mr, models, thr, pair_off=off, norm=norm, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(got, again))      # a second run has the same bits
            assert got[2][5] == 0 and got[1][5] == 0 and got[2][6] == 0 and got[2][7] == 0
            if M >= 4 and norm is None:
                assert not got[0][:, 1].any() and not got[0][:, 2].any() and got[2][8] > 100
            if M == 4 and norm is None:
                assert got[1][8] == 3                                         # the true pose
            if M == 1024:
                assert got[0][8][3] == got[0][8][7] and got[0][8][4] == got[0][8][5]     # equal models, equal counts


def test_score_largest_model_count_and_strided_form(ops):
    M = int(ops.epipolar_max_h())
    stride, counts = 16, np.array([0, 3, 16], np.int64)
    X, mr, _, truth = ac.make_pairs([stride] * 3 + [9], seed=400, outliers=0.3, holes=0.15)
    segs = ec.segments(3, X.shape[0], stride=stride, counts=counts)
    small = score_models(truth[:3], 64, 9)
    models = np.tile(small, (1, M // 64, 1, 1))
    # every model is there M / 64 times: the largest count is held by many indices and the lowest must win
    thr = np.full(3, 2e-3, F32)
    got = run_score(ops, X, mr, models, thr, stride=stride, counts=counts)
    ref = ac.score_reference(X, mr, segs, models, thr)
    check_score(got, ref, X.shape[0])
    assert got[0].shape == (3, M) and not got[0][0].any() and got[1][2] < 64 and got[2][2] > 0
    assert (got[0][2] == got[2][2]).sum() >= M // 64
    with pytest.raises(RuntimeError, match="absolute_score_by_pair"):
        ops.absolute_score_by_pair(cu(X), cu(mr), cu(np.zeros((3, M + 1, 3, 4), F32)), cu(thr), stride=stride, counts=cu(counts))


def test_score_walks_a_segment_too_long_to_stage(ops):
    n = 6144 + 131                                                           # past the staged capacity: read from global memory each pass
    c = ac.make_pair(500, n, outliers=0.3, holes=0.15)
    models = score_models([(c["R"], c["t"])], 8, 5)
    thr = np.full(1, 2e-3, F32)
    off = np.array([0, n], np.int64)
    got = run_score(ops, c["X"], c["xr"], models, thr, pair_off=off)
    check_score(got, ac.score_reference(c["X"], c["xr"], [(0, n)], models, thr), n)
    assert got[2][0] > 1000


# ---- 4. the chain through batch --------------------------------------------------------------------------------------------------
FOCAL = 60.0


def render_depth(h, w, seed):
    """A plane with a box on it, seen from the left camera at the origin: depth per pixel (i = y, j = x)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    y, x = (i - h / 2) / FOCAL, (j - w / 2) / FOCAL
    plane = 4.0 / (1.0 + 0.3 * x + 0.2 * y)                                   # n . X = 4 with n = (0.3, 0.2, 1)
    box = (np.abs(i - h * rng.uniform(0.3, 0.7)) < h / 6) & (np.abs(j - w * rng.uniform(0.3, 0.7)) < w / 6)
    return np.where(box, 2.5, plane).astype(F32)


def chain_case(shapes, n, seed):
    """Per pair (the CALLER's order): a depth map, n left pixels, the right pixels under a known metric pose (30 % outliers), 15 % of
    the matches on depth holes; everything in the hand-over's (y, x) order -> list of dicts."""
    P = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]])
    out = []
    for p, (h, w) in enumerate(shapes):
        rng = np.random.default_rng(seed + p)
        depth = render_depth(h, w, seed + 10 * p)
        ml = np.stack([rng.uniform(0, h - 1, n), rng.uniform(0, w - 1, n)], 1).astype(F32)
        hole = rng.random(n) < 0.15
        depth[np.rint(ml[hole, 0]).astype(int), np.rint(ml[hole, 1]).astype(int)] = 0.0
        norm = np.array([h / 2, w / 2, 1 / FOCAL, 1 / FOCAL] * 2, F32)
        X, ok = ac.lift32(ml, depth, norm[:4])
        R, t = ac.rodrigues(0.15 * rng.normal(size=3)), 0.4 * rng.normal(size=3)       # the reference's (x, y) frame
        Y = np.where(ok[:, None], X, 1.0).astype(np.float64) @ (P @ R @ P).T + P @ t
        mr = np.stack([Y[:, 0] / Y[:, 2] * FOCAL + h / 2, Y[:, 1] / Y[:, 2] * FOCAL + w / 2], 1)
        bad = rng.random(n) < 0.3
        mr[bad] = np.stack([rng.uniform(0, h, int(bad.sum())), rng.uniform(0, w, int(bad.sum()))], 1)
        out.append({"depth": depth, "ml": ml, "mr": mr.astype(F32), "norm": norm, "R": R, "t": t, "good": ok & ~bad})
    return out


def chain64(case, pair_seed, H, thr):
    """The float64 restatement of the chain for one pair -> the winner's t (reference frame) and its model index."""
    X, _ = ac.lift32(case["ml"], case["depth"], case["norm"][:4])
    xr = ac.right32(case["mr"], case["norm"])
    idx = ac.sample_idx3(pair_seed, X.shape[0], H, progressive=False)
    models = np.zeros((H, 4, 3, 4), F32)
    for h in range(H):
        if np.isfinite(X[idx[h]]).all():
            for s_, (R, t) in enumerate(ac.p3p64(X[idx[h]], xr[idx[h]])):
                models[h, s_] = np.concatenate([R, t[:, None]], 1)
    models = models.reshape(4 * H, 3, 4)
    counts = ac.emulate32(X, xr, ac.participates(X, xr), models, thr).sum(1)
    best = int(np.argmax(counts))
    return ac.pose_from_model(models[best], True), best, int(counts[best])


@pytest.mark.parametrize("on", ["all", "topk"])
def test_chain_through_batch_recovers_the_metric_pose(ops, on):
    from pats_amd import batch
    shapes, n, H, seed = [(40, 56), (48, 64), (40, 56)], 200, 64, 5
    pairs = len(shapes)
    cases = chain_case(shapes, n, 600)
    mixed = on == "all"
    caller_of = [1, 0, 2] if mixed else [0, 1, 2]                             # slot s holds the caller's pair caller_of[s]
    cap = batch.Capacities(pairs, 5, 6)
    ml = np.concatenate([cases[i]["ml"] for i in caller_of])
    mr = np.concatenate([cases[i]["mr"] for i in caller_of])
    summary = np.concatenate([np.arange(pairs + 1) * n, [pairs * n, 0, 0]]).astype(np.int64)
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if mixed:
        out["caller_of"] = caller_of
    else:                                                                     # the same rows as a top-K result
        out["topk"] = (dl.view(pairs, n, 2), dr.view(pairs, n, 2), torch.ones(pairs, n, device="cuda"),
                       torch.arange(n, dtype=torch.int32, device="cuda").repeat(pairs, 1), cu(np.full(pairs, n, np.int64)))
    norm = cu(np.stack([c["norm"] for c in cases]))
    thr = cu(np.full(pairs, 0.5 / FOCAL, F32))
    depths = [cu(c["depth"]) for c in cases]
    T1 = np.tile(np.eye(4), (pairs, 1, 1))
    for i, c in enumerate(cases):
        T1[i, :3, :3], T1[i, :3, 3] = c["R"], c["t"]
    # the other branches first: they must come through untouched
    E = np.stack([ac.pose_from_model(np.concatenate([c["R"], c["t"][:, None]], 1), False)[0] for c in cases]).astype(F32)
    batch.verify_by_pair(out, cap, cu(E.reshape(pairs, 1, 3, 3)), thr, norm=norm, on=on, moments=True)
    batch.pose_by_pair(out, cap, norm=norm, swapped=True)
    batch.verify_h_by_pair(out, cap, cu(np.tile(np.eye(3, dtype=F32), (pairs, 1, 1, 1))), thr, norm=norm, on=on)
    kept = {k: [t.clone() for t in out[k]] for k in ("pose", "verified", "verified_h")}
    held = {k: out[k] for k in kept}

    lifted = batch.lift_by_pair(out, cap, depths, norm, on=on)
    assert out["lifted"] is lifted and lifted[3] == on and tuple(lifted[0].shape) == (pairs * n, 3)
    models = batch.hypothesize_p3p_by_pair(out, cap, H, seed=seed, norm=norm, progressive=False)
    assert tuple(models.shape) == (pairs, 4 * H, 3, 4) and out["hypotheses_p3p"] is models
    ver = batch.verify_abs_by_pair(out, cap, models, thr, norm=norm)
    assert out["verified_abs"] is ver and out["verified_abs_on"] == on
    pose = batch.pose_abs_by_pair(out, cap, swapped=True)
    assert out["pose_abs"] is pose and len(pose) == 7
    view = batch.pose_branch(out, "absolute")
    err_R, err_t, err, status = (t.cpu().numpy() for t in batch.pose_error_by_pair(view, cap, cu(T1)))
    split = batch.split_pose_by_pair(view, cap)
    torch.cuda.synchronize()

    for k in kept:                                                            # bit-unchanged, and the same objects
        assert out[k] is held[k] and all(torch.equal(a, b) for a, b in zip(out[k], kept[k])), k
    assert "pose_error" not in out and "points" not in out
    lift_count = lifted[2].cpu().numpy()
    Rd, td, Ed = pose[1].cpu().numpy(), pose[2].cpu().numpy(), pose[0].cpu().numpy()
    front = pose[6].cpu().numpy().reshape(pairs, n)
    assert (status == 0).all(), status                                       # "scored"
    worst = 0.0
    for i, c in enumerate(cases):                                             # the CALLER's order
        slot = caller_of.index(i)
        assert lift_count[i] == ac.lift32(c["ml"], c["depth"], c["norm"][:4])[1].sum()
        (E64, R64, t64), best64, count64 = chain64(c, seed + i, H, np.float32(0.5 / FOCAL))
        e64 = abs(np.linalg.norm(t64) - np.linalg.norm(c["t"]))
        # 4 x what the float64 restatement of the same chain reaches on the same seed (docs/parity.md): the two chains' models differ
        # by the solvers' float64 rounding and one rounding to float32 each, a factor of 2 apiece; the floor is float32's step at |t|
        tol = 4 * max(e64, ac.EPS32 * np.linalg.norm(c["t"]))
        e = abs(np.linalg.norm(td[i]) - np.linalg.norm(c["t"]))
        worst = max(worst, e / tol)
        print("pair %d: | |t| - |t_gt| | = %.3g (float64 chain %.3g, tolerance %.3g), inliers %d of %d good" %
              (i, e, e64, tol, int(pose[3][i]), int(c["good"].sum())))
        assert e <= tol
        assert np.linalg.norm(Rd[i] - c["R"]) <= 1e-3 and np.linalg.norm(td[i] - c["t"]) <= 1e-3
        assert abs(np.linalg.norm(Ed[i]) - 1) <= 1e-12 and err_R[i] < 0.1 and err_t[i] < 0.1
        assert front[slot].sum() == int(pose[3][i]) >= 0.9 * c["good"].sum() and front[slot][~c["good"]].sum() <= 2
        assert torch.equal(split[i][0], pose[1][i]) and torch.equal(split[i][1], pose[2][i])
    print("chain (%s): the largest error / tolerance = %.3f" % (on, worst))


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["branch", "order", "length", "dtype", "interp"])
def test_argument_errors_name_the_function(case):
    from pats_amd import batch
    pairs, n = 2, 8
    cap = batch.Capacities(pairs, 5, 6)
    dl = torch.rand(pairs * n, 2, device="cuda") * 8
    ds = cu(np.array([0, n, 2 * n, 2 * n, 0, 0], np.int64))
    out = {"matches_l": dl, "matches_r": dl.clone(), "by_pair": (dl, dl.clone(), ds[:pairs + 1]), "summary": ds}
    depth = torch.ones(10, 10, device="cuda")
    if case == "branch":
        batch.lift_by_pair(out, cap, [depth, depth], None, on="all")
        with pytest.raises(ValueError, match="pose_branch.*pose_abs_by_pair"):
            batch.pose_branch(out, "absolute")
    elif case == "order":
        with pytest.raises(ValueError, match="hypothesize_p3p_by_pair.*lift_by_pair"):
            batch.hypothesize_p3p_by_pair(out, cap, 8)
    elif case == "length":
        with pytest.raises(ValueError, match="lift_by_pair.*depths"):
            batch.lift_by_pair(out, cap, [depth], None, on="all")
    elif case == "dtype":
        with pytest.raises(ValueError, match="lift_by_pair.*depths\\[1\\]"):
            batch.lift_by_pair(out, cap, [depth, depth.double()], None, on="all")
    else:
        with pytest.raises(ValueError, match="lift_by_pair.*interp"):
            batch.lift_by_pair(out, cap, [depth, depth], None, on="all", interp="cubic")
