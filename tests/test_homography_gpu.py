"""GPU: the per-pair homographies - ops.homography_{hypotheses,score,refit}_by_pair and batch.{hypothesize_h,verify_h,homography}_by_pair
- against the definition of include/pats_amd.h ("Per-pair homographies") restated in numpy (tests/homography_cases.py):
    sample_idx   equals the integer restatement bit for bit
    models       zero where the definition says so, otherwise finite with | |e| - 1 | <= 1e-5, the sign rule and the backward error
                 |A e|_2 <= B eps32 |A|_F, B = 8 * b32, b32 = numpy's float32 svd on the same samples in the same run.
                 The test prints the kernel's maximum; docs/parity.md ("Homographies") is where it is recorded
    verdicts     equal to float64 on every DECIDED cell (outside the relative band 1e-3 around thr^2 a2^2), strict <= counts <= loose,
                 best the lowest index of the largest count, the mask's population per segment == best_count
    moments      the float64 sum over the kernel's own mask to 64 eps64 |M|_F (an ordering difference), two calls byte-identical
    refit        r(h) = |M h - (h^T M h) h| / (eps64 |M|_F) <= 8 b64, b64 = numpy's eigh on the same moments in the same run (the
                 contract docs/parity.md sets for the pose's e_refit); H_px against numpy from the kernel's own H within 64 eps64
Every output lies inside a larger sentinel-filled buffer: a call defines every byte of the views and none around them."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import homography_cases as hm
import pose_cases as pc

pytestmark = pytest.mark.gpu

PAD = 64
SENT = {torch.int32: -123456, torch.int64: -123456, torch.uint8: 0xA5, torch.float64: -777.25, torch.float32: -777.25}
T, C = 2048, 256        # the score kernel's match tile (EPI_THREADS * EPI_R) and model chunk (EPI_CHUNK): asserted against the source
NORM = np.array([[0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3]], np.float32)      # scales between 1 and 1.3


def test_the_tile_constants_are_the_kernels():
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "pats_amd", "csrc", "epipolar.hip")).read()
    k = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))       # noqa: E731
    assert k("EPI_THREADS") * k("EPI_R") == T and k("EPI_CHUNK") == C


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bound():
    """B = MARGIN * b32, the baseline measured in this run on the tolerance cases (shared, computed once)."""
    b32 = hm.baseline32()
    assert np.isfinite(b32) and b32 > 0
    return hm.MARGIN * b32, b32


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def norm_for(pairs):
    """[pairs,8]: NORM with centres that differ from pair to pair (a wrong permutation shows)."""
    shift = np.linspace(0, 0.01, pairs, dtype=np.float32)[:, None] * np.array([1, -1, 0, 0, -1, 1, 0, 0], np.float32)
    return np.ascontiguousarray(np.repeat(NORM, pairs, 0) + shift)


def views_of(shapes):
    """Sentinel-filled buffers -> (views, check): check() asserts that the PAD elements around every view kept the sentinel."""
    views, whole = [], []
    for shape, dt in shapes:
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENT[dt], dtype=dt, device="cuda")
        whole.append(buf)
        views.append(buf[PAD:PAD + n].view(shape))

    def check():
        for buf in whole:
            assert bool((torch.cat([buf[:PAD], buf[-PAD:]]) == SENT[buf.dtype]).all()), "bytes around an output view changed"
    return tuple(views), check


def guarded(a):
    """A list as a view of a longer buffer whose rows beyond cap are NaN: a read past cap would zero a model or drop an inlier."""
    buf = torch.full((a.shape[0] + PAD, 2), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


def dev_kw(kw):
    return {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


def run_hyp(ops, ml, mr, H, seeds, **kw):
    pairs = len(seeds)
    (vm, vi), chk = views_of([((pairs, H, 3, 3), torch.float32), ((pairs, H, 4), torch.int32)])
    got = ops.homography_hypotheses_by_pair(guarded(ml), guarded(mr), H, cu(np.asarray(seeds, np.int64)), return_samples=True, out=(vm, vi),
                                            **dev_kw(kw))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == vm.data_ptr() and got[1].data_ptr() == vi.data_ptr()
    chk()
    return vm.cpu().numpy(), vi.cpu().numpy()


def check_hyp(got, ref, B=None, nonzero=True):
    models, idx = got
    assert models.dtype == np.float32 and idx.dtype == np.int32
    for p, r in enumerate(ref):
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        if r["n"] < 4:
            assert not models[p].any() and (idx[p] == -1).all()
        elif nonzero:                                                     # a generic sample: zero ONLY where the definition says so
            assert np.array_equal(models[p].reshape(-1, 9).any(1), r["finite"]), "pair %d: a zero model on a finite sample" % p
    return hm.check_models(models, ref, B)


def run_score(ops, ml, mr, models, thr, moments=False, **kw):
    pairs, H = models.shape[0], models.shape[1]
    shapes = [((pairs, H), torch.int32), ((pairs,), torch.int32), ((pairs,), torch.int64), ((ml.shape[0],), torch.uint8)]
    if moments:
        shapes.append(((pairs, 9, 9), torch.float64))
    views, chk = views_of(shapes)
    got = ops.homography_score_by_pair(guarded(ml), guarded(mr), cu(models), cu(np.asarray(thr, np.float32)), moments=moments, out=views,
                                       **dev_kw(kw))
    torch.cuda.synchronize()
    assert len(got) == len(shapes) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    chk()
    return [v.cpu().numpy() for v in views]


def check_score(got, ref, segs, cap):
    counts, best, best_count, inlier = got[:4]
    assert counts.dtype == np.int32 and best.dtype == np.int32 and best_count.dtype == np.int64 and inlier.dtype == np.uint8
    assert set(np.unique(inlier)) <= {0, 1}
    covered = np.zeros(cap, bool)
    for p, (r, (lo, n)) in enumerate(zip(ref, segs)):
        covered[lo:lo + n] = True
        assert (r["strict"] <= counts[p]).all() and (counts[p] <= r["loose"]).all(), "pair %d: counts outside [strict, loose]" % p
        b = int(best[p])
        assert b == int(np.argmax(counts[p])) and best_count[p] == counts[p, b]           # np.argmax: the lowest index of the maximum
        mask = inlier[lo:lo + n].astype(bool)
        assert mask.sum() == best_count[p], "pair %d: the mask and the winner's count disagree" % p
        dec = r["decided"][b]
        assert np.array_equal(mask[dec], r["inl"][b][dec]), "pair %d: the mask differs from float64 on a decided cell" % p
    assert not inlier[~covered].any(), "a row outside every segment is set"


def build(lengths, H, seed, tail=29):
    """Scenes concatenated; behind the last segment `tail` rows that WOULD be inliers of the last pair."""
    cases = [hm.make_case(seed + 17 * p, max(n, 4), H) for p, n in enumerate(lengths)]
    z = np.zeros((0, 2), np.float32)
    extra = hm.make_scene(seed + 17 * (len(lengths) - 1), tail + 4, outliers=0.0)
    ml = np.concatenate([c["ml"][:n] for c, n in zip(cases, lengths)] + [extra["ml"][:tail], z])
    mr = np.concatenate([c["mr"][:n] for c, n in zip(cases, lengths)] + [extra["mr"][:tail], z])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return ml, mr, np.stack([c["models"] for c in cases]), np.full(len(lengths), 2e-3, np.float32), off, cases


def score_and_check(ops, lengths, H, seed, **kw):
    ml, mr, models, thr, off, cases = build(lengths, H, seed)
    got = run_score(ops, ml, mr, models, thr, pair_off=off, **kw)
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    check_score(got, hm.verify_reference(ml, mr, segs, models, thr, **{k: v for k, v in kw.items() if k in ("norm", "conf", "min_conf")}),
                segs, ml.shape[0])
    return got, (ml, mr, models, thr, off, cases)


def run_refit(ops, bc, **kw):
    pairs = len(bc)
    views, chk = views_of([((pairs, 3, 3), torch.float64), ((pairs, 2), torch.float64), ((pairs, 3, 3), torch.float64)])
    got = ops.homography_refit_by_pair(cu(np.asarray(bc, np.int64)), return_pixel=True, out=views, **dev_kw(kw))
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    chk()
    out = {n: v.cpu().numpy() for n, v in zip(("H", "eig", "H_px"), views)}
    assert all(np.isfinite(v).all() and not (v == SENT[torch.float64]).any() for v in out.values())   # no NaN in any output, ever
    return out


# ---- 1. the sampler, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_sampler_on_ragged_segments_with_and_without_norm_progressive_or_not(ops, bound, H):
    lengths = [0, 3, 4, 5, 64, 600]
    ml, mr, off = hm.make_pairs(lengths, seed=100 + H)
    ml, mr = np.concatenate([ml, ml[:23]]), np.concatenate([mr, mr[:23]])              # rows inside cap behind the last segment
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    seeds = [5000 + H + 3 * p for p in range(len(lengths))]
    for norm in (None, norm_for(len(lengths))):
        for progressive in (False, True):
            got = run_hyp(ops, ml, mr, H, seeds, pair_off=off, norm=norm, progressive=progressive)
            check_hyp(got, hm.reference(ml, mr, segs, seeds, H, progressive, norm), B=bound[0])
    only = ops.homography_hypotheses_by_pair(cu(ml), cu(mr), H, cu(np.asarray(seeds, np.int64)), pair_off=cu(off))      # sample_idx optional
    assert np.array_equal(only.cpu().numpy().view(np.int32), run_hyp(ops, ml, mr, H, seeds, pair_off=off)[0].view(np.int32))


def test_sampler_on_strided_segments_clamped_counts_and_stale_offsets(ops, bound):
    stride, counts = 16, np.array([4, 16, 3, 20], np.int64)                             # 20 is clamped to 16
    ml, mr, _ = hm.make_pairs([stride] * 4 + [9], seed=200)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 4), (16, 16), (32, 3), (48, 16)]
    seeds = [1, 2, 3, 4]
    for norm in (None, norm_for(4)):
        for progressive in (False, True):
            got = run_hyp(ops, ml, mr, 65, seeds, stride=stride, counts=counts, norm=norm, progressive=progressive)
            check_hyp(got, hm.reference(ml, mr, segs, seeds, 65, progressive, norm), B=bound[0])
    a = run_hyp(ops, ml, mr, 65, seeds[:1], pair_off=np.array([0, 4], np.int64))        # the same rows in the ragged form: the same bits
    b = run_hyp(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    assert np.array_equal(a[0][0].view(np.int32), b[0][0].view(np.int32)) and np.array_equal(a[1][0], b[1][0])
    ml, mr, _ = hm.make_pairs([300], seed=300)
    cap = ml.shape[0]
    for bad in (np.array([-50, 120, 40, cap + 100000], np.int64),                       # negative, descending (empty), past cap
                np.array([cap + 5, cap + 9, 2 ** 40, -2 ** 40], np.int64)):
        got = run_hyp(ops, ml, mr, 40, [7, 8, 9], pair_off=bad)
        check_hyp(got, hm.reference(ml, mr, ec.segments(3, cap, pair_off=bad), [7, 8, 9], 40), B=bound[0])
    longer = np.array([0, 100, 300, 12345, -1, 7], np.int64)                            # a longer buffer that starts with the offsets
    got = run_hyp(ops, ml, mr, 9, [1, 2], pair_off=longer, pairs=2)
    check_hyp(got, hm.reference(ml, mr, [(0, 100), (100, 200)], [1, 2], 9), B=bound[0])
    z2 = np.zeros((0, 2), np.float32)                                                   # cap == 0
    m, i = run_hyp(ops, z2, z2, 70, [1, 2], pair_off=np.zeros(3, np.int64))
    assert not m.any() and (i == -1).all()


# ---- 2. the backward error ----------------------------------------------------------------------------------------------------
def test_backward_error_against_eight_times_the_float32_svd(ops, bound):
    B, b32 = bound
    cases = hm.tolerance_cases()
    ml, mr = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    H = hm.TOLERANCE_CASES[0][2]
    seeds = [c[3] for c in hm.TOLERANCE_CASES]
    off = np.concatenate([[0], np.cumsum([c[1] for c in hm.TOLERANCE_CASES])]).astype(np.int64)
    got = run_hyp(ops, ml, mr, H, seeds, pair_off=off)
    ref = hm.reference(ml, mr, ec.segments(3, ml.shape[0], pair_off=off), seeds, H)
    assert all(np.array_equal(r["idx"], c[2]) for r, c in zip(ref, cases))              # the samples b32 was measured on
    worst = check_hyp(got, ref)
    print("backward error over %d samples: device %.4f, b32 %.4f, B = %.1f * b32 = %.4f" % (3 * H, worst, b32, hm.MARGIN, B))
    assert worst <= B
    again = run_hyp(ops, ml, mr, H, seeds, pair_off=off)                                # deterministic
    assert np.array_equal(got[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(got[1], again[1])


# ---- 3. degenerate and non-finite samples -------------------------------------------------------------------------------------
def test_degenerate_samples_give_zero_or_finite_unit_models(ops):
    ml, mr, _ = hm.make_pairs([1, 4, 30], seed=400)
    ml = np.concatenate([np.repeat(ml[:1], 4, 0), ml[1:]])                              # pair 0: four identical matches
    mr = np.concatenate([np.repeat(mr[:1], 4, 0), mr[1:]])
    ml[4:7] = np.array([[-0.5, -0.25], [0.0, 0.0], [0.5, 0.25]], np.float32)            # pair 1: three collinear points plus one
    segs = [(0, 4), (4, 4), (8, 30)]
    got = run_hyp(ops, ml, mr, 70, [11, 12, 13], pair_off=np.array([0, 4, 8, 38], np.int64))
    check_hyp(got, hm.reference(ml, mr, segs, [11, 12, 13], 70), nonzero=False)         # zero or finite unit, the sign rule
    assert got[0][2].reshape(70, 9).any(1).all()                                        # the neighbour is unaffected


def test_a_nan_coordinate_zeroes_exactly_the_samples_that_hold_it(ops, bound):
    ml, mr, off = hm.make_pairs([40, 40], seed=500)
    ml[5, 1], mr[40 + 17, 0] = np.nan, np.inf
    H = 200
    got = run_hyp(ops, ml, mr, H, [21, 22], pair_off=off)
    check_hyp(got, hm.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H), B=bound[0])  # zero iff not finite (nonzero=True)
    for p, row in ((0, 5), (1, 17)):
        hit = (got[1][p] == row).any(1)
        assert 5 < hit.sum() < H - 10 and np.array_equal(~got[0][p].reshape(H, 9).any(1), hit)
    norm = norm_for(2)
    norm[1, 6] = np.inf                                                                 # a non-finite x after norm: the whole pair
    got = run_hyp(ops, ml, mr, H, [21, 22], pair_off=off, norm=norm)
    check_hyp(got, hm.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H, norm=norm), B=bound[0])
    assert not got[0][1].any() and (got[1][1] >= 0).all()


# ---- 4. verdicts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,H,n", hm.HOST_CASES)
def test_verdicts_against_float64_on_the_committed_seeds(ops, seed, H, n):
    c = hm.make_case(seed, n, H)
    off = np.array([0, n], np.int64)
    got = run_score(ops, c["ml"], c["mr"], c["models"][None], [c["thr"]], pair_off=off)
    ref = hm.verify_reference(c["ml"], c["mr"], [(0, n)], c["models"][None], [c["thr"]])
    check_score(got, ref, [(0, n)], n)
    assert got[0][0, c["true"]] == got[2][0] >= 0.9 * c["good"].sum()                   # no sample beats the true homography
    print("seed %d: %d x %d cells, %d undecided, best_count %d of %d planar matches"
          % (seed, H, n, int((~ref[0]["decided"]).sum()), got[2][0], c["good"].sum()))


# ---- 5. verification edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[0], [1, 0, 63], [T - 1, 0, T], [T + 1, 0, 65]])
def test_segment_lengths_around_the_wave_and_the_match_tile(ops, lengths):
    score_and_check(ops, lengths, 5, seed=2000 + sum(lengths))


@pytest.mark.parametrize("H", [1, C - 1, C, C + 1])
def test_model_counts_around_the_chunk(ops, H):
    score_and_check(ops, [300, 0, T + 7], H, seed=3000 + H)


def test_zero_models_bad_thresholds_and_empty_arrays(ops):
    ml, mr, models, thr, off, cases = build([900, 900, 900], 10, seed=6000)
    for p in range(3):                                       # the true model twice: the lower index wins; zero models in between
        Ht = models[p, cases[p]["true"]].copy()
        models[p, [cases[p]["true"], 0, 4, 9]] = 0.0
        models[p, 2], models[p, 7] = Ht, Ht
    segs = ec.segments(3, ml.shape[0], pair_off=off)
    base = run_score(ops, ml, mr, models, thr, pair_off=off, moments=True)
    check_score(base, hm.verify_reference(ml, mr, segs, models, thr), segs, ml.shape[0])
    assert base[1].tolist() == [2, 2, 2] and (base[0][:, 2] == base[0][:, 7]).all() and not base[0][:, [0, 4, 9]].any()
    got = run_score(ops, ml, mr, np.zeros_like(models), thr, pair_off=off, moments=True)      # every model zero
    assert not got[0].any() and got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0, 0, 0] and not got[3].any() and not got[4].any()
    for bad in (np.nan, -1e-3, -np.inf):                     # thr NaN / negative: zero inliers for that pair only
        t2 = thr.copy()
        t2[1] = bad
        got = run_score(ops, ml, mr, models, t2, pair_off=off, moments=True)
        assert not got[0][1].any() and got[1][1] == 0 and got[2][1] == 0 and not got[3][900:1800].any() and not got[4][1].any()
        for p in (0, 2):
            assert np.array_equal(got[0][p], base[0][p]) and got[1][p] == base[1][p] and got[4][p].tobytes() == base[4][p].tobytes()
        assert np.array_equal(got[3][:900], base[3][:900]) and np.array_equal(got[3][1800:], base[3][1800:])
    z2 = np.zeros((0, 2), np.float32)                        # cap == 0: every pair empty, the outputs still defined
    got = run_score(ops, z2, z2, models[:2], [1e-3, 1e-3], moments=True, pair_off=np.zeros(3, np.int64))
    assert not got[0].any() and not got[1].any() and not got[2].any() and got[3].shape == (0,) and not got[4].any()


def test_confidence_gate_is_inclusive_and_gates_a_nan(ops):
    ml, mr, models, thr, off, _ = build([1200, 0, T + 100], 6, seed=8000)
    rng = np.random.default_rng(8)
    conf = rng.random(ml.shape[0]).astype(np.float32)
    conf[rng.random(ml.shape[0]) < 0.2] = np.float32(0.5)             # a fifth of the matches sit exactly on the threshold
    conf[::37] = np.nan
    segs = ec.segments(3, ml.shape[0], pair_off=off)
    got = run_score(ops, ml, mr, models, thr, pair_off=off, conf=conf, min_conf=0.5)
    check_score(got, hm.verify_reference(ml, mr, segs, models, thr, conf=conf, min_conf=0.5), segs, ml.shape[0])
    free = run_score(ops, ml, mr, models, thr, pair_off=off)
    on_edge = np.flatnonzero((conf == np.float32(0.5)) & (free[3] == 1))
    assert len(on_edge) > 50 and got[3][on_edge].all()                # inclusive
    nan = np.flatnonzero(np.isnan(conf) & (free[3] == 1))
    assert len(nan) > 5 and not got[3][nan].any()                     # a NaN confidence takes no part
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got[3] == 1, (free[3] == 1) & (conf >= 0.5))
    same = run_score(ops, ml, mr, models, thr, pair_off=off, conf=conf)     # conf without a threshold: not read
    assert all(np.array_equal(a, b) for a, b in zip(same, free))


def test_strided_slack_and_rows_outside_the_segments_are_zero_and_norm_is_the_points(ops):
    stride = 300
    counts = np.array([250, 0, 300, 17], np.int64)
    cases = [hm.make_case(11000 + p, stride, 3, outliers=0.0) for p in range(4)]           # every row WOULD be an inlier
    ml = np.concatenate([c["ml"] for c in cases] + [cases[3]["ml"][:41]])
    mr = np.concatenate([c["mr"] for c in cases] + [cases[3]["mr"][:41]])
    models = np.stack([c["models"] for c in cases])
    thr = np.full(4, 2e-3, np.float32)
    got = run_score(ops, ml, mr, models, thr, stride=stride, counts=counts, moments=True)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    check_score(got, hm.verify_reference(ml, mr, segs, models, thr), segs, ml.shape[0])
    assert got[3][:250].sum() > 200 and not got[3][250:600].any() and not got[3][900 + 17:].any()
    assert np.isfinite(got[4]).all() and not got[4][1].any()
    # norm: stored coordinates whose normalisation lands near the scene's points score like the float32 points themselves
    norm = norm_for(4)
    xl, xr = ml.copy(), mr.copy()
    for p, (lo, n) in enumerate(segs):
        xl[lo:lo + n], xr[lo:lo + n] = ec.points32(ml[lo:lo + n], mr[lo:lo + n], norm[p])
    with_norm = run_score(ops, ml, mr, models, thr, stride=stride, counts=counts, norm=norm)
    pre = run_score(ops, xl, xr, models, thr, stride=stride, counts=counts)
    assert all(np.array_equal(a, b) for a, b in zip(with_norm, pre))
    check_score(with_norm, hm.verify_reference(ml, mr, segs, models, thr, norm=norm), segs, ml.shape[0])


# ---- 6. moments ---------------------------------------------------------------------------------------------------------------
def test_moments_against_float64_over_the_returned_mask(ops):
    ml, mr, models, thr, off, cases = build([1700, 0, 2 * T + 50], 9, seed=10000)
    got = run_score(ops, ml, mr, models, thr, pair_off=off, moments=True)
    again = run_score(ops, ml, mr, models, thr, pair_off=off, moments=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    worst = 0.0
    for p, (lo, n) in enumerate(ec.segments(3, ml.shape[0], pair_off=off)):
        mask = got[3][lo:lo + n].astype(bool)
        want = hm.moments64(ml[lo:lo + n], mr[lo:lo + n], mask)
        fro = np.linalg.norm(want)
        err = np.abs(got[4][p] - want).max()
        worst = max(worst, err / (hm.EPS64 * fro) if fro else 0.0)
        assert err <= 64 * hm.EPS64 * fro, p
        assert np.array_equal(got[4][p], got[4][p].T)
        if n:
            assert got[4][p][2, 2] == mask.sum() and mask.sum() > 100
            h = hm.sign_rule(np.linalg.eigh(got[4][p])[1][:, 0])          # the refit: the null vector is the true homography
            assert np.abs(h - cases[p]["H"].reshape(9)).max() < 2e-3
    print("moments: largest entry error %.2f eps64 |M|_F" % worst)
    assert not got[4][1].any()


# ---- 7. refit -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refit_scenes():
    """Six pairs of 20 .. 3000 matches with their float64 moments over the planar matches, with and without norm."""
    out = {}
    for key, norm in (("plain", None), ("norm", norm_for(6))):
        scenes = [hm.make_scene(201 + i, n) for i, n in enumerate((20, 65, 500, 1200, 3000, 4097))]
        M = []
        for i, s in enumerate(scenes):
            xl, xr = ec.points32(s["ml"], s["mr"], None if norm is None else norm[i])
            M.append(hm.moments64(xl, xr, s["good"]))
        out[key] = (scenes, np.stack(M), norm)
    return out


@pytest.mark.parametrize("key", ["plain", "norm"])
def test_refit_meets_the_eigen_residual_contract(ops, refit_scenes, key):
    scenes, M, norm = refit_scenes[key]
    bc = [int(s["good"].sum()) for s in scenes]
    out = run_refit(ops, bc, moments=M, **({} if norm is None else {"norm": norm}))
    b64 = max(pc.residual(m, pc.refit64(m)[0]) for m in M)
    worst = 0.0
    for p, (s, m) in enumerate(zip(scenes, M)):
        h = out["H"][p].reshape(9)
        e0, w = pc.refit64(m)
        fro = np.linalg.norm(m)
        r_dev = pc.residual(m, h)
        worst = max(worst, r_dev)
        assert abs(np.linalg.norm(h) - 1) <= 64 * hm.EPS64 and r_dev <= hm.MARGIN * b64
        assert np.array_equal(hm.sign_rule(h), h)
        tol = hm.MARGIN * b64 * hm.EPS64 * fro                            # the residual bounds of a symmetric matrix
        assert h @ m @ h <= w[0] + tol
        eig = out["eig"][p]
        assert eig[0] <= eig[1] and eig[0] >= -tol
        # two backward-stable solvers of one symmetric 9x9: each eigenvalue is exact for M + E, |E| <= c eps64 |M|_F with c a few
        # units per sweep (Weyl) - 64 is that with room, five orders below the gap between the two values
        assert np.abs(eig - w[:2]).max() <= 64 * hm.EPS64 * fro
        if norm is None:
            assert np.array_equal(out["H_px"][p], out["H"][p])
        else:
            want = hm.denormalise(out["H"][p], norm[p])                   # numpy's N_r^-1 H N_l from the kernel's own H
            assert np.abs(out["H_px"][p] - want).max() <= 64 * hm.EPS64
        if bc[p] >= 100:                                                  # ... which is the scene's homography of the stored points
            assert np.abs(out["H_px"][p] - s["H"]).max() < 5e-3
    print("refit (%s): device residual %.2f, numpy's eigh %.2f (x eps64 |M|_F); bound %.0f x" % (key, worst, b64, hm.MARGIN))
    # swapped: P H P of the swapped=0 call with the sign rule
    sw = run_refit(ops, bc, moments=M, swapped=True, **({} if norm is None else {"norm": norm}))
    for p in range(len(scenes)):
        assert np.array_equal(sw["H"][p], hm.swap(out["H"][p])) and np.array_equal(sw["H_px"][p], hm.swap(out["H_px"][p]))
    assert sw["eig"].tobytes() == out["eig"].tobytes()
    assert run_refit(ops, bc, moments=M, **({} if norm is None else {"norm": norm}))["H"].tobytes() == out["H"].tobytes()


def test_refit_without_a_model_writes_zeros_and_the_winning_model_is_promoted(ops, refit_scenes):
    scenes, M, _ = refit_scenes["plain"]
    M = M.copy()
    M[1, 3, 7] = np.nan                                                   # in the upper triangle, which is what is read
    M[2, 0, 0] = np.inf
    bc = [3, 500, 500, 4, 0, -5]
    out = run_refit(ops, bc, moments=M, norm=norm_for(6))
    for p in (0, 1, 2, 4, 5):
        assert not out["H"][p].any() and not out["H_px"][p].any() and not out["eig"][p].any(), p
    assert abs(np.linalg.norm(out["H"][3]) - 1) < 1e-12 and abs(np.linalg.norm(out["H_px"][3]) - 1) < 1e-12
    lower = M.copy()
    lower[3, 8, 0] = np.nan                                               # the lower triangle is not read
    assert run_refit(ops, bc, moments=lower, norm=norm_for(6))["H"][3].tobytes() == out["H"][3].tobytes()
    bad_norm = norm_for(6)
    bad_norm[3, 6] = 0.0                                                  # a zero scale: H stays, H_px has no finite value
    z = run_refit(ops, bc, moments=M, norm=bad_norm)
    assert z["H"][3].tobytes() == out["H"][3].tobytes() and not z["H_px"][3].any()
    # without moments: models[p, best[p]] promoted, eig 0
    models = np.stack([hm.make_case(700 + p, 50, 5)["models"] for p in range(3)])
    models[2] = 0.0
    best = np.array([1, 9, 0], np.int32)                                  # 9 is clamped to H - 1 = 4
    got = run_refit(ops, [10, 10, 10], models=models, best=best)
    assert np.array_equal(got["H"][0], models[0, 1].astype(np.float64)) and np.array_equal(got["H"][1], models[1, 4].astype(np.float64))
    assert not got["H"][2].any() and not got["eig"].any() and np.array_equal(got["H_px"], got["H"])


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------
def _handed_over(ml, mr, lengths):
    """A result dict as the batch path leaves it after group_by_pair, from plain lists."""
    from pats_amd import batch
    pairs = len(lengths)
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([[0], np.cumsum(lengths), [sum(lengths), 0, 0]]).astype(np.int64)          # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    return batch, cap, {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}


def test_hypothesize_verify_refit_end_to_end():
    H, thr = 512, np.float32(2e-3)
    scenes = [hm.make_scene(seed, 600, outliers=0.3) for seed in (11, 12, 13, 14)]
    ml, mr = np.concatenate([s["ml"] for s in scenes]), np.concatenate([s["mr"] for s in scenes])
    batch, cap, out = _handed_over(ml, mr, [600] * 4)
    dthr = cu(np.full(4, thr, np.float32))
    models, idx = batch.hypothesize_h_by_pair(out, cap, H, seed=2024, on="all", progressive=False, samples=True)
    assert out["hypotheses_h"][0] is models and tuple(models.shape) == (4, H, 3, 3) and tuple(idx.shape) == (4, H, 4)
    ver = batch.verify_h_by_pair(out, cap, models, dthr, moments=True)
    assert ver is out["verified_h"] and out["verified_h_on"] == "all" and "verified" not in out and "pose" not in out
    Hd, eig = batch.homography_by_pair(out, cap)
    assert out["homography"][0] is Hd
    again = batch.verify_h_by_pair(out, cap, Hd.float().unsqueeze(1), dthr)            # the refit as an H = 1 model
    idx_h, models_h, best, best_count = idx.cpu().numpy(), models.cpu().numpy(), ver[1].cpu().numpy(), ver[2].cpu().numpy()
    for p, s in enumerate(scenes):
        assert np.array_equal(idx_h[p], hm.sample_idx(2024 + p, 600, H))                # pair_seed = seed + p
        part = ec.participates(s["ml"], s["mr"])
        h64 = hm.sign_rule(hm.null64(hm.rows(s["ml"], s["mr"], idx_h[p])))              # the device's samples, solved on the host
        inl, dec = hm.classify(s["ml"], s["mr"], part, h64.astype(np.float32).reshape(H, 3, 3), thr)
        host_best = int((inl & dec).sum(1).max())
        inl, dec = hm.classify(s["ml"], s["mr"], part, models_h[p, best[p]][None], thr)
        first = int((inl & dec).sum())
        refit32 = Hd[p].float().cpu().numpy()
        inl, dec = hm.classify(s["ml"], s["mr"], part, refit32[None], thr)
        refit = int((inl & dec).sum())
        print("pair %d: %d planar matches, host-solved best %d strict, device best_count %d (strict %d), refit strict %d, count %d; "
              "eig %.3e %.3e" % (p, s["good"].sum(), host_best, best_count[p], first, refit, int(again[2][p]), *eig[p].tolist()))
        assert best_count[p] >= host_best and host_best > 0.5 * s["good"].sum()
        assert refit >= first
        assert np.abs(Hd[p].cpu().numpy() - s["H"]).max() < 5e-3


# ---- 9. both branches and mixed packs -----------------------------------------------------------------------------------------
def test_mixed_pack_follows_the_callers_pair_and_leaves_the_epipolar_branch_alone():
    from pats_amd import batch, ops
    from test_confidence_gpu import _small_batch
    K, H, seed = 50, 37, 31337
    runs = []
    for with_h in (False, True):
        _, cap, out, _ = _small_batch(True)
        norm = np.tile(np.array([160, 120, 1 / 200.0, 1 / 200.0, 160, 120, 1 / 200.0, 1 / 200.0], np.float32), (cap.pairs, 1))
        norm[:, 0] += np.arange(cap.pairs)                                              # distinct per pair: a wrong permutation shows
        dn, thr = cu(norm), cu(np.full(cap.pairs, 0.05, np.float32))
        top = batch.topk_by_pair(out, cap, K)
        e_models = batch.hypothesize_by_pair(out, cap, H, seed=seed, norm=dn)
        if with_h:
            models, idx = batch.hypothesize_h_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)      # on="topk", progressive
        batch.verify_by_pair(out, cap, e_models, thr, norm=dn, on="topk", moments=True)
        if with_h:
            ver = batch.verify_h_by_pair(out, cap, models, thr, norm=dn, on="topk", moments=True)
        batch.pose_by_pair(out, cap, norm=dn, swapped=True)
        if with_h:
            Hd, eig, Hpx = batch.homography_by_pair(out, cap, norm=dn, swapped=True, pixel=True)
        runs.append(out)
    plain, out = runs
    slot = out["caller_of"]
    assert slot != list(range(cap.pairs))
    for i in range(cap.pairs):                                                          # caller's pair i sits in slot s_
        s_ = slot.index(i)
        hand = ops.homography_hypotheses_by_pair(top[0][s_], top[1][s_], H, cu(np.array([seed + i], np.int64)), stride=K,
                                                 counts=top[4][s_:s_ + 1], norm=dn[i:i + 1], progressive=True, return_samples=True)
        assert torch.equal(models[i].view(torch.int32), hand[0][0].view(torch.int32)) and torch.equal(idx[i], hand[1][0])
        assert int(top[4][s_]) >= 4 and bool(models[i].reshape(H, 9).any(1).all())
        hv = ops.homography_score_by_pair(top[0][s_], top[1][s_], models[i:i + 1], thr[i:i + 1], stride=K, counts=top[4][s_:s_ + 1],
                                          norm=dn[i:i + 1], moments=True)
        assert torch.equal(ver[0][s_], hv[0][0]) and torch.equal(ver[1][s_], hv[1][0]) and torch.equal(ver[2][s_], hv[2][0])
        assert torch.equal(ver[3].view(cap.pairs, K)[s_], hv[3]) and torch.equal(ver[4][s_], hv[4][0])
        hr = ops.homography_refit_by_pair(hv[2], moments=hv[4], norm=dn[i:i + 1], swapped=True, return_pixel=True)
        assert torch.equal(Hd[i], hr[0][0]) and torch.equal(eig[i], hr[1][0]) and torch.equal(Hpx[i], hr[2][0])
    assert int(ver[2].min()) >= 4                                                       # a model fits its own four matches
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()          # noqa: E731
    assert set(plain) == set(out) - {"hypotheses_h", "verified_h", "verified_h_on", "verified_h_models", "homography"}
    assert all(same(a, b) for a, b in zip(out["verified"], plain["verified"])) and all(same(a, b) for a, b in zip(out["pose"], plain["pose"]))
    assert same(out["hypotheses"], plain["hypotheses"]) and all(same(a, b) for a, b in zip(out["topk"], plain["topk"]))


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    from pats_amd import _lib, batch
    lib = _lib.lib()
    live = torch.zeros(4096, dtype=torch.float32, device="cuda")                        # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    for which in sorted(hm.ENTRY):
        assert hm.check_refusals(lib, which, base) > 20
    torch.cuda.synchronize()
    assert not live.any()                                                               # nothing ran: nothing was written
    ml = torch.zeros((20, 2), device="cuda")
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 10, 20], device="cuda")
    models, thr = torch.zeros((2, 4, 3, 3), device="cuda"), torch.zeros(2, device="cuda")
    bc, mom = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((2, 9, 9), dtype=torch.float64, device="cuda")
    for kw, word in (({"H": 0}, "H = 0"), ({"H": ops.epipolar_max_h() + 1}, "H ="), ({"norm": torch.zeros((3, 8), device="cuda")}, "norm"),
                     ({"out": torch.zeros((2, 4, 3, 3), device="cuda").double()}, "models"),
                     ({"out": (torch.zeros((2, 4, 3, 3), device="cuda"),), "return_samples": True}, "out must be")):
        with pytest.raises(RuntimeError, match=word):
            ops.homography_hypotheses_by_pair(ml, ml, kw.pop("H", 4), seed, pair_off=off, **kw)
    with pytest.raises(RuntimeError, match="seed must hold one int64 per pair"):
        ops.homography_hypotheses_by_pair(ml, ml, 4, seed[:1], pair_off=off)
    with pytest.raises(RuntimeError, match="models must be \\[pairs,H,3,3\\]"):
        ops.homography_score_by_pair(ml, ml, models[0], thr, pair_off=off)
    with pytest.raises(RuntimeError, match="must hold 2 pairs"):
        ops.homography_score_by_pair(ml, ml, models, thr[:1], pair_off=off)
    with pytest.raises(RuntimeError, match="conf must be \\[cap\\]"):
        ops.homography_score_by_pair(ml, ml, models, thr, pair_off=off, conf=thr, min_conf=0.1)
    with pytest.raises(RuntimeError, match="min_conf"):
        ops.homography_score_by_pair(ml, ml, models, thr, pair_off=off, conf=torch.zeros(20, device="cuda"), min_conf=-0.5)
    with pytest.raises(RuntimeError, match="moments must be \\[pairs,9,9\\]"):
        ops.homography_refit_by_pair(bc, moments=mom[:1])
    with pytest.raises(RuntimeError, match="norm must be \\[pairs,8\\]"):
        ops.homography_refit_by_pair(bc, moments=mom, norm=torch.zeros((3, 8), device="cuda"))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.homography_refit_by_pair(bc, moments=mom, out=(mom,))
    _, cap, out = _handed_over(np.zeros((20, 2), np.float32), np.zeros((20, 2), np.float32), [10, 10])
    with pytest.raises(ValueError, match="verify_h_by_pair"):
        batch.homography_by_pair(out, cap)
    with pytest.raises(ValueError, match="topk_by_pair"):
        batch.hypothesize_h_by_pair(out, cap, 8)
    with pytest.raises(ValueError, match="on must be"):
        batch.verify_h_by_pair(out, cap, models, thr, on="best")
    with pytest.raises(ValueError, match="confidence=True"):
        batch.verify_h_by_pair(out, cap, models, thr, min_conf=0.3)
    assert set(out) == {"matches_l", "matches_r", "by_pair", "summary"}
