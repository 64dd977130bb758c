"""GPU: ops.epipolar_score_by_pair / batch.verify_by_pair against the definition of include/pats_amd.h restated in float64 numpy
(tests/epipolar_cases.py).  The kernel evaluates the test in float32, so a verdict is compared on DECIDED cells only (the float64
r^2 outside the relative band DELTA around thr^2 den; tests/test_epipolar_cases_host.py shows that float32 agrees there and that
the band holds far less than 1 % of the cells):
    strict <= counts <= loose for every model (strict = decided inliers, loose = strict + undecided cells)
    inlier == the float64 verdict on every decided cell of the best model, 0 outside the segments
    best == the float64 argmax where that is separated from the runner-up by more than the undecided cells of both; always the
            lowest index of the largest returned count, and best_count / the mask's population agree with counts[best]
Every output lies inside a larger sentinel-filled buffer: the call must define every byte of the views and none around them."""
import os
import re

import numpy as np
import pytest
import torch

import epipolar_cases as ec
from conftest import REPO

pytestmark = pytest.mark.gpu

PAD = 64
SENT = {torch.int32: -123456, torch.int64: -123456, torch.uint8: 0xA5, torch.float64: -777.25}


def _kernel_constant(name):
    src = open(os.path.join(REPO, "pats_amd", "csrc", "epipolar.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


T = _kernel_constant("EPI_THREADS") * _kernel_constant("EPI_R")        # matches per workgroup
C = _kernel_constant("EPI_CHUNK")                                      # models per workgroup


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def sentinel_outputs(pairs, H, cap, moments):
    shapes = [((pairs, H), torch.int32), ((pairs,), torch.int32), ((pairs,), torch.int64), ((cap,), torch.uint8)]
    if moments:
        shapes.append(((pairs, 9, 9), torch.float64))
    views, whole = [], []
    for shape, dt in shapes:
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENT[dt], dtype=dt, device="cuda")
        whole.append(buf)
        views.append(buf[PAD:PAD + n].view(shape))
    return tuple(views), whole


def run(ops, ml, mr, models, thr, moments=False, **kw):
    """One call on fresh sentinel buffers -> the outputs as numpy arrays (the surroundings checked)."""
    d = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs, H = models.shape[0], models.shape[1]
    views, whole = sentinel_outputs(pairs, H, ml.shape[0], moments)
    got = ops.epipolar_score_by_pair(torch.from_numpy(ml).cuda(), torch.from_numpy(mr).cuda(), torch.from_numpy(models).cuda(),
                                     torch.from_numpy(np.asarray(thr, np.float32)).cuda(), moments=moments, out=views, **d)
    torch.cuda.synchronize()
    assert len(got) == (5 if moments else 4) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    for buf in whole:
        edge = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
        assert bool((edge == SENT[buf.dtype]).all()), "bytes around an output view changed"
    return [v.cpu().numpy() for v in views]


def check(got, ref, segs, cap, true=None):
    """The four outputs against the float64 reference of every pair (see the module docstring)."""
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
        exact = r["inl"].sum(1)
        order = np.argsort(-exact, kind="stable")
        if len(order) == 1 or exact[order[0]] - exact[order[1]] > (~r["decided"][order[0]]).sum() + (~r["decided"][order[1]]).sum():
            top = exact[order[0]]
            if (exact == top).sum() == 1 and top > 0:
                assert b == order[0], "pair %d: best %d, float64 says %d" % (p, b, order[0])
        if true is not None and true[p] is not None:
            assert b == true[p]
    assert not inlier[~covered].any(), "a row outside every segment is set"


def build(lengths, H, seed, tail=29, thr=2e-3):
    """Pairs made by the generator, concatenated; behind the last segment `tail` rows that WOULD be inliers of the last pair."""
    cases = [ec.make_case(seed + 17 * p, max(n, 1), H, thr=thr) for p, n in enumerate(lengths)]
    ml = np.concatenate([c["ml"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 2), np.float32)])
    mr = np.concatenate([c["mr"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 2), np.float32)])
    extra = ec.make_case(seed + 17 * (len(lengths) - 1), tail, H, outliers=0.0, thr=thr)
    ml, mr = np.concatenate([ml, extra["ml"]]), np.concatenate([mr, extra["mr"]])
    models = np.stack([c["models"] for c in cases])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    true = [c["true"] if n >= 64 else None for c, n in zip(cases, lengths)]
    return ml, mr, models, np.full(len(lengths), thr, np.float32), off, true


def run_and_check(ops, lengths, H, seed, **kw):
    ml, mr, models, thr, off, true = build(lengths, H, seed)
    got = run(ops, ml, mr, models, thr, pair_off=off, **kw)
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    check(got, ec.reference(ml, mr, segs, models, thr), segs, ml.shape[0], true)
    return got


# ---- 1. counts ----------------------------------------------------------------------------------------------------------------
def test_counts_mask_and_best_against_float64(ops):
    run_and_check(ops, [3000, 700, 2 * T + 300], 96, seed=1000)


# ---- 2. edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [[0], [1], [2 * T + 1], [1, 0, 63], [64, 0, 65], [T - 1, 0, T], [T + 1, 0, 2 * T + 1]])
def test_segment_lengths_around_the_wave_and_the_workgroup(ops, lengths):
    run_and_check(ops, lengths, 5, seed=2000 + sum(lengths))


@pytest.mark.parametrize("H", [1, 2, C - 1, C, C + 1])
def test_model_counts_around_the_chunk(ops, H):
    run_and_check(ops, [300, 0, T + 7], H, seed=3000 + H)


def test_both_segment_forms_agree(ops):
    S = T + 40
    ml, mr, models, thr, off, true = build([S, S, 777], 40, seed=4000, tail=S - 777)
    assert ml.shape[0] == 3 * S
    ragged = run(ops, ml, mr, models, thr, pair_off=off)
    strided = run(ops, ml, mr, models, thr, stride=S, counts=np.array([S, S, 777], np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(ragged, strided))
    segs = ec.segments(3, 3 * S, stride=S, counts=[S, S, 777])
    check(strided, ec.reference(ml, mr, segs, models, thr), segs, 3 * S, true)


def test_corrupt_offsets_and_counts_stay_inside_the_arrays(ops):
    ml, mr, models, thr, off, _ = build([400, 400, 400], 12, seed=5000)
    cap = ml.shape[0]
    for bad in (np.array([-50, 700, 300, cap + 100000], np.int64),                         # past cap, negative, descending (disjoint)
                np.array([cap + 5, cap + 9, 2 ** 40, -2 ** 40], np.int64)):
        got = run(ops, ml, mr, models, thr, pair_off=bad)
        segs = ec.segments(3, cap, pair_off=bad)
        if bad[0] < 0:                                                                     # pairs 0 and 2 overlap on rows 300 .. 700:
            ref = ec.reference(ml, mr, segs, models, thr)                                  # the counts are defined, the shared rows' mask
            for p in range(3):                                                             # is that of one of the two pairs
                assert (ref[p]["strict"] <= got[0][p]).all() and (got[0][p] <= ref[p]["loose"]).all()
                assert got[1][p] == np.argmax(got[0][p]) and got[2][p] == got[0][p, got[1][p]]
            assert got[2][1] == 0 and set(np.unique(got[3])) <= {0, 1}
        else:
            check(got, ec.reference(ml, mr, segs, models, thr), segs, cap)
            assert not got[0].any() and not got[3].any()
    stride = 410
    counts = np.array([-7, stride + 1000, 2 ** 40], np.int64)
    ml2, mr2 = np.concatenate([ml, ml])[:3 * stride + 11], np.concatenate([mr, mr])[:3 * stride + 11]
    got = run(ops, ml2, mr2, models, thr, stride=stride, counts=counts)
    segs = ec.segments(3, ml2.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 0), (stride, stride), (2 * stride, stride)]
    check(got, ec.reference(ml2, mr2, segs, models, thr), segs, ml2.shape[0])


def test_empty_arrays_define_every_output(ops):
    """cap == 0: every pair empty, the outputs still defined."""
    z2 = np.zeros((0, 2), np.float32)
    models = ec.make_case(1, 1, 7)["models"][None].repeat(2, 0)
    got = run(ops, z2, z2, models, [1e-3, 1e-3], moments=True, pair_off=np.zeros(3, np.int64))
    assert not got[0].any() and not got[1].any() and not got[2].any() and got[3].shape == (0,) and not got[4].any()


# ---- 3. ties, padding, bad values ---------------------------------------------------------------------------------------------
def test_ties_zero_models_and_bad_thresholds(ops):
    ml, mr, models, thr, off, true = build([900, 900, 900], 10, seed=6000)
    for p in range(3):                                       # the true model twice: the lower index wins; zero models in between
        E = models[p, true[p]].copy()
        models[p, [true[p], 0, 4, 9]] = 0.0
        models[p, 2], models[p, 7] = E, E
    got = run_and_check_arrays(ops, ml, mr, models, thr, off)
    assert got[1].tolist() == [2, 2, 2] and (got[0][:, 2] == got[0][:, 7]).all() and not got[0][:, [0, 4, 9]].any()
    # every model zero: best 0, count 0, empty mask
    got = run(ops, ml, mr, np.zeros_like(models), thr, pair_off=off, moments=True)
    assert not got[0].any() and got[1].tolist() == [0, 0, 0] and got[2].tolist() == [0, 0, 0] and not got[3].any() and not got[4].any()
    # thr NaN / negative: zero inliers for that pair only
    base = run(ops, ml, mr, models, thr, pair_off=off, moments=True)
    for bad in (np.nan, -1e-3, -np.inf):
        t2 = thr.copy()
        t2[1] = bad
        got = run(ops, ml, mr, models, t2, pair_off=off, moments=True)
        assert not got[0][1].any() and got[1][1] == 0 and got[2][1] == 0 and not got[3][900:1800].any() and not got[4][1].any()
        for p in (0, 2):
            assert np.array_equal(got[0][p], base[0][p]) and got[1][p] == base[1][p] and np.array_equal(got[4][p], base[4][p])
        assert np.array_equal(got[3][:900], base[3][:900]) and np.array_equal(got[3][1800:], base[3][1800:])


def run_and_check_arrays(ops, ml, mr, models, thr, off, **kw):
    got = run(ops, ml, mr, models, thr, pair_off=off, **kw)
    segs = ec.segments(len(off) - 1, ml.shape[0], pair_off=off)
    check(got, ec.reference(ml, mr, segs, models, thr, **{k: v for k, v in kw.items() if k in ("norm", "conf", "min_conf")}), segs,
          ml.shape[0])
    return got


def test_non_finite_coordinates_are_not_inliers_and_hurt_nobody(ops):
    ml, mr, models, thr, off, true = build([1500, 300], 8, seed=7000)
    base = run(ops, ml, mr, models, thr, pair_off=off)
    inl = np.flatnonzero(base[3][:1500])
    assert len(inl) > 100
    hit = inl[:8]
    ml2, mr2 = ml.copy(), mr.copy()
    ml2[hit[0], 0], ml2[hit[1], 1], mr2[hit[2], 0], mr2[hit[3], 1] = np.nan, np.inf, -np.inf, np.nan
    ml2[hit[4]], mr2[hit[5]] = np.inf, np.nan
    got = run_and_check_arrays(ops, ml2, mr2, models, thr, off)
    assert not got[3][hit[:6]].any() and got[2][0] == base[2][0] - 6
    keep = np.ones(ml.shape[0], bool)
    keep[hit[:6]] = False
    assert np.array_equal(got[3][keep], base[3][keep]) and np.array_equal(got[0][1], base[0][1])


# ---- 4. gate ------------------------------------------------------------------------------------------------------------------
def test_confidence_gate(ops):
    ml, mr, models, thr, off, true = build([1200, 0, T + 100], 6, seed=8000)
    rng = np.random.default_rng(8)
    conf = rng.random(ml.shape[0]).astype(np.float32)
    conf[rng.random(ml.shape[0]) < 0.2] = np.float32(0.5)             # a fifth of the matches sit exactly on the threshold
    conf[::37] = np.nan
    got = run_and_check_arrays(ops, ml, mr, models, thr, off, conf=conf, min_conf=0.5)
    free = run(ops, ml, mr, models, thr, pair_off=off)
    on_edge = np.flatnonzero((conf == np.float32(0.5)) & (free[3] == 1))
    assert len(on_edge) > 50 and got[3][on_edge].all()                # inclusive
    nan = np.flatnonzero(np.isnan(conf) & (free[3] == 1))
    assert len(nan) > 5 and not got[3][nan].any()                     # a NaN confidence takes no part
    below = np.flatnonzero(conf < 0.5)
    assert not got[3][below].any()
    assert np.array_equal(got[3] == 1, (free[3] == 1) & (conf >= 0.5))
    same = run(ops, ml, mr, models, thr, pair_off=off, conf=conf)     # conf without a threshold: not read
    assert all(np.array_equal(a, b) for a, b in zip(same, free))
    with pytest.raises(RuntimeError, match="min_conf needs conf"):
        run(ops, ml, mr, models, thr, pair_off=off, min_conf=0.5)
    for bad in (float("nan"), -0.5):
        with pytest.raises(RuntimeError, match="min_conf"):
            run(ops, ml, mr, models, thr, pair_off=off, conf=conf, min_conf=bad)


# ---- 5. norm ------------------------------------------------------------------------------------------------------------------
def test_norm_equals_prenormalised_inputs_bit_for_bit(ops):
    ml, mr, models, thr, off, true = build([1000, T + 9], 20, seed=9000)
    rng = np.random.default_rng(9)
    norm = np.stack([np.array([511.7, 383.9, 1 / 701.3, 1 / 699.1, 498.2, 377.4, 1 / 688.8, 1 / 690.5]) * rng.uniform(0.9, 1.1, 8)
                     for _ in range(2)]).astype(np.float32)
    pl, pr = ml.copy(), mr.copy()                                     # pixels whose normalisation lands near the generator's points
    segs = ec.segments(2, ml.shape[0], pair_off=off)
    for p, (lo, n) in enumerate(segs):
        pl[lo:lo + n] = ml[lo:lo + n] / norm[p, 2:4] + norm[p, 0:2]
        pr[lo:lo + n] = mr[lo:lo + n] / norm[p, 6:8] + norm[p, 4:6]
    with_norm = run_and_check_arrays(ops, pl, pr, models, thr, off, norm=norm)
    xl, xr = pl.copy(), pr.copy()
    for p, (lo, n) in enumerate(segs):
        xl[lo:lo + n], xr[lo:lo + n] = ec.points32(pl[lo:lo + n], pr[lo:lo + n], norm[p])
    pre = run(ops, xl, xr, models, thr, pair_off=off)
    assert all(np.array_equal(a, b) for a, b in zip(with_norm[:4], pre[:4]))
    assert with_norm[1].tolist() == true


# ---- 6. moments ---------------------------------------------------------------------------------------------------------------
def test_moments_against_float64_over_the_returned_mask(ops):
    ml, mr, models, thr, off, true = build([1700, 0, 2 * T + 50], 9, seed=10000)
    got = run(ops, ml, mr, models, thr, pair_off=off, moments=True)
    again = run(ops, ml, mr, models, thr, pair_off=off, moments=True)
    assert all(np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
               for a, b in zip(got, again))
    segs = ec.segments(3, ml.shape[0], pair_off=off)
    for p, (lo, n) in enumerate(segs):
        mask = got[3][lo:lo + n].astype(bool)
        want, mag = ec.moments64(ml[lo:lo + n], mr[lo:lo + n], mask)
        bound = mask.sum() * 2.0 ** -52 * mag                          # two summation orders of the same float64 terms, nothing wider
        assert (np.abs(got[4][p] - want) <= bound).all(), p
        assert np.array_equal(got[4][p], got[4][p].T)
        if n:
            assert got[4][p][8, 8] == mask.sum() and mask.sum() > 100
            w, v = np.linalg.eigh(got[4][p])                           # the refit: the null vector is the true model up to sign
            e = v[:, 0].reshape(3, 3)
            assert min(np.abs(e - models[p, true[p]]).max(), np.abs(e + models[p, true[p]]).max()) < 2e-2
    assert not got[4][1].any()
    assert len(ops.epipolar_score_by_pair(*[torch.from_numpy(x).cuda() for x in (ml, mr, models, thr)],
                                          pair_off=torch.from_numpy(off).cuda())) == 4      # moments=False: no fifth buffer


# ---- 7. every byte of the outputs ---------------------------------------------------------------------------------------------
def test_every_output_byte_is_defined_slack_and_tail_included(ops):
    stride = 300
    counts = np.array([250, 0, 300, 17], np.int64)
    cases = [ec.make_case(11000 + p, stride, 3, outliers=0.0) for p in range(4)]           # every row WOULD be an inlier
    ml = np.concatenate([c["ml"] for c in cases] + [cases[3]["ml"][:41]])
    mr = np.concatenate([c["mr"] for c in cases] + [cases[3]["mr"][:41]])
    models = np.stack([c["models"] for c in cases])
    thr = np.full(4, 2e-3, np.float32)
    got = run(ops, ml, mr, models, thr, stride=stride, counts=counts, moments=True)         # sentinel-filled before the call (run)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    check(got, ec.reference(ml, mr, segs, models, thr), segs, ml.shape[0], [c["true"] for c in cases[:1]] + [None, cases[2]["true"], None])
    assert got[3][:250].sum() > 200 and not got[3][250:600].any() and not got[3][900 + 17:].any()
    assert np.isfinite(got[4]).all() and not got[4][1].any()


# ---- 8. through the batch path ------------------------------------------------------------------------------------------------
def _models_for(lists, H, seed):
    """Hypotheses in the caller's order: a model fitted to nothing in particular - random unit matrices, distinct per pair."""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(len(lists), H, 3, 3))
    m /= np.linalg.norm(m.reshape(len(lists), H, 9), axis=2)[:, :, None, None]
    return m.astype(np.float32)


@pytest.mark.parametrize("mixed", [False, True])
def test_through_the_batch_path(mixed, ops):
    from pats_amd import batch
    from test_confidence_gpu import _small_batch
    _, cap, out, _ = _small_batch(mixed)
    _, _, ref_out, _ = _small_batch(mixed)                   # a second, identical step that is never verified
    lists = batch.split_by_pair(ref_out, cap)                # caller's order
    K, H = 50, 37
    models = _models_for(lists, H, 12000)
    # image coordinates: centre and scale them, and use a threshold that leaves every random model a few inliers
    norm = np.tile(np.array([160, 120, 1 / 200.0, 1 / 200.0, 160, 120, 1 / 200.0, 1 / 200.0], np.float32), (cap.pairs, 1))
    thr = np.linspace(0.05, 0.08, cap.pairs).astype(np.float32)
    dm, dt, dn = (torch.from_numpy(x).cuda() for x in (models, thr, norm))
    top = batch.topk_by_pair(out, cap, K)
    ref_top = batch.topk_by_pair(ref_out, cap, K)
    keep = {k: out[k].clone() for k in ("matches_l", "matches_r", "match_conf")}
    before = [t.clone() for t in list(out["topk"]) + list(out["by_pair"])]
    slot = out.get("caller_of", list(range(cap.pairs)))
    sm, st, sn = dm[slot], dt[slot], dn[slot]                # by hand: slot order
    for on in ("all", "topk"):
        ver = batch.verify_by_pair(out, cap, dm, dt, norm=dn, on=on, moments=True, min_conf=0.3 if on == "topk" else None)
        assert ver is out["verified"] and len(ver) == 5
        if on == "all":
            hand = ops.epipolar_score_by_pair(out["by_pair"][0], out["by_pair"][1], sm, st, pair_off=out["summary"], norm=sn, moments=True,
                                              pairs=cap.pairs)
        else:
            hand = ops.epipolar_score_by_pair(top[0], top[1], sm, st, stride=K, counts=top[4], conf=top[2], min_conf=0.3, norm=sn,
                                              moments=True)
        assert all(torch.equal(a, b) for a, b in zip(ver, hand))
        assert on == "topk" or int(ver[2].min()) > 0
        copies = []
        real_cpu = torch.Tensor.cpu
        torch.Tensor.cpu = lambda self, *a, **k: (copies.append(self.numel()), real_cpu(self, *a, **k))[1]
        try:
            per = batch.split_verified_by_pair(out, cap)
        finally:
            torch.Tensor.cpu = real_cpu
        assert copies == [2 * cap.pairs + 4 if on == "topk" else cap.pairs + 4]              # ONE device-to-host copy
        for i, (l, r, m, b, bc) in enumerate(per):                                          # caller's order
            s_ = slot.index(i)
            if on == "all":
                assert torch.equal(l, lists[i][0]) and torch.equal(r, lists[i][1])
                conf, gate = None, None
            else:
                c = int(top[4][s_])
                assert torch.equal(l, top[0][s_, :c]) and l.shape[0] == min(K, lists[i][0].shape[0])
                conf, gate = top[2][s_, :c].cpu().numpy(), 0.3
            assert m.dtype == torch.bool and m.shape[0] == l.shape[0] and int(m.sum()) == int(bc) and int(b) == int(ver[1][s_])
            seg = [(0, l.shape[0])]
            ref = ec.reference(l.cpu().numpy(), r.cpu().numpy(), seg, models[i:i + 1], thr[i:i + 1], norm=norm[i:i + 1], conf=conf,
                               min_conf=gate)
            got = [ver[0][s_:s_ + 1].cpu().numpy(), ver[1][s_:s_ + 1].cpu().numpy(), ver[2][s_:s_ + 1].cpu().numpy(),
                   m.cpu().numpy().astype(np.uint8)]
            check(got, ref, seg, l.shape[0])
    if mixed:
        assert slot != list(range(cap.pairs))
    # the matches and the top-K of the same step are bit-identical with and without verification
    assert all(torch.equal(keep[k].view(torch.int32), out[k].view(torch.int32)) for k in keep)
    M = int(out["summary"][cap.pairs])                                       # the lists hold M rows; the rows behind are never written
    assert M == int(ref_out["summary"][cap.pairs]) > 100
    assert all(torch.equal(out[k][:M].view(torch.int32), ref_out[k][:M].view(torch.int32)) for k in keep)
    same = lambda a, b: torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)  # noqa: E731
    assert all(same(a, b) for a, b in zip(list(out["topk"]) + list(out["by_pair"]), before))
    assert all(same(a, b) for a, b in zip(out["topk"], ref_top))             # against the step that was never verified
    assert all(same(a[:M], b[:M]) for a, b in zip(out["by_pair"][:2] + out["by_pair"][3:], ref_out["by_pair"][:2] + ref_out["by_pair"][3:]))
    assert torch.equal(out["summary"], ref_out["summary"])
