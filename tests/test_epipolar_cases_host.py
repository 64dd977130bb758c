"""CPU-only: the numpy restatement of the per-pair model verification (tests/epipolar_cases.py) on its committed seeds.  With the
relative band DELTA around thr^2 den, (1) the undecided cells are at most 1 % of all cells in every case and (2) a float32
evaluation of the same formula agrees with the float64 one on every decided cell - so the GPU test may hold the float32 kernel to
the float64 verdict on decided cells.  docs/parity.md records DELTA and the measured shares."""
import numpy as np
import pytest

import epipolar_cases as ec


@pytest.mark.parametrize("seed,n,H", ec.HOST_CASES)
def test_undecided_share_and_float32_agreement(seed, n, H):
    c = ec.make_case(seed, n, H)
    xl, xr = ec.points32(c["ml"], c["mr"])
    part = ec.participates(xl, xr)
    inl, dec = ec.classify(xl, xr, part, c["models"], c["thr"])
    f32 = ec.emulate32(xl, xr, part, c["models"], c["thr"])
    share = 1.0 - dec.mean()
    differ = int((f32 != inl).sum())
    print("seed %d: %d x %d cells, undecided share %.3e, float32 differs on %d cells (%d of them decided), true model %d inliers"
          % (seed, H, n, share, differ, int(((f32 != inl) & dec).sum()), int(inl[c["true"]].sum())))
    assert share <= 0.01
    assert np.array_equal(f32[dec], inl[dec])
    # the generator's promise to the GPU test: the true model wins by a wide margin
    counts = inl.sum(1)
    assert counts.argmax() == c["true"] and counts[c["true"]] > 2 * np.partition(counts, -2)[-2] + 10


def test_normalisation_is_one_subtract_and_one_multiply():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1000, (100, 2)).astype(np.float32)
    norm = np.array([512.25, 384.5, 1 / 700.0, 1 / 710.0], np.float32)
    got = ec.normalise32(pts, norm)
    want = np.stack([(pts[:, 0] - norm[0]) * norm[2], (pts[:, 1] - norm[1]) * norm[3]], 1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))


def test_rules_that_do_not_depend_on_rounding():
    c = ec.make_case(7, 200, 4)
    xl, xr = ec.points32(c["ml"], c["mr"])
    conf = np.linspace(0, 1, 200).astype(np.float32)
    conf[3] = np.nan
    part = ec.participates(xl, xr, conf, 0.5)
    assert not part[3] and part[conf >= 0.5].all() and not part[conf < 0.5].any()
    models = c["models"].copy()
    models[1] = 0                                                                 # a zero model: den = 0, decided, no inliers
    for thr in (np.nan, -1.0):
        inl, dec = ec.classify(xl, xr, part, models, thr)
        assert not inl.any() and dec.all()
    inl, dec = ec.classify(xl, xr, part, models, c["thr"])
    assert not inl[1].any() and dec[1].all() and not inl[:, ~part].any() and dec[:, ~part].all()
    xl2 = xl.copy()
    xl2[5, 0], xl2[6, 1] = np.inf, np.nan
    part2 = ec.participates(xl2, xr)
    assert not part2[5] and not part2[6] and part2.sum() == 198
    assert ec.segments(3, 100, pair_off=[-5, 40, 30, 1000]) == [(0, 40), (40, 0), (30, 70)]
    assert ec.segments(3, 100, stride=10, counts=[-2, 4, 99]) == [(0, 0), (10, 4), (20, 10)]
