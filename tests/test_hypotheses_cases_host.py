"""CPU-only: the numpy restatement of the per-pair hypothesis generator (tests/hypotheses_cases.py).  The sampler: distinct indices
inside the pool, repeatable, the progressive pool's bounds, coverage, both forms of the definition agree, and literal rows pinned
once from the definition so that the restatement cannot drift with the kernel.  The baseline b32: the backward error numpy's
float32 svd reaches on the GPU test's tolerance cases - printed, and only required to be finite (the GPU test holds the kernel to
MARGIN * b32; docs/parity.md records the values)."""
import numpy as np
import pytest

import hypotheses_cases as hc


@pytest.mark.parametrize("n,H,progressive", [(8, 64, False), (9, 65, True), (16, 300, True), (600, 257, False), (600, 257, True),
                                             (2048, 1024, True), (100000, 50, True)])
def test_draws_are_distinct_inside_the_pool_and_repeatable(n, H, progressive):
    idx = hc.sample_idx(77 + n, n, H, progressive)
    assert idx.dtype == np.int32 and idx.shape == (H, 8)
    m = hc.pool(n, H, progressive)
    assert (idx >= 0).all() and (idx < m[:, None]).all() and (m <= n).all() and (m >= 8).all()
    assert all(len(set(row)) == 8 for row in idx.tolist())
    assert np.array_equal(idx, hc.sample_idx(77 + n, n, H, progressive))
    assert not np.array_equal(idx, hc.sample_idx(78 + n, n, H, progressive))
    for h in (0, H // 2, H - 1):                                          # the two forms of the definition
        assert idx[h].tolist() == hc.sample_idx_slow(77 + n, h, int(m[h]))


def test_fewer_than_eight_matches_have_no_sample():
    for n in (0, 1, 7):
        assert (hc.sample_idx(5, n, 9, True) == -1).all()


def test_progressive_pool_bounds():
    for n, H in ((8, 8), (16, 16), (600, 600), (600, 4096), (2048, 4096)):
        m = hc.pool(n, H, True)
        assert m[0] == 8 and m[-1] == n and (np.diff(m) >= 0).all()       # H >= n >= 8: the first pool is the minimum
    m = hc.pool(2048, 1024, True)
    assert m[0] == 8 and m[3] == 8 and m[4] == 10 and m[-1] == 2048       # ceil(2048 (h + 1) / 1024) = 2 (h + 1)
    assert (hc.pool(600, 77, False) == 600).all()


def test_every_index_is_hit():
    idx = hc.sample_idx(2024, 16, 4096)
    assert set(idx.reshape(-1).tolist()) == set(range(16))
    assert np.bincount(idx.reshape(-1), minlength=16).min() > 4096 * 8 // 16 // 2
    assert (np.bincount(idx[:, 0], minlength=16) > 0).all() and (np.bincount(idx[:, 7], minlength=16) > 0).all()


def test_pinned_rows():
    """Computed once from the definition's first form (pop the j-th remaining index) with Python integers."""
    assert hc.sample_idx(0x0123456789ABCDEF, 600, 16)[5].tolist() == [422, 343, 272, 389, 436, 191, 89, 30]
    assert hc.sample_idx(-7, 8, 3)[0].tolist() == [5, 7, 4, 1, 3, 6, 2, 0]                      # a negative seed: its 64 bits
    assert hc.sample_idx(42, 600, 200, True)[2].tolist() == [2, 1, 7, 4, 5, 3, 6, 0]            # progressive: m_2 = 9
    x = 1                                                                                     # mix(1) step by step
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(hc.mix(np.uint64(1))) == x


def test_constraint_rows_and_float64_null_vectors():
    xl, xr, idx, A = hc.tolerance_cases()[0]
    h, t = 13, 5
    i = idx[h, t]
    want = np.outer(np.append(xr[i].astype(np.float64), 1.0), np.append(xl[i].astype(np.float64), 1.0)).reshape(9)
    assert np.array_equal(A[h, t], want)
    e = hc.null64(A)
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-12
    assert hc.ratio(A, e).max() < 1e-6                                    # float64: nine orders below float32's eps


def test_baseline_b32_is_finite():
    b32 = hc.baseline32()
    print("b32 = %.4f over %d samples -> B = %.1f * b32 = %.4f" % (b32, sum(c[2] for c in hc.TOLERANCE_CASES), hc.MARGIN, hc.MARGIN * b32))
    assert np.isfinite(b32) and b32 > 0


def test_check_models_accepts_float64_vectors_and_refuses_broken_ones():
    ml, mr, off = hc.make_pairs([7, 40], seed=5)
    segs = [(0, 7), (7, 40)]
    ref = hc.reference(ml, mr, segs, [3, 4], 11)
    assert ref[0]["A"] is None and not ref[0]["finite"].any() and ref[1]["finite"].all()
    e = hc.null64(ref[1]["A"])
    e *= np.sign(e[np.arange(11), np.argmax(np.abs(e), axis=1)])[:, None]
    models = np.zeros((2, 11, 3, 3), np.float32)
    models[1] = e.reshape(11, 3, 3)
    assert hc.check_models(models, ref, B=1.0) < 1.0                      # float64 vectors rounded to float32: within one eps32
    bad = models.copy()
    bad[1, 3] *= -1
    with pytest.raises(AssertionError, match="sign"):
        hc.check_models(bad, ref)
    bad = models.copy()
    bad[1, 3, 2, 2] += 0.25
    with pytest.raises(AssertionError):
        hc.check_models(bad, ref, B=10.0)
    bad = models.copy()
    bad[0, 0, 0, 0] = 1.0
    with pytest.raises(AssertionError, match="must be zero"):
        hc.check_models(bad, ref)
