"""CPU-only: the numpy restatement of the per-pair 5-point hypotheses (tests/essential5_cases.py).  The five-draw sampler: both
forms of the definition agree, literal rows pinned once from the definition's first form (list.pop) so that the restatement cannot
drift with the kernel.  The float64 solver: its models are solutions (all three residuals at float64 level), the true essential
matrix of the exact cases is among them in at least 99 % of the samples, and the baselines b_epi, b_ess - its models rounded to
float32 - that the GPU test's bounds are MARGIN times of (docs/parity.md records the values)."""
import numpy as np
import pytest

import essential5_cases as e5


@pytest.mark.parametrize("n,H,progressive", [(5, 64, False), (6, 65, True), (16, 300, True), (600, 257, False), (600, 257, True),
                                             (2048, 1024, True), (100000, 50, True)])
def test_draws_are_distinct_inside_the_pool_and_both_forms_agree(n, H, progressive):
    idx = e5.sample_idx(77 + n, n, H, progressive)
    assert idx.dtype == np.int32 and idx.shape == (H, 5)
    m = e5.pool(n, H, progressive)
    assert (idx >= 0).all() and (idx < m[:, None]).all() and (m <= n).all() and (m >= 5).all()
    assert all(len(set(row)) == 5 for row in idx.tolist())
    assert np.array_equal(idx, e5.sample_idx(77 + n, n, H, progressive))
    for h in (0, H // 2, H - 1):                                          # the two forms of the definition
        assert idx[h].tolist() == e5.sample_idx_slow(77 + n, h, int(m[h]))


def test_fewer_than_five_matches_have_no_sample():
    for n in (0, 1, 4):
        assert (e5.sample_idx(5, n, 9, True) == -1).all()


def test_pinned_rows():
    """Computed once from the definition's first form (pop the j-th remaining index) with Python integers.  The draws of a sample
    are the first five of the 8-point sampler's whenever the pools agree: one generator, two draw counts."""
    import hypotheses_cases as hc
    assert e5.sample_idx(0x0123456789ABCDEF, 600, 16)[5].tolist() == [422, 343, 272, 389, 436]
    assert e5.sample_idx(-7, 5, 3)[0].tolist() == e5.sample_idx_slow(-7, 0, 5) == [3, 4, 2, 0, 1]
    assert e5.sample_idx(42, 600, 200, True)[2].tolist() == e5.sample_idx_slow(42, 2, 9) == [2, 1, 7, 4, 5]
    assert np.array_equal(e5.sample_idx(99, 600, 40), hc.sample_idx(99, 600, 40)[:, :5])


def test_the_float64_solver_returns_solutions():
    c = e5.cases(True)[0]
    k = np.array([e.shape[0] for e in c["host"]])
    e = np.concatenate(c["host"])
    assert k.max() <= 10 and k.min() >= 0 and (k % 2 == 0).mean() > 0.99       # real roots come in pairs
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-12
    assert np.median(e5.epi_ratio(np.repeat(c["A"], k, 0), e)) < 1e-6            # float64: nine orders below float32's eps
    assert np.median(e5.ess_ratio(e)) < 1e-6 and e5.ess_ratio(e).max() < 8.0     # the tail: ill-conditioned roots
    assert (e[np.arange(e.shape[0]), np.argmax(np.abs(e), 1)] > 0).all()


def test_the_true_essential_matrix_is_among_the_float64_solutions_of_the_exact_cases():
    found = total = 0
    for c in e5.cases(True):
        f = e5.true_found(e5.host_models(c), c)
        found, total = found + int(f.sum()), total + f.size
        # the true E is a solution of every sample: exact geometry, rounded to float32
        assert e5.epi_ratio(c["A"], np.repeat(c["true"][None], c["A"].shape[0], 0)).max() < 4.0
    print("the true E among the float64 solutions: %d/%d samples" % (found, total))
    assert total == 2100 and found >= 0.99 * total


def test_matches_counts_host_solutions_with_a_device_model_nearby():
    c = e5.cases(False)[1]
    host = c["host"][3]
    assert host.shape[0] >= 2
    dev = np.zeros((10, 9), np.float32)
    dev[0] = -host[1]                                                     # the sign does not count
    assert e5.matches(dev, host).tolist() == [i == 1 for i in range(host.shape[0])]
    assert not e5.matches(np.zeros((10, 9), np.float32), host).any()
    assert e5.matches(dev, np.zeros((0, 9))).size == 0


def test_baselines_are_finite_and_of_rounding_size():
    b_epi, b_ess = e5.baselines()
    print("b_epi = %.4f, b_ess = %.4f -> B_epi = %.3f, B_ess = %.3f (x eps32)" % (b_epi, b_ess, e5.MARGIN * b_epi, e5.MARGIN * b_ess))
    assert 0 < b_epi < 4.0 and 0.5 <= b_ess < 8.0                        # b_ess >= 0.5: the kernel's own 4 eps32 check lies below B_ess


def test_check_models_accepts_the_float64_solutions_and_refuses_broken_ones():
    c = e5.cases(True)[2]
    H = 40
    ref = [{"idx": c["idx"][:H], "A": c["A"][:H], "finite": np.ones(H, bool), "n": 600}]
    models = e5.host_models(c)[:H].astype(np.float32).reshape(1, H, 10, 3, 3)
    b_epi, b_ess = e5.baselines()
    w = e5.check_models(models, ref, B_epi=e5.MARGIN * b_epi, B_ess=e5.MARGIN * b_ess)
    assert 0 < w[0] <= b_epi and 0 < w[1] <= b_ess
    h = int(np.nonzero(models[0].reshape(H, 10, 9).any(2).sum(1) >= 2)[0][0])
    bad = models.copy()
    bad[0, h, 0] *= -1
    with pytest.raises(AssertionError, match="sign"):
        e5.check_models(bad, ref)
    bad = models.copy()
    bad[0, h, 0] = 0
    with pytest.raises(AssertionError, match="lowest"):
        e5.check_models(bad, ref)
    bad = models.copy()
    bad[0, h, 1] = bad[0, h, 0]
    with pytest.raises(AssertionError, match="coincide"):
        e5.check_models(bad, ref)
    bad = models.copy()
    bad[0, h, 0, 2, 2] += 0.25
    with pytest.raises(AssertionError):
        e5.check_models(bad, ref, B_epi=10.0, B_ess=10.0)
    with pytest.raises(AssertionError, match="n_models"):
        e5.check_models(models, ref, n_models=np.zeros((1, H), np.int32))
