"""CPU-only: the numpy restatement of the uncalibrated branch (tests/fundamental_cases.py) and the host side of its three entry points.
The seven-draw sampler: both forms of the definition agree, literal rows pinned from the definition's first form (list.pop).  The
float64 solver: its models are solutions, and the conditions the GPU test's completeness shares rely on hold for the reference
alone - the true model of the exact cases is among them in at least 99 % of the samples, and a second route to the roots (the
cubic in a / b instead of b / a) agrees on at least 99 % of the solutions within MATCH_TOL.  The refit: the gaps sigma2 - sigma3 of
the scenes the GPU test's Wedin bound divides by.  The library: symbols, zero workspaces, refusals, signatures."""
import ctypes
import inspect

import numpy as np
import pytest

import epipolar_cases as ec
import fundamental_cases as fc
import hypotheses_cases as hc


@pytest.mark.parametrize("n,H,progressive", [(7, 64, False), (8, 65, True), (16, 300, True), (600, 257, False), (600, 257, True),
                                             (2048, 1024, True), (100000, 50, True)])
def test_draws_are_distinct_inside_the_pool_and_both_forms_agree(n, H, progressive):
    idx = fc.sample_idx(77 + n, n, H, progressive)
    assert idx.dtype == np.int32 and idx.shape == (H, 7)
    m = fc.pool(n, H, progressive)
    assert (idx >= 0).all() and (idx < m[:, None]).all() and (m <= n).all() and (m >= 7).all()
    assert all(len(set(row)) == 7 for row in idx.tolist())
    for h in (0, H // 2, H - 1):                                          # the two forms of the definition
        assert idx[h].tolist() == fc.sample_idx_slow(77 + n, h, int(m[h]))


def test_fewer_than_seven_matches_have_no_sample_and_the_generator_is_the_hypotheses():
    for n in (0, 1, 6):
        assert (fc.sample_idx(5, n, 9, True) == -1).all()
    assert fc.sample_idx(-7, 7, 3)[0].tolist() == fc.sample_idx_slow(-7, 0, 7)
    assert sorted(fc.sample_idx(-7, 7, 3)[0].tolist()) == list(range(7))
    # one generator, two draw counts: the first seven of the 8-point sampler's draws whenever the pools agree
    assert np.array_equal(fc.sample_idx(99, 600, 40), hc.sample_idx(99, 600, 40)[:, :7])
    assert fc.sample_idx(0x0123456789ABCDEF, 600, 16)[5].tolist()[:5] == [422, 343, 272, 389, 436]


def test_the_float64_solver_meets_the_contract_on_its_own_output():
    c = fc.cases(True)[0]
    k = np.array([e.shape[0] for e in c["host"]])
    e = np.concatenate(c["host"])
    assert set(np.unique(k).tolist()) <= {1, 3}                           # a real cubic: one or three real roots
    assert fc.norm_error(e).max() < 1e-12
    assert np.median(fc.epi_ratio(np.repeat(c["A"], k, 0), e)) < 1e-6     # float64: nine orders below float32's eps
    assert np.median(fc.det_ratio(e)) < 1e-6 and fc.det_ratio(e).max() < 1e-3
    assert (e[np.arange(e.shape[0]), np.argmax(np.abs(e), 1)] > 0).all()
    H = 40
    ref = [{"idx": c["idx"][:H], "A": c["A"][:H], "finite": np.ones(H, bool), "n": 600}]
    models = fc.host_models(c)[:H].astype(np.float32).reshape(1, H, 3, 3, 3)
    b_epi, b_det = fc.baselines()
    print("b_epi = %.4f, b_det = %.4f -> B_epi = %.3f, B_det = %.3f (x eps32)" % (b_epi, b_det, fc.MARGIN * b_epi, fc.MARGIN * b_det))
    assert 0 < b_epi < 4.0 and 0 < b_det < 4.0
    w = fc.check_models(models, ref, B_epi=fc.MARGIN * b_epi, B_det=fc.MARGIN * b_det)
    assert 0 < w[0] <= b_epi and 0 < w[1] <= b_det
    h = int(np.nonzero(k[:H] == 3)[0][0])
    for change, word in ((lambda b: b[0, h, 0].__imul__(-1), "sign"), (lambda b: b[0, h, 0].fill(0), "lowest"),
                         (lambda b: b[0, h, 1].__setitem__(slice(None), b[0, h, 0]), "coincide")):
        bad = models.copy()
        change(bad)
        with pytest.raises(AssertionError, match=word):
            fc.check_models(bad, ref)
    bad = models.copy()
    bad[0, h, 0, 2, 2] += 0.25
    with pytest.raises(AssertionError):
        fc.check_models(bad, ref, B_epi=10.0, B_det=10.0)
    with pytest.raises(AssertionError, match="n_models"):
        fc.check_models(models, ref, n_models=np.zeros((1, H), np.int32))


def test_the_true_model_is_among_the_float64_solutions_of_the_exact_cases():
    found = total = 0
    for c in fc.cases(True):
        f = fc.true_found(fc.host_models(c), c)
        found, total = found + int(f.sum()), total + f.size
        assert fc.epi_ratio(c["A"], np.repeat(c["true"][None], c["A"].shape[0], 0)).max() < 4.0      # a solution of every sample
    print("the true model among the float64 solutions: %d/%d samples" % (found, total))
    assert total == 2100 and found >= 0.99 * total


def test_the_two_routes_to_the_roots_agree():
    missed = total = 0
    roots = np.zeros(4, np.int64)
    for exact in (True, False):
        for c in fc.cases(exact):
            other = fc.solve64(c["A"], route="a/b")
            for first, second in zip(c["host"], other):
                m = fc.matches(second, first)
                missed, total = missed + int((~m).sum()), total + m.size
                roots[min(first.shape[0], 3)] += 1
    print("%d of %d solutions of the b / a route without one of the a / b route within %g; samples by real roots %s"
          % (missed, total, fc.MATCH_TOL, roots.tolist()))
    assert total > 10000 and missed <= 0.01 * total and roots[0] == 0 and roots[2] == 0


def test_matches_counts_host_solutions_with_a_device_model_nearby():
    c = fc.cases(False)[1]
    host = next(e for e in c["host"] if e.shape[0] == 3)
    dev = np.zeros((3, 9), np.float32)
    dev[0] = -host[1]                                                     # the sign does not count
    assert fc.matches(dev, host).tolist() == [False, True, False]
    assert not fc.matches(np.zeros((3, 9), np.float32), host).any()
    assert fc.matches(dev, np.zeros((0, 9))).size == 0


def test_refit_restatement_and_the_gaps_of_the_scenes():
    for i, n in enumerate((20, 65, 500, 1200, 3000, 4097)):
        s = fc.make_scene(201 + i, n)
        M = ec.moments64(s["ml"], s["mr"], s["good"])[0]
        F, eig, sig, f = fc.refit64(M)
        print("scene %d: %d true matches, sigma %s, gap sigma2 - sigma3 = %.4f" % (201 + i, s["good"].sum(), sig.tolist(), sig[1] - sig[2]))
        assert s["good"].sum() >= fc.MIN_INLIERS and sig[1] - sig[2] > 0.5  # Wedin's bound of the GPU test: 64 eps64 / gap < 2.9e-14
        assert abs(np.linalg.norm(F) - 1) < 1e-15 and abs(np.linalg.det(F)) < 1e-16 and np.array_equal(fc.sign_rule(F), F)
        assert 0 <= eig[0] <= eig[1] and abs(np.linalg.norm(f) - 1) < 1e-14
        assert fc.closeness(F.reshape(1, 9), s["F"].reshape(1, 9))[0, 0] < 1e-3
        # the permutation and the denormalisation keep the epipolar constraint
        norm = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)
        xl, xr = s["ml"][s["good"]].astype(np.float64), s["mr"][s["good"]].astype(np.float64)
        pl, pr = xl / norm[2:4] + norm[0:2], xr / norm[6:8] + norm[4:6]
        h = lambda a: np.c_[a, np.ones(len(a))]                           # noqa: E731
        res = np.einsum("ni,ij,nj->n", h(xr), F, h(xl))
        G, scale = fc.denormalise(F, norm), np.linalg.norm(NrT_F_Nl(F, norm))
        assert np.abs(np.abs(np.einsum("ni,ij,nj->n", h(pr), G, h(pl))) * scale - np.abs(res)).max() < 1e-12
        assert np.abs(np.einsum("ni,ij,nj->n", h(xr[:, ::-1]), fc.swap(F), h(xl[:, ::-1]))) == pytest.approx(np.abs(res), abs=1e-15)
    assert fc.denormalise(F) is not None and np.array_equal(fc.denormalise(F), F)


def NrT_F_Nl(F, norm):
    import homography_cases as hm
    Nl, Nr = hm.norm_matrices(norm)
    return Nr.T @ F @ Nl


# ---- the library ------------------------------------------------------------------------------------------------------------------
SYMBOLS = {"pats_epipolar_hypotheses7_workspace_bytes": (ctypes.c_size_t, 2), "pats_epipolar_hypotheses7_by_pair_f32": (ctypes.c_int, 17),
           "pats_fundamental_refit_workspace_bytes": (ctypes.c_size_t, 1), "pats_fundamental_refit_by_pair_f64": (ctypes.c_int, 16),
           "pats_fundamental_polish_workspace_bytes": (ctypes.c_size_t, 3), "pats_fundamental_polish_by_pair_f32": (ctypes.c_int, 25)}
A16 = 0x7f0000001000                                                      # never dereferenced: every case below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    from pats_amd import _lib
    return _lib.lib()


def test_symbols_signatures_sources_and_zero_workspaces(lib):
    from pats_amd import _lib, batch, ops
    from pats_amd.build import SOURCES
    for name, (res, nargs) in SYMBOLS.items():
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    assert lib.pats_abi_version() == 8 == _lib.ABI_VERSION                # symbols were added, nothing else
    assert "hypotheses7.hip" in SOURCES and "fundamental.hip" in SOURCES
    assert lib.pats_epipolar_hypotheses7_workspace_bytes(48, 1024) == 0 == lib.pats_fundamental_refit_workspace_bytes(48)
    assert lib.pats_fundamental_polish_workspace_bytes(48, 1, 2 ** 31 - 2) == 0
    assert str(inspect.signature(ops.epipolar_hypotheses7_by_pair)) == str(inspect.signature(ops.epipolar_hypotheses5_by_pair))
    assert str(inspect.signature(ops.fundamental_refit_by_pair)) == (
        "(best_count, moments=None, models=None, best=None, norm=None, swapped=False, return_pixel=False, return_refit=False, out=None)")
    assert str(inspect.signature(ops.fundamental_polish_by_pair)) == str(inspect.signature(ops.epipolar_polish_by_pair))
    assert str(inspect.signature(batch.hypothesize7_by_pair)) == "(out, cap, H, seed=0, norm=None, on='topk', progressive=None, samples=False)"
    assert str(inspect.signature(batch.fundamental_by_pair)) == "(out, cap, norm=None, swapped=False, pixel=False)"
    assert str(inspect.signature(batch.polish_f_by_pair)) == "(out, cap, thr, rounds=4, norm=None, min_conf=None)"


def test_refusal_tables_are_well_formed_and_every_case_is_refused(lib):
    for which in ("hypotheses7", "refit"):
        e = fc.ENTRY[which]
        assert set(e["required"]) <= set(e["align"]) and set(e["align"]) | set(e["scalars"]) == set(e["order"])
        assert len(e["order"]) + 3 == SYMBOLS[e["fn"]][1]
        cases = fc.refusals(lib, which, A16)
        assert all(set(kw) <= set(e["order"]) and words for kw, words in cases)
        assert fc.check_refusals(lib, which, A16) == len(cases)
    assert fc.check_polish_refusals(lib, A16) > 70
    assert fc.c_call(lib, "hypotheses7", A16, ws_bytes=0, pairs=0) != 0 and b"pairs" in lib.pats_last_error()


def test_python_layers_refuse_before_any_device_work():
    import torch
    from pats_amd import batch, ops
    ml = torch.zeros((20, 2))
    seed, off = torch.zeros(2, dtype=torch.int64), torch.tensor([0, 10, 20])
    with pytest.raises(RuntimeError, match="epipolar_hypotheses7_by_pair: give either pair_off, or stride and counts"):
        ops.epipolar_hypotheses7_by_pair(ml, ml, 4, seed)
    with pytest.raises(RuntimeError, match="epipolar_hypotheses7_by_pair: seed must be an int64 GPU tensor"):
        ops.epipolar_hypotheses7_by_pair(ml, ml, 4, 7, pair_off=off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epipolar_hypotheses7_by_pair(ml, ml, 4, seed, pair_off=off)                 # CPU tensors
    with pytest.raises(RuntimeError, match="fundamental_refit_by_pair: give moments, or models and best"):
        ops.fundamental_refit_by_pair(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="fundamental_polish_by_pair: rounds = 17"):
        ops.fundamental_polish_by_pair(ml, ml, torch.zeros((2, 1, 3, 3)), torch.zeros(2), rounds=17, pair_off=off)
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": ml, "matches_r": ml}
    with pytest.raises(ValueError, match="hypothesize7_by_pair.*topk_by_pair"):
        batch.hypothesize7_by_pair(dict(plain), cap, 16)                  # on="topk" is the default
    with pytest.raises(ValueError, match="polish_f_by_pair: run verify_by_pair first"):
        batch.polish_f_by_pair(dict(plain), cap, None)
    with pytest.raises(ValueError, match="fundamental_by_pair: run verify_by_pair first"):
        batch.fundamental_by_pair(dict(plain), cap)
