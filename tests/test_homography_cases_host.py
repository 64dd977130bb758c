"""CPU-only: the numpy restatement of the per-pair homographies (tests/homography_cases.py) and the C-ABI surface of the feature.
The three figures the GPU test leans on are recomputed and asserted: the undecided share of the committed verification cases stays
far below the 1 % cap, a float32 emulation WITHOUT fused multiply-adds agrees with float64 on every decided cell, and the baseline
b32 (numpy's float32 svd on the tolerance cases; the GPU test holds the kernel to MARGIN * b32) is finite.  Literal sample rows are
pinned once from the definition so that the restatement cannot drift with the kernel.  The built library exports the six new symbols
with the header's prototypes and the ctypes table's."""
import ctypes
import os
import re

import numpy as np
import pytest

import epipolar_cases as ec
import homography_cases as hm
import hypotheses_cases as hc
from conftest import REPO

SYMBOLS = {"pats_homography_hypotheses_workspace_bytes": (ctypes.c_size_t, 2), "pats_homography_hypotheses_by_pair_f32": (ctypes.c_int, 16),
           "pats_homography_score_workspace_bytes": (ctypes.c_size_t, 3), "pats_homography_score_by_pair_f32": (ctypes.c_int, 22),
           "pats_homography_refit_workspace_bytes": (ctypes.c_size_t, 1), "pats_homography_refit_by_pair_f64": (ctypes.c_int, 14)}
CTYPE_OF = (("*", ctypes.c_void_p), ("pats_stream_t", ctypes.c_void_p), ("int64_t", ctypes.c_int64), ("size_t", ctypes.c_size_t),
            ("float", ctypes.c_float), ("int", ctypes.c_int))


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,progressive", [(4, 64, False), (5, 65, True), (16, 300, True), (600, 257, False), (600, 257, True),
                                             (100000, 50, True)])
def test_draws_are_distinct_inside_the_pool_and_both_forms_agree(n, H, progressive):
    idx = hm.sample_idx(77 + n, n, H, progressive)
    assert idx.dtype == np.int32 and idx.shape == (H, 4)
    m = hm.pool(n, H, progressive)
    assert (idx >= 0).all() and (idx < m[:, None]).all() and (m <= n).all() and (m >= 4).all()
    assert all(len(set(row)) == 4 for row in idx.tolist())
    assert not np.array_equal(idx, hm.sample_idx(78 + n, n, H, progressive))
    for h in (0, H // 2, H - 1):
        assert idx[h].tolist() == hm.sample_idx_slow(77 + n, h, int(m[h]))
    if not progressive and n >= 8:                                        # the same generator: the first four of the eight draws
        assert np.array_equal(idx, hc.sample_idx(77 + n, n, H)[:, :4])


def test_fewer_than_four_matches_have_no_sample():
    for n in (0, 1, 3):
        assert (hm.sample_idx(5, n, 9, True) == -1).all()


def test_pinned_rows():
    """Computed once from the definition's first form (pop the j-th remaining index) with Python integers."""
    assert hm.sample_idx(0x0123456789ABCDEF, 600, 16)[5].tolist() == [422, 343, 272, 389]
    assert hm.sample_idx(-7, 4, 3)[0].tolist() == [2, 3, 1, 0]                                  # a negative seed: its 64 bits
    assert hm.sample_idx(42, 600, 200, True)[2].tolist() == [2, 1, 7, 4]                        # progressive: m_2 = 9
    m = hm.pool(2048, 1024, True)
    assert m[0] == 4 and m[1] == 4 and m[2] == 6 and m[-1] == 2048                              # ceil(2048 (h + 1) / 1024) = 2 (h + 1)


# ---- rows and null vectors --------------------------------------------------------------------------------------------------------
def test_rows_and_float64_null_vectors():
    xl, xr, idx, A = hm.tolerance_cases()[0]
    h, t = 13, 2
    i = idx[h, t]
    l = np.append(xl[i].astype(np.float64), 1.0)
    r0, r1 = float(xr[i, 0]), float(xr[i, 1])
    assert np.array_equal(A[h, 2 * t], np.concatenate([-l, np.zeros(3), r0 * l]))
    assert np.array_equal(A[h, 2 * t + 1], np.concatenate([np.zeros(3), -l, r1 * l]))
    e = hm.null64(A)
    assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-12 and hm.ratio(A, e).max() < 1e-6
    # the rows annihilate the true homography of a noise-free scene: A_i h = r0 a2 - a0
    c = hm.make_scene(9, 50, outliers=0.0, noise=0.0)
    a, b = hm.match_rows(c["ml"], c["mr"])
    assert max(np.abs(a @ c["H"].reshape(9)).max(), np.abs(b @ c["H"].reshape(9)).max()) < 1e-6      # float32 rounding of x_r


def test_baseline_b32_is_finite():
    b32 = hm.baseline32()
    print("b32 = %.4f over %d samples -> B = %.1f * b32 = %.4f" % (b32, sum(c[2] for c in hm.TOLERANCE_CASES), hm.MARGIN, hm.MARGIN * b32))
    assert np.isfinite(b32) and b32 > 0


def test_check_models_accepts_float64_vectors_and_refuses_broken_ones():
    ml, mr, off = hm.make_pairs([3, 40], seed=5)
    ref = hm.reference(ml, mr, [(0, 3), (3, 40)], [3, 4], 11)
    assert ref[0]["A"] is None and not ref[0]["finite"].any() and ref[1]["finite"].all()
    models = np.zeros((2, 11, 3, 3), np.float32)
    models[1] = hm.sign_rule(hm.null64(ref[1]["A"])).reshape(11, 3, 3)
    assert hm.check_models(models, ref, B=1.0) < 1.0                      # float64 vectors rounded to float32: within one eps32
    bad = models.copy()
    bad[1, 3] *= -1
    with pytest.raises(AssertionError, match="sign"):
        hm.check_models(bad, ref)
    bad = models.copy()
    bad[0, 0, 0, 0] = 1.0
    with pytest.raises(AssertionError, match="must be zero"):
        hm.check_models(bad, ref)


# ---- the test's band and the float32 emulation ------------------------------------------------------------------------------------
def test_undecided_share_and_float32_emulation_on_the_committed_cases():
    share, wrong, cells = hm.host_figures()
    print("undecided share at most %.2e of a case's cells; %d of %d decided cells differ in float32" % (share, wrong, cells))
    assert share < 0.01                                                   # the cap; the measured share is some 1e-5
    assert wrong == 0
    c = hm.make_case(103, 500, 64)                                        # the true model explains the scene's inliers and only them
    inl, dec = hm.classify(c["ml"], c["mr"], ec.participates(c["ml"], c["mr"]), c["models"], c["thr"])
    assert 0.9 * c["good"].sum() <= inl[c["true"]].sum() <= c["good"].sum() + 5 and inl.sum(1).max() == inl[c["true"]].sum()


def test_verdicts_that_do_not_depend_on_rounding():
    c = hm.make_case(7, 40, 3)
    part = ec.participates(c["ml"], c["mr"])
    for thr in (np.nan, -1e-3):
        inl, dec = hm.classify(c["ml"], c["mr"], part, c["models"], thr)
        assert not inl.any() and dec.all() and not hm.emulate32(c["ml"], c["mr"], part, c["models"], thr).any()
    zero = np.zeros((1, 3, 3), np.float32)
    inl, dec = hm.classify(c["ml"], c["mr"], part, zero, 1.0)
    assert not inl.any() and dec.all() and not hm.emulate32(c["ml"], c["mr"], part, zero, 1.0).any()


# ---- moments and denormalisation --------------------------------------------------------------------------------------------------
def test_moments_refit_and_denormalisation():
    c = hm.make_scene(21, 400, outliers=0.25)
    M = hm.moments64(c["ml"], c["mr"], c["good"])
    assert np.array_equal(M, M.T) and M[2, 2] == M[5, 5] == c["good"].sum() and not M[:3, 3:6].any()
    w, v = np.linalg.eigh(M)
    assert np.abs(hm.sign_rule(v[:, 0]) - c["H"].reshape(9)).max() < 2e-3 and w[1] > 100 * abs(w[0])
    norm = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)
    xl, xr = ec.points32(c["ml"], c["mr"], norm)                          # a homography of the normalised points ...
    Hn = hm.sign_rule(np.linalg.eigh(hm.moments64(xl, xr, c["good"]))[1][:, 0]).reshape(3, 3)
    Hpx = hm.denormalise(Hn, norm)                                        # ... maps the stored ones after denormalisation
    assert abs(np.linalg.norm(Hpx) - 1) < 1e-12 and np.abs(Hpx - c["H"]).max() < 2e-3
    assert np.array_equal(hm.denormalise(Hn), Hn)
    assert np.array_equal(hm.swap(hm.swap(Hn)), Hn)


# ---- the C-ABI surface ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_library_exports_the_six_symbols_with_the_headers_prototypes(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in SYMBOLS.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and len(got_args) == nargs, name
        for p, a in zip(params, got_args):                                # the prototype's types against the ctypes table's
            want = next(ct for word, ct in CTYPE_OF if (word == "*" and "*" in p) or re.search(r"\b%s\b" % re.escape(word), p))
            assert a is want, (name, p, a)
    assert "homography.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.pats_homography_hypotheses_workspace_bytes(48, 1024) == 0 and lib.pats_homography_refit_workspace_bytes(48) == 0


@pytest.mark.parametrize("which", sorted(hm.ENTRY))
def test_every_bad_argument_is_refused_by_name_before_any_launch(lib, which):
    """Fake device addresses: validation refuses them before anything touches them (tests/test_homography_gpu.py repeats this with a
    real allocation behind the pointers, where a launch would be possible)."""
    assert hm.check_refusals(lib, which, 0x7f0000001000) > (20 if which == "refit" else 40)


def test_ops_and_batch_signatures_and_refusals_without_a_gpu():
    import inspect
    import torch
    from pats_amd import batch, ops
    assert str(inspect.signature(batch.hypothesize_h_by_pair)) == str(inspect.signature(batch.hypothesize_by_pair))
    assert str(inspect.signature(batch.verify_h_by_pair)) == str(inspect.signature(batch.verify_by_pair))
    assert str(inspect.signature(batch.homography_by_pair)) == "(out, cap, norm=None, swapped=False, pixel=False)"
    assert str(inspect.signature(ops.homography_hypotheses_by_pair)) == str(inspect.signature(ops.epipolar_hypotheses_by_pair))
    assert str(inspect.signature(ops.homography_score_by_pair)) == str(inspect.signature(ops.epipolar_score_by_pair))
    ml, off = torch.zeros(20, 2), torch.tensor([0, 10, 20])
    models, thr, seed = torch.zeros(2, 4, 3, 3), torch.zeros(2), torch.zeros(2, dtype=torch.int64)
    bc, mom, best = torch.tensor([10, 10]), torch.zeros(2, 9, 9, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.homography_hypotheses_by_pair(ml, ml, 4, seed, pair_off=off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.homography_score_by_pair(ml, ml, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.homography_refit_by_pair(bc, moments=mom)
    with pytest.raises(RuntimeError, match="matches_l must be contiguous"):
        ops.homography_score_by_pair(torch.zeros(20, 4)[:, ::2], ml, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="matches_r must be float32"):
        ops.homography_hypotheses_by_pair(ml, ml.double(), 4, seed, pair_off=off)
    with pytest.raises(RuntimeError, match="seed must be int64"):
        ops.homography_hypotheses_by_pair(ml, ml, 4, seed.int(), pair_off=off)
    with pytest.raises(RuntimeError, match="models must be float32"):
        ops.homography_score_by_pair(ml, ml, models.double(), thr, pair_off=off)
    with pytest.raises(RuntimeError, match="min_conf needs conf"):
        ops.homography_score_by_pair(ml, ml, models, thr, pair_off=off, min_conf=0.5)
    with pytest.raises(RuntimeError, match="moments must be float64"):
        ops.homography_refit_by_pair(bc, moments=mom.float())
    with pytest.raises(RuntimeError, match="moments must be contiguous"):
        ops.homography_refit_by_pair(bc, moments=mom.transpose(1, 2))
    with pytest.raises(RuntimeError, match="best_count must be int64"):
        ops.homography_refit_by_pair(bc.int(), moments=mom)
    with pytest.raises(RuntimeError, match="best must be int32"):
        ops.homography_refit_by_pair(bc, models=models, best=best.long())
    for kw in ({}, {"models": models}, {"best": best}):
        with pytest.raises(RuntimeError, match="give moments, or models and best"):
            ops.homography_refit_by_pair(bc, **kw)
    for fn, args in ((ops.homography_hypotheses_by_pair, (ml, ml, 4, seed)), (ops.homography_score_by_pair, (ml, ml, models, thr))):
        for kw in ({}, {"pair_off": off, "stride": 10, "counts": torch.tensor([3, 3])}, {"stride": 10}):
            with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
                fn(*args, **kw)
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": ml, "matches_r": ml, "match_row": None, "M": None, "P": None}
    with pytest.raises(ValueError, match="verify_h_by_pair"):
        batch.homography_by_pair(dict(plain), cap)
    with pytest.raises(ValueError, match="on must be"):
        batch.verify_h_by_pair(dict(plain), cap, models, thr, on="some")
    with pytest.raises(ValueError, match="topk_by_pair"):
        batch.hypothesize_h_by_pair(dict(plain), cap, 8)
    with pytest.raises(ValueError, match="confidence=True"):
        batch.verify_h_by_pair(dict(plain), cap, models, thr, min_conf=0.5)
