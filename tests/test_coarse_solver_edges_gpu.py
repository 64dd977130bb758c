"""-m gpu: the one-CU coarse Sinkhorn solver (csrc/sinkhorn.hip: sinkhorn_cu2_kernel<19,5>, every [M, N] with M <= 304,
N <= 320, M * N >= 96 * 96) at its shape and guard edges, and its dispatch neighbours (the streaming solver's smallest
shapes, sinkhorn_wg_kernel on both sides of its 256 / 1024-thread switch), against a float64 reference of the reference's
log-domain iteration (tests/coarse_cases.py; tests/test_coarse_cases_host.py holds the CPU oracle to the same gates).

Every test runs in both solver modes: "kernel" (the linear-domain kernels with their 2^30 guard, flagged problems redone by
sinkhorn_wg_kernel) and "log" (sinkhorn_wg_kernel for everything - which is also that fallback).

The shapes walk the kernel's layout - 16 waves x 19 row slots, 64 lanes x 5 column slices, slots paired (i, i + 10), five of
them in LDS: every slot and slice full, one short, held by one wave or lane only, empty; every pair's second half padding; an
LDS pair half filled.  The gates are the project's (assert_mass of tests/test_gpu_parity.py): exp(Z) within 1e-4 + 2e-6
relative, both marginals within 1e-4 + 3e-6 relative, |Z - Z_ref| <= 2e-4 wherever the mass exceeds 1e-6; every output finite.
Each test prints its largest error as a share of each gate (pytest -rA)."""
import numpy as np
import pytest
import torch

import coarse_cases as cc
from coarse_cases import cu

pytestmark = pytest.mark.gpu


def _ids(shapes):
    return ["%dx%d" % s for s in shapes]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


@pytest.fixture(params=["kernel", "log"])
def mode(request, ops):
    prev = ops.set_sinkhorn_mode(request.param)
    yield request.param
    ops.set_sinkhorn_mode(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. shape sweep, given marginals ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", cc.SINKHORN_SHAPES, ids=_ids(cc.SINKHORN_SHAPES))
def test_shape_sweep_given_marginals(ops, mode, M, N):
    """log_sinkhorn_iterations on three problems after 1, 2 and 100 sweeps: one sweep shows a wrong hand-over of a row or column
    scaling that a hundred sweeps iterate away."""
    c = cc.sinkhorn_case(M, N)
    Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
    for it in cc.SWEEPS_SINKHORN:
        got = ops.log_sinkhorn_iterations(Z, log_mu, log_nu, it).cpu().numpy()
        what = "%s sinkhorn %dx%d it=%d" % (mode, M, N, it)
        print("%s [%s]: %s" % (what, cc.expected_path(M, N, mode, cc.B_SINKHORN), cc.fmt(cc.check_plan(got, c["ref"][it], what, (M, N), "s"))))


# ---- 2. shape sweep, the OT entry point -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", cc.OT_SHAPES, ids=_ids(cc.OT_SHAPES))
def test_shape_sweep_ot_entry_point(ops, mode, M, N):
    """log_optimal_transport on scores [2, M - 1, N - 1]: the dustbin row and column are synthesised from alpha inside the kernel
    (SrcView / src_at), the marginals come from ot_prep_kernel and norm is subtracted in the epilogue."""
    c = cc.ot_case(M, N)
    S, ns = cu(c["scores"]), cu(c["ns"])
    for it in cc.SWEEPS_OT:
        got = ops.log_optimal_transport(S, c["alpha"], ns, it)
        assert got.shape == (cc.B_OT, M, N)
        what = "%s OT %dx%d it=%d" % (mode, M, N, it)
        print("%s [%s]: %s" % (what, cc.expected_path(M, N, mode, cc.B_OT), cc.fmt(cc.check_plan(got.cpu().numpy(), c["ref"][it], what, (M, N), "o"))))


@pytest.mark.parametrize("M,N", cc.COST_OT_SHAPES, ids=_ids(cc.COST_OT_SHAPES))
def test_cost_ot_is_cost_then_ot(ops, mode, M, N):
    """cost_ot (variant 1, D = 64) has the bits of cost followed by log_optimal_transport, and is within the gates of the
    float64 solve of the float64 cost."""
    c = cc.cost_ot_case(M, N)
    d0, d1, ns = cu(c["d0"]), cu(c["d1"]), cu(c["ns"])
    S = ops.cost(d0, d1)
    np.testing.assert_allclose(S.cpu().numpy(), cc.ref_cost(c["d0"], c["d1"]), atol=2e-5, rtol=1e-5)     # test_coarse_level's gate
    for it in cc.SWEEPS_OT:
        fused = ops.cost_ot(d0, d1, 1, c["alpha"], ns, it)
        assert torch.equal(bits(fused), bits(ops.log_optimal_transport(S, c["alpha"], ns, it)))
        what = "%s cost_ot %dx%d it=%d" % (mode, M, N, it)
        print("%s: %s" % (what, cc.fmt(cc.check_plan(fused.cpu().numpy(), c["ref"][it], what, (M, N), "c"))))


# ---- 3. zero sweeps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(301, 301), (96, 96)], ids=_ids([(301, 301), (96, 96)]))
def test_zero_sweeps_return_the_input(ops, mode, M, N):
    """iters = 0: the one-CU kernel solves nothing and flags every problem; sinkhorn_wg_kernel writes (Z + 0) + 0."""
    c = cc.sinkhorn_case(M, N)
    Z = cu(c["Z"])
    ops.sinkhorn_fallbacks(reset=True)
    got = ops.log_sinkhorn_iterations(Z, cu(c["log_mu"]), cu(c["log_nu"]), 0)
    trips = ops.sinkhorn_fallbacks(reset=True)
    assert torch.equal(bits(got), bits(Z))
    assert trips == (cc.B_SINKHORN if mode == "kernel" else 0)


# ---- 4. more problems than CUs ------------------------------------------------------------------------------------------------
def test_more_problems_than_cus(ops, oracle, mode):
    """260 problems at (161, 65), three sweeps: every problem against the oracle, problems 0, 255 and 259 against float64."""
    c = cc.many_case()
    M, N = cc.MANY_MN
    got = ops.log_sinkhorn_iterations(cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"]), cc.MANY_SWEEPS).cpu().numpy()
    want = oracle.log_sinkhorn_iterations(c["Z"], c["log_mu"], c["log_nu"], cc.MANY_SWEEPS)
    what = "%s sinkhorn %dx%d b=%d it=%d" % (mode, M, N, cc.MANY_B, cc.MANY_SWEEPS)
    print("%s against the oracle: %s" % (what, cc.fmt(cc.check_plan(got, want, what))))
    print("%s against float64: %s" % (what, cc.fmt(cc.check_plan(got[list(cc.MANY_REF)], c["ref"], what + " (0, 255, 259)"))))


# ---- 5. guard trips and flag isolation ---------------------------------------------------------------------------------------
def _solver(ops, g, entry, sweeps=cc.GUARD_SWEEPS):
    """Z [k, ...] and the problems' indices -> log-plan of those problems, through the entry point of the case."""
    def solve(Z, sel):
        if entry == "s":
            return ops.log_sinkhorn_iterations(cu(Z[sel]), cu(g["log_mu"][sel]), cu(g["log_nu"][sel]), sweeps)
        return ops.log_optimal_transport(cu(Z[sel]), g["alpha"], cu(g["ns"][sel]), sweeps)
    return solve


@pytest.mark.parametrize("entry", ["s", "o"], ids=["sinkhorn", "ot"])
@pytest.mark.parametrize("M,N", cc.GUARD_SHAPES, ids=_ids(cc.GUARD_SHAPES))
def test_guard_trips_and_flag_isolation(ops, mode, M, N, entry):
    """Six problems, 100 sweeps; problems 1 and 4 span about +-150 nats and at least one of them leaves the 2^30 guard by a factor
    above 2^10, the other four stay a factor 2^10 inside it (held on the CPU by tests/test_coarse_cases_host.py).  The flagged
    problems are redone by sinkhorn_wg_kernel(only_if), which must leave the unflagged ones as the one-CU kernel wrote them."""
    g = cc.guard_case(M, N, entry)
    solve = _solver(ops, g, entry)
    everyone, tame, wild = list(range(cc.GUARD_B)), list(cc.GUARD_TAME), list(cc.GUARD_WILD)
    ops.sinkhorn_fallbacks(reset=True)
    got_t = solve(g["Z"], everyone)
    trips = ops.sinkhorn_fallbacks(reset=True)
    assert (1 <= trips <= 2) if mode == "kernel" else trips == 0, trips
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    # the tame problems: as in a batch of their own, bit for bit
    alone = solve(g["Z"], tame)
    assert ops.sinkhorn_fallbacks(reset=True) == 0
    assert torch.equal(bits(got_t[tame]), bits(alone)), "a flagged problem's redo changed an unflagged problem"
    what = "%s guard %dx%d %s" % (mode, M, N, entry)
    print("%s, %d trips, tame problems: %s" % (what, trips, cc.fmt(cc.check_plan(got[tame], g["ref"][tame], what + " tame"))))
    # the wild ones: the log-plan to fp32 resolution of |Z| ~ 200
    print("%s wild problems: max |Z - Z_ref| %.3g" % (what, float(np.abs(got[wild] - g["ref"][wild]).max())))
    np.testing.assert_allclose(got[wild], g["ref"][wild], atol=cc.WILD_ATOL, rtol=cc.WILD_RTOL)
    # structural zeros in a tame batch: rows 0..4 x columns 7..19, and a block across column slices and LDS row slots
    got_i = solve(g["Z_inf"], everyone).cpu().numpy()
    ops.sinkhorn_fallbacks(reset=True)
    assert not np.isnan(got_i).any()
    assert np.array_equal(np.isneginf(got_i), np.isneginf(g["ref_inf"])) and not np.isposinf(got_i).any()
    fin = np.isfinite(g["ref_inf"])
    print("%s -inf blocks: max |Z - Z_ref| on finite entries %.3g" % (what, float(np.abs(got_i[fin] - g["ref_inf"][fin]).max())))
    np.testing.assert_allclose(got_i[fin], g["ref_inf"][fin], atol=cc.NEGINF_ATOL, rtol=0)


# ---- 6. repeatability ------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(ops, mode):
    """(289, 257), 100 sweeps, both entry points: the column sums are formed in a fixed order, without atomics."""
    M, N = 289, 257
    c, o = cc.sinkhorn_case(M, N), cc.ot_case(M, N)
    Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
    first = ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)
    S, ns = cu(o["scores"]), cu(o["ns"])
    first_ot = ops.log_optimal_transport(S, o["alpha"], ns, 100)
    assert torch.equal(bits(ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)), bits(first))
    assert torch.equal(bits(ops.log_optimal_transport(S, o["alpha"], ns, 100)), bits(first_ot))
