"""Host side (-m "not gpu", oracle only): the float64 reference and the shape table of tests/coarse_cases.py are held to what
tests/test_coarse_solver_edges_gpu.py relies on.  The CPU oracle (fp32 with double accumulation - the best an fp32 evaluation
does) must pass the GPU tests' own gates against the float64 reference on every case and both entry points, at 1 and 100
sweeps: its largest error per gate is printed (pytest -rA shows it).  The dispatch mirror is asserted against the table, every
shape fits launch_wg's LDS bound, the 'why' column's statements about row slots and column slices are recomputed, and the
guard-trip inputs are checked to lie on the side of the 2^30 guard the GPU test assumes."""
import numpy as np
import pytest

import coarse_cases as cc


def _ids(shapes):
    return ["%dx%d" % s for s in shapes]


# ---- the checker against float64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", cc.SINKHORN_SHAPES, ids=_ids(cc.SINKHORN_SHAPES))
def test_oracle_sinkhorn_within_the_gates_of_float64(oracle, M, N):
    c = cc.sinkhorn_case(M, N)
    for it in (1, 100):
        got = oracle.log_sinkhorn_iterations(c["Z"], c["log_mu"], c["log_nu"], it)
        e = cc.check_plan(got, c["ref"][it], "oracle sinkhorn %dx%d it=%d" % (M, N, it), (M, N), "s")
        print("oracle sinkhorn %3dx%-3d it=%-3d: %s" % (M, N, it, cc.fmt(e)))


@pytest.mark.parametrize("M,N", cc.OT_SHAPES, ids=_ids(cc.OT_SHAPES))
def test_oracle_ot_within_the_gates_of_float64(oracle, M, N):
    c = cc.ot_case(M, N)
    for it in (1, 100):
        got = oracle.log_optimal_transport(c["scores"], c["alpha"], c["ns"], it)
        assert got.shape == (cc.B_OT, M, N)
        e = cc.check_plan(got, c["ref"][it], "oracle OT %dx%d it=%d" % (M, N, it), (M, N), "o")
        print("oracle OT       %3dx%-3d it=%-3d: %s" % (M, N, it, cc.fmt(e)))


@pytest.mark.parametrize("M,N", cc.COST_OT_SHAPES, ids=_ids(cc.COST_OT_SHAPES))
def test_oracle_cost_then_ot_within_the_gates_of_float64(oracle, M, N):
    c = cc.cost_ot_case(M, N)
    S = oracle.cost(c["d0"], c["d1"])
    np.testing.assert_allclose(S, cc.ref_cost(c["d0"], c["d1"]), atol=2e-5, rtol=1e-5)      # test_coarse_level's gate on the cost
    for it in (1, 100):
        got = oracle.log_optimal_transport(S, c["alpha"], c["ns"], it)
        e = cc.check_plan(got, c["ref"][it], "oracle cost + OT %dx%d it=%d" % (M, N, it), (M, N), "c")
        print("oracle cost+OT  %3dx%-3d it=%-3d: %s" % (M, N, it, cc.fmt(e)))


def test_oracle_many_problems_within_the_gates_of_float64(oracle):
    c = cc.many_case()
    pick = list(cc.MANY_REF)
    got = oracle.log_sinkhorn_iterations(c["Z"][pick], c["log_mu"][pick], c["log_nu"][pick], cc.MANY_SWEEPS)
    print("oracle sinkhorn 161x65 b=260 (problems 0, 255, 259): %s" % cc.fmt(cc.check_plan(got, c["ref"], "oracle many")))


def test_no_case_needed_a_wider_gate():
    assert cc.GATE_SCALE == {}


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_reference_is_the_reference_iteration():
    """One and two sweeps written out with scipy-free, loop-free numpy on a small ragged problem; the column marginal after any
    sweep is exactly nu (v was updated last), the row marginal converges to mu."""
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((2, 7, 5)) * 3
    lmu, lnu = cc._marginal(rng, 2, 7).astype(np.float64), cc._marginal(rng, 2, 5).astype(np.float64)
    lse = lambda x, ax: np.log(np.exp(x).sum(ax))                                         # noqa: E731  (no stabiliser at this range)
    u1 = lmu - lse(Z, 2)
    v1 = lnu - lse(Z + u1[:, :, None], 1)
    np.testing.assert_allclose(cc.ref_sinkhorn(Z, lmu, lnu, 1), Z + u1[:, :, None] + v1[:, None, :], rtol=0, atol=1e-13)
    u2 = lmu - lse(Z + v1[:, None, :], 2)
    v2 = lnu - lse(Z + u2[:, :, None], 1)
    np.testing.assert_allclose(cc.ref_sinkhorn(Z, lmu, lnu, 2), Z + u2[:, :, None] + v2[:, None, :], rtol=0, atol=1e-13)
    assert np.array_equal(cc.ref_sinkhorn(Z, lmu, lnu, 0), Z)
    for it in (1, 2, 100):
        P = np.exp(cc.ref_sinkhorn(Z, lmu, lnu, it))
        np.testing.assert_allclose(P.sum(1), np.exp(lnu), rtol=1e-12)
    np.testing.assert_allclose(P.sum(2), np.exp(lmu), rtol=1e-6)               # convergence after 100 sweeps, not rounding
    # one run to the largest count gives every smaller count's plan
    many = cc.ref_sweeps(Z, lmu, lnu, (1, 2, 100))
    assert np.array_equal(many[2][0], cc.ref_sinkhorn(Z, lmu, lnu, 2)) and sorted(many) == [1, 2, 100]


def test_reference_ot_couples_dustbins_and_norm_as_the_oracle_does(oracle):
    rng = np.random.default_rng(2)
    S = (rng.standard_normal((2, 6, 9)) * 3).astype(np.float32)
    ns = rng.uniform(0.5, 2.0, (2, 1, 9)).astype(np.float32)
    C, lmu, lnu, norm = cc.ot_problem(S, 1.3, ns)
    assert C.shape == (2, 7, 10) and np.array_equal(C[:, :6, :9], S.astype(np.float64))
    a = float(np.float32(1.3))
    assert (C[:, 6, :] == a).all() and (C[:, :, 9] == a).all()
    np.testing.assert_allclose(norm, -np.log(6 + ns.astype(np.float64).sum((1, 2))), rtol=1e-15)
    np.testing.assert_allclose(np.exp(lmu).sum(1), 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.exp(lnu).sum(1), 1.0, rtol=1e-12)
    for it in (1, 100):
        cc.check_plan(oracle.log_optimal_transport(S, 1.3, ns, it), cc.ref_log_optimal_transport(S, 1.3, ns, it), "small OT")
    # multiplied by M + N: after 100 sweeps a real row carries mass 1, the dustbin row sum(ns)
    P = np.exp(cc.ref_log_optimal_transport(S, 1.3, ns, 100))
    np.testing.assert_allclose(P[:, :6].sum(2), 1.0, rtol=1e-6)
    np.testing.assert_allclose(P[:, 6].sum(1), ns.astype(np.float64).sum((1, 2)), rtol=1e-6)


def test_reference_cost_is_the_scaled_contraction(oracle):
    rng = np.random.default_rng(3)
    d0, d1 = rng.standard_normal((2, 64, 5)).astype(np.float32), rng.standard_normal((2, 64, 8)).astype(np.float32)
    want = np.stack([0.1 * (d0[b].astype(np.float64).T @ d1[b].astype(np.float64)) / 8.0 for b in range(2)])
    np.testing.assert_allclose(cc.ref_cost(d0, d1), want, rtol=1e-14)
    np.testing.assert_allclose(oracle.cost(d0, d1), want, atol=2e-6)


def test_reference_handles_structural_zeros():
    """-inf scores stay -inf in the plan, everything else stays finite, and the marginals hold on what is left; a row of -inf
    only (lse = -inf, stabiliser 0) gives -inf, not NaN, in its own row and leaves the other rows finite."""
    rng = np.random.default_rng(4)
    Z = rng.standard_normal((1, 9, 6))
    Z[0, :3, 1:4] = -np.inf
    lmu, lnu = cc._marginal(rng, 1, 9).astype(np.float64), cc._marginal(rng, 1, 6).astype(np.float64)
    P = cc.ref_sinkhorn(Z, lmu, lnu, 100)
    assert np.array_equal(np.isneginf(P), np.isneginf(Z)) and not np.isnan(P).any()
    np.testing.assert_allclose(np.exp(P).sum(1), np.exp(lnu), rtol=1e-12)
    assert np.isfinite(cc._lse(np.array([[0.0, -np.inf]]), 1)).all() and np.isneginf(cc._lse(np.full((1, 3), -np.inf), 1)).all()


def test_reference_is_finite_wherever_the_inputs_are():
    for M, N in cc.SINKHORN_SHAPES:
        c = cc.sinkhorn_case(M, N)
        assert c["Z"].dtype == np.float32 and c["Z"].shape == (cc.B_SINKHORN, M, N)
        assert all(np.isfinite(c["ref"][it]).all() for it in cc.SWEEPS_SINKHORN), (M, N)
        np.testing.assert_allclose(np.exp(c["log_mu"].astype(np.float64)).sum(1), 1.0, atol=1e-5)
        np.testing.assert_allclose(np.exp(c["log_nu"].astype(np.float64)).sum(1), 1.0, atol=1e-5)
    for M, N in cc.OT_SHAPES:
        c = cc.ot_case(M, N)
        assert c["scores"].shape == (cc.B_OT, M - 1, N - 1) and c["ns"].shape == (cc.B_OT, 1, N - 1)
        assert all(np.isfinite(c["ref"][it]).all() for it in cc.SWEEPS_OT), (M, N)
    for M, N in cc.COST_OT_SHAPES:
        assert all(np.isfinite(p).all() for p in cc.cost_ot_case(M, N)["ref"].values())
    assert np.isfinite(cc.many_case()["ref"]).all()
    for M, N in cc.GUARD_SHAPES:
        for entry in "so":
            g = cc.guard_case(M, N, entry)
            assert np.isfinite(g["ref"]).all(), (M, N, entry)                  # the wild problems included
            assert np.array_equal(np.isneginf(g["ref_inf"]), np.isneginf(_full(g, entry))) and not np.isnan(g["ref_inf"]).any()


def _full(g, entry):
    """The -inf batch as the solver sees it: the OT entry point appends a finite dustbin row and column."""
    if entry == "s":
        return g["Z_inf"]
    return cc.ot_problem(g["Z_inf"], g["alpha"], g["ns"])[0]


def test_every_amplitude_and_alpha_is_drawn():
    for M, N in cc.SINKHORN_SHAPES[:2]:                                         # both amplitudes within every batch
        Z = cc.sinkhorn_case(M, N)["Z"]
        for k in range(cc.B_SINKHORN):
            assert abs(float(Z[k].std()) / cc.AMPS[(cc.case_index(M, N) + k) % 2] - 1.0) < 0.02
    assert {cc.ot_case(M, N)["alpha"] for M, N in cc.OT_SHAPES} == set(cc.ALPHAS)
    assert len({cc.cost_ot_case(M, N)["alpha"] for M, N in cc.COST_OT_SHAPES}) >= 2
    for M, N in cc.COST_OT_SHAPES:                                              # the descriptors give scores of the case's spread
        c = cc.cost_ot_case(M, N)
        sd = float(cc.ref_cost(c["d0"], c["d1"]).std())
        assert 0.8 * cc.AMPS[cc.case_index(M, N) % 2] <= sd <= 1.25 * cc.AMPS[cc.case_index(M, N) % 2], (M, N, sd)


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_path_mirror_agrees_with_the_table():
    assert len(set(cc.SHAPES)) == len(cc.SHAPES) == 23
    for M, N, kernel_path, log_path, entries, why in cc.TABLE:
        assert cc.expected_path(M, N, "kernel", cc.B_SINKHORN) == kernel_path, (M, N)
        assert cc.expected_path(M, N, "log", cc.B_SINKHORN) == log_path, (M, N)
        assert log_path.startswith("wg") and why
    assert [s for s in cc.SHAPES if s not in cc.SINKHORN_SHAPES] == [(145, 145)] and cc.OT_SHAPES == cc.SHAPES
    assert all(s in cc.SHAPES for s in cc.COST_OT_SHAPES + cc.GUARD_SHAPES + [cc.MANY_MN])
    # the edges the table names, from the mirror
    assert cc.cu_shape(304, 320) and not cc.cu_shape(305, 320) and not cc.cu_shape(304, 321)
    assert cc.cu_shape(96, 96) and not cc.cu_shape(95, 97) and not cc.cu_shape(304, 30)
    assert cc.stream_shape(305, 319) and not cc.stream_shape(320, 304) and not cc.stream_shape(305, 300)
    assert cc.wg_threads(128, 128) == 1024 and cc.wg_threads(127, 129) == 256
    assert cc.expected_path(305, 320, "kernel", 65536) == "wg1024"              # the streaming solver takes at most 65 535 problems


def test_every_shape_fits_the_wg_kernel():
    """sinkhorn_wg_kernel is every case's log-mode solver and every flagged problem's fallback: (M + N) floats of LDS."""
    for M, N in cc.SHAPES:
        assert cc.wg_lds_bytes(M, N) <= 64 * 1024, (M, N)


def test_the_table_says_what_the_layout_gives():
    """slot_population / slice_population: how many waves hold a row in each of the 19 row slots, how many lanes a column in each
    of the 5 column slices - the statements of the 'why' column, recomputed."""
    sp, cp = cc.slot_population, cc.slice_population
    assert sp(304) == [16] * 19 and cp(320) == [64] * 5
    assert cp(319) == [64] * 4 + [63] and sp(303) == [16] * 18 + [15]
    assert sp(289)[17:] == [16, 1] and cp(257)[3:] == [64, 1]
    assert sp(288)[17:] == [16, 0] and cp(256)[3:] == [64, 0]
    assert sp(161)[9:12] == [16, 1, 0] and cp(65) == [64, 1, 0, 0, 0]
    assert sp(160)[9:] == [16] + [0] * 9 and cp(64) == [64, 0, 0, 0, 0]          # every second half (slots 10..18) is padding
    assert sp(120)[6:10] == [16, 8, 0, 0] and sp(145)[8:11] == [16, 1, 0]
    assert sp(29)[:3] == [16, 13, 0] and sp(30)[:3] == [16, 14, 0]
    assert cp(31) == [31, 0, 0, 0, 0]
    assert sp(301)[18] == 13 and cp(301)[4] == 45


# ---- the guard cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", cc.GUARD_SHAPES, ids=_ids(cc.GUARD_SHAPES))
@pytest.mark.parametrize("entry", ["s", "o"])
def test_guard_inputs_lie_where_the_gpu_test_assumes(M, N, entry):
    """The linear-domain solve is redone when a scaling a = exp(u + r), b = exp(v + c) ends outside (0, 2^30].  At the float64
    duals after 100 sweeps the tame problems' largest scaling is below 2^20 and the larger of the two wild problems' above 2^40,
    a thousandfold to either side of the guard: the GPU test's 1 <= trips <= 2 follows from the inputs, not from rounding.  (The
    other wild problem may end near the guard - 2^28.7 at (289, 257) with given marginals - and is held to its gate either way.)"""
    g = cc.guard_case(M, N, entry)
    big = np.maximum(g["amax"], g["bmax"])
    print("guard %dx%d %s: log2 of the largest final scaling per problem: %s" % (M, N, entry, np.round(np.log2(big), 1).tolist()))
    assert (big[list(cc.GUARD_TAME)] < 2.0 ** 20).all() and big[list(cc.GUARD_WILD)].max() > 2.0 ** 40
    assert np.abs(g["Z"][list(cc.GUARD_WILD)]).max() > 100.0 and np.abs(g["Z"][list(cc.GUARD_TAME)]).max() < 4.0
    # the -inf blocks: rows 0..4 x columns 7..19, and a block across column slices 0 / 1 and row slots 6..9
    assert np.isneginf(g["Z_inf"]).sum() == cc.GUARD_B * (5 * 13 + 40 * 10)
    rows, cols = cc.NEGINF_BLOCKS[1]
    assert {r // 16 for r in range(rows.start, rows.stop)} == {6, 7, 8, 9} and {c // 64 for c in range(cols.start, cols.stop)} == {0, 1}


def test_gates_are_the_projects():
    assert (cc.MASS_ATOL, cc.MASS_RTOL, cc.MARG_ATOL, cc.MARG_RTOL) == (1e-4, 2e-6, 1e-4, 3e-6)
    assert (cc.LOGPLAN_TOL, cc.LOGPLAN_MASS, cc.WILD_ATOL, cc.WILD_RTOL, cc.NEGINF_ATOL) == (2e-4, 1e-6, 2e-3, 2e-5, 3e-5)
    # plan_errors reports shares of those gates
    ref = np.log(np.array([[[0.5, 2.0], [1e-9, 1.0]]]))
    got = ref.copy()
    got[0, 0, 1] += 1e-4                                                       # mass 2 -> 2.0002: 2e-4 / (1e-4 + 4e-6)
    e = cc.plan_errors(got.astype(np.float32), got)
    assert max(e[k] for k in cc.GATES) < 0.01                                  # fp32 rounding of the plan alone
    e = cc.plan_errors(got, ref)
    assert abs(e["mass"] - 2.0001e-4 / (1e-4 + 4e-6)) < 1e-3 and abs(e["logplan"] - 0.5) < 1e-6
    with pytest.raises(AssertionError):
        cc.check_plan(got.astype(np.float32), ref, "moved entry")
    bad = ref.astype(np.float32)
    bad[0, 1, 0] = np.nan                                                      # a NaN on an entry of negligible mass still fails
    with pytest.raises(AssertionError):
        cc.check_plan(bad, ref, "nan entry")
