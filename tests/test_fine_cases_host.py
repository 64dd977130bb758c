"""Host side (-m "not gpu", oracle only): tests/fine_cases.py is held to what tests/test_fine_solver_edges_gpu.py relies on.
Every case lands in its regime under the fp32 model of the kernels' decisions, a factor 2^10 clear of the 2^30 guard on its side
of it, with the re-base counts and parities the table claims; the CPU oracle (fp32 with double accumulation - the best an fp32
evaluation does) passes the GPU tests' own gates against the float64 reference on every case and sweep count, with the
reference's non-finite pattern where there is one; the float64 reference satisfies its marginals; GATE_SCALE lists nothing that
the oracle's own error does not justify.  Each oracle figure is printed as a share of its gate (pytest -rA)."""
import numpy as np
import pytest

import coarse_cases as cc
import fine_cases as fc

# what the table claims of the stabilised re-solve at 100 sweeps: case -> (re-bases, parities of the sweeps they fall on)
CLAIMS = {
    "few_iid_16_o": (2, {0, 1}), "few_cols_8_o": (2, {1}), "few_iid_22_s": (2, {1}), "few_rows_16_s": (2, {0, 1}),
    "many_iid_36_o": (6, {0, 1}), "many_iid_70_o": (10, {0, 1}), "many_cols_25_o": (9, {0, 1}), "many_peak_24_o": (6, {0, 1}),
    "many_iid_70_s": (8, {0, 1}), "many_cols_35_s": (10, {0, 1}), "early_s": (4, {0, 1}), "early_o": (2, {0, 1}),
    "neginf_cols_25_o": (9, {0, 1}), "neginf_iid_36_o": (6, {0, 1}), "neginf_iid_70_s": (8, {0, 1}),
}


def oracle_plan(oracle, name, sweeps, bias=0.0):
    p = fc.problem(name)
    if fc.ROW[name][1] == "o":
        got = oracle.log_optimal_transport2(p["Z"][None], 1.0, p["ns"][None, None], sweeps)
        return (oracle.dustbin_bias(got, bias) if bias > 0 else got)[0]
    assert bias == 0
    return oracle.log_sinkhorn_iterations(p["Z"][None], p["log_mu"][None], p["log_nu"][None], sweeps)[0]


def biases(name):
    return fc.BIASES if fc.ROW[name][1] == "o" else (0.0,)


# ---- the regimes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_case_lands_in_its_regime(name):
    _, entry, regime, _, sweeps, _ = fc.ROW[name]
    v = fc.verdict(name)
    for it in sweeps:
        x = v[it]
        with np.errstate(divide="ignore"):
            print("%-18s %s (%s) it=%-3d plain: largest 2^%.1f smallest 2^%.1f %s | stabilised: re-bases at %s, guard %s" % (
                name, entry, regime, it, np.log2(x["hi"]), np.log2(x["lo"]), "FLAGGED" if x["tripped"] else "tame", x["rebases"],
                "holds" if x["ok"] else "fails -> log-sum-exp tail"))
        assert fc.clear_of_the_guard(x), (name, it, x["hi"], x["lo"])
        assert not x["rebases"] or x["rebases"][0] >= 1                       # no re-base at sweep 0
    full = v[100]
    reb = full["rebases"]
    if regime == "a":
        assert not any(v[it]["tripped"] for it in sweeps) and sweeps == fc.SWEEPS_ALL
        assert all(v[it]["hi"] <= fc.SCALE_GUARD / fc.MARGIN for it in sweeps)
    if regime == "b":
        assert full["tripped"] and full["ok"] and 1 <= len(reb) <= 2
    if regime == "c":
        assert full["tripped"] and full["ok"] and len(reb) >= 6
        assert not any(v[it]["tripped"] for it in sweeps if it < 100)          # at 1, 2 and 3 sweeps the block kernel keeps it
    if regime == "d":
        assert sweeps == fc.SWEEPS_ALL and all(v[it]["tripped"] for it in sweeps), "finite scores that trip by sweeps 1, 2 and 3"
        assert {s & 1 for s in reb} == {0, 1} and any(b - a == 1 for a, b in zip(reb, reb[1:])) and full["ok"]
        # one sweep: nothing re-bases, the stabilised solve is the plain one and fails its guard - the log-sum-exp tail
        assert v[1]["rebases"] == [] and not v[1]["ok"]
        assert np.isfinite(fc.problem(name)["Z"]).all()
    if regime == "e":
        Z = fc.problem(name)["Z"]
        assert full["tripped"] and full["ok"] and np.isneginf(Z).sum() == 5 * 13 + 10 * 11 and not np.isnan(Z).any()
        rows = fc.NEGINF_BLOCKS[1][0]
        assert rows.start < fc.SEAM_ROW <= rows.stop - 1 and fc.NEGINF_BLOCKS[0] == (slice(0, 5), slice(7, 20))
    if regime == "f":
        assert all(v[it]["tripped"] and not v[it]["ok"] for it in sweeps), "a non-finite problem must end in the log-sum-exp tail"
        assert not np.isfinite(fc.problem(name)["Z"]).all()
    if regime == "g":
        ns = fc.problem(name)["ns"].astype(np.float64)
        others = np.delete(ns, 31)
        assert ns[31] / others.max() >= fc.HEAVY / 4 and ns[31] / others.min() <= fc.HEAVY * 4      # 2^24 times the others' spread
        assert not full["tripped"]
    if name in CLAIMS:
        assert (len(reb), {s & 1 for s in reb}) == CLAIMS[name], (name, reb)
    else:
        assert regime in "afg"


def test_every_regime_and_entry_point_is_drawn():
    assert [t[2] for t in fc.TABLE] == sorted(t[2] for t in fc.TABLE) and {t[2] for t in fc.TABLE} == set(fc.REGIMES)
    for regime in "abcdef":
        assert {t[1] for t in fc.TABLE if t[2] == regime} == {"o", "s"}, regime
    assert any(t[4] == fc.SWEEPS_ALL for t in fc.TABLE if t[2] == "c")
    assert all(t[4] == fc.SWEEPS_ALL for t in fc.TABLE if t[2] in "ad")
    assert set(CLAIMS) == {t[0] for t in fc.TABLE if t[2] in "bcde"}
    # recipes: iid amplitude, a tenth of the rows / columns scaled, a planted permutation
    assert {"iid", "rows", "cols", "peak"} <= {t[3][0] for t in fc.TABLE}
    # the shared batches are what their names say
    assert all(fc.ROW[n][2] == "a" and fc.ROW[n][1] == "o" for n in fc.TAME_O)
    assert all(fc.flagged(n, 100) and fc.ROW[n][1] == "o" for n in fc.FLAGGED_O)
    assert all(fc.ROW[n][2] == "f" and fc.ROW[n][1] == "o" for n in fc.NONFINITE_O)
    assert {fc.ROW[n][2] for n in fc.MIXED_O} == set("abce") and {fc.ROW[n][2] for n in fc.DESC_O} == set("abcg")


@pytest.mark.parametrize("name", sorted(set(fc.DESC_O)))
def test_descriptor_form_of_a_case_keeps_its_verdict(name):
    """cost_ot sees the case through descriptors (fc.descriptors): the quantised scores, recovered exactly."""
    p, q = fc.problem(name), fc.problem(name, True)
    assert np.array_equal(q["Z"], fc.quantised(p["Z"])) and np.array_equal(q["Z64"], q["Z"].astype(np.float64))
    assert np.abs(q["Z"] - p["Z"]).max() <= 2.0 ** -(fc.DESC_BITS - 1) * np.abs(p["Z"]).max()
    v, w = fc.verdict(name)[100], fc.verdict(name, True)[100]
    assert fc.clear_of_the_guard(w) and w["tripped"] == v["tripped"] and w["ok"]
    d0, d1 = fc.descriptors([name])
    assert np.abs(d1).max() < 1023 and np.abs(d0).max() < 1023             # inside the fp16 split's range


# ---- the checker against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_oracle_within_the_gates_of_float64(oracle, name):
    """At every sweep count and every bias the GPU test runs (the oracle's own dustbin_bias on its fp32 plan)."""
    regime, sweeps = fc.ROW[name][2], fc.ROW[name][4]
    for it in sweeps:
        for k in biases(name):
            got = oracle_plan(oracle, name, it, k)
            rec = {}
            try:
                fc.check_case(got, name, it, k, what="oracle", record=rec)        # (the non-finite pattern is part of it)
            finally:
                print("oracle %-18s (%s) it=%-3d bias %g %s: %s" % (name, regime, it, k, "flagged" if fc.flagged(name, it) else "tame",
                                                                    " ".join("%s %.3f" % kv for kv in rec.items())))
            if regime in "ef":
                assert fc.same_nonfinite(got, fc.reference(name)[it]) and not np.isfinite(fc.reference(name)[it]).all()


@pytest.mark.parametrize("name", sorted(set(fc.DESC_O)))
def test_oracle_within_the_gates_of_float64_on_descriptor_cases(oracle, name):
    d0, d1 = fc.descriptors([name])
    S = oracle.cost(d0, d1)
    np.testing.assert_allclose(S[0], fc.problem(name, True)["Z64"], atol=2e-5, rtol=1e-5)           # test_coarse_level's gate on the cost
    got = oracle.log_optimal_transport2(S, 1.0, fc.problem(name)["ns"][None, None], 100)[0]
    e = fc.check_case(got, name, 100, what="oracle", desc=True)
    print("oracle %-18s through descriptors: %s" % (name, " ".join("%s %.3f" % kv for kv in e.items())))


def test_no_case_needed_a_wider_gate(oracle):
    """GATE_SCALE may list a (case, sweeps, entry, gate) only where the oracle itself misses the gate, with twice its error."""
    for ((name, it, k), entry, gate), factor in fc.GATE_SCALE.items():
        assert fc.ROW[name][1] == entry and it in fc.ROW[name][4] and k in biases(name)
        got, ref = oracle_plan(oracle, name, it, k), fc.with_bias(fc.reference(name)[it], k)
        e = fc.wild_errors(got, ref) if fc.flagged(name, it) else cc.plan_errors(got, ref)
        print("oracle %s it=%d bias %g: %.3f of gate '%s', listed factor %.3f" % (name, it, k, e[gate], gate, factor))
        assert e[gate] > 1.0 and abs(factor - 2.0 * e[gate]) <= 0.01 * factor, (name, it, k, gate, e[gate], factor)


def test_bias_is_the_oracles_dustbin_bias(oracle):
    ref = fc.reference("tame_iid_half_o")[100]
    for k in (2.0, 3.0):
        want = oracle.dustbin_bias(ref.astype(np.float32)[None], k)[0]
        got = fc.with_bias(ref, k)
        np.testing.assert_allclose(got, want, atol=2e-6)
        assert abs((got - ref)[fc.NB, fc.NB] - 2 * np.log(k)) < 1e-12 and abs((got - ref)[3, fc.NB] - np.log(k)) < 1e-12
        assert np.array_equal((got - ref)[:fc.NB, :fc.NB], np.zeros((fc.NB, fc.NB)))
    assert fc.with_bias(ref, 0.0) is ref


# ---- the reference itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [t[0] for t in fc.TABLE if t[2] == "a"])
def test_reference_satisfies_both_marginals_on_the_tame_cases(name):
    p, ref = fc.problem(name), fc.reference(name)[100]
    if fc.ROW[name][1] == "o":
        log_mu, log_nu, norm = fc.ot2_marginals(p["ns"][None])
        ref, log_mu, log_nu = ref + norm[0], log_mu[0], log_nu[0]
    else:
        log_mu, log_nu = p["log_mu"].astype(np.float64), p["log_nu"].astype(np.float64)
    P = np.exp(ref)
    np.testing.assert_allclose(P.sum(0), np.exp(log_nu), rtol=0, atol=1e-9)
    np.testing.assert_allclose(P.sum(1), np.exp(log_mu), rtol=0, atol=1e-9)


def test_ot2_marginals_are_the_reference_modules():
    """modules.py:165-182: ms = (m - 1) * one, norm = -log(ms + sum ns), log_nu = [log ns + norm, log ms + norm], log_mu =
    [norm x 144, log sum ns + norm]; in float32 as MODE 2 of sinkhorn_rc_kernel forms them, to fp32 rounding."""
    ns = fc.problem("tame_iid_4_o")["ns"]
    lmu, lnu, norm = fc.ot2_marginals(ns[None])
    s = ns.astype(np.float64).sum()
    assert abs(norm[0] + np.log(144 + s)) < 1e-14 and lmu.shape == lnu.shape == (1, 145)
    np.testing.assert_allclose(lmu[0], np.r_[np.full(144, norm[0]), np.log(s) + norm[0]], rtol=0, atol=1e-14)
    np.testing.assert_allclose(lnu[0], np.r_[np.log(ns.astype(np.float64)) + norm[0], np.log(144.0) + norm[0]], rtol=0, atol=1e-14)
    np.testing.assert_allclose(np.exp(lmu).sum(), 1.0, rtol=1e-12)
    np.testing.assert_allclose(np.exp(lnu).sum(), 1.0, rtol=1e-12)
    l32 = fc.ot2_marginals(ns[None], dtype=np.float32)
    assert l32[0].dtype == np.float32
    np.testing.assert_allclose(l32[0], lmu, atol=2e-6)
    np.testing.assert_allclose(l32[1], lnu, atol=2e-6)
    p = fc.problem("tame_iid_4_o")
    assert np.array_equal(p["log_mu32"], l32[0][0]) and np.array_equal(p["log_nu32"], l32[1][0])


# ---- the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["few_iid_16_o", "many_iid_70_o", "many_cols_35_s", "early_s", "early_o", "neginf_iid_70_s"])
def test_model_of_the_stabilised_solve_reaches_the_reference(name):
    """The model re-bases as the kernel does (r -= ln a, c -= ln b): its duals give the float64 plan to fp32 resolution of the
    scores.  With the sign of the absorption turned (the first mutant the GPU test must catch) it does not come near."""
    p, v = fc.problem(name), fc.verdict(name)[100]
    plan = p["Z"].astype(np.float64) + v["u"].astype(np.float64)[:, None] + v["v"].astype(np.float64)[None, :]
    if fc.ROW[name][1] == "o":
        plan = plan - fc.ot2_marginals(p["ns"][None])[2][0]
    ref = fc.reference(name)[100]
    fin = np.isfinite(ref)
    d = float(np.abs(plan[fin] - ref[fin]).max())
    print("%s: model's plan within %.3g of float64 (|Z| up to %.0f)" % (name, d, np.abs(ref[fin]).max()))
    assert v["ok"] and d <= fc.WILD_ATOL


def test_model_details():
    p = fc.problem("many_iid_70_o")
    v = fc.stab_model(p["Z"], p["log_mu32"], p["log_nu32"], (1, 2, 100))
    assert v[1]["rebases"] == [] and all(r >= 1 for r in v[100]["rebases"])
    assert v[2]["rebases"] == [r for r in v[100]["rebases"] if r < 2]        # one run gives every smaller count's prefix
    # a tame problem never drifts: both models iterate alike
    t = fc.problem("tame_iid_4_o")
    a, b = fc.plain_model(t["Z"], t["log_mu32"], t["log_nu32"], (100,))[100], fc.stab_model(t["Z"], t["log_mu32"], t["log_nu32"], (100,))[100]
    assert not a["tripped"] and b["ok"] and b["rebases"] == []
    # a dead scaling is not absorbed and fails the guard; exp results below 2^-126 are flushed
    K = fc._kernel_matrix(np.array([[0.0, -88.0]], np.float32), np.zeros(1, np.float32), np.zeros(2, np.float32))
    assert K[0, 0] == 1.0 and K[0, 1] == 0.0
    n = fc.problem("nan_score_o")
    assert not fc.stab_model(n["Z"], n["log_mu32"], n["log_nu32"], (100,))[100]["ok"]


def test_gates_are_the_projects():
    assert (fc.MASS_ATOL, fc.MASS_RTOL, fc.MARG_ATOL, fc.MARG_RTOL) == (1e-4, 2e-6, 1e-4, 3e-6)
    assert (fc.LOGPLAN_TOL, fc.LOGPLAN_MASS, fc.WILD_ATOL, fc.WILD_RTOL, fc.NEGINF_ATOL) == (2e-4, 1e-6, 2e-3, 2e-5, 3e-5)
    ref = fc.reference("few_iid_16_o")[100]
    good = ref.astype(np.float32)
    e = fc.check_case(good, "few_iid_16_o", 100)
    assert set(e) == {"wild", "mass"} and max(e.values()) < 0.2
    bad = good.copy()
    bad[5, 9] += np.float32(2 * (fc.WILD_ATOL + fc.WILD_RTOL * abs(ref[5, 9])))
    with pytest.raises(AssertionError):
        fc.check_case(bad, "few_iid_16_o", 100)
    bad = good.copy()
    bad[5, 9] = np.nan
    with pytest.raises(AssertionError):
        fc.check_case(bad, "few_iid_16_o", 100)
    i, j = np.unravel_index(int(np.argmax(ref[:fc.NB, :fc.NB])), (fc.NB, fc.NB))          # an entry that carries mass
    bad = good.copy()
    bad[i, j] += np.float32(3e-4 / np.exp(ref[i, j]) + 1e-5)
    with pytest.raises(AssertionError):
        fc.check_case(bad, "few_iid_16_o", 100)
    tame = fc.reference("tame_iid_4_o")[3].astype(np.float32)
    assert set(fc.check_case(tame, "tame_iid_4_o", 3)) == {"mass", "rows", "cols", "logplan"}
    allnan = fc.reference("nan_score_o")[100].astype(np.float32)
    assert fc.check_case(allnan, "nan_score_o", 100) == dict(neginf=0.0)
    with pytest.raises(AssertionError):
        fc.check_case(np.zeros_like(allnan), "nan_score_o", 100)
