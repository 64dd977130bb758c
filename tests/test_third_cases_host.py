"""Host side (-m "not gpu", oracle only): tests/third_cases.py is held to what tests/test_third_solver_edges_gpu.py relies on.
Every case lands in its regime under the fp32 model of the kernels' decisions with a factor 2^10 to spare; the stabilised
solve's final guard never fails in the model; the CPU oracle (oracle.cost -> log_optimal_transport2 -> compute_result) passes
the GPU tests' own gates against the float64 reference and the float64 restatement of Compute_result on every case and sweep
count; the near-tie mask leaves out at most 2 % of a regime's centre rows; GATE_SCALE lists nothing the oracle's own error does
not justify.  The oracle's largest share of every gate is printed per regime (pytest -rA)."""
import numpy as np
import pytest

import third_cases as tc

# what the table claims of the stabilised solve at 100 sweeps: case -> the sweeps after which it re-bases
CLAIMS = {
    "few_iid_20": [4, 9], "few_cols_10": [4, 11],
    "many_iid_40": [4, 9, 15, 22, 33, 84], "many_cols_20": [4, 10, 17, 27, 42, 65],
    "many_rows_40": [4, 9, 14, 19, 24, 30, 38, 49, 66, 90], "many_peak_40": [15, 32, 49, 66, 83, 100],
    "last_early_100": [1, 2, 3], "neginf_cols_20": [4, 10, 17, 28, 44, 67], "neginf_cols_10": [4, 11],
}
_WORST = {}


def oracle_case(oracle, name, sweeps):
    """(log-plan [65, 65], matches dict or None) of the CPU oracle; through descriptors where the case has them."""
    p = tc.problem(name)
    if tc.ROW[name][7] and tc.ROW[name][1] != "f":      # (an infinite score is a NaN in the kernels' cost build: predicted_scores)
        d0, d1 = tc.descriptors([name])
        S = oracle.cost(d0, d1)
        fin = np.isfinite(tc.kernel_scores(name))
        assert np.array_equal(S[0][fin], tc.kernel_scores(name)[fin]) and tc.same_nonfinite(S[0], tc.kernel_scores(name)), \
            "%s: the oracle's cost is not the predicted scores" % name
    else:
        S = tc.kernel_scores(name)[None]
    Z = oracle.log_optimal_transport2(S, 1.0, p["ns"][None, None], sweeps)
    if not tc.ROW[name][7]:
        return Z[0], None
    sq = np.sqrt(p["ns"] + np.float32(1e-8)).astype(np.float32)
    with np.errstate(all="ignore"):
        m0, m1, _, label, ifm = oracle.compute_result(np.exp(Z), sq[None], sq[None], p["p_s"][None], p["p_t"][None], True)
        conf = tc.compute_result_ref(np.exp(Z[0].astype(np.float64)), p["ns"], p["p_s"], p["p_t"])["conf"]      # the oracle returns none
    return Z[0], dict(m0=m0[0], m1=m1[0], label=label.reshape(16, 2), ifm=ifm[0], conf=conf)


# ---- the regimes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_case_lands_in_its_regime(name):
    _, regime, _, sweeps, _, _, _, desc = tc.ROW[name]
    v = tc.verdict(name)
    for it in sweeps:
        x = v[it]
        with np.errstate(divide="ignore"):
            print("%-15s (%s) it=%-3d plain: largest 2^%.1f smallest 2^%.1f %s | stabilised: re-bases after %s (band / 2^10: %d, * 2^10: %d), %s"
                  % (name, regime, it, np.log2(x["hi"]), np.log2(x["lo"]), "FLAGGED" if x["tripped"] else "tame", x["rebases"],
                     len(x["narrow"]), len(x["wide"]), "BAILS OUT at sweep %d" % x["bail"] if x["bail"] else "no bail-out"))
        assert x["sure"], (name, it, x["hi"], x["lo"])
        assert x["bail_sure"], (name, it, x["bail"])
        # the statement about the final guard: with at least one sweep the stabilised solve either bails out or passes it
        assert x["bail"] or x["ok"], (name, it)
    full = v[100]
    if regime == "a":
        assert sweeps == tc.SWEEPS_ALL and not any(v[it]["tripped"] for it in sweeps)
    if regime == "b":
        assert full["tripped"] and not full["bail"] and 1 <= len(full["rebases"]) <= 2
    if regime == "c":
        assert full["tripped"] and not full["bail"] and len(full["rebases"]) >= 6
    if regime == "d":
        assert np.isfinite(tc.kernel_scores(name)).all() and sweeps == tc.SWEEPS_ALL
        for it in tc.LAST_SWEEP_REBASE[name]:
            x = v[it]       # flagged, and the LAST sweep re-bases wherever the band's edges lie within 2^10 of 2^-20 / 2^20
            assert x["tripped"] and not x["bail"] and it in x["rebases"] and it in x["narrow"] and it in x["wide"], (name, it)
    if regime == "f":
        assert all(v[it]["tripped"] and v[it]["bail"] == 1 for it in sweeps) and not np.isfinite(tc.kernel_scores(name)).all()
    if regime == "g":
        Z = tc.kernel_scores(name)
        assert full["tripped"] and not full["bail"] and not desc and full["rebases"]
        assert np.isneginf(Z).sum() == 5 * 13 + 12 * 11 and not np.isnan(Z).any()
        assert set(tc.CENTRE_ROWS) & set(range(26, 38))                     # a block crosses centre rows
    if name in CLAIMS:
        assert full["rebases"] == CLAIMS[name], (name, full["rebases"])
    else:
        assert regime in "af"


def test_every_regime_is_drawn_and_no_finite_case_bails_out():
    assert [t[1] for t in tc.TABLE] == sorted(t[1] for t in tc.TABLE) and {t[1] for t in tc.TABLE} == set(tc.REGIMES)
    assert {"iid", "rows", "cols", "peak"} <= {t[2][0] for t in tc.TABLE if t[1] in "bc"}
    assert set(CLAIMS) == {t[0] for t in tc.TABLE if t[1] in "bcdg"}
    assert all(tc.ROW[n][1] == "a" for n in tc.TAME)
    # regime (e), a bail-out with finite inputs, has no case: the recipes hold no finite input whose stabilised solve bails out by 2^10 - the largest scaling of
    # one sweep is bounded by the smallest ns (2^-126 in float32: 2^131), short of 3e38 * 2^10; regime (f) carries the tail
    for n in tc.NAMES:
        if np.isfinite(tc.kernel_scores(n)).all():
            assert not any(x["bail"] for x in tc.verdict(n).values()), n
    rng = np.random.default_rng(5)
    Z = tc._build(("early", 200.0), rng).astype(np.float32)
    ns = (tc.synth_draw()["area"][0].astype(np.float64) * 2.0 ** -120).astype(np.float32)
    v = tc.model(Z, ns, (1,))[1]
    assert not (v["bail"] and v["bail_sure"]), "an extreme-marginal case bails out by the margin: regime (e) exists, add it"


def test_descriptor_form_is_the_score_form():
    names = [n for n in tc.NAMES if tc.ROW[n][7]]
    d0, d1 = tc.descriptors(names)
    S = tc.predicted_scores(d0, d1)
    for k, n in enumerate(names):
        p = tc.problem(n)
        if tc.ROW[n][1] != "f":
            assert np.array_equal(S[k], p["Z"]) and np.array_equal(p["Zq"], tc.quantised(p["Zq"])), n
            assert np.abs(p["Z"] - p["Zq"]).max() <= 2.0 ** -23 * np.abs(p["Zq"]).max(), n           # the one rounding of 0.1f * x
        else:
            assert np.isnan(S[k][:, 41]).sum() >= 64 and np.isfinite(np.delete(S[k], 41, 1)).all(), n     # one element, one column
    assert tc.DESC_D == 256 and np.abs(d1[np.isfinite(d1)]).max() * 160 < 2.0 ** 24 * 160


# ---- the checker against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES)
def test_oracle_within_the_gates_of_float64(oracle, name):
    regime = tc.ROW[name][1]
    for it in tc.all_sweeps(name):
        Z, got = oracle_case(oracle, name, it)
        rec = {}
        try:
            tc.check_plan(Z, name, it, what="oracle", record=rec)
            if got is not None:
                tc.check_matches(got, name, it, what="oracle", record=rec)
        finally:
            tc.fold(_WORST, regime, rec)
            print("oracle %-15s (%s) it=%-3d %s: %s" % (name, regime, it, "flagged" if tc.flagged(name, it) else "tame",
                                                        " ".join("%s %.3f" % kv for kv in rec.items())))
    print(tc.report({k: s for k, s in _WORST.items() if k[0] == regime}, "oracle, so far:"))


def test_near_tie_mask_leaves_out_at_most_two_percent_per_regime():
    for regime in tc.REGIMES:
        refs = [tc.match_reference(n, it) for n in tc.NAMES if tc.ROW[n][1] == regime and tc.ROW[n][7] for it in tc.all_sweeps(n)]
        if refs:
            share = tc.unclear_share(refs)
            print("regime (%s): the near-tie mask leaves out %.2f %% of %d finite centre rows" % (
                regime, 100 * share, sum(int(r["finite"].sum()) for r in refs)))
            assert share <= tc.CLEAR_CAP, (regime, share)


def test_no_case_needed_a_wider_gate(oracle):
    """GATE_SCALE may list a (case, sweeps, gate) only where the oracle itself misses the gate, with twice its share."""
    for ((name, it), gate), factor in tc.GATE_SCALE.items():
        assert it in tc.all_sweeps(name)
        Z, _ = oracle_case(oracle, name, it)
        ref = tc.reference(name)[it]
        e = tc.wild_errors(Z, ref) if tc.flagged(name, it) else tc.plan_errors(Z, ref)
        print("oracle %s it=%d: %.3f of gate '%s', listed factor %.3f" % (name, it, e[gate], gate, factor))
        assert e[gate] > 1.0 and abs(factor - 2.0 * e[gate]) <= 0.01 * factor, (name, it, gate, e[gate], factor)


def test_wild_family_oracle_within_the_gates(oracle):
    """The D = 128 family: the 32 amplified problems of the redo-walk base set, solved in float64 from the oracle's scores."""
    w = tc.wild_inputs()
    S = oracle.cost(w["d0"], w["d1"])
    ref, mref, verdicts = tc.wild_references(S)
    Z = oracle.log_optimal_transport2(S, 1.0, w["scale"][:, None, :], 100)
    sq = np.sqrt(w["scale"] + np.float32(1e-8)).astype(np.float32)
    m0, m1, _, label, ifm = oracle.compute_result(np.exp(Z), sq, sq, w["p_s"], w["p_t"], True)
    worst, scale = {}, tc.wild_gate_scale(Z, ref)
    for k in range(tc.WILD_N):
        conf = tc.compute_result_ref(np.exp(Z[k].astype(np.float64)), w["scale"][k], w["p_s"][k], w["p_t"][k])["conf"]
        got = dict(m0=m0[k], m1=m1[k], label=label.reshape(-1, 16, 2)[k], ifm=ifm[k], conf=conf)
        rec = {}
        tc.check_matches_case(got, mref[k], "oracle wild %d" % k, rec)
        e = tc.wild_errors(Z[k], ref[k])
        rec.update(wild=e["wild"], mass=e["mass"])
        tc.fold(worst, "x%g" % tc.WILD_AMPS[k], rec)
        assert all(e[g] <= scale[k][g] for g in ("wild", "mass")), (k, e, scale[k])
        assert all(scale[k][g] == 1.0 for g in ("wild", "mass")) or tc.WILD_AMPS[k] >= 9.0, (k, scale[k])      # amplitudes 3 and 5 need none
    print(tc.report(worst, "oracle, D = 128:"))
    print("model: %d of 32 flagged, %d of them by 2^10" % (sum(v["tripped"] for v in verdicts),
                                                          sum(v["tripped"] and tc.clear_of_the_guard(v) for v in verdicts)))
    assert tc.unclear_share(mref) <= tc.CLEAR_CAP
    assert sum(v["tripped"] for v in verdicts) >= 8


# ---- the reference and the restatement themselves ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.TAME)
def test_reference_satisfies_both_marginals_on_the_tame_cases(name):
    p = tc.problem(name)
    lmu, lnu, norm = tc.ot2_marginals(p["ns"][None])
    P = np.exp(tc.reference(name)[100] + norm[0])
    np.testing.assert_allclose(P.sum(0), np.exp(lnu[0]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(P.sum(1), np.exp(lmu[0]), rtol=0, atol=1e-9)
    s = p["ns"].astype(np.float64).sum()
    assert abs(norm[0] + np.log(64 + s)) < 1e-14 and abs(np.exp(lmu).sum() - 1) < 1e-12 and abs(np.exp(lnu).sum() - 1) < 1e-12
    assert np.array_equal(tc.reference(name)[0], p["Z"].astype(np.float64) - norm[0])        # 0 sweeps: Z - norm


def test_restatement_of_compute_result():
    assert list(tc.CENTRE_ROWS) == [18, 19, 20, 21, 26, 27, 28, 29, 34, 35, 36, 37, 42, 43, 44, 45]
    S = np.full((65, 65), 1e-6)
    area = np.full(64, 0.25, np.float32)
    S[18, 27] = 0.5                                   # centre row 0 points at target (3, 3): a symmetric window, no offset
    S[19, 0] = 0.5                                    # centre row 1 at the corner (0, 0): the padding pulls the mean
    S[20, 64] = 0.7                                   # centre row 2: the dustbin wins
    r = tc.compute_result_ref(S, area, (8, 12), (40, 44), True)
    assert np.allclose(r["m1"][0], ((3 + 0.5 - 4) * 2 + 40, (3 + 0.5 - 4) * 2 + 44), atol=1e-12)
    assert r["m1"][1][0] > (0 + 0.5 - 4) * 2 + 40 - 4 and r["m1"][1][0] != (0 + 0.5 - 4) * 2 + 40
    assert np.array_equal(r["m0"][0], (8 - 3, 12 - 3)) and np.array_equal(r["m0"][15], (8 + 3, 12 + 3))
    assert r["ifm"][0] and r["ifm"][1] and not r["ifm"][2]
    assert list(r["label"][0]) == [1e8, 1e8] and list(r["label"][2]) == [-10.0, 1e8]
    assert abs(r["conf"][0] - (0.5 + 24e-6) / (0.5 + 64e-6)) < 1e-12
    indoor = tc.compute_result_ref(S, area, (8, 12), (40, 44), False)
    assert [q for q in range(16) if indoor["label"][q][0] == 1e8] == [5, 7, 13, 15]
    assert tc.clear_rows(r)[0] and not tc.clear_rows(r)[3]                  # a uniform row is a tie
    nan = tc.compute_result_ref(np.full((65, 65), np.nan), area, (8, 12), (40, 44), True)
    assert nan["allnan"].all() and np.isnan(nan["m1"]).all() and nan["ifm"].all() and np.isnan(nan["conf"]).all()


def test_gates_bite():
    assert (tc.M1_TOL, tc.CONF_TOL, tc.CLEAR_REL, tc.MARGIN) == (3e-4 * 8, 1e-4, 1e-3, 1024.0)
    assert (tc.MASS_ATOL, tc.MASS_RTOL, tc.MARG_ATOL, tc.MARG_RTOL) == (1e-4, 2e-6, 1e-4, 3e-6)
    assert (tc.LOGPLAN_TOL, tc.LOGPLAN_MASS, tc.WILD_ATOL, tc.WILD_RTOL, tc.NEGINF_ATOL) == (2e-4, 1e-6, 2e-3, 2e-5, 3e-5)
    name = "few_iid_20"
    ref, m = tc.reference(name)[100], tc.match_reference(name, 100)
    good = {k: m[k].astype(np.float32) if k != "ifm" else m[k] for k in ("m0", "m1", "label", "ifm", "conf")}
    assert max(tc.check_matches(good, name, 100).values()) < 0.1
    q = int(np.flatnonzero(tc.clear_rows(m))[0])
    for key, delta in (("m1", 2 * tc.M1_TOL), ("conf", 2 * tc.CONF_TOL), ("m0", 1.0)):
        bad = dict(good, **{key: good[key].copy()})
        bad[key][q] += np.float32(delta)
        with pytest.raises(AssertionError):
            tc.check_matches(bad, name, 100)
    bad = dict(good, ifm=~good["ifm"])
    with pytest.raises(AssertionError):
        tc.check_matches(bad, name, 100)
    assert set(tc.check_plan(ref.astype(np.float32), name, 100)) == {"wild", "mass"}
    assert set(tc.check_plan(tc.reference(name)[3].astype(np.float32), name, 3)) == {"mass", "rows", "cols", "logplan"}
    z = ref.astype(np.float32)
    z[5, 9] += np.float32(2 * (tc.WILD_ATOL + tc.WILD_RTOL * abs(ref[5, 9])))
    with pytest.raises(AssertionError):
        tc.check_plan(z, name, 100)
    assert tc.expected_counts("kernel", tc.cases_at(100), 100) == (9, 2) and tc.expected_counts("log", tc.cases_at(100), 100) == (0, 0)
    assert tc.expected_counts("kernel", tc.cases_at(100), 100, stab=False) == (9, 0) and tc.expected_counts("kernel", tc.cases_at(0), 0) == (0, 0)


def test_model_of_the_stabilised_solve_reaches_the_reference():
    """The model re-bases as the kernel does (r -= ln a, c -= ln b): its duals give the float64 plan to fp32 resolution."""
    for name in ("few_iid_20", "many_rows_40", "last_early_100"):
        p, v = tc.problem(name), tc.verdict(name)[100]
        norm = tc.ot2_marginals(p["ns"][None])[2][0]
        plan = p["Z"].astype(np.float64) + v["u"].astype(np.float64)[:, None] + v["v"].astype(np.float64)[None, :] - norm
        d = float(np.abs(plan - tc.reference(name)[100]).max())
        print("%s: model's plan within %.3g of float64" % (name, d))
        assert d <= tc.WILD_ATOL + tc.WILD_RTOL * np.abs(tc.reference(name)[100]).max()
