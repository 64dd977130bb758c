"""Host side (-m "not gpu", oracle only): the dispatch mirror, the case tables and the float64 references of
tests/stream_cases.py are held to what tests/test_stream_solver_edges_gpu.py relies on.  The CPU oracle (fp32 with double
accumulation) must pass the GPU tests' own gates against float64 on every case - the four project gates and the every-entry
gate - and its share of each is printed (pytest -rA).  Every row's plan on 256 CUs is recomputed from the mirror, the guard
inputs are checked to lie on the side of the 2^30 guard the GPU test assumes, and the coverage of the project's masked log-plan
gate at these shapes - the reason for the every-entry gate - is measured."""
import numpy as np
import pytest

import coarse_cases as cc
import stream_cases as sc


def _ids(rows):
    return [sc.row_id(r) for r in rows]


# ---- the mirror and the tables ------------------------------------------------------------------------------------------------
def test_every_row_reaches_its_plan_on_256_cus():
    keys = [(r.M, r.N, r.batch) for r in sc.ALL_ROWS]
    assert len(set(keys)) == len(keys) == 16 + 3 + 8 + 2
    for r in sc.ALL_ROWS:
        assert cc.expected_path(r.M, r.N, "kernel", r.batch) == "stream", sc.row_id(r)
        assert cc.wg_lds_bytes(r.M, r.N) <= 64 * 1024                              # the hand-over's kernel takes the shape
        p = sc.stream_plan(r.M, r.N, r.batch)
        assert sc.plan_matches(p, r.plan), (sc.row_id(r), p, r.plan)
        print("%-14s %s" % (sc.row_id(r), sc.fmt_plan(p)))
    assert all(sc.stream_plan(r.M, r.N, r.batch).res_kind == 0 for r in sc.TWO_LAUNCH + sc.TWO_LAUNCH_BIG)
    assert all(sc.stream_plan(r.M, r.N, r.batch).res_kind == 2 for r in sc.RESIDENT_32)
    assert all(sc.stream_plan(r.M, r.N, r.batch).res_kind == 3 for r in sc.RESIDENT_64)


def test_mirror_on_the_shapes_the_suite_already_runs():
    """Plans the code's comments and the existing tests state: 4097^2 alone is <17, 9, 32> with 241 blocks; 16 x 769^2 is
    <64, 2, 64> with 13 blocks a problem behind a rounded stride (49 x 769 is odd); zero sweeps and more problems than CUs are
    never resident; a stream masked to 160 CUs does not hold 241 workgroups."""
    p = sc.stream_plan(4097, 4097, 1)
    assert (p.cpt, p.RB, p.nblk, p.res_kind, p.res_nblk, p.ngroups) == (9, 17, 241, 1, 241, 129)
    assert sc.stream_plan(4097, 4097, 1, n_cu=160).res_kind == 0 and sc.stream_plan(4097, 4097, 2).res_kind == 0
    p = sc.stream_plan(769, 769, 16)
    assert (p.res_kind, p.res_nblk, p.ngroups, p.rounded) == (3, 13, 13, True)
    assert sc.stream_plan(769, 769, 1).res_kind == 2 and sc.stream_plan(769, 769, 1).res_nblk == 25
    assert sc.stream_plan(500, 500, 3, iters=0).res_kind == 0 and sc.stream_plan(520, 501, 300).res_kind == 0
    assert sc.stream_plan(2000, 520, 1).res_nblk == 63
    # the rows whose batch is not three, and why: what three (or two) problems would reach instead
    assert sc.stream_plan(3100, 200, 3)[3:5] == (3, 49) and sc.stream_plan(4096, 62, 3)[3:5] == (3, 64)
    assert sc.stream_plan(4097, 62, 3)[3:5] == (3, 65) and sc.stream_plan(4097, 62, 2)[3:5] == (3, 65)
    # the four conditions behind `fits`, each the one that refuses
    assert sc.stream_plan(480, 1024, 3).why_not == "groups" and sc.stream_plan(4097, 62, 1).why_not == "slices"
    # (for N <= 1024 the grid and area conditions follow from `need` and M N >= 500^2: fewer CUs or more problems give 64-row
    #  blocks or no candidate at all, never a refusal)
    assert sc.stream_plan(2100, 300, 4)[3:5] == (3, 33) and sc.stream_plan(520, 501, 3, n_cu=40)[3:5] == (3, 9)
    assert {sc.stream_plan(M, N, b, n).why_not for M in (245, 500, 4096) for N in (62, 245, 1024) for b in (1, 7) for n in (40, 256)} <= {"", "groups", "slices"}
    assert sc.res_partial_stride(520, 501) == 16536 and sc.res_partial_stride(500, 500) == 16000


def test_the_tables_say_what_the_layout_gives():
    """The 'what it walks' column, recomputed."""
    def owners(N, q):                                                              # threads of the two-launch form holding a column in slot q
        return sum(1 for t in range(sc.ST) if t + sc.ST * q < N)
    for N, cpt in ((513, 2), (1025, 3), (1537, 4), (2049, 5), (2561, 6), (3073, 7), (3585, 8), (4097, 9)):
        assert owners(N, cpt - 1) == 1 and owners(N, cpt - 2) == sc.ST
    assert owners(4608, 8) == sc.ST and owners(250, 0) == 250
    assert 190 - 11 * 16 == 14 and 38 - 2 * 16 == 6 and 64 % 16 == 0 and 270 - 15 * 17 == 15
    # the column reduce: wave w sums blocks w + 16 q, 18 of them in flight, the rest in the tail loop
    tail = lambda nblk: [len(range(w + 16 * 18, nblk, 16)) for w in range(16)]      # noqa: E731
    assert sum(tail(288)) == 0 and tail(289) == [1] + [0] * 15 and tail(294) == [1] * 6 + [0] * 10
    # the resident reducer: slice rs < 32 holds blocks rs + 32 k
    held = lambda nblk, k: sum(1 for rs in range(sc.NSL) if rs + sc.NSL * k < nblk)   # noqa: E731
    assert [held(35, k) for k in range(4)] == [32, 3, 0, 0] and [held(66, k) for k in range(4)] == [32, 32, 2, 0]
    assert [held(97, k) for k in range(4)] == [32, 32, 32, 1] and [held(128, k) for k in range(4)] == [32] * 4
    assert [held(16, k) for k in range(4)] == [16, 0, 0, 0] and held(63, 1) == 31
    assert 500 - 15 * 32 == 20 and 481 - 15 * 32 == 1 and 520 - 8 * 64 == 8 and 513 - 8 * 64 == 1 and (501 + 3) & ~3 == 504
    # batch 16 of 270 rows: 272 workgroups of 16 rows, 256 of 17
    assert 16 * sc._ceil(270, 16) == 272 and 16 * sc._ceil(270, 17) == 256
    # the -inf blocks: a row-block boundary of the plan's form and the end of a reduce group of 64 columns
    for (M, N), blocks in sc.NEGINF_BLOCKS.items():
        rows, cols = blocks[1]
        rb = 16 if sc.stream_plan(M, N, 6).res_kind == 0 else 32
        assert len({i // rb for i in range(rows.start, rows.stop)}) == 2 and {j // 64 for j in range(cols.start, cols.stop)} == {3, 4}
        assert cols.stop <= N - 1 and rows.stop <= M - 1                           # inside the OT entry point's scores too
    # the guard rows reach the three forms, and the tame problems alone the same one
    kinds = []
    for M, N, batch, wild in sc.GUARD_ROWS:
        p, q = sc.stream_plan(M, N, batch), sc.stream_plan(M, N, batch - len(wild))
        assert (p.res_kind, p.res_nblk) == (q.res_kind, q.res_nblk)
        kinds.append(p.res_kind)
    assert kinds == [0, 2, 3]
    assert [sc.stream_plan(M, N, 1).res_kind for M, N in sc.LOUD_SHAPES] == [0, 2, 0]


def test_no_case_needed_a_wider_gate():
    assert sc.GATE_SCALE == {} and cc.GATE_SCALE == {}
    assert (sc.LOGPLAN_TOL, sc.WILD_ATOL, sc.WILD_RTOL, sc.NEGINF_ATOL) == (2e-4, 2e-3, 2e-5, 3e-5)


# ---- the oracle against float64 under the GPU tests' gates ------------------------------------------------------------------------
@pytest.mark.parametrize("row", sc.SMALL_ROWS, ids=_ids(sc.SMALL_ROWS))
def test_oracle_within_all_gates_of_float64(oracle, row):
    M, N, B = row.M, row.N, row.batch
    plan = sc.stream_plan(M, N, B)
    c = sc.sinkhorn_case(M, N, B)
    assert c["Z"].shape == (B, M, N) and c["Z"].dtype == np.float32
    for k in range(B):
        assert abs(float(c["Z"][k].std()) / sc.AMPS[((sc.row_index(M, N, B) if B > 1 else 1) + k) % 2] - 1.0) < 0.03
    for it in (1, 100):
        assert np.isfinite(c["ref"][it]).all()
        got = oracle.log_sinkhorn_iterations(c["Z"], c["log_mu"], c["log_nu"], it)
        e = sc.check_all(got, c["ref"][it], "oracle sinkhorn %s it=%d" % (sc.row_id(row), it), plan, (M, N, B), "s")
        print("oracle sinkhorn %-10s it=%-3d: %s; masked gate covers %.1f %%" % (
            sc.row_id(row), it, sc.fmt(e), 100 * sc.masked_coverage(c["ref"][it])))
    o = sc.ot_case(M, N, B)
    for it in (1, 100):
        got = oracle.log_optimal_transport(o["scores"], o["alpha"], o["ns"], it)
        assert got.shape == (B, M, N)
        e = sc.check_all(got, o["ref"][it], "oracle OT %s it=%d" % (sc.row_id(row), it), plan, (M, N, B), "o")
        print("oracle OT       %-10s it=%-3d: %s" % (sc.row_id(row), it, sc.fmt(e)))


@pytest.mark.parametrize("row", sc.BIG_ROWS, ids=_ids(sc.BIG_ROWS))
def test_oracle_on_the_big_batches_within_all_gates_of_float64(oracle, row):
    M, N, B = row.M, row.N, row.batch
    c = sc.big_case(M, N, B)
    pick = c["pick"]
    assert pick == list(sc.picks_of(B)) and sorted(c["ref"]) == list(sc.sweeps_of(B))
    for it in (1, max(c["ref"])):
        got = oracle.log_sinkhorn_iterations(c["Z"][pick], c["log_mu"][pick], c["log_nu"][pick], it)
        e = sc.check_all(got, c["ref"][it], "oracle sinkhorn %s it=%d" % (sc.row_id(row), it), sc.stream_plan(M, N, B), (M, N, B), "s")
        print("oracle sinkhorn %-12s it=%-3d (problems %s): %s" % (sc.row_id(row), it, pick, sc.fmt(e)))


def test_oracle_cost_then_ot_within_all_gates_of_float64(oracle):
    c = sc.cost_ot_case()
    M, N = sc.COST_MN
    S = oracle.cost(c["d0"], c["d1"])
    np.testing.assert_allclose(S, cc.ref_cost(c["d0"], c["d1"]), atol=2e-5, rtol=1e-5)
    assert 0.8 * sc.AMPS[1] <= float(S.std()) <= 1.25 * sc.AMPS[1]
    for it in (1, 100):
        got = oracle.log_optimal_transport(S, c["alpha"], c["ns"], it)
        e = sc.check_all(got, c["ref"][it], "oracle cost + OT it=%d" % it, sc.stream_plan(M, N, sc.COST_B), (M, N), "c")
        print("oracle cost+OT 520x501 it=%-3d: %s" % (it, sc.fmt(e)))


@pytest.mark.parametrize("M,N,a,b", [(520, 501, 1, 2), (500, 500, 1, 2), (1100, 500, 100, 3)])
def test_oracle_on_the_stale_workspace_problems(oracle, M, N, a, b):
    s = sc.stale_case(M, N, a, b)
    assert abs(float(s["P"].std()) - 0.5) < 0.01 and abs(float(s["Q"].std()) - 3.0) < 0.05
    got = oracle.log_sinkhorn_iterations(s["Q"], s["Q_mu"], s["Q_nu"], b)
    print("oracle, stale-workspace set Q %dx%d it=%d: %s" % (M, N, b, sc.fmt(sc.check_all(got, s["ref"], "oracle Q", sc.stream_plan(M, N, 3)))))


# ---- the guard cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["s", "o"])
@pytest.mark.parametrize("M,N,batch,wild", sc.GUARD_ROWS, ids=["%dx%db%d" % r[:3] for r in sc.GUARD_ROWS])
def test_guard_inputs_lie_where_the_gpu_test_assumes(oracle, M, N, batch, wild, entry):
    """Every wild problem's largest final scaling exceeds 2^40, every tame one's stays under 2^20 (float64 duals after 100 sweeps):
    the GPU test's count of trips follows from the inputs, not from rounding.  The oracle passes the tame problems' gates, the
    WILD gate on the wild ones and NEGINF_ATOL on the -inf batch."""
    g = sc.guard_case(M, N, batch, wild, entry)
    pick = g["pick"]
    big = np.maximum(g["amax"], g["bmax"])
    print("guard %dx%d b=%d %s: log2 of the largest final scaling of problems %s: %s" % (M, N, batch, entry, pick, np.round(np.log2(big), 1).tolist()))
    iw = [pick.index(k) for k in wild]
    it_ = [i for i, k in enumerate(pick) if k not in wild]
    assert (big[iw] > 2.0 ** 40).all() and (big[it_] < 2.0 ** 20).all() and len(it_) >= 3
    assert np.isfinite(g["ref"]).all()
    assert np.abs(g["Z"][list(wild)]).max() > 200.0 and np.abs(g["Z"][sc.guard_tame(batch, wild)]).max() < 4.0
    assert np.abs(g["Z_sub"]).max() < 4.0 and np.array_equal(g["Z_sub"][sc.guard_tame(batch, wild)], g["Z"][sc.guard_tame(batch, wild)])
    plan = sc.stream_plan(M, N, batch)
    if entry == "s":
        solve = lambda Z, sel, it: oracle.log_sinkhorn_iterations(Z[sel], g["log_mu"][sel], g["log_nu"][sel], it)     # noqa: E731
    else:
        solve = lambda Z, sel, it: oracle.log_optimal_transport(Z[sel], g["alpha"], g["ns"][sel], it)                  # noqa: E731
    got = solve(g["Z"], pick, sc.GUARD_SWEEPS)
    print("  oracle, tame: %s" % sc.fmt(sc.check_all(got[it_], g["ref"][it_], "oracle guard tame", plan)))
    print("  oracle, wild: %.3f of the WILD gate (|d Z| %.2e)" % sc.check_wild(got[iw], g["ref"][iw], "oracle guard wild", plan))
    if batch <= 6:
        ip = list(sc.NEGINF_PICK)
        n_inf = sum((r.stop - r.start) * (c.stop - c.start) for r, c in sc.NEGINF_BLOCKS[(M, N)])
        assert np.isneginf(g["Z_inf"]).sum() == batch * n_inf
        full = g["Z_inf"][ip] if entry == "s" else cc.ot_problem(g["Z_inf"][ip], g["alpha"], g["ns"][ip])[0]
        assert np.array_equal(np.isneginf(g["ref_inf"]), np.isneginf(full)) and not np.isnan(g["ref_inf"]).any()
        got_i = solve(g["Z_inf"], ip, sc.GUARD_SWEEPS)
        fin = np.isfinite(g["ref_inf"])
        assert np.array_equal(np.isneginf(got_i), ~fin)
        np.testing.assert_allclose(got_i[fin], g["ref_inf"][fin], atol=sc.NEGINF_ATOL, rtol=0)


@pytest.mark.parametrize("entry", ["s", "o"])
@pytest.mark.parametrize("M,N", sc.LOUD_SHAPES, ids=["%dx%d" % s for s in sc.LOUD_SHAPES])
def test_loud_inputs_stay_inside_the_guard(oracle, M, N, entry):
    """Amplitude 12: every final scaling lies in (2^-40, 2^25), so the linear path must keep the problem; the oracle passes the four
    gates and the WILD gate on every entry."""
    c = sc.loud_case(M, N, entry)
    print("loud %dx%d %s: log2 of the final scalings in [%.1f, %.1f]; masked gate covers %.2f %%" % (
        M, N, entry, c["log2_min"], c["log2_max"], 100 * sc.masked_coverage(c["ref"])))
    assert -40.0 < c["log2_min"] and c["log2_max"] < 25.0
    if entry == "s":
        got = oracle.log_sinkhorn_iterations(c["Z"], c["log_mu"], c["log_nu"], sc.GUARD_SWEEPS)
    else:
        got = oracle.log_optimal_transport(c["Z"], c["alpha"], c["ns"], sc.GUARD_SWEEPS)
    print("  oracle: %s" % sc.fmt(sc.check_all(got, c["ref"], "oracle loud", sc.stream_plan(M, N, 1), wild=True)))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def test_every_entry_gate_sees_what_the_masked_gate_does_not():
    """The small entries of a row (more than 400 of its 500) moved by 1e-3 nats pass the four project gates and miss the every-entry
    gate; the locator names the entry in the plan's terms."""
    c = sc.sinkhorn_case(1100, 500, 3)
    ref = c["ref"][100]
    plan = sc.stream_plan(1100, 500, 3)
    cover = sc.masked_coverage(ref[1])
    print("masked log-plan gate at (1100, 500), amplitude 3: %.1f %% of the entries" % (100 * cover))
    assert cover < 0.5
    got = ref.astype(np.float32)
    sc.check_all(got, ref, "rounded reference", plan)
    row = int((ref[1] > np.log(cc.LOGPLAN_MASS)).sum(1).argmin())                   # the row of problem 1 with the fewest entries under the gate
    small = ref[1, row] <= np.log(cc.LOGPLAN_MASS)
    assert small.sum() > 400
    got[1, row, small] += np.float32(1e-3)
    cc.check_plan(got, ref, "a small row moved")                                   # the project's gates do not see it
    with pytest.raises(AssertionError, match="every-entry gate missed.*problem 1, row %d," % row):
        sc.check_all(got, ref, "a small row moved", plan)
    # the locator's terms
    bad = ref.astype(np.float32)
    bad[2, 70, 333] += 1.0
    assert "problem 2, row 70, column 333: row block 4 row 6 (RB 16), resident block 2 row 6 (RB 32); thread 166 slot 1; reduce group 5 lane 13" in sc.locate(bad, ref, plan)
    p2 = sc.stream_plan(22, 4608, 3)
    r2 = np.zeros((1, 22, 4608))
    b2 = r2.astype(np.float32)
    b2[0, 17, 4100] = 1.0
    assert "row block 1 row 1 (RB 16); thread 4 slot 8; reduce group 64 lane 4" in sc.locate(b2, r2, p2)
    p1 = sc.stream_plan(4097, 4097, 1)
    assert p1.res_kind == 1
    r1 = np.zeros((1, 40, 4097))
    b1 = r1.astype(np.float32)
    b1[0, 35, 4096] = 1.0
    assert "resident block 2 row 1 (RB 17); thread 0 slot 8; reduce group 128 lane 0" in sc.locate(b1, r1, p1)
    # NaN anywhere fails, and the WILD gate is relative
    nan = ref.astype(np.float32)
    nan[0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        sc.check_all(nan, ref, "nan", plan)
    assert abs(sc.every_entry(np.full((1, 1, 1), 300.004, np.float32), np.full((1, 1, 1), 300.0), wild=True)[0] - 0.5) < 0.02
