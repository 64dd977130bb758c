"""-m gpu: the streaming Sinkhorn solver (csrc/sinkhorn_stream.hip: every coarse problem above 304 x 320) at its shape, grid and
guard edges, against a float64 reference of the reference's log-domain iteration (tests/stream_cases.py holds the cases and the
mirror of launch_stream's dispatch; tests/test_stream_cases_host.py holds the CPU oracle to the same gates).

Solver mode "kernel" only: the log mode is sinkhorn_wg_kernel for everything, which tests/test_coarse_solver_edges_gpu.py covers.

The rows walk the two-launch form (stream_sweep_kernel<16 | 17, 1..9> + stream_colreduce_kernel with its tail loop) and the two
batched shapes of stream_resident_kernel, <32, 2, 64> and <64, 2, 64> (grid barrier, {value, tag} granules, the four slices of
the reducer).  The 4097^2-class shape <17, 9, 32> stays with the tests it has (three rows of test_streaming_solver_block_shapes,
the roofline golden, the determinism test): its smallest problem is 4097 x 4097, and a float64 reference of that size does not
fit a test of seconds.

Gates: the project's four (mass, both marginals, the log-plan where the mass exceeds 1e-6) and |Z - Z_ref| <= 2e-4 on EVERY
entry - at these shapes the masked gate sees a few per cent of the entries.  Every tame solve also asserts that nothing was
flagged: a resident solve that gave up at a barrier or a poll would still return a correct plan, from the log-domain kernel.
A row whose plan on this device's CU count is not the table's (written for 256 CUs) is skipped with the reason.  Each test
prints its plan and its largest error as a share of each gate (pytest -rA)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coarse_cases as cc
import stream_cases as sc
from coarse_cases import cu

pytestmark = pytest.mark.gpu


def _ids(rows):
    return [sc.row_id(r) for r in rows]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def kernel_mode(ops):
    prev = ops.set_sinkhorn_mode("kernel")
    ops.sinkhorn_fallbacks(reset=True)
    yield
    ops.set_sinkhorn_mode(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def plan_here(M, N, batch, want=None, iters=100):
    """The plan on this device; skips when it is not the one the row is written for."""
    p = sc.stream_plan(M, N, batch, n_cu(), iters)
    if want is not None and not sc.plan_matches(p, want):
        pytest.skip("%d x %dx%d on %d CUs: %s, the row is written for %s" % (batch, M, N, n_cu(), sc.fmt_plan(p), want))
    return p


def tame_solve(ops, f, *a):
    """A solve nothing may flag: no guard trip, no give-up of the resident kernel."""
    out = f(*a)
    trips = ops.sinkhorn_fallbacks(reset=True)
    assert trips == 0, "%d problems were redone by the log-domain kernel" % trips
    return out


# ---- sections 3 and 4: the rows of three problems, both entry points -------------------------------------------------------------
@pytest.mark.parametrize("row", sc.SMALL_ROWS, ids=_ids(sc.SMALL_ROWS))
def test_shape_sweep_given_marginals(ops, row):
    """log_sinkhorn_iterations after 1 sweep (b from the set-up's vector), 2 (the first granule read), 3 (a granule overwritten
    once) and 100 (production)."""
    M, N, B = row.M, row.N, row.batch
    plan = plan_here(M, N, B, row.plan)
    c = sc.sinkhorn_case(M, N, B)
    Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
    for it in sc.sweeps_of(B):
        got = tame_solve(ops, ops.log_sinkhorn_iterations, Z, log_mu, log_nu, it).cpu().numpy()
        what = "sinkhorn %s it=%d" % (sc.row_id(row), it)
        print("%s [%s]: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(got, c["ref"][it], what, plan, (M, N, B), "s"))))


@pytest.mark.parametrize("row", sc.SMALL_ROWS, ids=_ids(sc.SMALL_ROWS))
def test_shape_sweep_ot_entry_point(ops, row):
    """log_optimal_transport on scores [B, M - 1, N - 1]: the alpha border is synthesised through SrcViewS in the set-up kernels and
    the epilogue, the marginals come from ot_prep_kernel and norm is subtracted in stream_finish_kernel."""
    M, N, B = row.M, row.N, row.batch
    plan = plan_here(M, N, B, row.plan)
    c = sc.ot_case(M, N, B)
    S, ns = cu(c["scores"]), cu(c["ns"])
    for it in sc.sweeps_of(B, "o"):
        got = tame_solve(ops, ops.log_optimal_transport, S, c["alpha"], ns, it)
        assert got.shape == (B, M, N)
        what = "OT %s it=%d" % (sc.row_id(row), it)
        print("%s [%s]: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(got.cpu().numpy(), c["ref"][it], what, plan, (M, N, B), "o"))))


# ---- sections 3 (batch 16) and 5: the big batches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sc.BIG_ROWS, ids=_ids(sc.BIG_ROWS))
def test_big_batches(ops, oracle, row):
    """Every problem against the oracle under all gates, the first, one inside and the last against float64."""
    M, N, B = row.M, row.N, row.batch
    plan = plan_here(M, N, B, row.plan)
    c = sc.big_case(M, N, B)
    Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
    for it in sc.sweeps_of(B):
        got = tame_solve(ops, ops.log_sinkhorn_iterations, Z, log_mu, log_nu, it).cpu().numpy()
        what = "sinkhorn %s it=%d" % (sc.row_id(row), it)
        want = oracle.log_sinkhorn_iterations(c["Z"], c["log_mu"], c["log_nu"], it)
        print("%s [%s] against the oracle: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(got, want, what + " (oracle)", plan))))
        print("%s problems %s against float64: %s" % (what, c["pick"], sc.fmt(sc.check_all(got[c["pick"]], c["ref"][it], what, plan, (M, N, B), "s"))))


# ---- section 6: stale workspace -------------------------------------------------------------------------------------------------------
def _solve(ops, s, name, it):
    return ops.log_sinkhorn_iterations(cu(s[name]), cu(s[name + "_mu"]), cu(s[name + "_nu"]), it)


@pytest.mark.parametrize("M,N,first,then", [(520, 501, 1, 2), (1100, 500, 100, 3)], ids=["tag1", "tag100"])
def test_stale_granules_of_an_earlier_solve(ops, M, N, first, then):
    """Inside workspace_cache consecutive calls share one scratch block.  Set P solved with `first` sweeps leaves {b_j, first} in every
    granule; set Q (other scores and marginals, amplitude 3 where P had 0.5) solved with `then` sweeps must not read them: sweep 1
    accepts a granule whose tag is 1, and workgroups that reduce nothing poll without waiting at the barrier.  Q is held to float64
    and to the bits of the same call on a fresh allocation.  (At these widths the set-up's column maxima overwrite the granule area
    before every solve as well; the case that depends on stream_granule_clear_kernel alone is the 4097 x 4097 one below.)"""
    plan = plan_here(M, N, 3, dict(res_kind=2))
    s = sc.stale_case(M, N, first, then)
    with ops.workspace_cache():
        tame_solve(ops, _solve, ops, s, "P", first)
        got = tame_solve(ops, _solve, ops, s, "Q", then)
    fresh = tame_solve(ops, _solve, ops, s, "Q", then)
    what = "stale tag %d, then %d sweeps at %dx%d" % (first, then, M, N)
    print("%s [%s]: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(got.cpu().numpy(), s["ref"], what, plan))))
    assert torch.equal(bits(got), bits(fresh)), "a solve in a used scratch block differs from the same solve in a fresh one"


def test_a_changed_layout_in_the_same_scratch_block(ops):
    """(500, 500), then (520, 501), then (500, 500) again in one scratch block: the third call has the bits of the first."""
    plan_here(500, 500, 3, dict(res_kind=2))
    plan_here(520, 501, 3, dict(res_kind=2))
    a, b = sc.stale_case(500, 500, 1, 2), sc.stale_case(520, 501, 1, 2)
    with ops.workspace_cache():
        first = tame_solve(ops, _solve, ops, a, "Q", 2)
        tame_solve(ops, _solve, ops, b, "Q", 2)
        third = tame_solve(ops, _solve, ops, a, "Q", 2)
    assert torch.equal(bits(first), bits(third))
    sc.check_all(first.cpu().numpy(), a["ref"], "500x500 it=2", sc.stream_plan(500, 500, 3, n_cu()))


def test_stale_granules_where_the_set_up_does_not_reach(ops, oracle, monkeypatch):
    """The one place where stream_granule_clear_kernel is all that stands between a solve and an earlier solve's granules.  For
    N <= 1024 the granules lie inside the area stream_colmax_partial_kernel fills with column maxima (<= 0: no such bit pattern is
    a tag), so a missing clear cannot show there - a build without it passes the two tests above.  For <17, 9, 32> they lie
    behind 241 rows of pitch 4100, past the 241 x 4097 floats the set-up writes.  So: 4097 x 4097 (the kernel's smallest problem),
    set P with one sweep, then set Q with two sweeps in the SAME scratch block (4097^2 is above workspace_cache's 64 MB, so the
    block is handed to both calls here); Q against the fp32 oracle - a float64 plan of this size does not fit a test of seconds,
    and the oracle's own |Z - Z_ref| is 6.3e-6 of the gate's 2e-4 (tests/test_stream_cases_host.py)."""
    M = N = 4097
    plan = plan_here(M, N, 1, dict(res_kind=1, res_nblk=241))
    rng = np.random.default_rng([27, M, N])
    Q = (3.0 * rng.standard_normal((1, M, N))).astype(np.float32)
    mu, nu = sc._marginal(rng, 1, M), sc._marginal(rng, 1, N)
    Zq, P = cu(Q), cu(Q) * (-1.0 / 6.0)                                            # P: another problem, amplitude 0.5
    lmu, lnu = cu(mu), cu(nu)
    block = torch.empty(ops._L().pats_sinkhorn_workspace_bytes(1, M, N), dtype=torch.uint8, device="cuda")
    monkeypatch.setattr(ops, "_workspace", lambda n, device: block if n <= block.numel() else torch.empty(n, dtype=torch.uint8, device=device))
    tame_solve(ops, ops.log_sinkhorn_iterations, P, lnu.flip(1).contiguous(), lmu.flip(1).contiguous(), 1)
    got = tame_solve(ops, ops.log_sinkhorn_iterations, Zq, lmu, lnu, 2).cpu().numpy()
    want = oracle.log_sinkhorn_iterations(Q, mu, nu, 2)
    print("stale tag 1 at 4097x4097 [%s] against the oracle: %s" % (sc.fmt_plan(plan), sc.fmt(sc.check_all(got, want, "4097x4097 it=2 after it=1", plan))))


# ---- section 7: guard trips and flag isolation ----------------------------------------------------------------------------------------
def _guard_solver(ops, g, entry, sweeps=sc.GUARD_SWEEPS):
    def solve(Z, sel):
        if entry == "s":
            return ops.log_sinkhorn_iterations(cu(Z[sel]), cu(g["log_mu"][sel]), cu(g["log_nu"][sel]), sweeps)
        return ops.log_optimal_transport(cu(Z[sel]), g["alpha"], cu(g["ns"][sel]), sweeps)
    return solve


@pytest.mark.parametrize("entry", ["s", "o"], ids=["sinkhorn", "ot"])
@pytest.mark.parametrize("M,N,batch,wild", sc.GUARD_ROWS, ids=["%dx%db%d" % r[:3] for r in sc.GUARD_ROWS])
def test_guard_trips_and_flag_isolation(ops, M, N, batch, wild, entry):
    """Problems of amplitude 0.5, the wild ones of amplitude 60: every wild problem's final scaling exceeds 2^40, every tame one's
    stays under 2^20 (tests/test_stream_cases_host.py).  The flagged problems are redone by sinkhorn_wg_kernel(only_if), which must
    leave the others as the streaming solver wrote them; fail[b] must belong to problem b."""
    g = sc.guard_case(M, N, batch, wild, entry)
    plan = plan_here(M, N, batch)
    solve = _guard_solver(ops, g, entry)
    everyone, tame, wild, pick = list(range(batch)), sc.guard_tame(batch, wild), list(wild), g["pick"]
    ops.sinkhorn_fallbacks(reset=True)
    got_t = solve(g["Z"], everyone)
    trips = ops.sinkhorn_fallbacks(reset=True)
    assert 1 <= trips <= len(wild), trips
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    # The tame problems, bit for bit: against a batch of the tame problems alone where that batch has the same plan (other fail[]
    # and row indices, the same summation order); where its plan differs (another block height sums in another order) against
    # a batch of the same size with the wild problems replaced by tame draws.
    alone_plan = sc.stream_plan(M, N, len(tame), n_cu())
    if (alone_plan.res_kind, alone_plan.res_nblk, alone_plan.RB) == (plan.res_kind, plan.res_nblk, plan.RB):
        alone, how = solve(g["Z"], tame), "the tame problems alone"
    else:
        alone, how = solve(g["Z_sub"], everyone)[tame], "a batch with the wild problems replaced"
    assert ops.sinkhorn_fallbacks(reset=True) == 0
    assert torch.equal(bits(got_t[tame]), bits(alone)), "a flagged problem's redo changed an unflagged problem (against %s)" % how
    what = "guard %dx%d b=%d %s" % (M, N, batch, entry)
    ip = [pick.index(k) for k in pick if k not in wild]
    tp = [k for k in pick if k not in wild]
    print("%s [%s], %d trips, bits of %s; tame problems %s: %s" % (
        what, sc.fmt_plan(plan), trips, how, tp, sc.fmt(sc.check_all(got[tp], g["ref"][ip], what + " tame", plan))))
    iw = [pick.index(k) for k in wild]
    print("%s wild problems: %.3f of the WILD gate (|d Z| %.2e)" % ((what,) + sc.check_wild(got[wild], g["ref"][iw], what + " wild", plan)))
    if batch > 6:
        return
    # structural zeros in the tame batch: the solve stays linear, K = 0 on the blocks
    got_i = tame_solve(ops, solve, g["Z_inf"], everyone).cpu().numpy()
    full = np.isneginf(g["Z_inf"])
    if entry == "o":
        full = np.pad(full, ((0, 0), (0, 1), (0, 1)))
    assert not np.isnan(got_i).any() and not np.isposinf(got_i).any()
    assert np.array_equal(np.isneginf(got_i), full)
    ipk = list(sc.NEGINF_PICK)
    fin = np.isfinite(g["ref_inf"])
    assert np.array_equal(~fin, full[ipk])
    print("%s -inf blocks: max |Z - Z_ref| on finite entries %.3g" % (what, float(np.abs(got_i[ipk][fin] - g["ref_inf"][fin]).max())))
    np.testing.assert_allclose(got_i[ipk][fin], g["ref_inf"][fin], atol=sc.NEGINF_ATOL, rtol=0)


@pytest.mark.parametrize("entry", ["s", "o"], ids=["sinkhorn", "ot"])
@pytest.mark.parametrize("M,N", sc.LOUD_SHAPES, ids=["%dx%d" % s for s in sc.LOUD_SHAPES])
def test_loud_but_inside_the_guard(ops, M, N, entry):
    """One problem of amplitude 12: its scalings stay within (2^-40, 2^25), so the linear path keeps it (no trip), although entries of
    exp(Z - r - c) below 2^-126 are flushed.  The four gates, and the WILD gate on every entry."""
    c = sc.loud_case(M, N, entry)
    plan = plan_here(M, N, 1)
    if entry == "s":
        got = tame_solve(ops, ops.log_sinkhorn_iterations, cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"]), sc.GUARD_SWEEPS)
    else:
        got = tame_solve(ops, ops.log_optimal_transport, cu(c["Z"]), c["alpha"], cu(c["ns"]), sc.GUARD_SWEEPS)
    what = "loud %dx%d %s" % (M, N, entry)
    print("%s [%s]: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(got.cpu().numpy(), c["ref"], what, plan, wild=True))))


# ---- section 8: zero sweeps, repeatability, the two forms side by side, cost_ot -----------------------------------------------------
@pytest.mark.parametrize("M,N", [(500, 500), (400, 250)], ids=["500x500", "400x250"])
def test_zero_sweeps_return_the_input(ops, M, N):
    """iters = 0: the streaming solver flags every problem and sinkhorn_wg_kernel writes (Z + 0) + 0."""
    c = sc.sinkhorn_case(M, N, 3)
    Z = cu(c["Z"])
    got = ops.log_sinkhorn_iterations(Z, cu(c["log_mu"]), cu(c["log_nu"]), 0)
    assert ops.sinkhorn_fallbacks(reset=True) == 3
    assert torch.equal(bits(got), bits(Z))


def test_two_calls_give_the_same_bits(ops):
    """(1100, 500) and 20 x (520, 501), 100 sweeps: fixed reduction orders, no atomics in the sums."""
    plan_here(1100, 500, 3, dict(res_kind=2))
    c, o = sc.sinkhorn_case(1100, 500, 3), sc.ot_case(1100, 500, 3)
    Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
    S, ns = cu(o["scores"]), cu(o["ns"])
    first = ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)
    first_ot = ops.log_optimal_transport(S, o["alpha"], ns, 100)
    assert torch.equal(bits(ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)), bits(first))
    assert torch.equal(bits(ops.log_optimal_transport(S, o["alpha"], ns, 100)), bits(first_ot))
    plan_here(520, 501, 20, dict(res_kind=3))
    b = sc.big_case(520, 501, 20)
    Z, log_mu, log_nu = cu(b["Z"]), cu(b["log_mu"]), cu(b["log_nu"])
    S, ns = Z[:, :-1, :-1].contiguous(), torch.exp(log_nu[:, :-1]).contiguous()
    first = ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)
    first_ot = ops.log_optimal_transport(S, 0.5, ns, 100)
    assert torch.equal(bits(ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 100)), bits(first))
    assert torch.equal(bits(ops.log_optimal_transport(S, 0.5, ns, 100)), bits(first_ot))
    assert ops.sinkhorn_fallbacks(reset=True) == 0


TWO_LAUNCH_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
import stream_cases as sc
from coarse_cases import cu
from pats_amd import ops
ops.set_sinkhorn_mode("kernel")
ops.sinkhorn_fallbacks(reset=True)
out = {}
for r in sc.RESIDENT_32 + sc.RESIDENT_64:
    Z, log_mu, log_nu = (cu(a) for a in sc.sinkhorn_inputs(r.M, r.N, r.batch))
    for it in (1, 100):
        got = ops.log_sinkhorn_iterations(Z, log_mu, log_nu, it)
        out["%%s_%%d" %% (sc.row_id(r), it)] = got[list(sc.picks_of(r.batch))].cpu().numpy()
out["trips"] = np.int64(ops.sinkhorn_fallbacks(reset=True))
np.savez(sys.argv[1], **out)
"""


def test_resident_and_two_launch_forms_side_by_side(ops, tmp_path):
    """The rows of the resident kernels solved once more by a child process with PATS_STREAM_RESIDENT=0 (two launches a sweep): both
    forms within all gates of the same float64 plans.  They sum in different orders, so they are not compared bit for bit."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "two_launch.npz")
    r = subprocess.run([sys.executable, "-c", TWO_LAUNCH_CHILD % {"repo": repo, "tests": os.path.join(repo, "tests")}, out],
                       env=dict(os.environ, PATS_STREAM_RESIDENT="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    two = np.load(out)
    assert int(two["trips"]) == 0
    for row in sc.RESIDENT_32 + sc.RESIDENT_64:
        M, N, B = row.M, row.N, row.batch
        plan = plan_here(M, N, B, row.plan)
        flat = sc.stream_plan(M, N, B, n_cu(), iters=0)                             # the plan without a resident kernel
        c = (sc.sinkhorn_case if B <= 3 else sc.big_case)(M, N, B)
        Z, log_mu, log_nu = cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"])
        for it in (1, 100):
            res = tame_solve(ops, ops.log_sinkhorn_iterations, Z, log_mu, log_nu, it)[c["pick"]].cpu().numpy()
            what = "%s it=%d" % (sc.row_id(row), it)
            e_res = sc.check_all(res, c["ref"][it], what + " resident", plan, (M, N, B), "s")
            e_two = sc.check_all(two["%s_%d" % (sc.row_id(row), it)], c["ref"][it], what + " two launches", flat, (M, N, B), "s")
            print("%-18s resident: %s" % (what, sc.fmt(e_res)))
            print("%-18s two launches: %s" % ("", sc.fmt(e_two)))


def test_cost_ot_is_cost_then_ot(ops):
    """cost_ot (variant 1, D = 64) at (520, 501) has the bits of cost followed by log_optimal_transport, and is within the gates of
    the float64 solve of the float64 cost."""
    M, N = sc.COST_MN
    plan = plan_here(M, N, sc.COST_B, dict(res_kind=2))
    c = sc.cost_ot_case()
    d0, d1, ns = cu(c["d0"]), cu(c["d1"]), cu(c["ns"])
    S = ops.cost(d0, d1)
    np.testing.assert_allclose(S.cpu().numpy(), cc.ref_cost(c["d0"], c["d1"]), atol=2e-5, rtol=1e-5)     # test_coarse_level's gate
    for it in (1, 100):
        fused = tame_solve(ops, ops.cost_ot, d0, d1, 1, c["alpha"], ns, it)
        assert torch.equal(bits(fused), bits(ops.log_optimal_transport(S, c["alpha"], ns, it)))
        what = "cost_ot %dx%d it=%d" % (M, N, it)
        print("%s [%s]: %s" % (what, sc.fmt_plan(plan), sc.fmt(sc.check_all(fused.cpu().numpy(), c["ref"][it], what, plan, (M, N), "c"))))


# ---- section 9: a shape the hand-over's kernel cannot take ----------------------------------------------------------------------------
def test_a_shape_beyond_the_fallback_kernel_is_refused_before_anything_is_queued(ops):
    """(16100, 300) is a streaming shape, but M + N > 16384 floats do not fit sinkhorn_wg_kernel's LDS, and that kernel is every
    flagged problem's re-solve: the call is refused (ahead of the streaming launches), and the next call on the stream is correct."""
    M, N = 16100, 300
    assert cc.stream_shape(M, N) and cc.wg_lds_bytes(M, N) > 64 * 1024
    Z = torch.zeros((1, M, N), device="cuda")
    log_mu, log_nu = torch.full((1, M), -float(np.log(M)), device="cuda"), torch.full((1, N), -float(np.log(N)), device="cuda")
    with pytest.raises(RuntimeError, match="M\\+N=16400 too large for the one-workgroup kernel"):
        ops.log_sinkhorn_iterations(Z, log_mu, log_nu, 3)
    torch.cuda.synchronize()
    c = sc.sinkhorn_case(400, 250, 3)
    got = tame_solve(ops, ops.log_sinkhorn_iterations, cu(c["Z"]), cu(c["log_mu"]), cu(c["log_nu"]), 100)
    sc.check_all(got.cpu().numpy(), c["ref"][100], "400x250 after the refusal", sc.stream_plan(400, 250, 3, n_cu()))
