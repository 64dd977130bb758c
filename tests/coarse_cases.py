"""Cases, float64 reference and the one comparison of tests/test_coarse_solver_edges_gpu.py (the one-CU coarse Sinkhorn solver
sinkhorn_cu2_kernel<19,5> of csrc/sinkhorn.hip and its dispatch neighbours); tests/test_coarse_cases_host.py holds the CPU oracle
to the same reference under the same gates - it checks the checker.

Numpy only apart from `cu`, which imports torch itself.

The reference is the reference's log-domain iteration (modules.py:137-143, as oracle_sinkhorn of oracle/pats_oracle.c reads it)
in float64: u = v = 0; iters x { u = log_mu - lse_j(Z + v); v = log_nu - lse_i(Z + u) }; Z + u + v, with a max-subtracted
log-sum-exp whose stabiliser is 0 where the maximum is infinite (ATen's masked_fill), so -inf scores are structural zeros.

Layout of the kernel under test, which the shape table walks: 16 waves own rows wave + 16 s (s < 19 row slots), 64 lanes own
columns lane + 64 c (c < 5 column slices); slots are paired (i, i + 10) for the packed row pass and the transposed row
reduction; pairs (7, 17), (8, 18) and the single slot 9 live in LDS, the other fourteen slots in registers."""
import functools

import numpy as np

# ---- the gates, all taken from the project (assert_mass of tests/test_gpu_parity.py) -------------------------------
MASS_ATOL, MASS_RTOL = 1e-4, 2e-6          # on exp(Z), element-wise
MARG_ATOL, MARG_RTOL = 1e-4, 3e-6          # on both marginals of exp(Z)
LOGPLAN_TOL, LOGPLAN_MASS = 2e-4, 1e-6     # |Z - Z_ref| where exp(Z_ref) > 1e-6
WILD_ATOL, WILD_RTOL = 2e-3, 2e-5          # log-plan of a guard-tripping problem (test_wide_dynamic_range_trips_guard_and_falls_back)
NEGINF_ATOL = 3e-5                         # finite log-plan entries of a problem with -inf scores (same test)
GATES = ("mass", "rows", "cols", "logplan")
# (case key, entry point, gate) -> factor on that gate: empty.  A case would be listed here with twice the fp32 oracle's own
# error against float64 if the oracle itself missed a gate there; tests/test_coarse_cases_host.py asserts that it misses none.
GATE_SCALE = {}

SWEEPS_SINKHORN = (1, 2, 100)
SWEEPS_OT = (1, 100)
B_SINKHORN, B_OT = 3, 2
AMPS = (0.5, 3.0)
ALPHAS = (0.0, 0.5, 1.3)
SCALE_GUARD = 2.0 ** 30                    # csrc/common.hpp: a linear-domain solve whose scalings leave (0, 2^30] is redone

# ---- the dispatch, mirrored (csrc/sinkhorn.hip: cu_shape, stream_shape, launch_wg) ------------------------------------------
CU_ROWS, CU_COLS = 16 * 19, 64 * 5         # 304 x 320


def cu_shape(M, N):
    return M <= CU_ROWS and N <= CU_COLS and M * N >= 96 * 96


def stream_shape(M, N):
    return M * N > CU_ROWS * CU_COLS and N <= 512 * 9


def wg_threads(M, N):
    return 1024 if M * N >= 128 * 128 else 256


def wg_lds_bytes(M, N):
    return (M + N) * 4                     # launch_wg: both dual vectors; at most 64 KiB


def expected_path(M, N, mode, batch=1):
    """The kernel that solves an [M, N] problem: 'cu2' (sinkhorn_cu2_kernel, then sinkhorn_wg_kernel on what it flagged),
    'stream' (the stream_* kernels of csrc/sinkhorn_stream.hip, same hand-over) or 'wg1024' / 'wg256' (sinkhorn_wg_kernel alone).
    M == N in {65, 145} are resident shapes of log_sinkhorn_iterations (other kernels) and not described here."""
    if mode == "kernel":
        if cu_shape(M, N):
            return "cu2"
        if stream_shape(M, N) and batch <= 65535:
            return "stream"
    return "wg%d" % wg_threads(M, N)


# (M, N, path in kernel mode, path in log mode, entry points, why)
TABLE = [
    (304, 320, "cu2", "wg1024", "so", "every slot and slice full"),
    (304, 319, "cu2", "wg1024", "so", "one column short: slice 4 ends at lane 62"),
    (303, 320, "cu2", "wg1024", "so", "one row short: slot 18 is empty in wave 15"),
    (301, 301, "cu2", "wg1024", "so", "production shape (anchor)"),
    (289, 257, "cu2", "wg1024", "so", "slot 18 held by wave 0 only; slice 4 held by lane 0 only"),
    (288, 256, "cu2", "wg1024", "so", "slot 18 and slice 4 entirely empty"),
    (161, 65, "cu2", "wg256", "so", "slot 10, the first second-half slot of a pair, in wave 0 only; slice 1 in lane 0 only"),
    (160, 64, "cu2", "wg256", "so", "every pair's second half is padding; one column slice"),
    (120, 100, "cu2", "wg256", "so", "LDS slot 7 partly filled, slots 8 and 9 empty"),
    (145, 145, "cu2", "wg1024", "o", "log_optimal_transport only: the fine size goes to THIS kernel there, not the block kernel; "
                                     "slot 9 (the single LDS slot) in wave 0 only"),
    (29, 320, "cu2", "wg256", "so", "fewer rows than 2 x 16: waves 13..15 hold one row"),
    (30, 320, "cu2", "wg256", "so", "fewer rows than 2 x 16: waves 14 and 15 hold one row"),
    (304, 31, "cu2", "wg256", "so", "lanes 31..63 own no column"),
    (96, 96, "cu2", "wg256", "so", "lower edge of cu_shape"),
    (95, 97, "wg256", "wg256", "so", "just below cu_shape (M * N = 9215)"),
    (304, 30, "wg256", "wg256", "so", "just below cu_shape (M * N = 9120)"),
    (128, 128, "cu2", "wg1024", "so", "the wg kernel's 1024-thread edge: a one-CU shape in kernel mode, a wg shape in log mode"),
    (127, 129, "cu2", "wg256", "so", "one element below the wg kernel's 1024-thread edge"),
    (305, 320, "stream", "wg1024", "so", "the streaming solver's smallest shapes: one row too many"),
    (304, 321, "stream", "wg1024", "so", "the streaming solver's smallest shapes: one column too many"),
    (305, 319, "stream", "wg1024", "so", "M > 304 and M * N = 97 295 > 304 * 320"),
    (320, 304, "wg1024", "wg1024", "so", "M > 304 but M * N <= 304 * 320: no linear-domain kernel takes it"),
    (305, 300, "wg1024", "wg1024", "so", "M > 304 but M * N <= 304 * 320: no linear-domain kernel takes it"),
]
SHAPES = [(t[0], t[1]) for t in TABLE]
SINKHORN_SHAPES = [(t[0], t[1]) for t in TABLE if "s" in t[4]]
OT_SHAPES = [(t[0], t[1]) for t in TABLE if "o" in t[4]]
COST_OT_SHAPES = [(304, 320), (289, 257), (145, 145), (305, 320)]
COST_D = 64


def case_index(M, N):
    return SHAPES.index((M, N))


def slot_population(M):
    """[waves holding a row in slot s for s < 19]: what the 'why' column of the table states about the row slots."""
    return [sum(1 for w in range(16) if w + 16 * s < M) for s in range(19)]


def slice_population(N):
    """[lanes holding a column in slice c for c < 5]."""
    return [sum(1 for l in range(64) if l + 64 * c < N) for c in range(5)]


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(np.log(np.exp(x - m).sum(axis=axis, keepdims=True)) + m, axis)


def ref_sweeps(Z, log_mu, log_nu, sweeps):
    """{iters: (plan, u, v)} for every count in `sweeps`, from ONE run to max(sweeps).  Z [b, M, N], float64 throughout."""
    Z, log_mu, log_nu = (np.asarray(a, np.float64) for a in (Z, log_mu, log_nu))
    u, v = np.zeros_like(log_mu), np.zeros_like(log_nu)
    out = {}
    for it in range(max(sweeps) + 1):
        if it in sweeps:
            out[it] = ((Z + u[:, :, None]) + v[:, None, :], u.copy(), v.copy())
        if it < max(sweeps):
            u = log_mu - _lse(Z + v[:, None, :], 2)
            v = log_nu - _lse(Z + u[:, :, None], 1)
    return out


def ref_sinkhorn(Z, log_mu, log_nu, iters):
    return ref_sweeps(Z, log_mu, log_nu, (iters,))[iters][0]


def ot_problem(scores, alpha, ns):
    """(couplings, log_mu, log_nu, norm) of modules.py:145-159 in float64 from the fp32 inputs' values, as
    oracle_log_optimal_transport builds them: dustbin row and column alpha, norm = -log(m + sum ns)."""
    S = np.asarray(scores, np.float64)
    b, m, n = S.shape
    a = float(np.float32(alpha))                          # the kernel reads alpha as fp32
    ns = np.asarray(ns, np.float64).reshape(b, n)
    C = np.full((b, m + 1, n + 1), a, np.float64)
    C[:, :m, :n] = S
    ns_sum = ns.sum(1)
    norm = -np.log(m + ns_sum)
    log_nu = np.concatenate([np.log(ns) + norm[:, None], (np.log(float(m)) + norm)[:, None]], 1)
    log_mu = np.concatenate([np.broadcast_to(norm[:, None], (b, m)), (np.log(ns_sum) + norm)[:, None]], 1)
    return C, log_mu, log_nu, norm


def ref_ot_sweeps(scores, alpha, ns, sweeps):
    C, log_mu, log_nu, norm = ot_problem(scores, alpha, ns)
    return {it: (p - norm[:, None, None], u, v) for it, (p, u, v) in ref_sweeps(C, log_mu, log_nu, sweeps).items()}


def ref_log_optimal_transport(scores, alpha, ns, iters):
    return ref_ot_sweeps(scores, alpha, ns, (iters,))[iters][0]


def ref_cost(d0, d1):
    """0.1 * (d0^T d1 / sqrt(D)) in float64: the scores first_layer.py:110-114 hands to log_optimal_transport, which is what
    ops.cost returns.  d0 [b, D, n], d1 [b, D, m] -> [b, n, m]."""
    d0, d1 = np.asarray(d0, np.float64), np.asarray(d1, np.float64)
    return 0.1 * (np.einsum("bdn,bdm->bnm", d0, d1) / np.sqrt(float(d0.shape[1])))


def final_scalings(Z, u, v):
    """(max a_i, max b_j) per problem of the linear-domain form at the duals (u, v): a = exp(u + r), b = exp(v + c) with the
    stabilisers r_i = max_j Z_ij, c_j = max_i (Z_ij - r_i) (csrc/sinkhorn.hip).  The guard trips when either leaves (0, 2^30]."""
    Z = np.asarray(Z, np.float64)
    r = Z.max(2)
    c = (Z - r[:, :, None]).max(1)
    with np.errstate(over="ignore"):
        return np.exp((u + r).max(1)), np.exp((v + c).max(1))


# ---- seeded inputs --------------------------------------------------------------------------------------------------------
def _marginal(rng, b, n):
    w = rng.uniform(0.5, 2.0, (b, n))
    return np.log(w / w.sum(1, keepdims=True)).astype(np.float32)


def _scores(rng, idx, b, m, n):
    """amp * N(0, 1) in float32; the amplitude alternates over the problems of a batch, starting with the case's own."""
    amp = np.array([AMPS[(idx + k) % 2] for k in range(b)], np.float64)
    return (amp[:, None, None] * rng.standard_normal((b, m, n))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sinkhorn_case(M, N):
    """Inputs of log_sinkhorn_iterations at B_SINKHORN problems and the float64 plans after 1, 2 and 100 sweeps."""
    idx = case_index(M, N)
    rng = np.random.default_rng([11, M, N])
    Z = _scores(rng, idx, B_SINKHORN, M, N)
    log_mu, log_nu = _marginal(rng, B_SINKHORN, M), _marginal(rng, B_SINKHORN, N)
    ref = {it: p for it, (p, _, _) in ref_sweeps(Z, log_mu, log_nu, SWEEPS_SINKHORN).items()}
    return _frozen(dict(Z=Z, log_mu=log_mu, log_nu=log_nu, ref=ref))


@functools.lru_cache(maxsize=None)
def ot_case(M, N):
    """Inputs of log_optimal_transport (scores [B_OT, M - 1, N - 1]) and the float64 plans after 1 and 100 sweeps."""
    idx = case_index(M, N)
    rng = np.random.default_rng([12, M, N])
    m, n = M - 1, N - 1
    S = _scores(rng, idx, B_OT, m, n)
    ns = rng.uniform(0.5, 2.0, (B_OT, 1, n)).astype(np.float32)
    alpha = ALPHAS[idx % 3]
    ref = {it: p for it, (p, _, _) in ref_ot_sweeps(S, alpha, ns, SWEEPS_OT).items()}
    return _frozen(dict(scores=S, ns=ns, alpha=alpha, ref=ref))


@functools.lru_cache(maxsize=None)
def cost_ot_case(M, N):
    """Descriptors d0 [B_OT, 64, M - 1], d1 [B_OT, 64, N - 1] whose scores have the spread of the case's amplitude, ns, alpha
    and the float64 plans (1 and 100 sweeps) of the FLOAT64 cost."""
    idx = case_index(M, N)
    rng = np.random.default_rng([13, M, N])
    m, n = M - 1, N - 1
    sd = np.sqrt(10.0 * AMPS[idx % 2])                   # 0.1 * sd^2 * N(0, 1)-like scores
    d0 = (sd * rng.standard_normal((B_OT, COST_D, m))).astype(np.float32)
    d1 = (sd * rng.standard_normal((B_OT, COST_D, n))).astype(np.float32)
    ns = rng.uniform(0.5, 2.0, (B_OT, 1, n)).astype(np.float32)
    alpha = ALPHAS[(idx + 1) % 3]
    ref = {it: p for it, (p, _, _) in ref_ot_sweeps(ref_cost(d0, d1), alpha, ns, SWEEPS_OT).items()}
    return _frozen(dict(d0=d0, d1=d1, ns=ns, alpha=alpha, ref=ref))


MANY_B, MANY_MN, MANY_SWEEPS, MANY_REF = 260, (161, 65), 3, (0, 255, 259)


@functools.lru_cache(maxsize=None)
def many_case():
    """More problems than the chip has CUs (256): 260 at (161, 65), three sweeps; float64 plans of problems 0, 255 and 259."""
    M, N = MANY_MN
    rng = np.random.default_rng([14, M, N])
    Z = _scores(rng, 0, MANY_B, M, N)
    log_mu, log_nu = _marginal(rng, MANY_B, M), _marginal(rng, MANY_B, N)
    pick = list(MANY_REF)
    ref = ref_sinkhorn(Z[pick], log_mu[pick], log_nu[pick], MANY_SWEEPS)
    return _frozen(dict(Z=Z, log_mu=log_mu, log_nu=log_nu, ref=ref))


GUARD_SHAPES = [(301, 301), (289, 257)]
GUARD_B, GUARD_WILD, GUARD_TAME, GUARD_FACTOR, GUARD_SWEEPS = 6, (1, 4), (0, 2, 3, 5), 60.0, 100
NEGINF_BLOCKS = ((slice(0, 5), slice(7, 20)), (slice(110, 150), slice(60, 70)))


@functools.lru_cache(maxsize=None)
def guard_case(M, N, entry):
    """Six problems of 0.5 * N(0, 1) scores, problems 1 and 4 multiplied by 60 (30 * N(0, 1): about +-150 nats), for
    `entry` 's' (log_sinkhorn_iterations, Z [6, M, N]) or 'o' (log_optimal_transport, scores [6, M - 1, N - 1], alpha 0.5).
    ref: float64 plans after 100 sweeps; amax, bmax: the linear-domain scalings at those duals (final_scalings), which
    tests/test_coarse_cases_host.py holds to either side of the guard.  The second batch (`*_inf`) is the tame draw with the two
    NEGINF_BLOCKS set to -inf: rows 0..4 x columns 7..19, and rows 110..149 x columns 60..69, which straddles column slices
    0 / 1 and row slots 6 (registers), 7 and 8 (LDS pairs) and 9 (the single LDS slot)."""
    rng = np.random.default_rng([15, M, N, ord(entry)])
    m, n = (M, N) if entry == "s" else (M - 1, N - 1)
    tame = (AMPS[0] * rng.standard_normal((GUARD_B, m, n))).astype(np.float32)
    Z = tame.copy()
    for k in GUARD_WILD:
        Z[k] *= np.float32(GUARD_FACTOR)
    Zi = tame.copy()
    for rows, cols in NEGINF_BLOCKS:
        Zi[:, rows, cols] = -np.inf
    d = dict(Z=Z, Z_inf=Zi)
    if entry == "s":
        d["log_mu"], d["log_nu"] = _marginal(rng, GUARD_B, M), _marginal(rng, GUARD_B, N)
        (p, u, v), = ref_sweeps(Z, d["log_mu"], d["log_nu"], (GUARD_SWEEPS,)).values()
        d["amax"], d["bmax"] = final_scalings(Z, u, v)
        d["ref_inf"] = ref_sinkhorn(Zi, d["log_mu"], d["log_nu"], GUARD_SWEEPS)
    else:
        d["ns"] = rng.uniform(0.5, 2.0, (GUARD_B, 1, n)).astype(np.float32)
        d["alpha"] = 0.5
        (p, u, v), = ref_ot_sweeps(Z, d["alpha"], d["ns"], (GUARD_SWEEPS,)).values()
        d["amax"], d["bmax"] = final_scalings(ot_problem(Z, d["alpha"], d["ns"])[0], u, v)
        d["ref_inf"] = ref_log_optimal_transport(Zi, d["alpha"], d["ns"], GUARD_SWEEPS)
    d["ref"] = p
    return _frozen(d)


def _frozen(d):
    """The cached arrays are shared among tests: read-only."""
    for v in d.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


# ---- the one comparison ---------------------------------------------------------------------------------------------------
def plan_errors(got, ref):
    """The figures the gates bound, for a log-plan `got` (float32) against the float64 `ref`: per gate the largest error as a
    share of the gate (<= 1 passes) and, under '<gate>_abs', the largest absolute error."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    eg, er = np.exp(g), np.exp(r)
    out = {}
    for name, a, b, atol, rtol in (("mass", eg, er, MASS_ATOL, MASS_RTOL),
                                   ("rows", eg.sum(-1), er.sum(-1), MARG_ATOL, MARG_RTOL),
                                   ("cols", eg.sum(-2), er.sum(-2), MARG_ATOL, MARG_RTOL)):
        d = np.abs(a - b)
        out[name] = float((d / (atol + rtol * np.abs(b))).max())
        out[name + "_abs"] = float(d.max())
    big = er > LOGPLAN_MASS
    with np.errstate(invalid="ignore"):
        dz = float(np.abs(g[big] - r[big]).max()) if big.any() else 0.0
    out["logplan"], out["logplan_abs"] = dz / LOGPLAN_TOL, dz
    return out


def check_plan(got, ref, what, key=None, entry=None):
    """Asserts `got` finite and within the four gates of `ref`; returns plan_errors.  NaN anywhere fails (NaN <= x is False)."""
    got = np.asarray(got)
    assert got.dtype == np.float32, (what, got.dtype)
    assert np.isfinite(got).all(), "%s: %d non-finite entries" % (what, int((~np.isfinite(got)).sum()))
    e = plan_errors(got, ref)
    for gate in GATES:
        lim = GATE_SCALE.get((key, entry, gate), 1.0)
        assert e[gate] <= lim, "%s: gate '%s' missed: %.3g of the gate (largest absolute error %.3g)%s" % (
            what, gate, e[gate], e[gate + "_abs"], worst(got, ref))
    return e


def worst(got, ref):
    """Where the largest log-plan error sits, in the kernel's terms: problem, row (wave, slot), column (lane, slice)."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(r), np.abs(g - r), 0.0)
    d = np.where(np.isnan(d), np.inf, d)
    b, i, j = np.unravel_index(int(d.argmax()), d.shape)
    return "; largest |Z - Z_ref| = %.3g at problem %d, row %d (wave %d, slot %d), column %d (lane %d, slice %d)" % (
        d[b, i, j], b, i, i % 16, i // 16, j, j % 64, j // 64)


def fmt(e):
    return "mass %.3f rows %.3f cols %.3f logplan %.3f of the gate (|d mass| %.2e, |d Z| %.2e)" % (
        e["mass"], e["rows"], e["cols"], e["logplan"], e["mass_abs"], e["logplan_abs"])


def cu(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the cached arrays are read-only
