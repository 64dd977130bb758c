"""Cases, dispatch mirror and the comparison of tests/test_stream_solver_edges_gpu.py (the streaming Sinkhorn solver of
csrc/sinkhorn_stream.hip: every coarse problem above 304 x 320); tests/test_stream_cases_host.py holds the CPU oracle and the
tables to what the GPU tests rely on.  The float64 reference, the seeded draws and the four project gates are coarse_cases'.

The solver has three forms, chosen on the host (launch_stream) from the shape, the batch and the stream's CU count:
  two launches a sweep   stream_sweep_kernel<RB, CPT> (a workgroup of 512 threads per block of RB = 16 | 17 rows; thread t owns
                         columns t + 512 q, q < CPT = ceil(N / 512)) + stream_colreduce_kernel (64 columns a workgroup, 16 waves
                         split the row blocks, 18 partials a wave in flight, a tail loop above 288 blocks);
  <32 | 64, 2, 64>       stream_resident_kernel, all sweeps in one launch, N <= 1024, M N >= 500^2: thread t owns columns 2 t and
                         2 t + 1; workgroup g < ceil(N / 64) reduces columns 64 g .. over the row blocks in 32 slices (slice rs
                         holds blocks rs, rs + 32, rs + 64, rs + 96);
  <17, 9, 32>            the same kernel for ONE problem of the 4097^2 class.  Its smallest problem is 4097 x 4097: a float64
                         reference of that size does not fit a test of seconds, and test_streaming_solver_block_shapes, the
                         roofline golden and the determinism test run it.  It has no row here.
stream_plan mirrors that choice; every row of the tables carries the plan it is meant to reach on 256 CUs.

Numpy only (coarse_cases.cu imports torch itself)."""
import collections
import functools

import numpy as np

import coarse_cases as cc
from coarse_cases import (ref_sweeps, ref_ot_sweeps, final_scalings, plan_errors, check_plan, _marginal, _scores, cu,  # noqa: F401
                          GATES, LOGPLAN_TOL, WILD_ATOL, WILD_RTOL, NEGINF_ATOL, AMPS, ALPHAS)

ST = 512                                   # threads of a streaming workgroup (csrc/sinkhorn_stream.hip)
N_CU = 256                                 # the CU count the tables' plans are written for
# (case key, entry point, gate) -> factor, coarse_cases' rule: twice the fp32 oracle's own error where the oracle misses a gate
GATE_SCALE = {}
ALL_GATES = GATES + ("every",)

Plan = collections.namedtuple("Plan", "cpt RB nblk res_kind res_nblk ngroups rounded why_not")


def _ceil(a, b):
    return -(-a // b)


def res_partial_stride(M, N):
    return (_ceil(M, 16) * N + 3) & ~3


def stream_plan(M, N, batch, n_cu=N_CU, iters=100):
    """launch_stream's choices for `batch` problems of [M, N] on a stream of n_cu CUs (PATS_STREAM_RESIDENT unset):
    cpt, RB, nblk of the two-launch form and the set-up kernels; res_kind 0 (two launches a sweep), 1 (<17, 9, 32>), 2
    (<32, 2, 64>) or 3 (<64, 2, 64>) with res_nblk row blocks a problem; ngroups, the workgroups that reduce columns (of 32
    for res_kind 1, else of 64); rounded, whether res_partial_stride rounded a problem's share of the partial area up;
    why_not, which of the four conditions behind `fits` sent a resident candidate back to two launches ('' otherwise)."""
    cpt = _ceil(N, ST)

    def rounds(rb):
        return (batch * _ceil(M, rb) + n_cu - 1) // n_cu
    rb17 = cpt >= 7 and rounds(17) < rounds(16)
    RB = 17 if rb17 else 16
    nblk = _ceil(M, RB)
    res_kind, res_nblk, why_not = 0, 0, ""
    if iters > 0:
        if batch == 1 and rb17 and cpt == 9:
            res_kind, res_nblk = 1, nblk
        elif N <= 1024 and M * N >= 500 * 500:
            per = n_cu // batch
            need = _ceil(M, per) if per >= 1 else 1 << 30
            if need <= 32:
                res_kind, res_nblk = 2, _ceil(M, 32)
            elif need <= 64:
                res_kind, res_nblk = 3, _ceil(M, 64)
        if res_kind:
            gw = 32 if res_kind == 1 else 64
            nsl = ST // (gw // 4)
            conds = (("grid", res_nblk * batch <= n_cu), ("slices", res_nblk <= 4 * nsl), ("groups", _ceil(N, gw) <= res_nblk),
                     ("area", res_nblk * ((N + 3) & ~3) + 2 * N <= _ceil(M, 16) * N))
            failed = [name for name, ok in conds if not ok]
            if failed:
                res_kind, res_nblk, why_not = 0, 0, failed[0]
    gw = 32 if res_kind == 1 else 64
    return Plan(cpt, RB, nblk, res_kind, res_nblk, _ceil(N, gw), res_partial_stride(M, N) != _ceil(M, 16) * N, why_not)


def res_rb(plan):
    return {0: 0, 1: 17, 2: 32, 3: 64}[plan.res_kind]


def fmt_plan(p):
    if p.res_kind == 0:
        return "two launches: <%d, %d>, %d blocks%s" % (p.RB, p.cpt, p.nblk, ", not resident (%s)" % p.why_not if p.why_not else "")
    return "resident <%d, %d, %d>: %d blocks, %d reduce groups%s" % (res_rb(p), 9 if p.res_kind == 1 else 2, 32 if p.res_kind == 1 else 64,
                                                                  p.res_nblk, p.ngroups, ", rounded stride" if p.rounded else "")


Row = collections.namedtuple("Row", "M N batch plan why")


def _row(M, N, batch, why, **plan):
    return Row(M, N, batch, plan, why)


# ---- the tables: (M, N, batch, the plan on 256 CUs, what the row walks) ----------------------------------------------------------
# Three problems a row unless the plan needs another batch: 97 or 128 blocks of 32 rows fit 256 CUs twice, not three times, so
# (3100, 200) and (4096, 62) run TWO problems (three would be <64, 2, 64> with 49 / 64 blocks), and (4097, 62) runs ONE (two or
# three problems may have fewer CUs each, which makes it <64, 2, 64> with 65 blocks instead of the refusal the row is about).
TWO_LAUNCH = [
    _row(400, 250, 3, "below 500^2, so never resident; N < 512, so threads 250.. own nothing", cpt=1, RB=16, nblk=25, res_kind=0),
    _row(190, 513, 3, "slot 1 held by thread 0 only; last block 14 rows", cpt=2, RB=16, nblk=12, res_kind=0),
    _row(96, 1025, 3, "slot 2 held by thread 0 only", cpt=3, RB=16, nblk=6, res_kind=0),
    _row(64, 1537, 3, "slot 3 held by thread 0 only; every block full", cpt=4, RB=16, nblk=4, res_kind=0),
    _row(48, 2049, 3, "slot 4 held by thread 0 only", cpt=5, RB=16, nblk=3, res_kind=0),
    _row(38, 2561, 3, "slot 5 held by thread 0 only; last block 6 rows", cpt=6, RB=16, nblk=3, res_kind=0),
    _row(32, 3073, 3, "slot 6 held by thread 0 only; two blocks", cpt=7, RB=16, nblk=2, res_kind=0),
    _row(28, 3585, 3, "slot 7 held by thread 0 only", cpt=8, RB=16, nblk=2, res_kind=0),
    _row(24, 4097, 3, "the ninth slot in thread 0 only", cpt=9, RB=16, nblk=2, res_kind=0),
    _row(22, 4608, 3, "the widest problem; every slot of every thread in use", cpt=9, RB=16, nblk=2, res_kind=0),
    _row(4608, 22, 3, "the column reduce's 18 in-flight partials per wave exactly full; tail loop empty", cpt=1, nblk=288, res_kind=0),
    _row(4609, 22, 3, "the tail loop takes one block, in wave 0", cpt=1, nblk=289, res_kind=0),
    _row(4700, 21, 3, "the tail loop in six waves", cpt=1, nblk=294, res_kind=0),
    _row(480, 1024, 3, "15 blocks of 32 rows would be fewer than the 16 reduce groups; the neighbour of (481, 1024)",
         cpt=2, nblk=30, res_kind=0, why_not="groups"),
    _row(499, 501, 3, "M N = 249 999, one below the resident threshold; the neighbour of (500, 500)", cpt=1, nblk=32, res_kind=0, why_not=""),
    _row(4097, 62, 1, "129 blocks of 32 rows exceed the reducer's four slices; the neighbour of (4096, 62)",
         cpt=1, nblk=257, res_kind=0, why_not="slices"),
]
TWO_LAUNCH_BIG = [
    _row(270, 3073, 16, "16 x 17 blocks of 16 rows is 272 workgroups, a second round on 256 CUs; 16 x 16 blocks of 17 rows is one; "
                        "last block 15 rows", cpt=7, RB=17, nblk=16, res_kind=0),
    _row(270, 3585, 16, "the same at eight columns a thread", cpt=8, RB=17, nblk=16, res_kind=0),
    _row(270, 4097, 16, "the same at nine; a batch, so not the 4097^2-class resident kernel", cpt=9, RB=17, nblk=16, res_kind=0),
]
RESIDENT_32 = [
    _row(500, 500, 3, "the smallest resident shape; half the workgroups reduce, half only arrive; last block 20 rows",
         res_kind=2, res_nblk=16, ngroups=8, rounded=False),
    _row(520, 501, 3, "N odd: the last owning thread holds one column; row pitch 504; ceil(M / 16) N = 16 533 floats, rounded to "
                      "16 536, so problems 1 and 2 sit behind a rounded stride", res_kind=2, res_nblk=17, ngroups=8, rounded=True),
    _row(481, 1024, 3, "every workgroup reduces; last block one row; every thread owns two columns", res_kind=2, res_nblk=16, ngroups=16),
    _row(512, 1024, 3, "everything full", res_kind=2, res_nblk=16, ngroups=16),
    _row(1100, 500, 3, "reducer slice rs + NSL holds three blocks", res_kind=2, res_nblk=35, ngroups=8),
    _row(2100, 300, 3, "slice rs + 2 NSL holds two", res_kind=2, res_nblk=66, ngroups=5),
    _row(3100, 200, 2, "slice rs + 3 NSL holds one", res_kind=2, res_nblk=97, ngroups=4),
    _row(4096, 62, 2, "all four slices full (nblk == 4 NSL); N < 64, so lanes 62 and 63 of the group publish nothing",
         res_kind=2, res_nblk=128, ngroups=1),
]
RESIDENT_64 = [
    _row(520, 501, 20, "9 blocks x 20 problems = 180 workgroups: per-problem counters, strides and granules at 20 problems; "
                       "last block 8 rows", res_kind=3, res_nblk=9, ngroups=8, rounded=True),
    _row(600, 513, 17, "10 blocks, 9 groups: group 8 holds one column", res_kind=3, res_nblk=10, ngroups=9),
]
SMALL_ROWS = TWO_LAUNCH + RESIDENT_32
BIG_ROWS = TWO_LAUNCH_BIG + RESIDENT_64
ALL_ROWS = SMALL_ROWS + BIG_ROWS
NSL = 32                                   # slices of the row blocks in the <RB, 2, 64> reducer


def row_id(r):
    return "%dx%d" % (r.M, r.N) + ("" if r.batch == 3 else "b%d" % r.batch)


def row_index(M, N, batch):
    return [(r.M, r.N, r.batch) for r in ALL_ROWS].index((M, N, batch))


def plan_matches(plan, want):
    return all(getattr(plan, k) == v for k, v in want.items())


def sweeps_of(batch, entry="s"):
    if entry == "o":
        return (1, 100)
    return (1, 2, 3, 100) if batch <= 3 else (1, 10) if batch == 16 else (1, 2, 100)


def picks_of(batch):
    """The problems of a batch that get a float64 reference: all of three, else the first, one inside and the last."""
    return tuple(range(batch)) if batch <= 3 else (0, 7, 15) if batch == 16 else (0, 1, batch - 1)


# ---- seeded inputs with their float64 plans --------------------------------------------------------------------------------------
def sinkhorn_inputs(M, N, batch):
    """(Z, log_mu, log_nu) of a row, without its references (the two-launch child process needs no more)."""
    idx = row_index(M, N, batch) if batch > 1 else 1                # one problem alone: amplitude 3
    rng = np.random.default_rng([21, M, N, batch])
    Z = _scores(rng, idx, batch, M, N)
    return Z, _marginal(rng, batch, M), _marginal(rng, batch, N)


def _sinkhorn_case(M, N, batch):
    Z, log_mu, log_nu = sinkhorn_inputs(M, N, batch)
    pick = list(picks_of(batch))
    ref = {it: p for it, (p, _, _) in ref_sweeps(Z[pick], log_mu[pick], log_nu[pick], sweeps_of(batch)).items()}
    return cc._frozen(dict(Z=Z, log_mu=log_mu, log_nu=log_nu, ref=ref, pick=pick))


sinkhorn_case = functools.lru_cache(maxsize=None)(_sinkhorn_case)     # the rows of up to three problems
big_case = functools.lru_cache(maxsize=2)(_sinkhorn_case)              # 16, 17 and 20 problems: 21 to 71 MB of scores each


@functools.lru_cache(maxsize=None)
def ot_case(M, N, batch):
    """Inputs of log_optimal_transport (scores [batch, M - 1, N - 1]) and the float64 plans after 1 and 100 sweeps."""
    idx = row_index(M, N, batch) if batch > 1 else 1
    rng = np.random.default_rng([22, M, N, batch])
    m, n = M - 1, N - 1
    S = _scores(rng, idx, batch, m, n)
    ns = rng.uniform(0.5, 2.0, (batch, 1, n)).astype(np.float32)
    alpha = ALPHAS[idx % 3]
    ref = {it: p for it, (p, _, _) in ref_ot_sweeps(S, alpha, ns, sweeps_of(batch, "o")).items()}
    return cc._frozen(dict(scores=S, ns=ns, alpha=alpha, ref=ref))


COST_MN, COST_D, COST_B = (520, 501), 64, 3


@functools.lru_cache(maxsize=None)
def cost_ot_case():
    """coarse_cases.cost_ot_case's construction at (520, 501): descriptors whose scores have the spread of the problem's amplitude,
    and the float64 plans (1 and 100 sweeps) of the FLOAT64 cost."""
    M, N = COST_MN
    rng = np.random.default_rng([23, M, N])
    m, n = M - 1, N - 1
    sd = np.sqrt(10.0 * AMPS[1])
    d0 = (sd * rng.standard_normal((COST_B, COST_D, m))).astype(np.float32)
    d1 = (sd * rng.standard_normal((COST_B, COST_D, n))).astype(np.float32)
    ns = rng.uniform(0.5, 2.0, (COST_B, 1, n)).astype(np.float32)
    ref = {it: p for it, (p, _, _) in ref_ot_sweeps(cc.ref_cost(d0, d1), ALPHAS[1], ns, (1, 100)).items()}
    return cc._frozen(dict(d0=d0, d1=d1, ns=ns, alpha=ALPHAS[1], ref=ref))


# ---- stale workspace ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stale_case(M, N, first_sweeps, then_sweeps):
    """Two unrelated problem sets of one shape: P (amplitude 0.5, solved first with first_sweeps) and Q (amplitude 3, other scores
    and marginals, solved in the same scratch block with then_sweeps) and Q's float64 plan."""
    rng = np.random.default_rng([24, M, N, first_sweeps])
    d = {}
    for name, amp in (("P", AMPS[0]), ("Q", AMPS[1])):
        d[name] = (amp * rng.standard_normal((3, M, N))).astype(np.float32)
        d[name + "_mu"], d[name + "_nu"] = _marginal(rng, 3, M), _marginal(rng, 3, N)
    d["ref"] = ref_sweeps(d["Q"], d["Q_mu"], d["Q_nu"], (then_sweeps,))[then_sweeps][0]
    return cc._frozen(d)


# ---- guard trips ---------------------------------------------------------------------------------------------------------------------
# (M, N, batch, wild problems): two launches, <32, 2, 64>, <64, 2, 64>
GUARD_ROWS = [(330, 320, 6, (1, 4)), (520, 501, 6, (1, 4)), (520, 501, 20, (1, 4, 19))]
GUARD_FACTOR, GUARD_SWEEPS = 120.0, 100    # 60 * N(0, 1): test_wide_dynamic_range's amplitude; 30 stays inside the guard at (520, 501)
# rows 0..4 x columns 7..19, and rows x columns 250..262 across a row-block boundary (16 at (330, 320); 32, the resident block, at
# (520, 501)) and column 256, where a reduce group of 64 columns ends.  (Columns 508..516, across the column where a thread's slot
# changes in the two-launch layout, do not exist at N = 501 or 320.)
NEGINF_BLOCKS = {(330, 320): ((slice(0, 5), slice(7, 20)), (slice(12, 21), slice(250, 263))),
                 (520, 501): ((slice(0, 5), slice(7, 20)), (slice(28, 41), slice(250, 263)))}
NEGINF_PICK = (0, 2, 5)


def guard_tame(batch, wild):
    return [k for k in range(batch) if k not in wild]


def guard_pick(batch, wild):
    """The problems with a float64 reference: all six, or the wild ones and three tame ones of twenty."""
    return list(range(batch)) if batch <= 6 else sorted(set(wild) | {0, 10, 18})


@functools.lru_cache(maxsize=None)
def guard_case(M, N, batch, wild, entry):
    """`batch` problems of 0.5 * N(0, 1) scores, the wild ones multiplied by 120, for `entry` 's' (Z [batch, M, N]) or 'o' (scores
    [batch, M - 1, N - 1], alpha 0.5).  ref: float64 plans after 100 sweeps of the problems guard_pick names, amax / bmax their
    linear-domain scalings; Z_sub: the batch with the wild problems replaced by further tame draws (same size, so the same plan);
    for six problems Z_inf, the tame draw with the two NEGINF_BLOCKS at -inf, and ref_inf for problems NEGINF_PICK."""
    rng = np.random.default_rng([25, M, N, batch, ord(entry)])
    m, n = (M, N) if entry == "s" else (M - 1, N - 1)
    tame = (AMPS[0] * rng.standard_normal((batch, m, n))).astype(np.float32)
    Z = tame.copy()
    for k in wild:
        Z[k] *= np.float32(GUARD_FACTOR)
    Zs = tame.copy()
    Zs[list(wild)] = (AMPS[0] * rng.standard_normal((len(wild), m, n))).astype(np.float32)
    d = dict(Z=Z, Z_sub=Zs, pick=guard_pick(batch, wild))
    pick = d["pick"]
    if batch <= 6:
        Zi = tame.copy()
        for rows, cols in NEGINF_BLOCKS[(M, N)]:
            Zi[:, rows, cols] = -np.inf
        d["Z_inf"] = Zi
    ip = list(NEGINF_PICK)
    if entry == "s":
        d["log_mu"], d["log_nu"] = _marginal(rng, batch, M), _marginal(rng, batch, N)
        (p, u, v), = ref_sweeps(Z[pick], d["log_mu"][pick], d["log_nu"][pick], (GUARD_SWEEPS,)).values()
        d["amax"], d["bmax"] = final_scalings(Z[pick], u, v)
        if batch <= 6:
            d["ref_inf"] = cc.ref_sinkhorn(Zi[ip], d["log_mu"][ip], d["log_nu"][ip], GUARD_SWEEPS)
    else:
        d["ns"] = rng.uniform(0.5, 2.0, (batch, 1, n)).astype(np.float32)
        d["alpha"] = 0.5
        (p, u, v), = ref_ot_sweeps(Z[pick], d["alpha"], d["ns"][pick], (GUARD_SWEEPS,)).values()
        d["amax"], d["bmax"] = final_scalings(cc.ot_problem(Z[pick], d["alpha"], d["ns"][pick])[0], u, v)
        if batch <= 6:
            d["ref_inf"] = cc.ref_log_optimal_transport(Zi[ip], d["alpha"], d["ns"][ip], GUARD_SWEEPS)
    d["ref"] = p
    return cc._frozen(d)


LOUD_SHAPES, LOUD_AMP = [(330, 320), (520, 501), (22, 4608)], 12.0


@functools.lru_cache(maxsize=None)
def loud_case(M, N, entry):
    """One problem of 12 * N(0, 1) scores: loud, but its scalings stay inside the guard, so the linear path must keep it.  amin /
    amax: the smallest and largest final scaling of either side at the float64 duals after 100 sweeps."""
    rng = np.random.default_rng([26, M, N, ord(entry)])
    m, n = (M, N) if entry == "s" else (M - 1, N - 1)
    Z = (LOUD_AMP * rng.standard_normal((1, m, n))).astype(np.float32)
    d = dict(Z=Z)
    if entry == "s":
        d["log_mu"], d["log_nu"] = _marginal(rng, 1, M), _marginal(rng, 1, N)
        (p, u, v), = ref_sweeps(Z, d["log_mu"], d["log_nu"], (GUARD_SWEEPS,)).values()
        C = Z.astype(np.float64)
    else:
        d["ns"] = rng.uniform(0.5, 2.0, (1, 1, n)).astype(np.float32)
        d["alpha"] = 0.5
        (p, u, v), = ref_ot_sweeps(Z, d["alpha"], d["ns"], (GUARD_SWEEPS,)).values()
        C = cc.ot_problem(Z, d["alpha"], d["ns"])[0]
    r = C.max(2)
    c = (C - r[:, :, None]).max(1)
    la, lb = (u + r) / np.log(2.0), (v + c) / np.log(2.0)
    d["log2_min"], d["log2_max"] = float(min(la.min(), lb.min())), float(max(la.max(), lb.max()))
    d["ref"] = p
    return cc._frozen(d)


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def locate(got, ref, plan):
    """Where the largest |Z - Z_ref| sits, in the streaming solver's terms under `plan`: problem, row, column; the row block and
    the row within it for the set-up's and two-launch form's RB and for the resident RB; the thread and slot that own the column;
    the workgroup (reduce group) and lane that sum it."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(r), np.abs(g - r), 0.0)
    d = np.where(np.isnan(d), np.inf, d)
    b, i, j = (int(x) for x in np.unravel_index(int(d.argmax()), d.shape))
    s = "; largest |Z - Z_ref| = %.3g at problem %d, row %d, column %d: row block %d row %d (RB %d)" % (
        d[b, i, j], b, i, j, i // plan.RB, i % plan.RB, plan.RB)
    if plan.res_kind:
        s += ", resident block %d row %d (RB %d)" % (i // res_rb(plan), i % res_rb(plan), res_rb(plan))
    if plan.res_kind == 0:
        t, q, gw = j % ST, j // ST, 64
    elif plan.res_kind == 1:
        t, q, gw = (j // 8, j % 8, 32) if j < 4096 else (j - 4096, 8, 32)
    else:
        t, q, gw = j // 2, j % 2, 64
    return s + "; thread %d slot %d; reduce group %d lane %d" % (t, q, j // gw, j % gw)


def every_entry(got, ref, wild=False):
    """(share of the gate, largest |Z - Z_ref|) over ALL finite entries of ref: LOGPLAN_TOL for a tame problem, WILD_ATOL +
    WILD_RTOL |Z_ref| for a loud one.  The error of Z + u + v is an error of the duals, whatever the entry's mass."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(r)
    d = np.abs(g[fin] - r[fin])
    lim = (WILD_ATOL + WILD_RTOL * np.abs(r[fin])) if wild else LOGPLAN_TOL
    return float((d / lim).max()), float(d.max())


def check_all(got, ref, what, plan, key=None, entry=None, wild=False):
    """The four project gates through coarse_cases.check_plan, then the every-entry gate; a miss is located in the plan's terms."""
    try:
        e = check_plan(got, ref, what, key, entry)
    except AssertionError as x:
        raise AssertionError(str(x) + locate(got, ref, plan)) from None
    e["every"], e["every_abs"] = every_entry(got, ref, wild)
    lim = GATE_SCALE.get((key, entry, "every"), 1.0)
    assert e["every"] <= lim, "%s: every-entry gate missed: %.3g of the gate (largest |Z - Z_ref| %.3g)%s" % (
        what, e["every"], e["every_abs"], locate(got, ref, plan))
    return e


def check_wild(got, ref, what, plan):
    """A guard-tripping problem (|Z| of hundreds): finite, and every entry within the WILD gate."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    share, dz = every_entry(got, ref, wild=True)
    assert share <= 1.0, "%s: WILD gate missed: %.3g of the gate (largest |Z - Z_ref| %.3g)%s" % (what, share, dz, locate(got, ref, plan))
    return share, dz


def fmt(e):
    return cc.fmt(e) + "; every entry %.3f of the gate (|d Z| %.2e)" % (e["every"], e["every_abs"])


def masked_coverage(ref):
    """Share of the entries the project's log-plan gate looks at: exp(Z_ref) > LOGPLAN_MASS."""
    return float((np.asarray(ref) > np.log(cc.LOGPLAN_MASS)).mean())
