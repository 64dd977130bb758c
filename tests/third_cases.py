"""Cases, float64 reference and fp32 decision model of tests/test_third_solver_edges_gpu.py: the third level's 65 x 65 solve
(csrc/third_fused3.hip: third_fused3_kernel in the linear domain, every problem whose scalings end outside (0, 2^30] re-solved by
third_fused3_stab_kernel with its scalings absorbed into the stabilisers; csrc/third_fused.hip: third_fused_kernel's log-sum-exp
sweeps for what the stabilised solve gives up on, and for everything in forced-log mode; csrc/sinkhorn.hip: sinkhorn65_kernel for
every call that returns the plan) and the epilogue behind it (Compute_result and the label rule).
tests/test_third_cases_host.py holds every case to its regime under the model and the CPU oracle to the gates - it checks the checker.

Numpy only apart from `cu` (coarse_cases), which imports torch itself, and the seeded draws of pats_amd.synth.

Four things live here:

* the float64 REFERENCE of the solve (ref_sweeps of tests/coarse_cases.py with log_optimal_transport2's marginals and norm for
  64 + 1: ms = 64 * one, real rows exp(norm), dustbin row sum(ns) exp(norm), column j ns_j exp(norm), dustbin column ms exp(norm));
* a float64 RESTATEMENT of Compute_result and the label rule (third_layer.py:161-170, 184-217, as compute_result_problem of
  csrc/third_device.hpp reads them), which also returns what the near-tie mask is built from;
* an fp32 numpy MODEL of what the kernels DECIDE (plain_model, stab_model, written from third3_problem as it is): which problems
  the plain solve flags, after which sweeps the stabilised solve re-bases, and whether it bails out to the log-sum-exp kernel.
  It classifies cases and is no reference for values;
* the CASE TABLE.  Every verdict a test relies on holds with a factor 2^10 to spare (MARGIN): the flag by the final scalings
  (beyond 2^40 or dead, or below 2^20), the bail-out by the scalings of every sweep (dead in float32 AND in a float64 run of the
  same iteration, or inside [2^-100, 2^100] throughout), and regime (d)'s claim that the LAST sweep re-bases with the band
  [2^-20, 2^20] moved by 2^10 either way.  The re-base COUNTS of regimes (b) and (c) are the model's at the band as it is: the
  drift grows by a few powers of two per sweep, so a band moved by 2^10 re-bases on other sweeps (the host test prints all
  three counts); no assertion of the GPU tests depends on them.

What the model says of third3_problem<ST = 1>: the band is tested after every FULL sweep, the last included, and a scaling
outside it is either absorbed in that same sweep (a = b = 1) or sends the problem to the log-sum-exp kernel at once.  With at
least one sweep its final guard therefore cannot fail: the bail-out is the only way to the tail.

What the model did NOT find: a finite input that bails out by the margin (the planned regime (e)).  The largest scaling one
sweep can reach is bounded by the smallest marginal, 2^131 for ns = 2^-126, short of 3e38 * 2^10; the extreme-marginal recipe
(every ns about 2^-50, the real rows 100 nats down in the dustbin column) is flagged after ONE sweep and re-bases after sweeps
1, 2 and 3 instead, which is regime (d).  Regime (f), the non-finite inputs, carries the bail-out and the tail."""
import functools

import numpy as np

from coarse_cases import (LOGPLAN_MASS, LOGPLAN_TOL, MARG_ATOL, MARG_RTOL, MASS_ATOL, MASS_RTOL, NEGINF_ATOL,  # noqa: F401
                          WILD_ATOL, WILD_RTOL, _frozen, cu, plan_errors, ref_sweeps)
from fine_cases import fold, quantised, same_nonfinite, wild_errors  # noqa: F401  (none of them knows a size)

N, NB = 65, 64
SCALE_GUARD = 2.0 ** 30                    # a scaling outside (0, 2^30] after the LAST sweep flags the problem (sc_ok)
DRIFT_LO, DRIFT_HI = 2.0 ** -20, 2.0 ** 20  # the stabilised solve absorbs every scaling once one leaves this band
FIN_HI = 3.0e38                            # ... unless one is outside (0, 3e38]: the bail-out
MARGIN = 2.0 ** 10
FLUSH = np.float32(2.0 ** -126)            # v_exp_f32 flushes denormal results
SWEEPS_ALL = (1, 2, 3, 100)
SWEEPS_FULL = (100,)
M1_TOL = 3e-4 * 8                          # tests/test_gpu_parity.py's gate on mkpts1_f, px
CONF_TOL = 1e-4                            # tests/test_confidence_gpu.py's gate on conf
CLEAR_REL = 1e-3                           # the near-tie mask of the older third-level tests
CLEAR_CAP = 0.02                           # share of a regime's centre rows the mask may leave out
NEGINF_BLOCKS = ((slice(0, 5), slice(7, 20)), (slice(26, 38), slice(40, 51)))      # the second one crosses centre rows 26..29, 34..37
# ((case name, sweeps), gate) -> factor on that gate.  A case is listed only if the fp32 CPU oracle itself misses the gate
# there, with twice the oracle's own share; tests/test_third_cases_host.py asserts that nothing else is listed.
# What is listed: the ZERO-sweep plan exp(Z - norm) of the wild cases.  It is no transport plan - its entries reach e^300 - and a
# float32 log-plan of 100 resolves 3.8e-6 of such a mass, against the gate's 2e-6: no fp32 output can meet it.
GATE_SCALE = {
    (("few_iid_20", 0), "mass"): 3.706, (("few_iid_20", 0), "rows"): 2.471, (("few_iid_20", 0), "cols"): 2.471,
    (("many_iid_40", 0), "mass"): 2.218,
    (("many_cols_20", 0), "mass"): 3.269, (("many_cols_20", 0), "rows"): 2.179, (("many_cols_20", 0), "cols"): 2.179,
    (("many_rows_40", 0), "mass"): 4.360, (("many_rows_40", 0), "rows"): 2.907, (("many_rows_40", 0), "cols"): 2.907,
    (("many_peak_40", 0), "mass"): 2.218,
}

f32 = np.float32


# ---- float64 reference of the solve ----------------------------------------------------------------------------------------
def ot2_marginals(ns, one=1.0, dtype=np.float64):
    """(log_mu, log_nu, norm) of log_optimal_transport2 for ns [b, 64] (modules.py:165-182)."""
    ns = np.asarray(ns, dtype).reshape(len(ns), NB)
    ms = dtype(NB) * dtype(one)
    s = ns.sum(1, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = -np.log(ms + s)
        log_mu = np.concatenate([np.broadcast_to(norm[:, None], (len(ns), NB)), (np.log(s) + norm)[:, None]], 1)
        log_nu = np.concatenate([np.log(ns) + norm[:, None], (np.log(ms) + norm)[:, None]], 1)
    return log_mu.astype(dtype), log_nu.astype(dtype), norm


def ref_ot2_sweeps(scores, ns, sweeps):
    """{iters: log-plan [b, 65, 65]} of log_optimal_transport2 in float64; iters = 0 is Z - norm."""
    log_mu, log_nu, norm = ot2_marginals(ns)
    with np.errstate(all="ignore"):
        return {it: p - norm[:, None, None] for it, (p, _, _) in ref_sweeps(scores, log_mu, log_nu, sweeps).items()}


# ---- float64 restatement of Compute_result and the label rule -------------------------------------------------------------
CENTRE_ROWS = np.array([8 * (q // 4 + 2) + (q % 4 + 2) for q in range(16)])     # [:, 2:6, 2:6] of the 8 x 8 source grid
SELECT = (5, 15, 7, 13)                    # third_layer.py:163-166


def compute_result_ref(S, area, p_s, p_t, outdoor=True):
    """Compute_result + label of ONE problem in float64.  S [65, 65]: the plan exp(Z); area [64] float32: the OT's target areas,
    scale_x = scale_y = sqrt(area + 1e-8) formed in float32 (third_layer.py:153-154); p_s, p_t [2] integers.
    -> dict(m0 [16, 2], m1 [16, 2], label [16, 2], ifm [16] bool, conf [16], and for the masks: top_gap [16] = (top - second)
    / top over the 64 real entries, bin_gap [16] = |dustbin - top| / max(dustbin, top), finite [16] = the row holds no NaN /
    inf and its sum is within float32's range (a zero-sweep plan of wild scores is not), allnan [16]).  The argmax is the kernels': first index, `>` (a NaN never wins)."""
    S = np.asarray(S, np.float64)
    scale = np.sqrt(np.asarray(area, f32).reshape(NB) + f32(1e-8)).astype(np.float64)
    pad, eps7, eps8 = float(f32(1e-2)), float(f32(1e-7)), float(f32(1e-8))
    out = dict(m0=np.zeros((16, 2)), m1=np.zeros((16, 2)), label=np.zeros((16, 2)), ifm=np.zeros(16, bool), conf=np.zeros(16),
               top_gap=np.zeros(16), bin_gap=np.zeros(16), finite=np.zeros(16, bool), allnan=np.zeros(16, bool))
    with np.errstate(all="ignore"):
        for q in range(16):
            row = S[CENTRE_ROWS[q]]
            bi, bv = 0, row[0]
            for k in range(1, NB):
                if row[k] > bv:
                    bi, bv = k, row[k]
            mx, my = bi % 8, bi // 8
            wpx = wpy = sumx = sumy = win = 0.0
            for ty in range(5):
                for tx in range(5):
                    ux, uy = mx + tx - 2, my + ty - 2                        # index3 on the pad-2 map (:189-191)
                    inside = 0 <= ux < 8 and 0 <= uy < 8
                    sb = row[uy * 8 + ux] if inside else 0.0                  # ZeroPad2d(2)
                    sc = scale[uy * 8 + ux] if inside else pad                # ConstantPad2d(2, 1e-2)
                    fx = np.sqrt(sb + eps7) / sc
                    wpx += fx * (tx * 2.0 - 4.0)
                    wpy += fx * (ty * 2.0 - 4.0)
                    sumx += fx
                    sumy += fx
                    win += sb
            out["m1"][q] = (wpx / sumx + (mx + 0.5 - 4.0) * 2.0 + float(p_t[0]), wpy / sumy + (my + 0.5 - 4.0) * 2.0 + float(p_t[1]))
            out["m0"][q] = (float(p_s[0]) + (q % 4) * 2.0 - 3.0, float(p_s[1]) + (q // 4) * 2.0 - 3.0)
            xd = row[NB]
            out["ifm"][q] = not (xd + eps8 > bv + eps8)
            out["conf"][q] = np.fmin(win / row.sum(), 1.0) if not np.isnan(win / row.sum()) else np.nan
            l0 = (1e8 if q in SELECT else -10.0) if not outdoor else (1e8 if out["ifm"][q] else -10.0)
            out["label"][q] = (l0, 1e8)
            top = np.sort(row[:NB])[-2:]
            out["finite"][q] = bool(np.isfinite(row).all()) and row.sum() <= FIN_HI        # ... and float32 can hold it
            out["allnan"][q] = bool(np.isnan(row).all())
            if out["finite"][q]:
                out["top_gap"][q] = (top[1] - top[0]) / top[1] if top[1] > 0 else 0.0
                out["bin_gap"][q] = abs(xd - top[1]) / max(xd, top[1]) if max(xd, top[1]) > 0 else 0.0
    return out


def clear_rows(ref):
    """Centre rows away from near-ties: the top real entry leads the second, and differs from the dustbin entry, by CLEAR_REL."""
    return ref["finite"] & (ref["top_gap"] > CLEAR_REL) & (ref["bin_gap"] > CLEAR_REL)


def match_errors(got, ref):
    """One problem's outputs `got` (dict of m0, m1, label, ifm, conf as the library returns them) against compute_result_ref's:
    {gate: share of the gate} for m1 and conf on the clear rows, 0 / inf for the exact ones (m0 everywhere; ifm and label on
    clear rows; on a row the reference has all NaN: m1 and conf NaN, ifm and label what `not (NaN > NaN)` gives)."""
    clear, nan = clear_rows(ref), ref["allnan"]
    e = dict(m0=0.0 if np.array_equal(np.asarray(got["m0"], np.float64), ref["m0"]) else np.inf, m1=0.0, conf=0.0, ifm=0.0, label=0.0,
             nanrows=0.0)
    if clear.any():
        d1 = np.abs(np.asarray(got["m1"], np.float64)[clear] - ref["m1"][clear])
        dc = np.abs(np.asarray(got["conf"], np.float64)[clear] - ref["conf"][clear])
        e["m1"] = float(np.where(np.isnan(d1), np.inf, d1).max() / M1_TOL)
        e["conf"] = float(np.where(np.isnan(dc), np.inf, dc).max() / CONF_TOL)
    rows = clear | nan
    if not np.array_equal(np.asarray(got["ifm"]).astype(bool)[rows], ref["ifm"][rows]):
        e["ifm"] = np.inf
    if not np.array_equal(np.asarray(got["label"], np.float64)[rows], ref["label"][rows]):
        e["label"] = np.inf
    if nan.any() and not (np.isnan(np.asarray(got["m1"])[nan]).all() and np.isnan(np.asarray(got["conf"])[nan]).all()):
        e["nanrows"] = np.inf
    return e


MATCH_GATES = ("m0", "m1", "conf", "ifm", "label", "nanrows")


# ---- fp32 model of what the kernels decide -------------------------------------------------------------------------------
def _kernel_matrix(Z, r, c, dtype):
    K = np.exp((Z - r[:, None]) - c[None, :], dtype=dtype)
    if dtype is f32:
        K[K < FLUSH] = 0                   # (NaN < x is False: a NaN stays)
    return K


def _start(Z, ns, dtype):
    """Stabilisers r_i = max_j Z_ij, c_j = max_i (Z_ij - r_i) over all 65 (fmaxf: a NaN operand is ignored), K, the marginals
    exp(log_mu), exp(log_nu), b = exp(c)."""
    Z = np.asarray(Z, dtype)
    assert Z.shape == (N, N)
    lmu, lnu, _ = ot2_marginals(np.asarray(ns, f32)[None], dtype=dtype)
    r = np.fmax.reduce(Z, 1)
    c = np.fmax.reduce(Z - r[:, None], 0)
    return Z, r, c, _kernel_matrix(Z, r, c, dtype), np.exp(lmu[0], dtype=dtype), np.exp(lnu[0], dtype=dtype), np.exp(c, dtype=dtype)


def _guard_ok(a, b):
    return bool(np.all((a > 0) & (a <= SCALE_GUARD)) and np.all((b > 0) & (b <= SCALE_GUARD)))


def plain_model(Z, ns, sweeps):
    """third_fused3_kernel's (and sinkhorn65_kernel's) linear iteration a = mu / (K b), b = nu / (K^T a) in float32.
    {iters: dict(hi, lo, tripped)}: the largest and smallest scaling after the last sweep (inf / 0 if one is not finite) and
    whether the 2^30 guard trips, which is tested after the LAST sweep only."""
    with np.errstate(all="ignore"):
        Z, r, c, K, mu, nu, b = _start(Z, ns, f32)
        out = {}
        for it in range(max(sweeps)):
            a = mu / (K @ b)
            b = nu / (K.T @ a)
            if it + 1 in sweeps:
                s = np.concatenate([a, b])
                fin = bool(np.isfinite(s).all())
                out[it + 1] = dict(hi=float(s.max()) if fin else np.inf, lo=float(s.min()) if fin else 0.0, tripped=not _guard_ok(a, b))
        return out


def stab_model(Z, ns, sweeps, shift=1.0, dtype=f32):
    """third3_problem<ST = 1> as it is written: after each FULL sweep (the last included) all four scalings are held to the band
    [2^-20 / shift, 2^20 * shift]; outside it, a scaling outside (0, 3e38] is the bail-out (the problem is left to the
    log-sum-exp kernel), otherwise EVERY scaling is absorbed (r -= ln a, c -= ln b), K is rebuilt from the scores and a = b = 1.
    {iters: dict(rebases = the sweeps (1-based) after which a re-base happens, bail = the sweep of the bail-out or 0,
    ok = the final guard holds, hi, lo = the extreme scalings seen before any absorption over all sweeps, u, v = the duals)}.
    dtype float64: the same iteration without fp32's range, for the margin of the bail-out."""
    with np.errstate(all="ignore"):
        Z, r, c, K, mu, nu, b = _start(Z, ns, dtype)
        rebases, out, hi, lo, bail = [], {}, 0.0, np.inf, 0
        for it in range(max(sweeps)):
            a = mu / (K @ b)
            b = nu / (K.T @ a)
            s = np.concatenate([a, b])
            dead = not bool(np.all((s > 0) & (s <= FIN_HI)))
            hi, lo = (np.inf, 0.0) if dead or not np.isfinite(s).all() else (max(hi, float(s.max())), min(lo, float(s.min())))
            if not bool(np.all((s >= DRIFT_LO / shift) & (s <= DRIFT_HI * shift))):
                if dead:
                    bail = it + 1
                    break
                r, c = (r - np.log(a, dtype=dtype)).astype(dtype), (c - np.log(b, dtype=dtype)).astype(dtype)
                K = _kernel_matrix(Z, r, c, dtype)
                a, b = np.ones(N, dtype), np.ones(N, dtype)
                rebases.append(it + 1)
            if it + 1 in sweeps:
                out[it + 1] = dict(rebases=list(rebases), bail=0, ok=_guard_ok(a, b), hi=hi, lo=lo,
                                   u=np.log(a, dtype=dtype) - r, v=np.log(b, dtype=dtype) - c)
        for n in sweeps:
            if n not in out:
                out[n] = dict(rebases=list(rebases), bail=bail, ok=False, hi=np.inf, lo=0.0, u=None, v=None)
        return out


def clear_of_the_guard(v):
    """The plain verdict does not rest on rounding: tame with every scaling in [2^-100, 2^20], or flagged by a scaling beyond
    2^40, dead (0) or not finite."""
    if v["tripped"]:
        return v["hi"] >= SCALE_GUARD * MARGIN or v["lo"] <= 0.0
    return v["hi"] <= SCALE_GUARD / MARGIN and v["lo"] >= 2.0 ** -100


def model(Z, ns, sweeps):
    """{iters: dict(tripped, hi, lo, sure; rebases, bail, ok, u, v; narrow, wide = the re-base sweeps with the band moved by
    MARGIN inwards / outwards; bail_sure)}.  sure: the flag holds by MARGIN.  bail_sure: so does the bail-out verdict - a
    problem that bails does so in float64 too, by a scaling beyond 3e38 * MARGIN or below 2^-149 / MARGIN or a NaN, in all
    three bands; one that does not keeps every scaling of every sweep inside [2^-100, 2^100] in all three bands."""
    plain = plain_model(Z, ns, sweeps)
    stab, narrow, wide = (stab_model(Z, ns, sweeps, s) for s in (1.0, 1.0 / MARGIN, MARGIN))
    exact = stab_model(Z, ns, sweeps, 1.0, np.float64)
    out = {}
    for it in sweeps:
        v = dict(plain[it], **{k: stab[it][k] for k in ("rebases", "bail", "ok", "u", "v")})
        v["sure"] = clear_of_the_guard(plain[it])
        v["narrow"], v["wide"] = narrow[it]["rebases"], wide[it]["rebases"]
        three = (stab[it], narrow[it], wide[it])
        if v["bail"]:
            v["bail_sure"] = all(x["bail"] == v["bail"] for x in three) and exact[it]["bail"] == v["bail"]
        else:
            v["bail_sure"] = all(not x["bail"] and x["hi"] <= 2.0 ** 100 and x["lo"] >= 2.0 ** -100 for x in three) and not exact[it]["bail"]
        out[it] = v
    return out


# ---- recipes ---------------------------------------------------------------------------------------------------------------
def _iid(rng, amp):
    return amp * rng.standard_normal((N, N))


def _tenth(rng, factor, axis):
    """2 N(0, 1) with a tenth of the rows (axis 0) or columns (axis 1) multiplied by `factor`."""
    Z = 2.0 * rng.standard_normal((N, N))
    pick = rng.permutation(N)[:max(N // 10, 1)]
    if axis == 0:
        Z[pick, :] *= factor
    else:
        Z[:, pick] *= factor
    return Z


def _peak(rng, amp):
    """2 N(0, 1) with a planted permutation of the 64 real rows raised by 3 amp."""
    Z = 2.0 * rng.standard_normal((N, N))
    Z[np.arange(NB), rng.permutation(NB)] += 3.0 * amp
    return Z


def _neginf(Z):
    for rows, cols in NEGINF_BLOCKS:
        Z[rows, cols] = -np.inf
    return Z


def _build(recipe, rng):
    kind, args = recipe[0], recipe[1:]
    if kind == "iid":
        return _iid(rng, *args)
    if kind == "rows":
        return _tenth(rng, args[0], 0)
    if kind == "cols":
        return _tenth(rng, args[0], 1)
    if kind == "peak":
        return _peak(rng, *args)
    if kind == "neginf":
        return _neginf(_build(args, rng))
    if kind == "early":                    # the fine table's `early_o`: the real rows `args[0]` nats down in the dustbin column
        Z = 0.5 * rng.standard_normal((N, N))
        Z[:NB, NB] = -float(args[0])
        return Z
    if kind in ("nan", "posinf"):
        Z = _iid(rng, 0.5)
        Z[27, 41] = np.nan if kind == "nan" else np.inf                     # row 27 is a centre row
        return Z
    if kind == "neginf_row":
        Z = _iid(rng, 0.5)
        Z[27, :] = -np.inf
        return Z
    raise KeyError(kind)


# name, regime, recipe, sweep counts, seed (None: the case's index; the seeded ones were picked by the model from a scan over
# amplitudes and seeds - the re-base count of a recipe varies with the draw), row of the synth draw its areas come from, log2 of
# the factor on them, descriptors: the case can be made from descriptors (no -inf score)
TABLE = [
    ("tame_iid_half", "a", ("iid", 0.5), SWEEPS_ALL, None, 10, 0, True),
    ("tame_iid_3", "a", ("iid", 3.0), SWEEPS_ALL, None, 11, 0, True),
    ("tame_peak_1", "a", ("peak", 1.0), SWEEPS_ALL, None, 12, 0, True),
    ("few_iid_20", "b", ("iid", 20.0), SWEEPS_ALL, (41, 1, 20), 1, 0, True),
    ("few_cols_10", "b", ("cols", 10.0), SWEEPS_ALL, (42, 7, 10), 7, 0, True),
    ("many_iid_40", "c", ("iid", 40.0), SWEEPS_FULL, (41, 2, 40), 2, 0, True),
    ("many_cols_20", "c", ("cols", 20.0), SWEEPS_FULL, (42, 0, 20), 0, 0, True),
    ("many_rows_40", "c", ("rows", 40.0), SWEEPS_FULL, (43, 0, 40), 0, 0, True),
    ("many_peak_40", "c", ("peak", 40.0), SWEEPS_FULL, (44, 2, 40), 2, 0, True),
    ("last_early_100", "d", ("early", 100.0), SWEEPS_ALL, (45, 100), 0, -50, True),
    ("nan_desc", "f", ("nan",), SWEEPS_FULL, None, 13, 0, True),
    ("posinf_desc", "f", ("posinf",), (1, 100), None, 14, 0, True),
    ("neginf_row", "f", ("neginf_row",), SWEEPS_FULL, None, 15, 0, False),
    ("neginf_cols_20", "g", ("neginf", "cols", 20.0), SWEEPS_FULL, (42, 0, 20), 0, 0, False),
    ("neginf_cols_10", "g", ("neginf", "cols", 10.0), SWEEPS_FULL, (42, 7, 10), 7, 0, False),
]
NAMES = [t[0] for t in TABLE]
ROW = {t[0]: t for t in TABLE}
REGIMES = "abcdfg"                          # (e), a bail-out with finite inputs, has no case: see the module's docstring
REGIME_NAME = dict(a="tame", b="one or two re-bases", c="six or more re-bases", d="re-base on the last sweep",
                   f="not finite", g="flagged with -inf blocks")
# the sweep counts of regime (d) at which the stabilised solve leaves its loop with a = b = 1 and a freshly built K
LAST_SWEEP_REBASE = {"last_early_100": (1, 2, 3)}
AREA_SEED_OFFSET, AREA_ROWS = 65, 32
DESC_D = 256                               # sqrt(D) = 16: see descriptors()
DESC_BITS = 18                             # mantissa bits a case's scores keep


@functools.lru_cache(maxsize=None)
def synth_draw():
    """area [32, 64], p_s, p_t [32, 2] of one pats_amd.synth.third_inputs draw: every case takes its row of them."""
    from pats_amd import synth
    inp = synth.third_inputs(seed=synth.SEED + AREA_SEED_OFFSET, P=AREA_ROWS)
    return _frozen(dict(area=inp["scale"].reshape(AREA_ROWS, NB).astype(f32), p_s=inp["p_s"], p_t=inp["p_t"]))


def predicted_scores(d0, d1):
    """What cost65_accumulate + cost65_scale give for descriptors() in float32: every product and sum of the contraction is
    exact (one term per score is not zero), / sqrt(256) is exact, and 0.1f * x is the one rounding.  A NaN or inf element
    makes its NaN through 0 * inf in any order of summation, and an INFINITE accumulator becomes a NaN score as well:
    div_invariant (csrc/common.hpp) corrects x * rd by the residual fma(-q, d, x), which is inf - inf (the reference's
    inf / 16 * 0.1 stays inf; the problem is not finite either way)."""
    with np.errstate(all="ignore"):
        acc = np.einsum("bdn,bdm->bnm", np.asarray(d0, np.float64), np.asarray(d1, np.float64)).astype(f32)
        q = acc * f32(1.0 / 16.0)
        return (f32(0.1) * (q + (acc - q * f32(16.0)) * f32(1.0 / 16.0))).astype(f32)


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case's fp32 inputs: Z [65, 65] (as the kernels see it: cut to DESC_BITS bits and through predicted_scores, so that
    the descriptor form and the score form of a case are ONE problem), ns = area [64], p_s, p_t [2]."""
    _, regime, recipe, _, seed, arow, e2, _ = ROW[name]
    rng = np.random.default_rng([31, NAMES.index(name)] if seed is None else list(seed))
    draw = synth_draw()
    Zq = quantised(_build(recipe, rng).astype(f32))
    with np.errstate(all="ignore"):
        Z = (f32(0.1) * (f32(10.0) * Zq)).astype(f32)
    ns = (draw["area"][arow].astype(np.float64) * 2.0 ** e2).astype(f32)
    return _frozen(dict(Z=Z, Zq=Zq, ns=ns, p_s=draw["p_s"][arow], p_t=draw["p_t"][arow]))


def descriptors(names):
    """d0, d1 [b, 256, 65] whose cost 0.1 * (d0^T d1 / sqrt(256)) is problem(name)['Z']: d0 = 160 on the diagonal of its first 65
    channels, d1 = the quantised draw in them."""
    d0, d1 = np.zeros((len(names), DESC_D, N), f32), np.zeros((len(names), DESC_D, N), f32)
    for k, n in enumerate(names):
        assert ROW[n][7], n
        d0[k, np.arange(N), np.arange(N)] = 160.0
        d1[k, :N, :] = problem(n)["Zq"]
    return d0, d1


def kernel_scores(name):
    """The scores of a case as the kernels have them.  Through descriptors a NaN / +inf ELEMENT spreads over its score column
    (0 * NaN); the `f` cases that can be made from descriptors are defined that way for every entry point."""
    if ROW[name][1] == "f" and ROW[name][7]:
        return predicted_scores(*descriptors([name]))[0]
    return problem(name)["Z"]


def all_sweeps(name):
    return (0,) + tuple(ROW[name][3])


@functools.lru_cache(maxsize=None)
def reference(name):
    """{iters: float64 log-plan [65, 65]} at 0 sweeps and the case's sweep counts, from one run to the largest."""
    p = problem(name)
    ref = ref_ot2_sweeps(kernel_scores(name)[None], p["ns"][None], all_sweeps(name))
    return _frozen({it: r[0] for it, r in ref.items()})


@functools.lru_cache(maxsize=None)
def match_reference(name, sweeps, outdoor=True):
    p = problem(name)
    with np.errstate(all="ignore"):
        return compute_result_ref(np.exp(reference(name)[sweeps]), p["ns"], p["p_s"], p["p_t"], outdoor)


@functools.lru_cache(maxsize=None)
def verdict(name):
    return model(kernel_scores(name), problem(name)["ns"], ROW[name][3])


def flagged(name, sweeps):
    return sweeps > 0 and verdict(name)[sweeps]["tripped"]


def tail(name, sweeps):
    """The stabilised solve gives the problem up (the bail-out): it ends in third_fused_kernel's log-sum-exp sweeps."""
    return flagged(name, sweeps) and bool(verdict(name)[sweeps]["bail"])


def cases_at(sweeps, descriptors_only=True):
    return [t[0] for t in TABLE if (sweeps == 0 or sweeps in t[3]) and (t[7] or not descriptors_only)]


def expected_counts(mode, names, sweeps, stab=True):
    """(sinkhorn_fallbacks, sinkhorn_tail_solves) of one throughput launch: the model's in kernel mode, 0 / 0 in the forced log
    domain and at 0 sweeps (launch_third_fused sends both to third_fused_kernel directly, whose iters == 0 leaves before the
    guard); no tail solve without the stabilised kernel (PATS_THIRD_STAB=0) and none through sinkhorn65_kernel."""
    if mode != "kernel" or sweeps == 0:
        return 0, 0
    return sum(flagged(n, sweeps) for n in names), sum(tail(n, sweeps) for n in names) if stab else 0


TAME = ("tame_iid_half", "tame_iid_3", "tame_peak_1")


# ---- the production family: D = 128, the redo-walk base set's wild problems -------------------------------------------------
WILD_K, WILD_N = 96, 32
WILD_AMPS = np.tile(np.array([3.0, 5.0, 9.0, 14.0], f32), WILD_N // 4)


@functools.lru_cache(maxsize=None)
def wild_inputs():
    """The 32 amplified problems of tests/test_third_redo_walk_gpu.py's base set (d0, d1 [32, 128, 65], scale, p_s, p_t)."""
    from pats_amd import synth
    inp = synth.third_inputs(seed=synth.SEED + 64, P=WILD_K)
    d0, d1 = inp["d0"][:WILD_N] * WILD_AMPS[:, None, None], inp["d1"][:WILD_N] * WILD_AMPS[:, None, None]
    return _frozen(dict(d0=d0.astype(f32), d1=d1.astype(f32), scale=inp["scale"][:WILD_N].reshape(WILD_N, NB).astype(f32),
                        p_s=inp["p_s"][:WILD_N], p_t=inp["p_t"][:WILD_N]))


def wild_references(scores, sweeps=100):
    """From the fp32 scores `scores` [32, 65, 65] somebody built for wild_inputs(): (float64 log-plans, match references, model
    verdicts) - the solve and the epilogue are measured, not the cost build."""
    w = wild_inputs()
    scores = np.asarray(scores, f32)
    ref = ref_ot2_sweeps(scores, w["scale"], (sweeps,))[sweeps]
    with np.errstate(all="ignore"):
        mref = [compute_result_ref(np.exp(ref[k]), w["scale"][k], w["p_s"][k], w["p_t"][k], True) for k in range(WILD_N)]
    return ref, mref, [plain_model(scores[k], w["scale"][k], (sweeps,))[sweeps] for k in range(WILD_N)]


def wild_gate_scale(oracle_Z, ref):
    """[{gate: factor}] per problem of the D = 128 family for the two gates on its log-plan: 1, or twice the fp32 CPU oracle's
    own share where the oracle (`oracle_Z`, its log-plans from its own scores) misses the gate against `ref`.  The family's
    scores reach +-3000, where one ulp is 2.4e-4: the oracle misses the wild gate on every problem amplified by 9 or 14.
    Computed from the oracle wherever it is used, the GPU test included - never from the kernel."""
    out = []
    for k in range(WILD_N):
        e = wild_errors(oracle_Z[k], ref[k])
        out.append({g: (2.0 * e[g] if e[g] > 1.0 else 1.0) for g in ("wild", "mass")})
    return out


# ---- the comparisons ------------------------------------------------------------------------------------------------------
def check_plan_case(got, ref, is_flagged, regime, what, scale=None, record=None):
    """One problem's log-plan `got` [65, 65] (float32) against the float64 `ref`: the same NaN / -inf / +inf pattern, and on the
    finite entries the gates of section 'Gates' of docs/parity.md's third-level section: a problem the model does not flag
    takes the coarse suite's four (mass, rows, cols, logplan); a flagged one the wild gate on the log-plan and the mass gate
    where exp(Z_ref) > 1e-6; regimes (f) and (g), whose scores are not finite, NEGINF_ATOL on the finite entries."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (N, N), (what, got.dtype, got.shape)
    scale = scale or {}
    record = {} if record is None else record
    pattern = same_nonfinite(got, ref)
    if regime in "fg":
        fin = np.isfinite(ref) & np.isfinite(got)
        d = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
        e, gates = dict(neginf=d / NEGINF_ATOL, neginf_abs=d), ("neginf",)
    elif is_flagged:
        e, gates = wild_errors(got, ref), ("wild", "mass")
    else:
        assert np.isfinite(ref).all(), what
        e, gates = plan_errors(got, ref), ("mass", "rows", "cols", "logplan")
    record.update({g: e[g] for g in gates})
    if not pattern:
        record["pattern"] = np.inf
    assert pattern, "%s: the NaN / -inf / +inf pattern differs from the reference's (%d / %d / %d against %d / %d / %d)" % (
        (what,) + tuple(int(f(x).sum()) for x in (got, ref) for f in (np.isnan, np.isneginf, np.isposinf)))
    for gate in gates:
        assert e[gate] <= scale.get(gate, 1.0), "%s: gate '%s' missed: %.3g of the gate (largest absolute error %.3g)" % (
            what, gate, e[gate], e[gate + "_abs"])
    return {g: e[g] for g in gates}


def check_plan(got, name, sweeps, what="", record=None):
    scale = {g: f for ((n, it), g), f in GATE_SCALE.items() if (n, it) == (name, sweeps)}
    return check_plan_case(got, reference(name)[sweeps], flagged(name, sweeps), ROW[name][1],
                           "%s %s it=%d" % (what, name, sweeps), scale, record)


def check_matches_case(got, ref, what, record=None):
    """One problem's matches against compute_result_ref's under match_errors' gates."""
    e = match_errors(got, ref)
    if record is not None:
        record.update(e)
    for gate in MATCH_GATES:
        assert e[gate] <= 1.0, "%s: '%s' missed: %.3g of the gate" % (what, gate, e[gate])
    return e


def check_matches(got, name, sweeps, outdoor=True, what="", record=None):
    return check_matches_case(got, match_reference(name, sweeps, outdoor), "%s %s it=%d" % (what, name, sweeps), record)


def unclear_share(refs):
    """Share of the finite centre rows of `refs` (compute_result_ref results) that the near-tie mask leaves out."""
    fin = np.concatenate([r["finite"] for r in refs])
    clear = np.concatenate([clear_rows(r) for r in refs])
    return float(1.0 - clear[fin].mean()) if fin.any() else 0.0


def report(worst, head):
    return "\n".join("%s regime (%s) %s: %s" % (head, g, REGIME_NAME.get(g, g), ", ".join(
        "%s %.3f" % (gate, s) for (gg, gate), s in sorted(worst.items()) if gg == g)) for g in sorted({k[0] for k in worst}))
