"""The per-pair pose error and the AUC over accumulated errors as include/pats_amd.h defines them ("Per-pair pose error and AUC"),
restated in numpy float64 from the header alone - the same operations in the same order, one scalar at a time - plus the bounds the
tests hold both against and the seeded case generators.  No kernel, no library: the CPU tests check this file against the
reference's recorded outputs (tests/golden/pose_metrics.npz), the GPU tests check the kernels against this file.

Bounds
  angles   an angle is acos of a cosine c that is a sum of products divided by norms; a float64 evaluation in ANY order moves c by a
           few 2^-53 of the sum of the |terms|, and near c = +-1 acos turns that into far more than an ulp of the angle.  So the
           bound is the angle's own conditioning: move c by `moves` * 2^-53 * sum|terms| in both directions, clip, take the spread
           of acos over that interval in degrees, and add 8 ulps of the result.  moves = 16 against the reference (np.dot, np.trace
           and np.linalg.norm fix no summation order), 4 against the device (the same order: only acos differs, 4 ulps by OpenCL's
           bound)
  auc      both sides add at most n + 1 non-negative float64 terms: n * 2^-50, relative"""
import math

import numpy as np

DEG = 57.29577951308232                                # 180 / pi rounded to float64
F = np.float64
THRESHOLDS = (5.0, 10.0, 20.0)
MAX_N = 16384


# ---- the definition -------------------------------------------------------------------------------------------------------------
def _angle(c):
    """acos(clip(c)) in degrees; a NaN stays a NaN."""
    if c < -1.0:
        c = F(-1.0)
    if c > 1.0:
        c = F(1.0)
    return np.arccos(c) * F(DEG)


def ground_truth64(T1, T0=None):
    """(R_gt [3,3], t_gt [3]) of one pair, the header's order."""
    A = np.asarray(T1, F)
    if T0 is None:
        return A[:3, :3].copy(), A[:3, 3].copy()
    B = np.asarray(T0, F)
    G, g = np.empty((3, 3), F), np.empty(3, F)
    for i in range(3):
        for j in range(3):
            G[i, j] = (A[i, 0] * B[j, 0] + A[i, 1] * B[j, 1]) + A[i, 2] * B[j, 2]
    for i in range(3):
        g[i] = A[i, 3] - ((G[i, 0] * B[0, 3] + G[i, 1] * B[1, 3]) + G[i, 2] * B[2, 3])
    return G, g


def pose_error64(R, t, T1, T0=None, counts=None, min_matches=15, min_gt_t=0.0):
    """The stage for a batch -> dict of err_R, err_t, err [pairs] float64, status [pairs] int32, and for the bounds cos_R, abs_R,
    cos_t, abs_t, e_t: the two cosines before the clip, the sums of the |terms| behind them (in the cosine's units) and the
    translation angle before the fold (NaN where a pair was not evaluated or the quantity does not exist)."""
    R, t, T1 = np.asarray(R, F), np.asarray(t, F), np.asarray(T1, F)
    pairs = R.shape[0]
    out = {k: np.full(pairs, np.inf, F) for k in ("err_R", "err_t", "err")}
    out.update({k: np.full(pairs, np.nan, F) for k in ("cos_R", "abs_R", "cos_t", "abs_t", "e_t")})
    out["status"] = np.zeros(pairs, np.int32)
    with np.errstate(all="ignore"):
        for p in range(pairs):
            read = [T1[p, :3, :4]] + ([np.asarray(T0, F)[p, :3, :4]] if T0 is not None else [])
            if counts is not None and int(counts[p]) < min_matches:
                st = 1
            elif not (np.isfinite(R[p]).all() and np.isfinite(t[p]).all()) or not t[p].any():
                st = 2
            elif not all(np.isfinite(a).all() for a in read):
                st = 3
            else:
                st = 0
            out["status"][p] = st
            if st:
                continue
            G, g = ground_truth64(T1[p], None if T0 is None else T0[p])
            r, gg = R[p].reshape(9), G.reshape(9)
            s = r[0] * gg[0]
            for k in range(1, 9):
                s = s + r[k] * gg[k]
            c = (s - F(1.0)) / F(2.0)
            eR = _angle(c)
            out["cos_R"][p], out["abs_R"][p] = c, (np.abs(r * gg).sum() + 1.0) / 2.0
            ng = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            if ng <= min_gt_t:
                eT = F(0.0)
            else:
                d = (t[p, 0] * g[0] + t[p, 1] * g[1]) + t[p, 2] * g[2]
                nt = np.sqrt((t[p, 0] * t[p, 0] + t[p, 1] * t[p, 1]) + t[p, 2] * t[p, 2])
                c = d / (nt * ng)
                e = _angle(c)
                f = F(180.0) - e
                eT = f if f < e else e
                out["cos_t"][p], out["abs_t"][p], out["e_t"][p] = c, np.abs(t[p] * g).sum() / (nt * ng), e
            eR = F(np.inf) if np.isnan(eR) else eR
            eT = F(np.inf) if np.isnan(eT) else eT
            out["err_R"][p], out["err_t"][p], out["err"][p] = eR, eT, (eR if eR > eT else eT)
    return out


def auc64(errors, thresholds=THRESHOLDS):
    """The aggregate -> (auc [n_thr] float64, below [n_thr] int64, sorted [n]): the header's closed form, the sum by math.fsum (the
    device's order is its own; the bound covers any)."""
    e = np.asarray(errors, F).reshape(-1)
    e = np.sort(np.where(np.isnan(e), np.inf, np.where(e == 0.0, 0.0, e)))         # a NaN is +inf, -0.0 is +0.0
    n = e.size
    auc, below = np.zeros(len(thresholds), F), np.zeros(len(thresholds), np.int64)
    if n == 0:
        return auc, below, e
    inv = F(1.0) / F(n)
    x = np.concatenate([[0.0], e])
    for j, thr in enumerate(thresholds):
        k = int(np.searchsorted(e, thr, side="left"))
        i = np.arange(k, dtype=F)
        with np.errstate(all="ignore"):
            terms = ((x[1:k + 1] - x[:k]) * (i * inv + (i + 1.0) * inv)) * 0.5
        area = F(math.fsum(terms.tolist())) + (F(thr) - x[k]) * (F(k) * inv)
        auc[j], below[j] = area / F(thr), k
    return auc, below, e


# ---- the bounds -----------------------------------------------------------------------------------------------------------------
def angle_bound(c, abs_terms, result, moves):
    """Degrees an angle may differ by: acos's spread over c -+ moves 2^-53 abs_terms (clipped) plus 8 ulps of `result`.  Arrays."""
    c, abs_terms, result = np.asarray(c, F), np.asarray(abs_terms, F), np.asarray(result, F)
    d = moves * 2.0 ** -53 * abs_terms
    spread = (np.arccos(np.clip(c - d, -1.0, 1.0)) - np.arccos(np.clip(c + d, -1.0, 1.0))) * DEG
    return spread + 8.0 * np.spacing(np.abs(result))


def ulps(a, b):
    """|a - b| in ulps of b (float64 arrays; 0 where both are equal, infinities included)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.abs(b)))


def auc_bound(n, auc):
    return max(int(n), 1) * 2.0 ** -50 * np.abs(np.asarray(auc, F))


# ---- generators -----------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' formula, float64."""
    axis = np.asarray(axis, F)
    axis = axis / np.linalg.norm(axis)
    A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], F)
    return np.eye(3) + np.sin(angle) * A + (1 - np.cos(angle)) * (A @ A)


def random_rotation(rng):
    return rotation(rng.normal(size=3), rng.uniform(0.0, np.pi))


ANGLES = (0.0, 1e-7, 3e-7, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 2.0, np.pi - 1e-6, np.pi)
T_KINDS = ("random", "parallel", "opposite", "orthogonal", "near", "near_opposite")


def pose_sets(seed, n):
    """n seeded (R, t, R_gt, t_gt): the rotation between R and R_gt walks through ANGLES (identical up to pi), the translations
    through T_KINDS (parallel, opposite and orthogonal among them); |t| = 1 as the pose stage writes it, |t_gt| is free."""
    rng = np.random.default_rng(seed)
    R, t, Rg, tg = np.empty((n, 3, 3), F), np.empty((n, 3), F), np.empty((n, 3, 3), F), np.empty((n, 3), F)
    for i in range(n):
        Rg[i] = random_rotation(rng)
        ang = ANGLES[i % len(ANGLES)]
        R[i] = Rg[i].copy() if ang == 0.0 else rotation(rng.normal(size=3), ang) @ Rg[i]
        g = rng.normal(size=3) * rng.uniform(0.1, 30.0)
        kind = T_KINDS[(i // len(ANGLES) + i) % len(T_KINDS)]
        if kind == "random":
            v = rng.normal(size=3)
        elif kind == "parallel":
            v = g.copy()
        elif kind == "opposite":
            v = -g
        elif kind == "orthogonal":
            v = np.cross(g, rng.normal(size=3))
        elif kind == "near":
            v = rotation(rng.normal(size=3), 10.0 ** rng.uniform(-8, -2)) @ g
        else:
            v = -(rotation(rng.normal(size=3), 10.0 ** rng.uniform(-8, -2)) @ g)
        t[i], tg[i] = v / np.linalg.norm(v), g
    return R, t, Rg, tg


def as_T(Rm, tv):
    """[n,4,4] rigid transforms from [n,3,3] and [n,3]."""
    T = np.zeros((len(Rm), 4, 4), F)
    T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = Rm, tv, 1.0
    return T


def extrinsic_sets(seed, R_gt, t_gt):
    """Seeded (T0, T1) with T1 inv(T0) = (R_gt | t_gt) up to rounding: T0 a random rigid transform, T1 = (R_gt | t_gt) T0."""
    rng = np.random.default_rng(seed)
    n = len(R_gt)
    T0 = as_T(np.stack([random_rotation(rng) for _ in range(n)]), rng.normal(size=(n, 3)) * 2.0)
    return T0, as_T(R_gt, t_gt) @ T0


AUC_SIZES = (0, 1, 2, 3, 15, 64, 65, 1000, 4000)


def error_lists(seed):
    """name -> (err_R list, err_t list): what aggregate_metrics takes; their elementwise maximum is pose_auc's input.  Plain lists of
    every size of AUC_SIZES, the same with a fifth of the entries inf, and one list with entries exactly 5, 10 and 20."""
    rng = np.random.default_rng(seed)
    out = {}
    for n in AUC_SIZES:
        for kind in ("plain", "inf"):
            eR, eT = rng.gamma(1.2, 6.0, n), rng.gamma(1.0, 8.0, n)
            if kind == "inf" and n:
                lost = rng.random(n) < 0.2
                eR[lost], eT[lost] = np.inf, np.inf
            out["%s_%d" % (kind, n)] = (eR, eT)
    eR, eT = rng.gamma(1.2, 6.0, 200), rng.gamma(1.0, 3.0, 200)
    eR[[3, 50, 51, 120, 121, 122]] = [5.0, 10.0, 10.0, 20.0, 20.0, 20.0]
    eT[[3, 50, 51, 120, 121, 122]] = [1.0, 10.0, 2.0, 20.0, 0.5, 3.0]
    out["ties_200"] = (eR, eT)
    return out
