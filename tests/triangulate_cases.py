"""The per-pair triangulation of include/pats_amd.h ("Per-pair triangulation") restated in numpy float64, a seeded generator of
two-view scenes that keeps the true 3-D points, two degenerate scenes, and the classifiers of the cells a float64 evaluation in
another order may decide differently.  Shared by tests/test_triangulate_cases_host.py (CPU) and tests/test_triangulate_gpu.py;
written from the header's definition alone, in the header's operation order.

Definition (per match; x = the float32 point after the optional normalisation, promoted to float64):
    R_p, t_p   swapped ? (P R P, P t) : (R, t); a pair with a non-finite entry or t = 0 has no valid match
    a = R_p x_l,  b = x_r,  c = a x b,  cc = c.c,  lambda = c.(b x t_p) / cc,  mu = c.(a x t_p) / cc
    X = R_p^T ((lambda a + t_p + mu b) / 2 - t_p),  Y = R_p X + t_p
    e2 = |pi(X) - x_l|^2 + |pi(Y) - x_r|^2,  cosp = a.b / (|a| |b|)
    valid      used, cc > 0, lambda > 0, mu > 0, X[2] > 0, Y[2] > 0, everything finite and within float32's range, under the limits
A match is UNDECIDED when |lambda|, |mu|, X[2] or Y[2] lies within BAND = 2^10 eps64, relative, of the sum of the |terms| of its
defining dot product - the float64 analogue of pose_cases.fronts' band - and NEAR A LIMIT when e2 or cosp lies within BAND,
relative, of its limit.

Measured on the committed seeds (tests/test_triangulate_cases_host.py prints them; docs/parity.md records them):
    C_MEASURED  the largest |X - X_gt| / (eps32 kappa |X_gt|) on the noise-free scenes, kappa = |a|^2 |b|^2 / cc.  The inputs are
                rounded to float32 and nothing else, so this is the triangulation's sensitivity to half a float32 step per
                coordinate: 0.0842.  C = 4 C_MEASURED = 0.337, the margin for seeds not tried.
    the undecided share is 0 of 16 240 matches on the committed seeds (the cap is 1e-3)."""
import numpy as np

import epipolar_cases as ec
import pose_cases as pc

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = pc.EPS64
FLT_MAX = float(np.finfo(np.float32).max)
BAND = 2.0 ** 10 * EPS64
UNDECIDED_CAP = 1e-3
P_SWAP = pc.P_SWAP
C_MEASURED = 0.0842     # seed 308; the other seeds 0.03 .. 0.08
C = 4 * C_MEASURED

# the committed seeds: (seed, matches)
HOST_CASES = [(301, 20), (302, 65), (303, 500), (304, 513), (305, 1025), (306, 1200), (307, 3000), (308, 4097), (309, 5820)]


def make_scene(seed, n, outliers=0.3, noise=5e-4):
    """One pair with pose_cases.make_scene's distributions - depth 3..8, |t| = 1, a rotation of 0.05..0.4 rad - that keeps the true
    points.  -> dict(ml, mr [n,2] float32, R, t, X [n,3] the points in the LEFT camera's frame, good [n] bool)."""
    rng = np.random.default_rng(seed)
    R = ec._rotation(rng, rng.uniform(0.05, 0.4))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    Z = rng.uniform(3.0, 8.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.6, 0.6, n) * Z, Z], 1)
    Y = X @ R.T + t[None, :]
    xl = X[:, :2] / X[:, 2:3]
    xr = Y[:, :2] / Y[:, 2:3] + rng.normal(scale=noise, size=(n, 2))
    bad = rng.random(n) < outliers
    xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
    return {"ml": xl.astype(np.float32), "mr": xr.astype(np.float32), "R": R, "t": t, "X": X, "good": ~bad}


def pure_rotation_scene(seed, n, exact=False):
    """x_r generated with t = 0, to be triangulated under a unit t: every ray pair is parallel, cc is rounding noise - or, with
    exact (R = I, x_r = x_l bit for bit), exactly 0."""
    rng = np.random.default_rng(seed)
    R = np.eye(3) if exact else ec._rotation(rng, rng.uniform(0.05, 0.4))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    Z = rng.uniform(3.0, 8.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.6, 0.6, n) * Z, Z], 1)
    Y = X @ R.T
    ml = (X[:, :2] / X[:, 2:3]).astype(np.float32)
    mr = ml.copy() if exact else (Y[:, :2] / Y[:, 2:3]).astype(np.float32)
    return {"ml": ml, "mr": mr, "R": R, "t": t, "X": X, "good": np.ones(n, bool)}


def baseline_scene(seed, n):
    """Matches on the baseline: every point lies on the line through the two camera centres, so both rays are that line and every
    match is the pair of epipoles - cc is rounding noise."""
    rng = np.random.default_rng(seed)
    R = ec._rotation(rng, rng.uniform(0.05, 0.4))
    t = np.array([0.3, -0.2, 1.0]) + 0.05 * rng.normal(size=3)
    t /= np.linalg.norm(t)
    centre = -R.T @ t                                   # the right camera's centre in the left frame (third component < 0)
    X = -rng.uniform(2.0, 6.0, n)[:, None] * centre[None, :]          # beyond the left camera, away from the right one
    Y = X @ R.T + t[None, :]
    return {"ml": (X[:, :2] / X[:, 2:3]).astype(np.float32), "mr": (Y[:, :2] / Y[:, 2:3]).astype(np.float32), "R": R, "t": t, "X": X,
            "good": np.ones(n, bool)}


def point_frame(R, t, swapped=False):
    """(R_p, t_p): the pose in the frame of the points."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return (P_SWAP @ R @ P_SWAP, P_SWAP @ t) if swapped else (R, t)


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _absdot(u, v):
    return np.abs(u[0] * v[0]) + np.abs(u[1] * v[1]) + np.abs(u[2] * v[2])


def triangulate64(xl, xr, used, R, t, swapped=False, max_reproj=None, max_cos=None):
    """The definition for one pair from the float32 points xl, xr [n,2], in the header's operation order.
    -> dict(valid [n] bool; points [n,3], depths [n,2], reproj [n], cos [n] float64, zeros where not valid and `points` in the
    OUTPUT frame (P X for swapped); X [n,3] in the frame of the points; cc, kappa, lambda, mu, e2 [n] as computed, for every row; undecided, near_reproj,
    near_cos [n] bool)."""
    n = xl.shape[0]
    used = np.asarray(used, bool) & np.isfinite(xl).all(1) & np.isfinite(xr).all(1)
    Rp, tp = point_frame(R, t, swapped)
    posed = bool(np.isfinite(Rp).all() and np.isfinite(tp).all() and tp.any())
    if not posed:
        Rp, tp = np.eye(3), np.array([0.0, 0.0, 1.0])   # anything finite: no row is valid
    one = np.ones(n)
    with np.errstate(all="ignore"):
        l = [xl[:, 0].astype(np.float64), xl[:, 1].astype(np.float64), one]
        b = [xr[:, 0].astype(np.float64), xr[:, 1].astype(np.float64), one]
        a = [(Rp[i, 0] * l[0] + Rp[i, 1] * l[1]) + Rp[i, 2] for i in range(3)]
        c = [a[1] - a[2] * b[1], a[2] * b[0] - a[0], a[0] * b[1] - a[1] * b[0]]
        bt = [b[1] * tp[2] - tp[1], tp[0] - b[0] * tp[2], b[0] * tp[1] - b[1] * tp[0]]
        at = _cross(a, tp)
        cc = _dot(c, c)
        dl, dr = _dot(c, bt), _dot(c, at)
        lam, mu = dl / cc, dr / cc
        q = [((lam * a[0] + tp[0]) + mu * b[0]) * 0.5 - tp[0], ((lam * a[1] + tp[1]) + mu * b[1]) * 0.5 - tp[1],
             ((lam * a[2] + tp[2]) + mu) * 0.5 - tp[2]]
        X = [(Rp[0, j] * q[0] + Rp[1, j] * q[1]) + Rp[2, j] * q[2] for j in range(3)]
        Y = [((Rp[i, 0] * X[0] + Rp[i, 1] * X[1]) + Rp[i, 2] * X[2]) + tp[i] for i in range(3)]
        d = [X[0] / X[2] - l[0], X[1] / X[2] - l[1], Y[0] / Y[2] - b[0], Y[1] / Y[2] - b[1]]
        e2 = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])
        aa, bb = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + 1.0
        cosp = ((a[0] * b[0] + a[1] * b[1]) + a[2]) / (np.sqrt(aa) * np.sqrt(bb))
        valid = used & posed & (cc > 0) & (lam > 0) & (mu > 0) & (X[2] > 0) & (Y[2] > 0) & np.isfinite(Y[0]) & np.isfinite(Y[1]) & np.isfinite(Y[2])
        for v in (X[0], X[1], X[2], lam, mu, e2, cosp):
            valid &= np.abs(v) <= FLT_MAX               # False for a NaN
        near_r, near_c = np.zeros(n, bool), np.zeros(n, bool)
        if max_reproj is not None:
            lim = np.float64(np.float32(max_reproj)) ** 2
            valid &= e2 <= lim
            near_r = used & (np.abs(e2 - lim) <= BAND * lim)
        if max_cos is not None:
            lim = np.float64(np.float32(max_cos))
            valid &= cosp <= lim
            near_c = used & (np.abs(cosp - lim) <= BAND * np.abs(lim))
        # the sign margins: each quantity against the sum of the |terms| of the dot product that defines it
        sX2 = np.abs(Rp[0, 2] * q[0]) + np.abs(Rp[1, 2] * q[1]) + np.abs(Rp[2, 2] * q[2])
        sY2 = np.abs(Rp[2, 0] * X[0]) + np.abs(Rp[2, 1] * X[1]) + np.abs(Rp[2, 2] * X[2]) + np.abs(tp[2])
        und = used & posed & ~((np.abs(dl) > BAND * _absdot(c, bt)) & (np.abs(dr) > BAND * _absdot(c, at)) &
                               (np.abs(X[2]) > BAND * sX2) & (np.abs(Y[2]) > BAND * sY2))     # a NaN anywhere: undecided
        kappa = aa * bb / cc
    X = np.stack(X, 1)
    pts = X[:, [1, 0, 2]] if swapped else X
    z = lambda v: np.where(valid.reshape((n,) + (1,) * (v.ndim - 1)), v, 0.0)              # noqa: E731
    return {"valid": valid, "points": z(pts), "depths": z(np.stack([lam, mu], 1)), "reproj": z(e2), "cos": z(cosp), "X": X, "cc": cc,
            "kappa": kappa, "undecided": und, "near_reproj": near_r, "near_cos": near_c, "used": used, "lambda": lam, "mu": mu, "e2": e2}


def reference(ml, mr, segs, mask, R, t, norm=None, swapped=False, max_reproj=None, max_cos=None):
    """Per pair triangulate64's dict (plus lo, n) for the segments `segs` = [(lo, n)] of the flat lists."""
    out = []
    for p, (lo, n) in enumerate(segs):
        xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        ref = triangulate64(xl, xr, np.asarray(mask[lo:lo + n]) != 0, R[p], t[p], swapped, None if max_reproj is None else max_reproj[p],
                            None if max_cos is None else max_cos[p])
        out.append(dict(ref, lo=lo, n=n, xl=xl, xr=xr))
    return out
