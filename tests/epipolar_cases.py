"""The per-pair model verification of include/pats_amd.h ("Per-pair model verification") restated in numpy, a seeded generator of
two-view cases and a float32 emulation of the test.  Shared by tests/test_epipolar_cases_host.py (CPU) and
tests/test_epipolar_gpu.py; written from the header's definition alone.

Definition (per pair; x = the float32 point after the optional normalisation, promoted to float64):
    a = E x_l,  b = E^T x_r,  r = x_r . a,  den = a0^2 + a1^2 + b0^2 + b1^2
    inlier iff the match participates and den > 0 and r^2 <= thr^2 den
A (match, model) cell is DECIDED when the float64 r^2 lies outside [thr^2 den (1 - DELTA), thr^2 den (1 + DELTA)] - or when the
verdict does not depend on rounding at all (the match does not participate, thr is NaN or negative, den is exactly 0, a NaN).
A float32 evaluation may differ from the float64 verdict on undecided cells only."""
import numpy as np

DELTA = 1e-3            # relative half-width of the undecided band around thr^2 den (docs/parity.md records the measured shares)


def normalise32(pts, norm_side):
    """pts [n,2] float32, norm_side = (c0, c1, s0, s1): one float32 subtract, then one float32 multiply."""
    pts = np.ascontiguousarray(pts, np.float32)
    c = np.asarray(norm_side[:2], np.float32)
    s = np.asarray(norm_side[2:4], np.float32)
    return ((pts - c[None, :]).astype(np.float32) * s[None, :]).astype(np.float32)


def points32(ml, mr, norm_row=None):
    """The float32 x_l, x_r [n,2] of a segment (the third coordinate is 1)."""
    ml, mr = np.ascontiguousarray(ml, np.float32), np.ascontiguousarray(mr, np.float32)
    if norm_row is None:
        return ml, mr
    norm_row = np.asarray(norm_row, np.float32)
    return normalise32(ml, norm_row[:4]), normalise32(mr, norm_row[4:])


def participates(xl, xr, conf=None, min_conf=None):
    part = np.isfinite(xl).all(1) & np.isfinite(xr).all(1)
    if min_conf is not None:
        with np.errstate(invalid="ignore"):
            part &= np.asarray(conf, np.float32) >= np.float32(min_conf)        # False for a NaN confidence
    return part


def _cells(xl, xr, E, dtype):
    """r^2 and den [H,n] in `dtype`, every operation rounded to it (np.float32: the emulation; np.float64: the restatement)."""
    E = np.asarray(E, np.float32).astype(dtype).reshape(-1, 3, 3)
    l0, l1 = xl[:, 0].astype(dtype)[None, :], xl[:, 1].astype(dtype)[None, :]
    r0, r1 = xr[:, 0].astype(dtype)[None, :], xr[:, 1].astype(dtype)[None, :]
    e = lambda i, j: E[:, i, j][:, None]                                         # noqa: E731
    with np.errstate(all="ignore"):
        a0 = e(0, 0) * l0 + e(0, 1) * l1 + e(0, 2)
        a1 = e(1, 0) * l0 + e(1, 1) * l1 + e(1, 2)
        a2 = e(2, 0) * l0 + e(2, 1) * l1 + e(2, 2)
        b0 = e(0, 0) * r0 + e(1, 0) * r1 + e(2, 0)
        b1 = e(0, 1) * r0 + e(1, 1) * r1 + e(2, 1)
        r = r0 * a0 + r1 * a1 + a2
        den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1
        return r * r, den


def classify(xl, xr, part, E, thr, delta=DELTA):
    """-> (inlier64 [H,n] bool, decided [H,n] bool) of one pair."""
    H, n = np.asarray(E).reshape(-1, 3, 3).shape[0], xl.shape[0]
    thr = np.float32(thr)
    if not thr >= 0:                                                             # NaN or negative: no inliers, nothing to round
        return np.zeros((H, n), bool), np.ones((H, n), bool)
    r2, den = _cells(xl, xr, E, np.float64)
    lim = np.float64(thr) ** 2 * den
    with np.errstate(invalid="ignore"):
        inl = part[None, :] & (den > 0) & (r2 <= lim)
        outside = (r2 < lim * (1 - delta)) | (r2 > lim * (1 + delta))
        certain = ~part[None, :] | np.isnan(r2) | np.isnan(lim) | (den == 0)     # no rounding can turn these into inliers
    return inl, outside | certain


def emulate32(xl, xr, part, E, thr):
    """The same formula with every operation in np.float32 -> inlier [H,n] bool."""
    thr = np.float32(thr)
    H, n = np.asarray(E).reshape(-1, 3, 3).shape[0], xl.shape[0]
    if not thr >= 0:
        return np.zeros((H, n), bool)
    r2, den = _cells(xl, xr, E, np.float32)
    with np.errstate(all="ignore"):
        lim = (thr * thr).astype(np.float32) * den
        return part[None, :] & (den > 0) & (r2 <= lim)


def segments(pairs, cap, pair_off=None, stride=None, counts=None):
    """(lo, n) per pair as the device resolves them (clamped: never outside [0, cap])."""
    out = []
    for p in range(pairs):
        if pair_off is not None:
            lo, hi = (min(max(int(v), 0), cap) for v in (pair_off[p], pair_off[p + 1]))
            out.append((lo, max(hi - lo, 0)))
        else:
            out.append((p * stride, min(max(int(counts[p]), 0), stride)))
    return out


def reference(ml, mr, segs, models, thr, norm=None, conf=None, min_conf=None, delta=DELTA):
    """Per pair a dict: inl [H,n] (float64 verdicts), decided [H,n], strict [H] (decided inliers), loose [H] (strict + undecided),
    xl, xr (float32 points), part."""
    out = []
    for p, (lo, n) in enumerate(segs):
        xl, xr = points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        part = participates(xl, xr, None if conf is None else conf[lo:lo + n], min_conf)
        inl, dec = classify(xl, xr, part, models[p], thr[p], delta)
        strict = (inl & dec).sum(1)
        out.append({"inl": inl, "decided": dec, "strict": strict, "loose": strict + (~dec).sum(1), "xl": xl, "xr": xr, "part": part,
                    "lo": lo, "n": n})
    return out


def moments64(xl, xr, mask):
    """sum over mask of q q^T, q = vec(x_r x_l^T) in float64 -> (M [9,9], A [9,9] = the sum of |terms|)."""
    l = np.concatenate([xl.astype(np.float64), np.ones((xl.shape[0], 1))], 1)[mask]
    r = np.concatenate([xr.astype(np.float64), np.ones((xr.shape[0], 1))], 1)[mask]
    q = (r[:, :, None] * l[:, None, :]).reshape(-1, 9)
    t = q[:, :, None] * q[:, None, :]
    return t.sum(0), np.abs(t).sum(0)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _unit(E):
    return E / np.linalg.norm(E)


def make_case(seed, n, H, outliers=0.4, thr=2e-3, noise=5e-4):
    """One pair: n matches in normalised coordinates of order 1 (float32), H hypotheses (float32, Frobenius norm 1): the true
    essential matrix at a seeded index, perturbed copies of it and random matrices.  -> dict(ml, mr, models, thr, true)."""
    rng = np.random.default_rng(seed)
    R = _rotation(rng, rng.uniform(0.05, 0.4))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = _unit(tx @ R)
    Z = rng.uniform(3.0, 8.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.6, 0.6, n) * Z, Z], 1)
    Y = X @ R.T + t[None, :]
    xl = X[:, :2] / X[:, 2:3]
    xr = Y[:, :2] / Y[:, 2:3] + rng.normal(scale=noise, size=(n, 2))
    bad = rng.random(n) < outliers
    xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
    models = np.empty((H, 3, 3))
    true = int(rng.integers(0, H))
    for h in range(H):
        if h == true:
            models[h] = E
        elif h % 2:
            models[h] = _unit(E + rng.normal(scale=rng.uniform(0.02, 0.2), size=(3, 3)))
        else:
            models[h] = _unit(rng.normal(size=(3, 3)))
    return {"ml": xl.astype(np.float32), "mr": xr.astype(np.float32), "models": models.astype(np.float32), "thr": np.float32(thr),
            "true": true}


# the committed seeds of the host test: (seed, matches, models)
HOST_CASES = [(101, 3000, 96), (102, 2049, 257), (103, 500, 64), (104, 4097, 33), (105, 1200, 128), (106, 65, 300)]
