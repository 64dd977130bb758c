"""The absolute-pose branch of include/pats_amd.h ("Per-pair absolute pose from depth") restated in numpy: the lift in float32 (bit
for bit by construction: every operation is one rounded float32 operation in the header's order), the K = 3 sampler, a float64 P3P
(Grunert's quartic through numpy.roots and an SVD alignment - the device brackets the quartic's roots, polishes the three distances
and aligns two orthonormal frames), the reprojection test as a float32 emulation in the kernel's order (its FMAs emulated exactly)
and as a float64 classification with an undecided band, and a generator of solver cases.  Shared by
tests/test_absolute_cases_host.py (CPU) and tests/test_absolute_gpu.py; written from the header's definition alone.

Definition of the test (per pair; X = the lifted float32 point, r = the float32 right point after the optional normalisation):
    Y = R X + t,  inlier iff X and r are finite, the confidence gate passes, Y2 > 0 and (Y0 - r0 Y2)^2 + (Y1 - r1 Y2)^2 <= thr^2 Y2^2
A (match, model) cell is DECIDED when the float64 left side lies outside [lim (1 - DELTA), lim (1 + DELTA)], lim = thr^2 Y2^2, and Y2
is not within rounding of 0 - or when the verdict does not depend on rounding at all (the match does not take part, thr is NaN or
negative, Y is exactly 0, a NaN)."""
import numpy as np

import epipolar_cases as ec
import essential5_cases as e5
import hypotheses_cases as hc

EPS32 = float(np.finfo(np.float32).eps)
DELTA = 1e-3            # relative half-width of the undecided band around thr^2 Y2^2: epipolar_cases.classify's scheme
MARGIN = e5.MARGIN      # the hypotheses' argument, not widened: 4 (another method than the reference's) x 2 (operation order)
POSE_TOL = 1e-3         # |R - R_true|_F + |t - t_true|_2: "the true pose is among the models"
F32 = np.float32


# ---- the lift ---------------------------------------------------------------------------------------------------------------------
def lift32(pts, depth, norm_left=None, max_depth=None, interp=0, max_jump=None):
    """pts [n,2] float32 in (c0, c1) order, depth a float32 [h,w] map or None (a null or empty map) -> (X [n,3] float32 with NaN rows
    for invalid matches, valid [n] bool).  Every arithmetic step is one float32 operation, in the header's order."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = pts.shape[0]
    X = np.full((n, 3), np.nan, F32)
    if depth is None or depth.ndim != 2 or depth.shape[0] < 1 or depth.shape[1] < 1 or n == 0:
        return X, np.zeros(n, bool)
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    p0, p1 = pts[:, 0], pts[:, 1]
    ok = np.isfinite(p0) & np.isfinite(p1)
    q0, q1 = np.where(ok, p0, F32(0)), np.where(ok, p1, F32(0))
    with np.errstate(all="ignore"):
        if interp == 0:
            i, j = np.rint(q0), np.rint(q1)                                   # round half to even, still float32
            inb = (i >= 0) & (i < h) & (j >= 0) & (j < w)
            ii, jj = np.where(inb, i, 0).astype(np.int64), np.where(inb, j, 0).astype(np.int64)
            d = depth[ii, jj]
            ok = ok & inb & np.isfinite(d) & (d > 0)
        else:
            i0, j0 = np.floor(q0), np.floor(q1)
            a, b = (q0 - i0).astype(F32), (q1 - j0).astype(F32)
            row1, col1 = a > 0, b > 0                                         # the taps with a zero weight are not used
            i1, j1 = i0.astype(np.float64) + 1, j0.astype(np.float64) + 1
            inb = (i0 >= 0) & (i0 < h) & (j0 >= 0) & (j0 < w) & (~row1 | (i1 < h)) & (~col1 | (j1 < w))
            ii, jj = np.where(inb, i0, 0).astype(np.int64), np.where(inb, j0, 0).astype(np.int64)
            ii1, jj1 = np.where(inb & row1, ii + 1, ii), np.where(inb & col1, jj + 1, jj)
            used = [np.ones(n, bool), col1, row1, row1 & col1]
            taps = [depth[ii, jj], depth[ii, jj1], depth[ii1, jj], depth[ii1, jj1]]
            taps = [np.where(u, t, F32(0)).astype(F32) for u, t in zip(used, taps)]    # an unused tap enters the sum as 0
            good = np.ones(n, bool)
            for u, t in zip(used, taps):
                good &= ~u | (np.isfinite(t) & (t > 0))
            ok = ok & inb & good
            wa, wb = (F32(1) - a).astype(F32), (F32(1) - b).astype(F32)
            w00, w01, w10, w11 = (wa * wb).astype(F32), (wa * b).astype(F32), (a * wb).astype(F32), (a * b).astype(F32)
            d = (w00 * taps[0]).astype(F32)
            d = (d + (w01 * taps[1]).astype(F32)).astype(F32)
            d = (d + (w10 * taps[2]).astype(F32)).astype(F32)
            d = (d + (w11 * taps[3]).astype(F32)).astype(F32)
            if max_jump is not None:
                mx, mn = taps[0].copy(), taps[0].copy()
                for u, t in zip(used[1:], taps[1:]):
                    mx = np.where(u, np.maximum(mx, t), mx)
                    mn = np.where(u, np.minimum(mn, t), mn)
                ok = ok & ~((mx - mn).astype(F32) > (F32(max_jump) * mn).astype(F32))
        if max_depth is not None:
            ok = ok & ~(d > F32(max_depth))
        x0, x1 = p0, p1
        if norm_left is not None:
            nl = np.asarray(norm_left, F32)
            x0 = ((p0 - nl[0]).astype(F32) * nl[2]).astype(F32)
            x1 = ((p1 - nl[1]).astype(F32) * nl[3]).astype(F32)
        out = np.stack([(x0 * d).astype(F32), (x1 * d).astype(F32), d.astype(F32)], 1)
    X[ok] = out[ok]
    return X, ok


def lift_reference(pts, segs, depths, norm=None, max_depth=None, interp=0, max_jump=None):
    """The whole call: pts [cap,2], segs [(lo, n)], depths a list of maps (None = null) -> (points [cap,3], valid [cap] uint8,
    lift_count [pairs] int64); rows of cap outside every segment are zero."""
    cap = pts.shape[0]
    X, valid, count = np.zeros((cap, 3), F32), np.zeros(cap, np.uint8), np.zeros(len(segs), np.int64)
    for p, (lo, n) in enumerate(segs):
        x, ok = lift32(pts[lo:lo + n], depths[p], None if norm is None else norm[p][:4], None if max_depth is None else max_depth[p],
                       interp, max_jump)
        X[lo:lo + n], valid[lo:lo + n], count[p] = x, ok, ok.sum()
    return X, valid, count


# ---- the sampler, K = 3 -----------------------------------------------------------------------------------------------------------
def pool3(n, H, progressive):
    h = np.arange(H, dtype=np.int64)
    if not progressive:
        return np.full(H, n, np.int64)
    return np.maximum(3, (np.int64(n) * (h + 1) + H - 1) // H)


def sample_idx3(pair_seed, n, H, progressive=False):
    """-> [H,3] int32: hypotheses_cases' sampler with three draws and the pool's minimum of 3; all -1 for n < 3."""
    if n < 3:
        return np.full((H, 3), -1, np.int32)
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF
    s_lo, s_hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    h = np.arange(H, dtype=np.uint64)
    k = hc.mix((hc.mix(hc.mix(s_lo) ^ s_hi) + h) & hc.M32)
    m = pool3(n, H, progressive).astype(np.uint64)
    out = np.empty((H, 3), np.int64)
    for t in range(3):
        u = hc.mix((k + ((hc.GOLDEN * np.uint64(t + 1)) & hc.M32)) & hc.M32)
        j = ((u * (m - np.uint64(t))) >> np.uint64(32)).astype(np.int64)
        prev = np.sort(out[:, :t], axis=1)
        for i in range(t):
            j = j + (prev[:, i] <= j)
        out[:, t] = j
    return out.astype(np.int32)


# ---- P3P in float64 ----------------------------------------------------------------------------------------------------------------
def residual3(R, t, X, xr):
    """The largest reprojection residual (infinity norm) of the three sample points under (R, t), float64."""
    Y = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        return float(np.abs(Y[:, :2] / Y[:, 2:3] - np.asarray(xr, np.float64)).max())


def p3p64(X, xr, self_check=1e-8):
    """X [3,3], xr [3,2] (float32 values) -> [(R [3,3], t [3])] float64 with x_r ~ R X + t, ordered by the camera distance of the first
    point: Grunert's quartic in v = s3 / s1 through numpy.roots, the distances, the rotation by an SVD alignment."""
    X, xr = np.asarray(X, np.float64), np.asarray(xr, np.float64)
    if not (np.isfinite(X).all() and np.isfinite(xr).all()):
        return []
    f = np.concatenate([xr, np.ones((3, 1))], 1)
    f /= np.linalg.norm(f, axis=1)[:, None]
    a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
    a2, b2, c2 = float(a2), float(b2), float(c2)                              # Python floats: a numpy scalar times a poly1d is an array
    ca, cb, cg = float(f[1] @ f[2]), float(f[0] @ f[2]), float(f[0] @ f[1])
    if not (a2 > 0 and b2 > 0 and c2 > 0):
        return []
    P = np.poly1d([1.0, -2 * cb, 1.0])                                        # 1 + v^2 - 2 v cos(beta) = b^2 / s1^2
    N = (a2 - c2) * P - b2 * np.poly1d([1.0, 0.0, -1.0])                      # u = s2 / s1 = N(v) / D(v)
    D = 2 * b2 * np.poly1d([-ca, cg])
    Q = b2 * (D * D + N * N - 2 * cg * N * D) - c2 * P * D * D
    sols = []
    with np.errstate(all="ignore"):
        for v in np.roots(Q.coeffs):
            if abs(v.imag) > 1e-7 * max(1.0, abs(v.real)) or not v.real > 0:
                continue
            v = v.real
            u = N(v) / D(v)
            s1 = np.sqrt(b2 / P(v))
            s = np.array([s1, u * s1, v * s1])
            if not (np.isfinite(s).all() and (s > 0).all()):
                continue
            Y = s[:, None] * f
            Xc, Yc = X - X.mean(0), Y - Y.mean(0)
            # three points span a plane: the alignment's third axis comes from the normals
            A = np.vstack([Xc, np.cross(Xc[1] - Xc[0], Xc[2] - Xc[0])[None, :]])
            B = np.vstack([Yc, np.cross(Yc[1] - Yc[0], Yc[2] - Yc[0])[None, :]])
            U, _, Vt = np.linalg.svd(B.T @ A)
            R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
            t = Y.mean(0) - R @ X.mean(0)
            if not (np.isfinite(R).all() and np.isfinite(t).all()):
                continue
            Yr = X @ R.T + t
            if not (Yr[:, 2] > 0).all() or residual3(R, t, X, xr) > self_check:
                continue
            if any(np.abs(R - R2).sum() + np.abs(t - t2).sum() < 1e-9 for _, R2, t2 in sols):
                continue
            sols.append((s1, R, t))
    sols.sort(key=lambda q: q[0])
    return [(R, t) for _, R, t in sols]


def pose_distance(R, t, R2, t2):
    return float(np.linalg.norm(np.asarray(R, np.float64) - R2) + np.linalg.norm(np.asarray(t, np.float64) - t2))


def rodrigues(r):
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_pair(seed, n, outliers=0.0, holes=0.0):
    """The generator of the solver cases: left normalised points uniform in [-0.6, 0.6]^2, depths uniform in [1, 8], rotation vector
    0.25 N(0, I), t = 0.5 N(0, I), redrawn while any right-camera depth is below 0.3; X and x_r rounded to float32.
    -> dict(X [n,3], xr [n,2] float32, R, t float64).  outliers: that share of right points is replaced; holes: of X rows NaN."""
    rng = np.random.default_rng(seed)
    while True:
        xl = rng.uniform(-0.6, 0.6, (n, 2))
        d = rng.uniform(1.0, 8.0, n)
        R, t = rodrigues(0.25 * rng.normal(size=3)), 0.5 * rng.normal(size=3)
        X = np.concatenate([xl * d[:, None], d[:, None]], 1)
        Y = X @ R.T + t
        if (Y[:, 2] >= 0.3).all():
            break
    xr = Y[:, :2] / Y[:, 2:3]
    bad = rng.random(n) < outliers
    xr[bad] = rng.uniform(-0.8, 0.8, (int(bad.sum()), 2))
    X = X.astype(F32)
    X[rng.random(n) < holes] = np.nan
    return {"X": X, "xr": xr.astype(F32), "R": R, "t": t}


def make_pairs(lengths, seed, **kw):
    """Pairs of make_pair, concatenated -> (X [cap,3], xr [cap,2], pair_off int64, [(R, t)])."""
    cases = [make_pair(seed + 17 * p, max(n, 1), **kw) for p, n in enumerate(lengths)]
    X = np.concatenate([c["X"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 3), F32)])
    xr = np.concatenate([c["xr"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 2), F32)])
    return X, xr, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), [(c["R"], c["t"]) for c in cases]


def right32(mr, norm_row=None):
    mr = np.ascontiguousarray(mr, F32)
    if norm_row is None:
        return mr
    with np.errstate(all="ignore"):
        return ec.normalise32(mr, np.asarray(norm_row, F32)[4:])


def hypotheses_reference(X, mr, segs, seeds, H, progressive=False, norm=None, solve=True):
    """Per pair a dict: idx [H,3] int32, finite [H] (the sample's three points and right points are finite), sols [H] lists of the
    float64 solver's (R, t) (empty without solve), X, xr (float32, normalised), lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        x, r = X[lo:lo + n], right32(mr[lo:lo + n], None if norm is None else norm[p])
        idx = sample_idx3(seeds[p], n, H, progressive)
        fin = np.zeros(H, bool)
        sols = [[] for _ in range(H)]
        if n >= 3:
            fin = np.isfinite(x[idx]).all((1, 2)) & np.isfinite(r[idx]).all((1, 2))
            if solve:
                sols = [p3p64(x[idx[h]], r[idx[h]]) if fin[h] else [] for h in range(H)]
        out.append({"idx": idx, "finite": fin, "sols": sols, "X": x, "xr": r, "lo": lo, "n": n})
    return out


def baseline(cases=((11, 400, 300, 2001), (12, 400, 300, 2002))):
    """b: the largest three-point reprojection residual / eps32 of the float64 solver's solutions ROUNDED TO FLOAT32, over seeded pairs
    (make_pair seed, matches, samples, pair_seed) - what float32 storage alone costs."""
    worst = 0.0
    for seed, n, H, ps in cases:
        c = make_pair(seed, n)
        idx = sample_idx3(ps, n, H)
        for h in range(H):
            for R, t in p3p64(c["X"][idx[h]], c["xr"][idx[h]]):
                worst = max(worst, residual3(R.astype(F32), t.astype(F32), c["X"][idx[h]], c["xr"][idx[h]]) / EPS32)
    return worst


# ---- the reprojection test ---------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, correctly rounded: the product is exact in float64, the sum is made exact with its error term
    and rounded to odd, and the last rounding to float32 is then the only one that counts."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                                       # p + c = s + e exactly
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0)
        toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))            # the float64 neighbour on the exact value's side
        trunc = np.where((e > 0) == (s > 0), s, toward)                       # the exact value truncated towards zero
        trunc = np.where(s == 0, s, trunc)
        odd = (np.ascontiguousarray(trunc).view(np.uint64) | np.uint64(1)).view(np.float64)
        return np.where(fix, odd, s).astype(F32)


def _project(X, xr, models, dtype):
    """(s, lim / thr^2, Y2) [M,n] in `dtype`: np.float32 = the kernel's order with its FMAs, np.float64 = the restatement."""
    Rt = np.asarray(models, F32).reshape(-1, 3, 4)
    m = lambda i, j: Rt[:, i, j][:, None]                                      # noqa: E731
    X0, X1, X2 = (X[:, k][None, :] for k in range(3))
    r0, r1 = xr[:, 0][None, :], xr[:, 1][None, :]
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            Y = [fma32(m(k, 0), X0, fma32(m(k, 1), X1, fma32(m(k, 2), X2, m(k, 3)))) for k in range(3)]
            d0, d1 = fma32(-r0, Y[2], Y[0]), fma32(-r1, Y[2], Y[1])
            s = fma32(d0, d0, (d1 * d1).astype(F32))
            return s, (Y[2] * Y[2]).astype(F32), Y
        X0, X1, X2, r0, r1 = (v.astype(np.float64) for v in (X0, X1, X2, r0, r1))
        Y = [m(k, 0).astype(np.float64) * X0 + m(k, 1) * X1 + m(k, 2) * X2 + m(k, 3) for k in range(3)]
        d0, d1 = Y[0] - r0 * Y[2], Y[1] - r1 * Y[2]
        return d0 * d0 + d1 * d1, Y[2] * Y[2], Y


def participates(X, xr, conf=None, min_conf=None):
    part = np.isfinite(X).all(1) & np.isfinite(xr).all(1)
    if min_conf is not None:
        with np.errstate(invalid="ignore"):
            part &= np.asarray(conf, F32) >= F32(min_conf)
    return part


def emulate32(X, xr, part, models, thr):
    """The kernel's arithmetic, operation for operation -> inlier [M,n] bool."""
    thr = F32(thr)
    M = np.asarray(models).reshape(-1, 3, 4).shape[0]
    if not thr >= 0:
        return np.zeros((M, X.shape[0]), bool)
    s, w, Y = _project(X, xr, models, np.float32)
    with np.errstate(all="ignore"):
        lim = ((thr * thr).astype(F32) * w).astype(F32)
        return part[None, :] & (Y[2] > 0) & (s <= lim)


def classify(X, xr, part, models, thr, delta=DELTA):
    """-> (inlier64 [M,n], decided [M,n])."""
    M = np.asarray(models).reshape(-1, 3, 4).shape[0]
    thr = F32(thr)
    if not thr >= 0:
        return np.zeros((M, X.shape[0]), bool), np.ones((M, X.shape[0]), bool)
    s, w, Y = _project(X, xr, models, np.float64)
    lim = np.float64(thr) ** 2 * w
    with np.errstate(all="ignore"):
        inl = part[None, :] & (Y[2] > 0) & (s <= lim)
        outside = (s < lim * (1 - delta)) | (s > lim * (1 + delta))
        size = np.maximum(np.maximum(np.abs(Y[0]), np.abs(Y[1])), np.abs(Y[2]))
        clear = np.abs(Y[2]) > delta * size                                   # the sign of Y2 survives float32 rounding
        certain = ~part[None, :] | np.isnan(s) | np.isnan(lim) | (size == 0)
    return inl, (outside & clear) | certain


def score_reference(X, mr, segs, models, thr, norm=None, conf=None, min_conf=None):
    """Per pair a dict: emu [M,n] (the float32 emulation), inl, decided, strict, loose [M], counts [M] (the emulation's), best,
    best_count, mask [n] (the winner's)."""
    out = []
    for p, (lo, n) in enumerate(segs):
        x, r = X[lo:lo + n], right32(mr[lo:lo + n], None if norm is None else norm[p])
        part = participates(x, r, None if conf is None else conf[lo:lo + n], min_conf)
        emu = emulate32(x, r, part, models[p], thr[p])
        inl, dec = classify(x, r, part, models[p], thr[p])
        counts = emu.sum(1).astype(np.int32)
        best = int(np.argmax(counts))                                         # the lowest index among the largest counts; 0 for none
        strict = (inl & dec).sum(1)
        out.append({"emu": emu, "inl": inl, "decided": dec, "strict": strict, "loose": strict + (~dec).sum(1), "counts": counts,
                    "best": best, "best_count": int(counts[best]), "mask": emu[best], "lo": lo, "n": n})
    return out


# ---- the pose ---------------------------------------------------------------------------------------------------------------------
def pose_from_model(Rt, swapped):
    """The winner [3,4] float32 -> (E, R, t) float64 as pose_abs_by_pair defines them."""
    Rt = np.asarray(Rt, F32).astype(np.float64)
    R, t = Rt[:, :3].copy(), Rt[:, 3].copy()
    if swapped:
        P = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]])
        R, t = P @ R @ P, P @ t
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    nrm = np.linalg.norm(E)
    return (E / nrm if nrm > 0 else np.zeros((3, 3))), R, t
