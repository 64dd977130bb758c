"""The local optimisation of the absolute-pose branch (include/pats_amd.h, "Per-pair absolute local optimisation") restated in
float64 numpy from the header's definition alone: the sums of a model over a mask in the header's fixed order, the Gauss-Newton step
(Cholesky in index order with the pivot rule, the Rodrigues update), the refit (G steps on one mask, the orthonormalising step, the
cast), the walk over the rounds and the rule that picks the best one.  The support of a model is absolute_cases.emulate32 /
participates - the device's float32 test operation for operation - so masks and counts are the device's bits.  Shared by
tests/test_absolute_polish_cases_host.py (CPU) and tests/test_absolute_polish_gpu.py."""
import numpy as np

import absolute_cases as ac

F32 = np.float32
EPS32 = ac.EPS32
MIN_INLIERS = 4
PIVOT = 1e-12
THREADS, WAVE = 512, 64                 # the walk's width and the wave: the header's fixed order of the sums
SIGMA, THR, SAMPLES = 0.5 / 500, 1.5 / 500, 64
SEEDS = tuple(range(40, 52))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def noisy_pair(seed, n=300, sigma=SIGMA, outliers=0.3, holes=0.1):
    """absolute_cases.make_pair with N(0, sigma^2) added to the right points, rounded to float32."""
    c = ac.make_pair(seed, n, outliers=outliers, holes=holes)
    rng = np.random.default_rng([seed, 7919])
    c["xr"] = (c["xr"].astype(np.float64) + rng.normal(scale=sigma, size=c["xr"].shape)).astype(F32)
    return c


def ransac_models(c, thr=THR, H=SAMPLES, pair_seed=None):
    """The float64 P3P's solutions of H samples, rounded to float32 -> (models [M,3,4] float32, best: the verification's winner)."""
    X, xr = c["X"], c["xr"]
    idx = ac.sample_idx3(1000 + (0 if pair_seed is None else pair_seed), X.shape[0], H)
    models = [np.concatenate([R, t[:, None]], 1) for h in range(H) if np.isfinite(X[idx[h]]).all() for R, t in ac.p3p64(X[idx[h]], xr[idx[h]])]
    models = np.stack(models).astype(F32)
    counts = ac.emulate32(X, xr, ac.participates(X, xr), models, thr).sum(1)
    return models, int(np.argmax(counts))


def model_distance(m, c):
    m = np.asarray(m, np.float64)
    return ac.pose_distance(m[:, :3], m[:, 3], c["R"], c["t"])


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def support(X, xr, part, m, thr):
    """(c, mask) of one float32 model: the device's test."""
    mask = ac.emulate32(X, xr, part, np.asarray(m, F32).reshape(1, 3, 4), thr)[0]
    return int(mask.sum()), mask


def residual_jacobian(m, X, xr):
    """m [3,4] float64, X [n,3], xr [n,2] -> (e [n,2], J [n,2,6]) in the header's operation order."""
    m = np.asarray(m, np.float64)
    X, xr = np.asarray(X, np.float64), np.asarray(xr, np.float64)
    with np.errstate(all="ignore"):
        Y = [((m[k, 0] * X[:, 0] + m[k, 1] * X[:, 1]) + m[k, 2] * X[:, 2]) + m[k, 3] for k in range(3)]
        iz = 1.0 / Y[2]
        u, v = Y[0] * iz, Y[1] * iz
        e = np.stack([u - xr[:, 0], v - xr[:, 1]], 1)
        uv, zero = u * v, np.zeros_like(u)
        J0 = np.stack([-uv, 1.0 + u * u, -v, iz, zero, -(u * iz)], 1)
        J1 = np.stack([-(1.0 + v * v), uv, u, zero, iz, -(v * iz)], 1)
    return e, np.stack([J0, J1], 1)


def ordered_sum(terms, mask):
    """terms [n,k] float64, mask [n] -> [k]: thread j adds the masked rows j, j + THREADS, ... in order; the xor tree over each wave;
    the waves in order from 0.0."""
    n, k = terms.shape
    trips = max(1, -(-n // THREADS))
    grid = np.zeros((trips * THREADS, k))
    with np.errstate(all="ignore"):
        grid[:n][mask] = terms[mask]
        acc = np.zeros((THREADS, k))
        for t in range(trips):
            acc = acc + grid[t * THREADS:(t + 1) * THREADS]
        acc = acc.reshape(THREADS // WAVE, WAVE, k)
        lanes = np.arange(WAVE)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        total = np.zeros(k)
        for w in range(THREADS // WAVE):
            total = total + acc[w, 0]
    return total


def sums(m, X, xr, mask):
    """-> [28] float64: A's upper triangle row by row (21), b (6), S (1)."""
    mask = np.asarray(mask, bool)
    e, J = residual_jacobian(m, X, xr)
    with np.errstate(all="ignore"):
        cols = [J[:, 0, r] * J[:, 0, c] + J[:, 1, r] * J[:, 1, c] for r in range(6) for c in range(r, 6)]
        cols += [J[:, 0, r] * e[:, 0] + J[:, 1, r] * e[:, 1] for r in range(6)]
        cols.append(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    return ordered_sum(np.stack(cols, 1), mask)


def unpack(s):
    A = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = s[k]
            k += 1
    return A, s[21:27].copy(), float(s[27])


def solve(A, b):
    """d = -A^-1 b through A = L L^T in index order without pivoting, or None by the pivot rule."""
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            p = A[j, j]
            for q in range(j):
                p = p - L[j, q] * L[j, q]
            if not (np.isfinite(p) and p > PIVOT * A[j, j]):
                return None
            L[j, j] = np.sqrt(p)
            for i in range(j + 1, 6):
                x = A[i, j]
                for q in range(j):
                    x = x - L[i, q] * L[j, q]
                L[i, j] = x / L[j, j]
        y, d = np.zeros(6), np.zeros(6)
        for i in range(6):
            x = -b[i]
            for q in range(i):
                x = x - L[i, q] * y[q]
            y[i] = x / L[i, i]
        for i in range(5, -1, -1):
            x = y[i]
            for q in range(i + 1, 6):
                x = x - L[q, i] * d[q]
            d[i] = x / L[i, i]
    return d


def exp_so3(w):
    th2 = float(w @ w)
    if not th2 > 0:
        return np.eye(3)
    th = np.sqrt(th2)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + (np.sin(th) / th) * W + (2 * np.sin(0.5 * th) ** 2 / th2) * (np.outer(w, w) - th2 * np.eye(3))


def step(m, s):
    """One Gauss-Newton step of the float64 model m [3,4] on the sums s -> (m', d), or (None, None) for "no step"."""
    A, b, _ = unpack(s)
    d = solve(A, b)
    if d is None:
        return None, None
    with np.errstate(all="ignore"):
        E = exp_so3(d[:3])
        out = np.concatenate([E @ m[:, :3], (E @ m[:, 3] + d[3:])[:, None]], 1)
    return (out, d) if np.isfinite(out).all() else (None, None)


def orthonormal(m):
    R = m[:, :3]
    return np.concatenate([R + 0.5 * R @ (np.eye(3) - R.T @ R), m[:, 3:]], 1)


def refit(m32, X, xr, mask, c, G, first=None):
    """-> (the refit as float32 [3,4], the last step's d) - or (m32 itself, None) for "no refit".  first: sums(m32, mask), if the
    caller has them (the walk: the pass that gave S_r)."""
    m32 = np.asarray(m32, F32).reshape(3, 4)
    if c < MIN_INLIERS:
        return m32, None
    m, d = m32.astype(np.float64), None
    for g in range(G):
        s = first if (g == 0 and first is not None) else sums(m, X, xr, mask)
        m, d = step(m, s)
        if m is None:
            return m32, None
    with np.errstate(all="ignore"):
        out = orthonormal(m).astype(F32)
    return (out, d) if np.isfinite(out).all() else (m32, None)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def pick(counts, cost):
    """The best rule: the largest count, among those the smallest cost, among those the lowest round."""
    b = 0
    for r in range(1, len(counts)):
        if counts[r] > counts[b] or (counts[r] == counts[b] and cost[r] < cost[b]):
            b = r
    return b


def walk(X, xr, part, m0, thr, T, G):
    """The whole definition for one pair -> dict(models [T+1,3,4] float32, counts [T+1] int32, cost [T+1] float64, masks [T+1,n],
    best_round, model, best_count, mask)."""
    n = X.shape[0]
    models, counts, cost, masks = np.zeros((T + 1, 3, 4), F32), np.zeros(T + 1, np.int32), np.zeros(T + 1), np.zeros((T + 1, n), bool)
    m = np.asarray(m0, F32).reshape(3, 4)
    for r in range(T + 1):
        c, mask = support(X, xr, part, m, thr)
        s = sums(m.astype(np.float64), X, xr, mask) if c > 0 else np.zeros(28)
        models[r], counts[r], cost[r], masks[r] = m, c, s[27], mask
        if r == T:
            break
        nxt, _ = refit(m, X, xr, mask, c, G, first=s)
        if same_bits(nxt, m):                         # every later round repeats this one
            models[r + 1:], counts[r + 1:], cost[r + 1:], masks[r + 1:] = m, c, s[27], mask
            break
        m = nxt
    b = pick(counts, cost)
    return {"models": models, "counts": counts, "cost": cost, "masks": masks, "best_round": b, "model": models[b],
            "best_count": int(counts[b]), "mask": masks[b]}


def walk_reference(X, mr, segs, m0, thr, T, G, norm=None, conf=None, min_conf=None):
    """Per pair (segs = [(lo, n)], m0 [pairs,3,4] float32) the walk's dict, with lo and n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        x, r = X[lo:lo + n], ac.right32(mr[lo:lo + n], None if norm is None else norm[p])
        part = ac.participates(x, r, None if conf is None else conf[lo:lo + n], min_conf)
        w = walk(x, r, part, m0[p], thr[p], T, G)
        w.update(lo=lo, n=n)
        out.append(w)
    return out
