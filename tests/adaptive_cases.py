"""The stopping rule of the per-pair adaptive verification (include/pats_amd.h, "Per-pair adaptive verification") restated in plain
Python - Python floats are IEEE float64, so the restatement is the device's arithmetic bit for bit - and the planted inputs of
tests/test_adaptive_gpu.py: matches generated from known models at chosen inlier shares, so that the round in which a pair stops is
known before anything runs."""
import numpy as np

CONFIDENCE = 1 - 1e-5       # the reference's prob (utils/metrics.py:42-44)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def miss(q, k):
    """q^k by square-and-multiply from k's most significant bit; k = 0 gives 1.0."""
    m = 1.0
    for b in range(int(k).bit_length() - 1, -1, -1):
        m = m * m
        if (k >> b) & 1:
            m = m * q
    return m


def stops(c, participating, s, k, confidence):
    """The pair stops after a round with c = the largest count so far and k samples seen."""
    eta = 1.0 - confidence
    w = float(c) / float(participating) if participating > 0 else 0.0
    ws = w
    for _ in range(s - 1):
        ws = ws * w
    q = 1.0 - ws
    return miss(q, k) <= eta


def used_from_counts(counts, participating, H, B, g, s, confidence):
    """used of one pair from its fixed-budget counts [H]: T_r of the first round after which it stops, H if it never does."""
    counts = np.asarray(counts)
    best = -1
    for r in range(-(-H // B)):
        T = min(H, (r + 1) * B)
        best = max(best, int(counts[r * B:T].max()))              # the count alone decides: which index holds it does not matter
        if stops(best, int(participating), s, T // g, confidence):
            return T
    return H


def stop_round(w_num, w_den, s, g, B, confidence, H):
    """The round after which a pair stops whose best count is w_num of w_den participating matches from round 0 on; None: never."""
    for r in range(-(-H // B)):
        if stops(w_num, w_den, s, min(H, (r + 1) * B) // g, confidence):
            return r
    return None


# ---- planted inputs ---------------------------------------------------------------------------------------------------------------
def unit(M):
    return M / np.linalg.norm(M)


def random_model(rng, kind):
    """A unit 3x3 model: any matrix is a model of the epipolar test; a homography stays near the identity (a2 far from 0)."""
    if kind == "epi":
        return unit(rng.normal(size=(3, 3)))
    return unit(np.eye(3) + rng.normal(scale=0.15, size=(3, 3)))


def inliers_of(rng, kind, M, n):
    """n matches (x_l, x_r) [n,2] float64 that satisfy model M exactly: x_r on the epipolar line M x_l (the foot of a random point),
    or x_r = M x_l dehomogenised."""
    xl = rng.uniform(-0.6, 0.6, (n, 2))
    a = np.concatenate([xl, np.ones((n, 1))], 1) @ M.T
    if kind == "epi":
        u = rng.uniform(-0.6, 0.6, (n, 2))
        d = (a[:, 0] * u[:, 0] + a[:, 1] * u[:, 1] + a[:, 2]) / (a[:, 0] ** 2 + a[:, 1] ** 2)
        return xl, u - d[:, None] * a[:, :2]
    return xl, a[:, :2] / a[:, 2:3]


def plant_pair(seed, kind, n, H, planted, norm_row=None):
    """One pair: n matches, H float32 unit models.  planted = [(share, index)]: round(share n) matches satisfy a model of their own,
    which sits at `index` of the models; the other matches are uniform outliers, the other models random.  The matches are shuffled.
    With norm_row the points are stored so that the NORMALISED points satisfy the models.  -> (ml, mr [n,2] float32, models)."""
    rng = np.random.default_rng(seed)
    models = np.stack([random_model(rng, kind) for _ in range(H)])
    xl = rng.uniform(-0.6, 0.6, (n, 2))
    xr = rng.uniform(-0.8, 0.8, (n, 2))
    lo = 0
    for share, index in planted:
        m = int(round(share * n))
        xl[lo:lo + m], xr[lo:lo + m] = inliers_of(rng, kind, models[index], m)
        lo += m
    assert lo <= n
    order = rng.permutation(n)
    xl, xr = xl[order], xr[order]
    if norm_row is not None:                                              # x = (p - c) * s  ->  p = x / s + c
        c0l, c1l, s0l, s1l, c0r, c1r, s0r, s1r = [float(v) for v in norm_row]
        xl = xl / np.array([s0l, s1l]) + np.array([c0l, c1l])
        xr = xr / np.array([s0r, s1r]) + np.array([c0r, c1r])
    return xl.astype(np.float32), xr.astype(np.float32), models.astype(np.float32)


def plant_batch(seed, kind, H, pairs, norm=None):
    """pairs = [(n, planted)] -> (ml [cap,2], mr [cap,2], pair_off [pairs + 1] int64, models [pairs,H,3,3]), ragged."""
    got = [plant_pair(seed + 101 * p, kind, n, H, planted, None if norm is None else norm[p]) for p, (n, planted) in enumerate(pairs)]
    ml = np.concatenate([g[0] for g in got] + [np.zeros((0, 2), np.float32)])
    mr = np.concatenate([g[1] for g in got] + [np.zeros((0, 2), np.float32)])
    off = np.concatenate([[0], np.cumsum([n for n, _ in pairs])]).astype(np.int64)
    return ml, mr, off, np.stack([g[2] for g in got])
