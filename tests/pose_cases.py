"""The per-pair relative pose of include/pats_amd.h ("Per-pair relative pose") restated in numpy float64, a seeded generator of
two-view scenes that keeps the ground-truth (R, t), and the classifier of the cheirality test's undecided cells.  Shared by
tests/test_pose_cases_host.py (CPU) and tests/test_pose_gpu.py; written from the header's definition alone.

Definition (per pair; x = the float32 point after the optional normalisation):
    e_refit     a unit eigenvector of the 9x9 moment matrix for its smallest eigenvalue
    E           U diag(s, s, 0) V^T of e_refit = U diag(s1, s2, s3) V^T, Frobenius norm 1, the largest component positive
    candidates  det U, det V > 0, W = [[0,-1,0],[1,0,0],[0,0,1]]: (R1, u), (R2, u), (R1, -u), (R2, -u), R1 = U W V^T, R2 = U W^T V^T
    in front    a = R x_l, b = x_r, c = a x b:  c.c > 0 and c.(b x t) > 0 and c.(a x t) > 0, R and t rounded to float32
A (match, candidate) cell is UNDECIDED when |c.(b x t)| <= DELTA * (the sum of the |terms| of that dot product), or the same holds
for c.(a x t): a float32 evaluation may differ from the float64 verdict on undecided cells only."""
import numpy as np

import epipolar_cases as ec

DELTA = ec.DELTA        # 1e-3, the verification's band
EPS64 = float(np.finfo(np.float64).eps)
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
P_SWAP = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
MIN_INLIERS = 8

# the committed seeds: (seed, matches)
HOST_CASES = [(201, 20), (202, 65), (203, 500), (204, 513), (205, 1025), (206, 1200), (207, 3000), (208, 4097)]
REFIT_CASES = [c for c in HOST_CASES if c[1] in (20, 65, 500, 1200, 3000, 4097)]


def make_scene(seed, n, outliers=0.4, noise=5e-4):
    """One pair with make_case's distributions: n matches in normalised coordinates (float32), the ground truth kept.
    -> dict(ml, mr, R, t, good [n] bool: the matches that follow (R, t))."""
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
    return {"ml": xl.astype(np.float32), "mr": xr.astype(np.float32), "R": R, "t": t, "good": ~bad}


def cross_matrix(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def true_model(scene):
    """The ground truth's unit essential matrix as a float32 model."""
    E = cross_matrix(scene["t"]) @ scene["R"]
    return (E / np.linalg.norm(E)).astype(np.float32)


def residual(M, e):
    """r(e) = |M e - (e^T M e) e|_2 / (eps64 |M|_F) in float64."""
    M, e = np.asarray(M, np.float64), np.asarray(e, np.float64).reshape(9)
    return float(np.linalg.norm(M @ e - (e @ M @ e) * e) / (EPS64 * np.linalg.norm(M)))


def refit64(M):
    """-> (e [9] unit, eigenvalues ascending) of numpy's eigh."""
    w, v = np.linalg.eigh(np.asarray(M, np.float64))
    return v[:, 0].copy(), w


def sign_rule(E):
    """The component of largest magnitude positive, the lowest index among equals."""
    f = E.reshape(-1)
    return -E if f[int(np.argmax(np.abs(f)))] < 0 else E


def svd_pos(e):
    """e [9] -> (U, s, V) of its 3x3 with det U = det V = +1."""
    U, s, Vt = np.linalg.svd(np.asarray(e, np.float64).reshape(3, 3))
    V = Vt.T
    if np.linalg.det(U) < 0:
        U = U.copy()
        U[:, 2] = -U[:, 2]
    if np.linalg.det(V) < 0:
        V = V.copy()
        V[:, 2] = -V[:, 2]
    return U, s, V


def project64(e):
    """The essential matrix nearest to e, Frobenius norm 1, the sign rule applied."""
    U, _, V = svd_pos(e)
    return sign_rule(U @ np.diag([np.sqrt(0.5), np.sqrt(0.5), 0.0]) @ V.T)


def candidates64(e):
    """[(R, t)] x 4 in the definition's order (which member is R1 depends on the SVD: compare as a set, see match_candidates)."""
    U, _, V = svd_pos(e)
    R1, R2, u = U @ W @ V.T, U @ W.T @ V.T, U[:, 2]
    return [(R1, u), (R2, u), (R1, -u), (R2, -u)]


def match_candidates(cands, R, t):
    """The index of the candidate nearest to (R, t)."""
    return int(np.argmin([np.abs(Rc - R).max() + np.abs(tc - t).max() for Rc, tc in cands]))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def fronts(xl, xr, used, cands, dtype=np.float64, delta=DELTA):
    """-> (front [4,n] bool, undecided [4,n] bool) of one pair: the sign tests with R, t rounded to float32 and every operation in
    `dtype` (np.float64: the restatement; np.float32: an emulation).  undecided is judged on the dtype's own values."""
    n = xl.shape[0]
    front, und = np.zeros((len(cands), n), bool), np.zeros((len(cands), n), bool)
    one = np.ones(n, dtype)
    l = [xl[:, 0].astype(dtype), xl[:, 1].astype(dtype), one]
    b = [xr[:, 0].astype(dtype), xr[:, 1].astype(dtype), one]
    with np.errstate(all="ignore"):
        for k, (R, t) in enumerate(cands):
            R, t = np.asarray(R, np.float32).astype(dtype), np.asarray(t, np.float32).astype(dtype)
            a = [R[i, 0] * l[0] + R[i, 1] * l[1] + R[i, 2] * l[2] for i in range(3)]
            c = _cross(a, b)
            bt, at = _cross(b, t), _cross(a, t)
            cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
            dl = c[0] * bt[0] + c[1] * bt[1] + c[2] * bt[2]
            dr = c[0] * at[0] + c[1] * at[1] + c[2] * at[2]
            sl = np.abs(c[0] * bt[0]) + np.abs(c[1] * bt[1]) + np.abs(c[2] * bt[2])
            sr = np.abs(c[0] * at[0]) + np.abs(c[1] * at[1]) + np.abs(c[2] * at[2])
            front[k] = used & (cc > 0) & (dl > 0) & (dr > 0)
            und[k] = used & ((np.abs(dl) <= delta * sl) | (np.abs(dr) <= delta * sr))
    return front, und


def choose(counts):
    """The lowest index of the largest count."""
    return int(np.argmax(np.asarray(counts)))


def angle_R(R, R_gt):
    cos = np.clip((np.trace(R.T @ R_gt) - 1) / 2, -1.0, 1.0)
    return float(np.rad2deg(np.abs(np.arccos(cos))))


def angle_t(t, t_gt):
    """The reference's translation error: min(e, 180 - e) (utils/metrics.py)."""
    e = float(np.rad2deg(np.arccos(np.clip(np.dot(t, t_gt) / (np.linalg.norm(t) * np.linalg.norm(t_gt)), -1.0, 1.0))))
    return min(e, 180.0 - e)


def reference(xl, xr, used, M=None, model=None, best_count=None):
    """The whole definition for one pair from the float32 points -> dict(ok, e, E, cands, front [4,n], undecided [4,n], counts [4],
    choice, R, t).  M: the moments (else `model`, promoted).  best_count defaults to used.sum()."""
    best_count = int(used.sum()) if best_count is None else int(best_count)
    n = xl.shape[0]
    none = {"ok": False, "e": np.zeros(9), "E": np.zeros((3, 3)), "R": np.eye(3), "t": np.zeros(3), "counts": np.zeros(4, np.int64),
            "choice": 0, "front": np.zeros((4, n), bool), "undecided": np.zeros((4, n), bool), "cands": None}
    if best_count < MIN_INLIERS:
        return none
    if M is not None:
        if not np.isfinite(M).all():
            return none
        e = refit64(M)[0]
    else:
        e = np.asarray(model, np.float32).astype(np.float64).reshape(9)
    if not np.isfinite(e).all():
        return none
    if np.linalg.svd(e.reshape(3, 3), compute_uv=False)[1] == 0:
        return dict(none, e=e)
    cands = candidates64(e)
    front, und = fronts(xl, xr, used, cands)
    counts = front.sum(1)
    ch = choose(counts)
    return {"ok": True, "e": e, "E": project64(e), "cands": cands, "front": front, "undecided": und, "counts": counts, "choice": ch,
            "R": cands[ch][0], "t": cands[ch][1]}
