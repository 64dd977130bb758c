"""The per-pair pose from a homography and the E-or-H decision of include/pats_amd.h ("Per-pair pose from a homography and the E-or-H
decision") restated in numpy float64 in the header's operation order, a second, independent route (numpy's SVD of the moments and of
G', the cosine / sine form of the four solutions) that serves as the yardstick, the classifiers of the float32 decisions' undecided
cells, a seeded generator of planar scenes that keeps the ground truth, and the table of the C entry points' refusals.  Shared by
tests/test_pose_h_cases_host.py (CPU) and tests/test_pose_h_gpu.py; written from the header's definition alone.

    spectrum    G^T G = V diag(lambda) V^T (numpy's eigh), descending, v3 = v1 x v2;  G' = G / sqrt(lambda2),  l1, l3 the ratios
    sign        q = x_r . (G' x_l) over the used matches with G' rounded to float32: G' = -G' if more are negative than positive
    candidates  u = (sqrt(1 - l3) v1 +- sqrt(l1 - 1) v3) / sqrt(l1 - l3),  U = [v2, u, v2 x u],  W = [G' v2, G' u, G' v2 x G' u],
                R = W U^T, n = v2 x u, t = (G' - R) n;  then (R_0, -t_0, -n_0), (R_1, -t_1, -n_1)
    choice      the lowest k with the largest (vis[k], sup[k])
The signs of v1 and v2 are the eigen-solver's: they permute the four candidates as k -> k ^ m, m in 0 .. 3 (the SET is unique), so
two implementations are compared after matching one candidate - match_xor.
A float32 verdict is UNDECIDED when the float64 value lies within DELTA times the sum of the |terms| of its dot product (sign, vis) or
within the verification's relative band around thr^2 den (sup)."""
import numpy as np

import epipolar_cases as ec
import homography_cases as hmc

DELTA = ec.DELTA        # 1e-3, the verification's band
EPS64 = float(np.finfo(np.float64).eps)
P_SWAP = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
MIN_INLIERS = 4
EPI_MIN_INLIERS = 8
GAP = 1e-3              # comparison scenes have min(l1 - 1, 1 - l3) >= GAP: below it sqrt(l1 - 1) amplifies rounding without bound
MAX_DROPPED = 0.05      # at most this share of the generated scenes may fail GAP
MARGIN = 16.0           # the device's Jacobi against LAPACK: a different rounding path through the same conditioning
BAND_CAP = 0.01         # the undecided band may hold at most this share of a scene's compared matches

# the committed seeds: (seed, plane matches, off-plane matches, outliers)
HOST_CASES = [(301, 40, 10, 6), (302, 65, 20, 10), (303, 200, 57, 30), (304, 300, 100, 113), (305, 500, 100, 50), (306, 700, 200, 125)]
ROTATION_CASES = [(321, 60, 0, 10), (322, 257, 0, 40)]
SMALL_BASELINE_CASES = [(331, 120, 30, 20), (332, 300, 60, 40)]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def make_scene(seed, n_plane, n_off=0, n_out=0, noise=3e-4, family="plane", exact=False):
    """One pair looking at a plane n . X = d: rotation angles uniform within 0.3 rad, t uniform in [-1,1]^3, n within 0.4 of the axis,
    d in [3,6]; left points uniform in +-0.6.  n_plane matches on the plane, n_off off it (depths 2.5 .. 9, at least 0.5 from the plane
    along the ray), n_out uniform outliers, N(0, noise) on the right points, float32 unless exact.  family "rotation": t = 0;
    "small": |t| / d = 0.01.  -> dict(ml, mr, R, t, n, d, kind [N]: 0 plane, 1 off the plane, 2 outlier, H: R + t n^T / d)."""
    rng = np.random.default_rng(seed)
    R = hmc._rot(*rng.uniform(-0.3, 0.3, 3))
    t = rng.uniform(-1.0, 1.0, 3)
    nv = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
    nv /= np.linalg.norm(nv)
    d = rng.uniform(3.0, 6.0)
    if family == "rotation":
        t = np.zeros(3)
    elif family == "small":
        t *= 0.01 * d / np.linalg.norm(t)
    N = n_plane + n_off + n_out
    xl = rng.uniform(-0.6, 0.6, (N, 2))
    ray = np.concatenate([xl, np.ones((N, 1))], 1)
    z_plane = d / (ray @ nv)                                                  # the depth at which the ray meets the plane
    z = z_plane.copy()
    off = np.arange(N) >= n_plane
    shift = rng.uniform(0.5, 3.0, N) * np.where(rng.random(N) < 0.5, -1.0, 1.0)
    z[off] = np.clip(z_plane[off] + shift[off], 2.5, 9.0)
    z[off] = np.where(np.abs(z[off] - z_plane[off]) < 0.5, z_plane[off] + 0.5, z[off])
    Y = (ray * z[:, None]) @ R.T + t[None, :]
    xr = Y[:, :2] / Y[:, 2:3] + (0.0 if exact else rng.normal(scale=noise, size=(N, 2)))
    kind = np.zeros(N, np.int64)
    kind[n_plane:n_plane + n_off] = 1
    kind[n_plane + n_off:] = 2
    xr[kind == 2] = rng.uniform(-0.8, 0.8, (n_out, 2))
    dt = np.float64 if exact else np.float32
    return {"ml": xl.astype(dt), "mr": xr.astype(dt), "R": R, "t": t, "n": nv, "d": d, "kind": kind, "H": R + np.outer(t, nv) / d}


def gap_of(H):
    """min(l1 - 1, 1 - l3) of a homography."""
    lam = np.linalg.eigvalsh(H.T @ H)[::-1]
    return float(min(lam[0] / lam[1] - 1.0, 1.0 - lam[2] / lam[1]))


def comparison_scenes():
    """-> (the committed comparison scenes - HOST_CASES and SMALL_BASELINE_CASES - that pass GAP, number generated)."""
    made = [make_scene(*c) for c in HOST_CASES] + [make_scene(*c, family="small") for c in SMALL_BASELINE_CASES]
    return [s for s in made if gap_of(s["H"]) >= GAP], len(made)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def spectrum(G):
    """-> (lambda [3] descending, V with columns v1, v2, v1 x v2) of G^T G by numpy's eigh."""
    w, v = np.linalg.eigh(G.T @ G)
    V = v[:, ::-1].copy()
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    return w[::-1].copy(), V


def _terms(rows, xl):
    """rows [..., 3] against (l0, l1, 1): the dot products [..., n] and the sums of their |terms|."""
    l0, l1 = xl[:, 0].astype(np.float64), xl[:, 1].astype(np.float64)
    r = np.asarray(rows, np.float32).astype(np.float64)
    val = r[..., 0:1] * l0 + r[..., 1:2] * l1 + r[..., 2:3]
    mag = np.abs(r[..., 0:1] * l0) + np.abs(r[..., 1:2] * l1) + np.abs(r[..., 2:3]) + 0.0 * l0
    return val, mag


def sign_vote(Gp, xl, xr, used, delta=DELTA):
    """-> (pos, neg, undecided) counts of q = x_r . (G' x_l) over the used matches, G' rounded to float32."""
    with np.errstate(all="ignore"):
        a, am = _terms(Gp, xl)                                                # [3,n]
        r0, r1 = xr[:, 0].astype(np.float64), xr[:, 1].astype(np.float64)
        q = r0 * a[0] + r1 * a[1] + a[2]
        mag = np.abs(r0) * am[0] + np.abs(r1) * am[1] + am[2]
        und = used & (np.abs(q) <= delta * mag)
        return int((used & (q > 0) & ~und).sum()), int((used & (q < 0) & ~und).sum()), int(und.sum())


def candidates_eig(Gp, V, l1, l3):
    """The four (R, t, n) in the definition's order; t not normalised."""
    v1, v2, v3 = V[:, 0], V[:, 1], V[:, 2]
    out = []
    for s in (1.0, -1.0):
        u = (np.sqrt(1.0 - l3) * v1 + s * np.sqrt(l1 - 1.0) * v3) / np.sqrt(l1 - l3)
        U = np.stack([v2, u, np.cross(v2, u)], 1)
        W = np.stack([Gp @ v2, Gp @ u, np.cross(Gp @ v2, Gp @ u)], 1)
        R = W @ U.T
        nn = np.cross(v2, u)
        out.append((R, (Gp - R) @ nn, nn))
    return out + [(R, -t, -nn) for R, t, nn in out]


def candidates_svd(Gp):
    """The yardstick: the four solutions of G' = R + t n^T in the cosine / sine form, from numpy's SVD G' = U diag(d1, d2, d3) V^T
    (Faugeras and Lustman's case d' = +d2; d2 = 1 up to rounding).  Order: its own - compare with match_xor / nearest."""
    U, dd, Vt = np.linalg.svd(Gp)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    assert s > 0, "det G' < 0: the two cameras on opposite sides of the plane - not a scene of this generator"
    d1, d2, d3 = dd
    x1 = np.sqrt(max(d1 * d1 - d2 * d2, 0.0) / (d1 * d1 - d3 * d3))
    x3 = np.sqrt(max(d2 * d2 - d3 * d3, 0.0) / (d1 * d1 - d3 * d3))
    st = np.sqrt(max(d1 * d1 - d2 * d2, 0.0) * max(d2 * d2 - d3 * d3, 0.0)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    out = []
    for e1, e3 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        sth = st * e1 * e3
        Rp = np.array([[ct, 0.0, -sth], [0.0, 1.0, 0.0], [sth, 0.0, ct]])
        R = s * U @ Rp @ Vt
        t = U @ (np.array([e1 * x1, 0.0, -e3 * x3]) * (d1 - d3))
        nn = Vt.T @ np.array([e1 * x1, 0.0, e3 * x3])
        out.append((R, t / d2, nn))
    return out


def nearest(cands, R, t, n):
    """(index, distance) of the candidate nearest to (R, t, n) in the largest absolute difference."""
    dist = [max(np.abs(Rc - R).max(), np.abs(tc - t).max(), np.abs(nc - n).max()) for Rc, tc, nc in cands]
    return int(np.argmin(dist)), float(np.min(dist))


def match_xor(cands, R, t, n):
    """m such that candidate 0 of another implementation, (R, t, n), is cands[m]: its candidate k is then cands[k ^ m]."""
    return nearest(cands, R, t, n)[0]


def essential(R, t):
    """[t / |t|]x R scaled to Frobenius norm 1, the hypotheses' sign rule applied."""
    q = t / np.linalg.norm(t)
    E = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]]) @ R
    return hmc.sign_rule(E / np.linalg.norm(E))


def refit_eigh(M):
    return np.linalg.eigh(np.asarray(M, np.float64))[1][:, 0].copy()


def refit_svd(M):
    """The yardstick's refit: the last right singular vector of the moments."""
    return np.linalg.svd(np.asarray(M, np.float64))[2][8].copy()


def no_pose(n_matches=0):
    return {"status": 0, "E": np.zeros((3, 3)), "R": np.eye(3), "t": np.zeros(3), "n": np.zeros(3), "baseline": 0.0,
            "vis": np.zeros(4, np.int64), "sup": np.zeros(4, np.int64), "choice": 0, "front_count": 0, "cands": None,
            "front": np.zeros(n_matches, bool), "cand_R": np.stack([np.eye(3)] * 2), "cand_t": np.zeros((2, 3)), "cand_n": np.zeros((2, 3))}


def restate(xl, xr, used, G=None, M=None, model=None, best_count=None, thr=None, min_baseline=0.0, delta=DELTA, refit=refit_eigh):
    """The whole definition for one pair from its points (float32, or float64 for an exact scene) -> dict: status, E, R, t, n,
    baseline, cands (four (R, t, n), t not normalised), vis / sup (float64 verdicts), their sure counts vis_lo / sup_lo and sure-plus-
    band counts vis_hi / sup_hi, side [4,n] / side_und [4,n] (the verdicts of the used matches and their band), choice, choice_sure,
    sign_sure, front_count, front [n], cand_R, cand_t, cand_n.  G: h_refit given directly; M: the moments; model: a float32 model."""
    n = xl.shape[0]
    fin = ec.participates(xl, xr)
    used = np.asarray(used, bool) & fin
    best_count = int(used.sum()) if best_count is None else int(best_count)
    if best_count < MIN_INLIERS:
        return no_pose(n)
    if G is None:
        if M is not None:
            if not np.isfinite(M).all():
                return no_pose(n)
            G = refit(M)
        else:
            G = np.asarray(model, np.float32).astype(np.float64)
    G = np.asarray(G, np.float64).reshape(3, 3)
    if not np.isfinite(G).all():
        return no_pose(n)
    lam, V = spectrum(G)
    if not lam[1] > 0:
        return no_pose(n)
    Gp = G / np.sqrt(lam[1])
    l1, l3 = max(lam[0] / lam[1], 1.0), min(max(lam[2] / lam[1], 0.0), 1.0)
    pos, neg, und = sign_vote(Gp, xl, xr, used, delta)
    if neg > pos:
        Gp = -Gp
    out = {"sign_sure": abs(pos - neg) > und, "Gp": Gp, "l1": l1, "l3": l3, "used": int(used.sum())}
    base = np.sqrt(l1) - np.sqrt(l3)
    if l1 - l3 <= 0 or base <= min_baseline:
        if l3 <= 0:
            return no_pose(n)
        R = Gp @ V @ np.diag([1 / np.sqrt(l1), 1.0, 1 / np.sqrt(l3)]) @ V.T
        if not np.isfinite(R).all():
            return no_pose(n)
        out.update(no_pose(n))
        out.update(status=2, R=R, baseline=base, vis=np.full(4, out["used"], np.int64), front_count=out["used"], front=used.copy(),
                   cand_R=np.stack([R, R]), choice_sure=True)
        out["vis_lo"] = out["vis_hi"] = out["vis"]
        out["sup_lo"] = out["sup_hi"] = out["sup"]
        return out
    cands = candidates_eig(Gp, V, l1, l3)
    if not all(np.isfinite(x).all() for c in cands for x in c) or not all(np.linalg.norm(c[1]) > 0 for c in cands):
        return no_pose(n)
    with np.errstate(all="ignore"):
        dval, dmag = _terms(np.stack([cands[0][2], cands[1][2]]), xl)            # [2,n]
        side = np.concatenate([used[None, :] & (dval > 0), used[None, :] & (dval < 0)])
        s_und = np.tile(used[None, :] & (np.abs(dval) <= delta * dmag), (2, 1))
    vis = side.sum(1)
    vis_lo, vis_hi = (side & ~s_und).sum(1), (side | s_und).sum(1)
    sup = sup_lo = sup_hi = np.zeros(4, np.int64)
    if thr is not None:
        E2 = np.stack([essential(cands[k][0], cands[k][1]) for k in range(2)])
        inl, dec = ec.classify(xl, xr, fin, E2, thr, delta)
        sup = np.tile(inl.sum(1), 2)
        sup_lo, sup_hi = np.tile((inl & dec).sum(1), 2), np.tile((inl & dec).sum(1) + (~dec).sum(1), 2)
    ch = max(range(4), key=lambda k: (vis[k], sup[k], -k))
    sure = all(k == ch or vis_lo[ch] > vis_hi[k] or
               (vis_lo[ch] == vis_hi[ch] == vis_lo[k] == vis_hi[k] and sup_lo[ch] > sup_hi[k]) for k in range(4))
    R, t, nn = cands[ch]
    out.update(status=1, cands=cands, baseline=base, vis=vis, vis_lo=vis_lo, vis_hi=vis_hi, sup=sup, sup_lo=sup_lo, sup_hi=sup_hi,
               side=side, side_und=s_und, choice=ch, choice_sure=sure, front_count=int(vis[ch]), front=side[ch], R=R,
               t=t / np.linalg.norm(t), n=nn, E=essential(R, t), cand_R=np.stack([cands[0][0], cands[1][0]]),
               cand_t=np.stack([cands[0][1], cands[1][1]]), cand_n=np.stack([cands[0][2], cands[1][2]]))
    return out


def swap(res):
    """The outputs of swapped = 1 from those of swapped = 0: the exact permutation."""
    P = P_SWAP
    out = dict(res)
    out.update(R=P @ res["R"] @ P, t=P @ res["t"], n=P @ res["n"], E=hmc.sign_rule(P @ res["E"] @ P),
               cand_R=np.stack([P @ r @ P for r in res["cand_R"]]), cand_t=res["cand_t"] @ P, cand_n=res["cand_n"] @ P)
    return out


def select(best_count_e, best_count_h, status_h, ratio):
    """The E-or-H rule for one pair -> branch."""
    epi_ok, planar_ok = int(best_count_e) >= EPI_MIN_INLIERS, int(status_h) != 0
    with np.errstate(invalid="ignore"):
        enough = bool(np.float64(int(best_count_h)) >= np.float64(np.float32(ratio)) * np.float64(int(best_count_e)))      # False for a NaN
    if planar_ok and (not epi_ok or enough):
        return 3 if int(status_h) == 2 else 2
    return 1 if epi_ok else 0


def angle_R(R, R_gt):
    return float(np.rad2deg(np.arccos(np.clip((np.trace(R.T @ R_gt) - 1) / 2, -1.0, 1.0))))


def angle_t(t, t_gt):
    e = float(np.rad2deg(np.arccos(np.clip(np.dot(t, t_gt) / (np.linalg.norm(t) * np.linalg.norm(t_gt)), -1.0, 1.0))))
    return min(e, 180.0 - e)


def plane_moments(scene, norm_row=None):
    """(xl, xr float32 points, used = the plane matches, M = their float64 homography moments)."""
    xl, xr = ec.points32(scene["ml"], scene["mr"], norm_row)
    used = scene["kind"] == 0
    return xl, xr, used, hmc.moments64(xl, xr, used)


def float64_constant(scenes, thr=2e-3):
    """The measured float64 constant: the largest difference, over the scenes and over R, t, n of the four candidates, E, the chosen
    pose and the baseline, between the restatement (eigh of the moments, eigh of G^T G) and the independent route (SVD of the moments,
    SVD of G', the cosine / sine form)."""
    worst = 0.0
    for s in scenes:
        xl, xr, used, M = plane_moments(s)
        a = restate(xl, xr, used, M=M, thr=thr)
        b = restate(xl, xr, used, M=M, thr=thr, refit=refit_svd)
        assert a["status"] == 1 and b["status"] == 1
        other = candidates_svd(b["Gp"])
        for R, t, nn in a["cands"]:
            worst = max(worst, nearest(other, R, t, nn)[1])
        j = nearest(other, *a["cands"][a["choice"]])[0]
        Rb, tb, nb = other[j]
        worst = max(worst, np.abs(essential(Rb, tb) - a["E"]).max(), np.abs(tb / np.linalg.norm(tb) - a["t"]).max(),
                    abs(np.linalg.svd(b["Gp"], compute_uv=False)[0] - np.linalg.svd(b["Gp"], compute_uv=False)[2] - a["baseline"]))
    return float(worst)


# ---- the C entry points' refusals -----------------------------------------------------------------------------------------------------
# per entry point: the argument order of the prototype (before workspace, workspace_bytes, stream), the pointers that must not be
# null, every pointer's alignment, the scalars of a valid call
ENTRY = {
    "pose": {
        "fn": "pats_homography_pose_by_pair_f64", "tag": b"homography_pose_by_pair",
        "order": ("matches_l", "matches_r", "inlier", "pair_off", "stride", "counts_in", "pairs", "cap", "best_count", "moments", "models",
                  "H", "best", "norm", "thr", "swapped", "min_baseline", "E", "R", "t", "n", "baseline", "vis", "sup", "choice", "status",
                  "front_count", "cand_R", "cand_t", "cand_n", "front"),
        "required": ("matches_l", "matches_r", "inlier", "best_count", "E", "R", "t", "n", "baseline", "vis", "sup", "choice", "status",
                     "front_count"),
        "align": {"matches_l": 8, "matches_r": 8, "inlier": 1, "pair_off": 8, "counts_in": 8, "best_count": 8, "moments": 8, "models": 4,
                  "best": 4, "norm": 4, "thr": 4, "E": 8, "R": 8, "t": 8, "n": 8, "baseline": 8, "vis": 4, "sup": 4, "choice": 4, "status": 4,
                  "front_count": 8, "cand_R": 8, "cand_t": 8, "cand_n": 8, "front": 1},
        "scalars": {"stride": 0, "pairs": 2, "cap": 100, "H": 8, "swapped": 0, "min_baseline": 0.0}},
    "select": {
        "fn": "pats_pose_select_by_pair", "tag": b"pose_select_by_pair",
        "order": ("pair_off", "stride", "counts_in", "pairs", "cap", "R_e", "t_e", "E_e", "front_count_e", "front_e", "best_count_e",
                  "inlier_e", "R_h", "t_h", "E_h", "front_count_h", "front_h", "status_h", "best_count_h", "inlier_h", "ratio", "R", "t", "E",
                  "front_count", "branch", "inlier_sel", "front_sel"),
        "required": ("R_e", "t_e", "E_e", "front_count_e", "best_count_e", "inlier_e", "R_h", "t_h", "E_h", "front_count_h", "status_h",
                     "best_count_h", "inlier_h", "ratio", "R", "t", "E", "front_count", "branch", "inlier_sel"),
        "align": {"pair_off": 8, "counts_in": 8, "R_e": 8, "t_e": 8, "E_e": 8, "front_count_e": 8, "front_e": 1, "best_count_e": 8,
                  "inlier_e": 1, "R_h": 8, "t_h": 8, "E_h": 8, "front_count_h": 8, "front_h": 1, "status_h": 4, "best_count_h": 8,
                  "inlier_h": 1, "ratio": 4, "R": 8, "t": 8, "E": 8, "front_count": 8, "branch": 4, "inlier_sel": 1, "front_sel": 1},
        "scalars": {"stride": 0, "pairs": 2, "cap": 100}},
}


def c_call(lib, which, base, ws_bytes=1 << 20, **kw):
    """One raw call of an entry point with `base` behind every pointer (the ragged form), `kw` overriding arguments by name."""
    import ctypes
    e = ENTRY[which]
    a = {n: base for n in e["align"]}
    a["counts_in"] = 0
    a.update(e["scalars"])
    a.update(kw)
    args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in e["align"] else a[n] for n in e["order"]]
    return getattr(lib, e["fn"])(*args, ctypes.c_void_p(base), ws_bytes, None)


def refusals(lib, which, base):
    """Every refusal of the header's list -> [(keyword arguments of c_call(), the words the message must hold)]."""
    e = ENTRY[which]
    strided = {"pair_off": 0, "counts_in": base}
    out = [({name: 0}, (b"null", name.encode())) for name in e["required"]]
    for name, al in sorted(e["align"].items()):
        if al == 1:
            continue
        form = dict(strided, stride=10) if name == "counts_in" else {}
        out += [(dict(form, **{name: base + off}), (b"%d-byte aligned" % al, name.encode())) for off in ((1, 2, 3) if al == 4 else (1, 2, 4))]
    out += [(dict(strided, pair_off=base, stride=10), (b"pair_off", b"counts_in")), ({"pair_off": 0}, (b"pair_off", b"counts_in"))]
    out += [(kw, (b"pairs",)) for kw in ({"pairs": 0}, {"pairs": -3})]
    out += [(kw, (b"cap",)) for kw in ({"cap": -1}, {"cap": 2 ** 31 - 1}, {"cap": 2 ** 40})]
    out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                            {"stride": 1, "cap": 0})]
    if which == "pose":
        max_h = lib.pats_epipolar_max_h()
        out += [({"swapped": 2}, (b"swapped",)), ({"swapped": -1}, (b"swapped",))]
        out += [(kw, (b"moments", b"models", b"best")) for kw in ({"moments": 0, "models": 0}, {"moments": 0, "best": 0},
                                                                   {"moments": 0, "models": 0, "best": 0})]
        out += [(dict(kw, moments=0), (word,)) for kw, word in (({"H": 0}, b"H ="), ({"H": -1}, b"H ="), ({"H": max_h + 1}, b"max_h"))]
        out += [({"min_baseline": bad}, (b"min_baseline",)) for bad in (float("nan"), -0.5, float("-inf"))]
        out += [(kw, (b"cand_R", b"cand_t", b"cand_n")) for kw in ({"cand_R": 0}, {"cand_t": 0, "cand_n": 0})]
    else:
        out += [(kw, (b"front_sel", b"front_e", b"front_h")) for kw in ({"front_e": 0}, {"front_h": 0})]
    out.append(({"ws_bytes": 0}, ()))                                         # accepted sizes are 0 today: see check_refusals
    return out


def check_refusals(lib, which, base):
    """Every refusal is refused with a message that names the entry point and the argument -> the number of cases.  The workspace is
    0 bytes today, so "too small" cannot be provoked: that case only checks that the size function says 0."""
    cases = refusals(lib, which, base)
    for kw, words in cases:
        if "ws_bytes" in kw:
            size = lib.pats_homography_pose_workspace_bytes if which == "pose" else lib.pats_pose_select_workspace_bytes
            assert size(2, 100) == 0
            continue
        assert c_call(lib, which, base, **kw) != 0, (which, kw)
        msg = lib.pats_last_error()
        assert ENTRY[which]["tag"] in msg and all(w in msg for w in words), (which, kw, msg)
    return len(cases)
