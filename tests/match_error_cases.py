"""The match-error stage of include/pats_amd.h ("Per-pair match error against ground truth") restated in numpy float64, and a builder
of scenes with analytic depth in both views.  Shared by tests/test_match_error_cases_host.py (CPU) and tests/test_match_error_gpu.py;
written from the header's definition alone.

Definition (per match of a segment that takes part: finite right point, conf >= min_conf):
    Y = Rg X + tg (rows ((a + b) + c) + t),  u = Y[:2] / Y2,  q = u / s + c,  err = |q - p|
    status: 0 takes no part, 2 X not finite, 3 Y2 <= 0 or Y not finite, 4 outside size_r, 5 no right depth at the tap rint(q), 6 not
    covisible (|Y2 - d1| > occl_rel d1), 1 scored
The scene (make_pair): the left camera at the origin looks at a tilted background plane with a fronto-parallel occluder in front of it;
the right camera sees both through a known rigid motion.  The depth of every pixel of either view is the nearest ray-plane
intersection, in closed form.  Left points sit on integer pixels (the nearest-tap lift is then exact), right points are the exact
projection plus a known offset.  Holes, near blobs (behind the right camera), an out-of-view strip, NaN right points and low
confidences are placed deliberately, so every status value occurs; the builder asserts the margins that make every comparison of a
GPU run with this restatement exact (margins)."""
import numpy as np

import absolute_cases as ac
import pose_error_cases as pc

F32 = np.float32
F = np.float64
THR = (1.0, 3.0, 5.0)
OCCL = 0.2
FOCAL = 90.0
MARGIN = 1e-6           # relative margin of every status decision, absolute margin (px) of every threshold comparison
PERM = [1, 0, 2]        # P: the exchange of the first two components


def conjugate(R, t):
    """(P R P, P t): the reference's (x, y) frame <-> the hand-over's (y, x) frame; an index permutation, exact."""
    R, t = np.asarray(R, F), np.asarray(t, F)
    return R[PERM][:, PERM].copy(), t[PERM].copy()


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def one_pair(X, p, Rg, tg, norm_right=None, depth_r=None, occl_rel=OCCL, size_r=None, part=None):
    """X [n,3] float32, p [n,2] float32, (Rg, tg) float64 in the frame of the points -> (err [n] float64 with NaN where not scored,
    status [n] uint8, slack [n] float64: the smallest relative distance of a status decision of that match from its limit)."""
    X, p = np.asarray(X, F32).reshape(-1, 3), np.asarray(p, F32).reshape(-1, 2)
    n = X.shape[0]
    status = np.zeros(n, np.uint8)
    err = np.full(n, np.nan, F)
    slack = np.full(n, np.inf, F)
    part = (np.ones(n, bool) if part is None else part) & np.isfinite(p).all(1)
    with np.errstate(all="ignore"):
        Xd, pd = X.astype(F), p.astype(F)
        Y = np.stack([((Rg[i, 0] * Xd[:, 0] + Rg[i, 1] * Xd[:, 1]) + Rg[i, 2] * Xd[:, 2]) + tg[i] for i in range(3)], 1)
        open_ = part.copy()                                                       # still undecided

        def decide(which, value):
            nonlocal open_
            status[open_ & which] = value
            open_ = open_ & ~which

        decide(~np.isfinite(X).all(1), 2)
        slack[open_] = np.minimum(slack[open_], np.abs(Y[open_, 2]) / np.maximum(1.0, np.abs(Xd[open_]).max(1)))      # NaN for a Y that is not finite
        slack[np.isnan(slack)] = np.inf                                           # ... which no rounding decides
        decide(~np.isfinite(Y).all(1) | ~(Y[:, 2] > 0), 3)
        q = Y[:, :2] / Y[:, 2:3]
        if norm_right is not None:
            c, s = np.asarray(norm_right, F32)[:2].astype(F), np.asarray(norm_right, F32)[2:].astype(F)
            q = q / s + c
        if size_r is not None:
            hw = np.asarray(size_r, F32).astype(F)
            inside = (q[:, 0] >= 0) & (q[:, 0] <= hw[0] - 1) & (q[:, 1] >= 0) & (q[:, 1] <= hw[1] - 1)
            edge = np.minimum(np.minimum(np.abs(q[:, 0]), np.abs(q[:, 0] - (hw[0] - 1))), np.minimum(np.abs(q[:, 1]), np.abs(q[:, 1] - (hw[1] - 1))))
            slack[open_] = np.minimum(slack[open_], edge[open_] / max(hw[0], hw[1], 1.0))
            decide(~inside, 4)
        has_map = depth_r is not None and depth_r.ndim == 2 and depth_r.shape[0] >= 1 and depth_r.shape[1] >= 1
        if has_map:
            h, w = depth_r.shape
            ij = np.rint(q)                                                       # round half to even
            tie = np.abs(np.abs(q - np.floor(q)) - 0.5).min(1)                    # the distance of the tap's choice from a tie
            slack[open_] = np.minimum(slack[open_], tie[open_] / max(h, w))
            inb = (ij[:, 0] >= 0) & (ij[:, 0] < h) & (ij[:, 1] >= 0) & (ij[:, 1] < w)
            ii, jj = np.where(inb, ij[:, 0], 0).astype(np.int64), np.where(inb, ij[:, 1], 0).astype(np.int64)
            d1 = np.asarray(depth_r, F32)[ii, jj].astype(F)
            decide(~inb | ~np.isfinite(d1) | ~(d1 > 0), 5)
            gap, lim = np.abs(Y[:, 2] - d1), occl_rel * d1
            slack[open_] = np.minimum(slack[open_], np.abs(gap[open_] - lim[open_]) / d1[open_])
            decide(gap > lim, 6)
        e = q - pd
        err[open_] = np.sqrt(e[open_, 0] * e[open_, 0] + e[open_, 1] * e[open_, 1])
        status[open_] = 1
    return err, status, slack


def reference(points, mr, segs, T1, T0=None, thr=THR, norm=None, swapped=False, depths_r=None, occl_rel=OCCL, size_r=None, conf=None,
              min_conf=None, edges=None, mask=None):
    """The whole call: points [cap,3], mr [cap,2] float32, segs [(lo, n)] -> dict of the seven outputs (sweep / confusion None when not
    asked for) and `slack` [cap].  Rows of cap outside every segment are zero."""
    cap, pairs, n_thr = points.shape[0], len(segs), len(thr)
    thr = np.asarray(thr, F)
    out = {"err": np.zeros(cap, F), "status": np.zeros(cap, np.uint8), "tally": np.zeros((pairs, 8), np.int64),
           "correct": np.zeros((pairs, n_thr), np.int64), "err_sum": np.zeros(pairs, F), "sweep": None, "confusion": None,
           "slack": np.full(cap, np.inf, F)}
    if edges is not None:
        edges = np.asarray(edges, F32)
        out["sweep"] = np.zeros((pairs, len(edges), 1 + n_thr), np.int64)
    if mask is not None:
        out["confusion"] = np.zeros((pairs, 4), np.int64)
    for k, (lo, n) in enumerate(segs):
        sl = slice(lo, lo + n)
        R, t = pc.ground_truth64(T1[k], None if T0 is None else T0[k])
        if swapped:
            R, t = conjugate(R, t)
        part = None
        if min_conf is not None:
            with np.errstate(invalid="ignore"):
                part = np.asarray(conf[sl], F32) >= F32(min_conf)
        depth = None if depths_r is None else depths_r[k]
        err, status, slack = one_pair(points[sl], mr[sl], R, t, None if norm is None else norm[k][4:], depth, occl_rel,
                                      None if size_r is None else size_r[k], part)
        out["err"][sl], out["status"][sl], out["slack"][sl] = err, status, slack
        out["tally"][k, :7] = np.bincount(status, minlength=7)[:7]
        sc = status == 1
        with np.errstate(invalid="ignore"):
            within = sc[:, None] & (err[:, None] <= thr[None, :])
        out["correct"][k] = within.sum(0)
        out["err_sum"][k] = err[sc].sum()
        if edges is not None:
            with np.errstate(invalid="ignore"):
                at = sc[:, None] & (np.asarray(conf[sl], F32)[:, None] >= edges[None, :])        # [n,B], float32 comparison
            out["sweep"][k, :, 0] = at.sum(0)
            out["sweep"][k, :, 1:] = (at[:, :, None] & within[:, None, :]).sum(0)
        if mask is not None:
            m, good = np.asarray(mask[sl]) != 0, within[:, 0]
            out["confusion"][k] = [(sc & m & good).sum(), (sc & m & ~good).sum(), (sc & ~m & good).sum(), (sc & ~m & ~good).sum()]
    return out


# ---- the scene --------------------------------------------------------------------------------------------------------------------
def _ray_depth(C, dirs, planes):
    """The depth along each ray C + lam dirs (lam >= 0 is the camera-frame depth: the direction's own third component is 1) of the
    nearest plane hit.  planes: [(normal, offset, box or None)]: n . X = offset, box = (x0, x1, y0, y1) bounds of X[:2] / X[2] in the
    left frame.  -> [m] float64, +inf for no hit."""
    best = np.full(dirs.shape[0], np.inf, F)
    for nrm, off, box in planes:
        nrm = np.asarray(nrm, F)
        with np.errstate(all="ignore"):
            lam = (off - C @ nrm) / (dirs @ nrm)
            X = C + lam[:, None] * dirs
            ok = np.isfinite(lam) & (lam > 0)
            if box is not None:
                a, b = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
                ok &= (X[:, 2] > 0) & (a >= box[0]) & (a <= box[1]) & (b >= box[2]) & (b <= box[3])
        best = np.where(ok & (lam < best), lam, best)
    return best


def make_pair(seed, n, h=96, w=128, holes=0.06, near=0.04, nan_right=0.03):
    """One pair in the hand-over's (y, x) order -> dict:
        depth_l [h,w], depth_r [h,w] float32   analytic depth per pixel (holes 0, near blobs 0.4 in the left map)
        ml [n,2] float32 integer pixels, mr [n,2] float32 = the exact projection + delta (NaN rows: no right point)
        delta [n] float64 = |offset|, conf [n] float32, norm [8] float32, size_r [2] float32 (an out-of-view strip is cut off)
        T1, T0 [4,4] float64: extrinsics in the reference's (x, y) frame with T1 inv(T0) = the motion;  R, t: the motion there."""
    rng = np.random.default_rng(seed)
    norm = np.array([h / 2, w / 2, 1 / FOCAL, 1 / (FOCAL * 1.05)] * 2, F32)       # different focal lengths along the two axes
    nl = norm.astype(F)
    # the motion, (y, x, z) frame of the points: forward by 0.9 (so the near blobs at depth 0.4 fall behind the right camera)
    Rm = ac.rodrigues(np.array([0.05, -0.08, 0.03]) + 0.02 * rng.normal(size=3))
    tm = np.array([0.25, -0.35, -0.9]) + 0.05 * rng.normal(size=3)
    planes = [((0.2, 0.3, 1.0), 4.0 + 0.2 * rng.uniform(), None),                 # the tilted background
              ((0.0, 0.0, 1.0), 2.2, (-0.25, 0.05, -0.3, 0.1))]                   # the occluder, fronto-parallel to the left camera

    def grid_dirs():
        i, j = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
        return np.stack([(i.ravel() - nl[0]) * nl[2], (j.ravel() - nl[1]) * nl[3], np.ones(h * w)], 1)

    dl = grid_dirs()
    depth_l = _ray_depth(np.zeros(3), dl, planes).reshape(h, w)
    C = -Rm.T @ tm                                                                # the right camera's centre in the left frame
    dr = grid_dirs() @ Rm                                                         # rows R^T d: the right rays in the left frame
    depth_r = _ray_depth(C, dr, planes).reshape(h, w)
    depth_r = np.where(np.isfinite(depth_r), depth_r, 0.0)
    assert np.isfinite(depth_l).all() and depth_l.min() > 2.0

    size_r = np.array([h, w - 9], F32)                                            # the last 9 columns are pad: out of view
    depth_l = depth_l.astype(F32)

    def project(ml):
        """The exact projection of the left pixels through the (float32) depth that the lift will read."""
        d = depth_l[ml[:, 0].astype(int), ml[:, 1].astype(int)].astype(F)
        X = np.stack([(ml[:, 0].astype(F) - nl[0]) * nl[2] * d, (ml[:, 1].astype(F) - nl[1]) * nl[3] * d, d], 1)
        Y = X @ Rm.T + tm
        with np.errstate(all="ignore"):
            return np.stack([Y[:, 0] / Y[:, 2] / nl[6] + nl[4], Y[:, 1] / Y[:, 2] / nl[7] + nl[5]], 1)

    # left pixels whose projection is 1e-3 px clear of every tie of the tap's rounding and of every bound of the view (the margins
    # of assert_margins are a tenth of that); a pixel that is not is drawn again
    ml = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(F32)
    for _ in range(20):
        q = project(ml)
        tie = np.abs(np.abs(q - np.floor(q)) - 0.5).min(1)
        bounds = np.abs(q[:, :, None] - np.array([[0.0, h - 1.0], [0.0, w - 10.0]])[None]).min((1, 2))
        again = (tie < 1e-3) | (bounds < 1e-3)
        if not again.any():
            break
        ml[again] = np.stack([rng.integers(0, h, int(again.sum())), rng.integers(0, w, int(again.sum()))], 1).astype(F32)
    assert not again.any()
    ii, jj = ml[:, 0].astype(int), ml[:, 1].astype(int)
    kind = rng.random(n)
    blob = (kind >= holes) & (kind < holes + near)
    depth_l[ii[blob], jj[blob]] = 0.4
    depth_l[ii[kind < holes], jj[kind < holes]] = 0.0                             # a pixel drawn twice: the hole wins
    q = project(ml)
    mag = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.9, n), rng.uniform(0.0, 8.0, n))
    mag[::7] = 0.0
    ang = rng.uniform(0, 2 * np.pi, n)
    mr = (np.where(np.isfinite(q), q, 0.0) + mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(F32)
    lost = rng.random(n) < nan_right
    mr[lost] = np.nan
    conf = rng.uniform(0.05, 0.95, n).astype(F32)
    depth_r = depth_r.astype(F32)
    hole_r = rng.random((h, w)) < 0.05
    depth_r[hole_r] = 0.0
    # extrinsics in the reference's (x, y) frame: T1 inv(T0) = the motion
    R, t = conjugate(Rm, tm)
    R0, t0 = ac.rodrigues(0.3 * rng.normal(size=3)), rng.normal(size=3)
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, t0
    T1[:3, :3], T1[:3, 3] = R @ R0, R @ t0 + t
    return {"depth_l": depth_l, "depth_r": depth_r, "ml": ml, "mr": mr, "delta": mag, "conf": conf, "norm": norm, "size_r": size_r,
            "T1": T1, "T0": T0, "R": R, "t": t, "h": h, "w": w}


EDGES = (0.0, 0.2, 0.35, 0.5, 0.65, 0.8)
MIN_CONF = 0.15


def assert_margins(ref, conf, thr=THR, edges=None, min_conf=None):
    """What makes every comparison with a float64 device run exact: no scored error within MARGIN px of a threshold, no status
    decision within a relative MARGIN of its limit, no confidence on an edge."""
    sc = ref["status"] == 1
    err = ref["err"][sc]
    assert np.isfinite(err).all()
    for v in thr:
        assert np.abs(err - v).min(initial=np.inf) > MARGIN, "a scored error lies on the threshold %g" % v
    assert ref["slack"].min(initial=np.inf) > MARGIN, "a status decision lies on its limit"
    if edges is not None:
        assert not np.isin(np.asarray(conf, F32), np.asarray(edges, F32)).any(), "a confidence equals an edge"
    if min_conf is not None:
        assert not (np.asarray(conf, F32) == F32(min_conf)).any()


def make_batch(lengths, seed, slack_rows=0, stride=None, shapes=None, **kw):
    """Pairs of these lengths as ONE call's inputs -> dict: points / ml / mr / conf / mask over cap rows (the lift done by
    absolute_cases.lift32; a strided batch has `stride` rows per pair; rows in no segment hold plausible finite values, which a call
    must not score), segs,
    pair_off or counts, per-pair norm / size_r / T1 / T0 / depths_r, and the pairs themselves.  shapes: (h, w) per pair."""
    shapes = [(96, 128)] * len(lengths) if shapes is None else shapes             # (h, w) of each pair's images
    pairs = [make_pair(seed + 17 * k, n, h=shapes[k][0], w=shapes[k][1], **kw) for k, n in enumerate(lengths)]
    if stride is None:
        lo = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        segs, cap = [(int(lo[k]), int(n)) for k, n in enumerate(lengths)], int(lo[-1]) + slack_rows
    else:
        assert all(n <= stride for n in lengths)
        segs, cap = [(k * stride, int(n)) for k, n in enumerate(lengths)], len(lengths) * stride + slack_rows
    rng = np.random.default_rng(seed + 5)
    b = {"points": rng.uniform(1, 3, (cap, 3)).astype(F32), "ml": np.full((cap, 2), 3.0, F32), "mr": rng.uniform(0, 90, (cap, 2)).astype(F32),
         "conf": rng.uniform(0.3, 0.9, cap).astype(F32), "mask": (rng.random(cap) < 0.5).astype(np.uint8), "delta": np.zeros(cap, F)}
    for (lo_, n), c in zip(segs, pairs):
        sl = slice(lo_, lo_ + n)
        X, _ = ac.lift32(c["ml"], c["depth_l"], c["norm"][:4])
        b["points"][sl], b["ml"][sl], b["mr"][sl], b["conf"][sl], b["delta"][sl] = X, c["ml"], c["mr"], c["conf"], c["delta"]
    b.update(segs=segs, cap=cap, pairs=pairs, lengths=list(lengths), stride=stride,
             pair_off=None if stride is not None else np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
             counts=None if stride is None else np.asarray(lengths, np.int64),
             norm=np.stack([c["norm"] for c in pairs]), size_r=np.stack([c["size_r"] for c in pairs]),
             T1=np.stack([c["T1"] for c in pairs]), T0=np.stack([c["T0"] for c in pairs]), depths_r=[c["depth_r"] for c in pairs])
    return b


def reference_of(b, **kw):
    """reference() on a make_batch result: the full option set unless a keyword overrides it (None switches an option off)."""
    args = dict(T0=b["T0"], thr=THR, norm=b["norm"], swapped=True, depths_r=b["depths_r"], occl_rel=OCCL, size_r=b["size_r"], conf=b["conf"],
                min_conf=None, edges=None, mask=None)
    args.update(kw)
    T1 = args.pop("T1", b["T1"])
    return reference(b["points"], b["mr"], b["segs"], T1, **args)


def epipolar_distance(ml, mr, norm, R, t):
    """The distance of every right point from the epipolar line of its left point under the ground truth, in pixels: what the
    reference's get_pose_error (utils/utils.py) returns as `result` - p2^T F p1 / |(F p1)[:2]| with F = K1^-T [t]x R K0^-1 and (x, y)
    pixel coordinates; norm = (c0, c1, s0, s1) twice in (y, x) order, so K = [[1 / s1, 0, c1], [0, 1 / s0, c0], [0, 0, 1]]."""
    nl = np.asarray(norm, F32).astype(F)

    def K(half):
        c0, c1, s0, s1 = half
        return np.array([[1 / s1, 0, c1], [0, 1 / s0, c0], [0, 0, 1]])

    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Fm = np.linalg.inv(K(nl[4:])).T @ (tx @ R) @ np.linalg.inv(K(nl[:4]))
    one = np.ones((ml.shape[0], 1))
    p1 = np.concatenate([np.asarray(ml, F)[:, ::-1], one], 1)                     # (x, y, 1)
    p2 = np.concatenate([np.asarray(mr, F)[:, ::-1], one], 1)
    line = p1 @ Fm.T
    with np.errstate(all="ignore"):
        return np.abs(np.einsum("ij,ij->i", p2, line)) / np.sqrt(line[:, 0] ** 2 + line[:, 1] ** 2)
