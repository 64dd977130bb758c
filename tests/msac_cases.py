"""The per-pair MSAC scoring of include/pats_amd.h ("Per-pair MSAC scoring") restated in numpy: the gain of every (model, match) cell
in float64, a per-cell bound on what a float32 evaluation may differ from it, a float32 emulation of the definition, and the seeded
"disagreement" cases in which counting picks a perturbed model and the MSAC gain the true one.  Shared by
tests/test_msac_cases_host.py (CPU) and tests/test_msac_gpu.py; written from the header's definition alone.

Definition (per pair; s, lim, w the family's: Epipolar s = r^2, w = den, Homography s = d0^2 + d1^2, w = a2^2; lim = thr^2 w):
    inlier iff the match participates and w > 0 and s <= lim
    g = 0 for a non-inlier; for an inlier u = s / lim (0 when lim == 0), q = min(floor(u 2^20), 2^20), g = 2^20 - q
    gains[h] = sum of g over the pair's matches (int64);  best = the lowest index of the largest gain
In real terms g / 2^20 = max(0, 1 - s / lim): gain64 below.

The bound (slack).  eps = 8 * 2^-24: every intermediate of the test is a sum of at most four products, each formed and added in
float32 - at most eight roundings between an input and a result, fewer with fused multiply-adds.  With A_i = sum_j |M_ij| |x_l,j|
and B_j = sum_i |M_ij| |x_r,i| (the magnitudes a rounding is relative to) the first-order error of every quantity follows by
propagation, written out in slack().  A cell's gain moves by at most (ds + u dlim) / (lim - dlim) for the quotient, 2^-20 for the floor
and 4 * 2^-24 for the reciprocal-and-multiply form of the division (1 ulp + half an ulp, rounded up); a cell whose verdict rounding
can flip has a gain near 0 on both sides, which the same expression covers; a cell that is an outlier beyond the errors, or whose
w is exactly 0 with every magnitude 0 (a zero model), gains 0 in every arithmetic: b = 0."""
import numpy as np

import epipolar_cases as ec
import homography_cases as hm

ONE = 1 << 20
EPS = 8 * 2.0 ** -24
FLOOR = 2.0 ** -20 + 4 * 2.0 ** -24
FAMILIES = ("epipolar", "homography")
THRS = (5e-4, 2e-3, 1e-2)
CELLS = {"epipolar": ec._cells, "homography": hm._cells}
HOST_CASES = {"epipolar": [(seed, n, H) for seed, n, H in ec.HOST_CASES], "homography": [(seed, n, H) for seed, H, n in hm.HOST_CASES]}


def make_case(family, seed, n, H, thr):
    """-> dict(ml, mr, models [H,3,3] float32, thr float32, true) of either family's seeded generator."""
    return ec.make_case(seed, n, H, thr=thr) if family == "epipolar" else hm.make_case(seed, n, H, thr=thr)


def _live(thr):
    return bool(np.float32(thr) >= 0)                                            # False for a NaN


def gain64(family, xl, xr, part, models, thr):
    """max(0, 1 - s / lim) over the float64 verdicts -> [H,n] float64; an inlier with lim == 0 gains 1."""
    H, n = np.asarray(models).reshape(-1, 3, 3).shape[0], xl.shape[0]
    if not _live(thr):
        return np.zeros((H, n))
    s, w = CELLS[family](xl, xr, models, np.float64)
    lim = np.float64(np.float32(thr)) ** 2 * w
    with np.errstate(all="ignore"):
        inl = part[None, :] & (w > 0) & (s <= lim)
        g = np.where(lim > 0, np.maximum(0.0, 1.0 - s / np.where(lim > 0, lim, 1.0)), 1.0)
    return np.where(inl, g, 0.0)


def cost64_loop(family, xl, xr, part, models, thr):
    """The MSAC cost per model, sum over the participating matches of min(e^2 / thr^2, 1), by a plain loop over scalars in float64
    (independent of gain64's array code) -> (cost [H], participating)."""
    M = np.asarray(models, np.float32).astype(np.float64).reshape(-1, 3, 3)
    t2 = float(np.float32(thr)) ** 2
    cost = np.zeros(M.shape[0])
    for h in range(M.shape[0]):
        for i in range(xl.shape[0]):
            if not part[i]:
                continue
            l, r = (float(xl[i, 0]), float(xl[i, 1]), 1.0), (float(xr[i, 0]), float(xr[i, 1]), 1.0)
            a = [sum(M[h, k, j] * l[j] for j in range(3)) for k in range(3)]
            if family == "epipolar":
                b = [sum(M[h, k, j] * r[k] for k in range(3)) for j in range(3)]
                s = (r[0] * a[0] + r[1] * a[1] + a[2]) ** 2
                w = a[0] * a[0] + a[1] * a[1] + b[0] * b[0] + b[1] * b[1]
            else:
                d0, d1 = a[0] - r[0] * a[2], a[1] - r[1] * a[2]
                s, w = d0 * d0 + d1 * d1, a[2] * a[2]
            lim = t2 * w
            inl = _live(thr) and w > 0 and s <= lim
            cost[h] += (s / lim if lim > 0 else 0.0) if inl else 1.0
    return cost, int(part.sum())


def slack(family, xl, xr, part, models, thr):
    """The per-cell bound b [H,n] float64 on |g32 / 2^20 - gain64| of a float32 evaluation (the module's docstring)."""
    M = np.asarray(models, np.float32).astype(np.float64).reshape(-1, 3, 3)
    H, n = M.shape[0], xl.shape[0]
    if not _live(thr):
        return np.zeros((H, n))
    t2 = np.float64(np.float32(thr)) ** 2
    l = np.concatenate([xl.astype(np.float64), np.ones((n, 1))], 1)               # [n,3]
    r = np.concatenate([xr.astype(np.float64), np.ones((n, 1))], 1)
    with np.errstate(all="ignore"):
        a = np.einsum("hij,nj->hin", M, l)                                       # a = M x_l   [H,3,n]
        A = np.einsum("hij,nj->hin", np.abs(M), np.abs(l))
        r0, r1 = r[:, 0][None, :], r[:, 1][None, :]
        if family == "epipolar":
            bb = np.einsum("hij,ni->hjn", M, r)                                  # b = M^T x_r
            B = np.einsum("hij,ni->hjn", np.abs(M), np.abs(r))
            rr = r0 * a[:, 0] + r1 * a[:, 1] + a[:, 2]
            s = rr * rr
            w = a[:, 0] ** 2 + a[:, 1] ** 2 + bb[:, 0] ** 2 + bb[:, 1] ** 2
            dr = EPS * (np.abs(r0) * A[:, 0] + np.abs(r1) * A[:, 1] + A[:, 2])
            ds = 2 * np.abs(rr) * dr + dr * dr
            dw = EPS * (2 * (np.abs(a[:, 0]) * A[:, 0] + np.abs(a[:, 1]) * A[:, 1] + np.abs(bb[:, 0]) * B[:, 0] + np.abs(bb[:, 1]) * B[:, 1]) + w)
        else:
            d0, d1 = a[:, 0] - r0 * a[:, 2], a[:, 1] - r1 * a[:, 2]
            s = d0 * d0 + d1 * d1
            w = a[:, 2] ** 2
            dd0, dd1 = EPS * (A[:, 0] + np.abs(r0) * A[:, 2]), EPS * (A[:, 1] + np.abs(r1) * A[:, 2])
            ds = 2 * (np.abs(d0) * dd0 + np.abs(d1) * dd1) + dd0 ** 2 + dd1 ** 2 + EPS * s
            dw = 2 * np.abs(a[:, 2]) * EPS * A[:, 2] + (EPS * A[:, 2]) ** 2
        lim = t2 * w
        dlim = t2 * dw + EPS * lim
        certain = (s - ds > lim + dlim) | (w + dw == 0)                          # an outlier beyond the errors; w is 0 in every arithmetic
        low = lim - dlim
        u = np.minimum(s / np.where(lim > 0, lim, 1.0), 1.0)
        b = np.minimum(1.0, (ds + u * dlim) / np.where(low > 0, low, 1.0) + FLOOR)
        b = np.where((low <= 0) | np.isnan(b) | np.isnan(low), 1.0, b)
        b = np.where(certain, 0.0, b)
    return np.where(part[None, :], b, 0.0)


def gain32(family, xl, xr, part, models, thr):
    """The definition with every operation in np.float32 and no FMA (an IEEE division for u) -> g [H,n] int64 in units of 2^-20."""
    H, n = np.asarray(models).reshape(-1, 3, 3).shape[0], xl.shape[0]
    thr = np.float32(thr)
    if not thr >= 0:
        return np.zeros((H, n), np.int64)
    s, w = CELLS[family](xl, xr, models, np.float32)
    with np.errstate(all="ignore"):
        lim = (thr * thr).astype(np.float32) * w
        inl = part[None, :] & (w > 0) & (s <= lim)
        u = np.where(lim > 0, (s / np.where(lim > 0, lim, np.float32(1))).astype(np.float32), np.float32(0))
        q = np.minimum(np.floor(np.where(inl, u, 0).astype(np.float64) * ONE), ONE).astype(np.int64)
    return np.where(inl, ONE - q, 0)


def reference(family, ml, mr, segs, models, thr, norm=None, conf=None, min_conf=None):
    """Per pair a dict: G64 [H] (the float64 gains in units of one inlier), S [H] (the summed bound), strict / loose [H] (the count
    restatement's), xl, xr, part, lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        with np.errstate(all="ignore"):
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        part = ec.participates(xl, xr, None if conf is None else conf[lo:lo + n], min_conf)
        cls = ec.classify if family == "epipolar" else hm.classify
        inl, dec = cls(xl, xr, part, models[p], thr[p])
        strict = (inl & dec).sum(1)
        out.append({"G64": gain64(family, xl, xr, part, models[p], thr[p]).sum(1), "S": slack(family, xl, xr, part, models[p], thr[p]).sum(1),
                    "strict": strict, "loose": strict + (~dec).sum(1), "xl": xl, "xr": xr, "part": part, "lo": lo, "n": n})
    return out


# ---- the disagreement cases ---------------------------------------------------------------------------------------------------------
# Recipe: a seeded case of 600 or 257 matches at thr = 1e-2 with four models - 0: the true model + N(0, SIGMA) per entry (from
# default_rng(seed + 7000)) rescaled to norm 1, 1: the true model, 2: a random model, 3: the zero model.  A seed is kept iff the count
# decidedly picks 0 - strict[0] > loose[h] for h > 0 - and the gain decidedly picks 1 - G64[1] - S[1] > G64[h] + S[h] + 1 for h != 1.
# Search settings, find_disagreements() at both sizes: epipolar SIGMA 0.004 over seeds 300 .. 539 (480 cases, 50 kept; four listed,
# two of each size); homography SIGMA 0.001 over seeds 300 .. 1259 (1920 cases, 6 kept, all of 600 matches; four listed) - the
# scenes' noise is 3e-4 against 5e-4, and the forward transfer error is more sensitive to a perturbed entry than the Sampson error:
# at 0.004 the perturbed homography loses the count as well, below 0.0008 it no longer wins it decidedly.
# test_msac_cases_host.py re-checks every listed seed's two conditions.
SIGMA = {"epipolar": 0.004, "homography": 0.001}
DISAGREE_THR = 1e-2
DISAGREEMENTS = {"epipolar": [(308, 600), (318, 600), (319, 257), (331, 257)],
                 "homography": [(390, 600), (428, 600), (801, 600), (868, 600)]}   # (seed, matches)


def disagreement_case(family, seed, n):
    """-> dict(ml, mr, models [4,3,3] float32, thr) of the recipe above."""
    c = make_case(family, seed, n, 4, DISAGREE_THR)
    true = c["models"][c["true"]].astype(np.float64)
    rng = np.random.default_rng(seed + 7000)
    pert = true + rng.normal(scale=SIGMA[family], size=(3, 3))
    rand = rng.normal(size=(3, 3))
    models = np.stack([pert / np.linalg.norm(pert), true, rand / np.linalg.norm(rand), np.zeros((3, 3))])
    if family == "homography":
        models = hm.sign_rule(models)
    return {"ml": c["ml"], "mr": c["mr"], "models": models.astype(np.float32), "thr": np.float32(DISAGREE_THR)}


def disagrees(family, c):
    """The two conditions on one case -> (kept, reference dict)."""
    n = c["ml"].shape[0]
    r = reference(family, c["ml"], c["mr"], [(0, n)], c["models"][None], [c["thr"]])[0]
    count0 = all(r["strict"][0] > r["loose"][h] for h in (1, 2, 3))
    gain1 = all(r["G64"][1] - r["S"][1] > r["G64"][h] + r["S"][h] + 1 for h in (0, 2, 3))
    return count0 and gain1, r


def find_disagreements(family, seeds=range(300, 540), sizes=(600, 257)):
    return [(seed, n) for seed in seeds for n in sizes if disagrees(family, disagreement_case(family, seed, n))[0]]


def committed_cases():
    """Every committed case -> [(family, label, case dict)]: both families' HOST_CASES at the three thresholds, then the disagreement
    seeds."""
    out = []
    for fam in FAMILIES:
        for seed, n, H in HOST_CASES[fam]:
            out += [(fam, "host %d thr %g" % (seed, thr), make_case(fam, seed, n, H, thr)) for thr in THRS]
        out += [(fam, "disagreement %d n %d" % (seed, n), disagreement_case(fam, seed, n)) for seed, n in DISAGREEMENTS[fam]]
    return out


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------------
# the count entries' table (homography_cases.ENTRY["score"]) with the two new outputs behind `stream`
ENTRY = {fam: dict(hm.ENTRY["score"], fn="pats_%s_score_msac_by_pair_f32" % fam, tag=("%s_score_msac_by_pair" % fam).encode())
         for fam in FAMILIES}
COUNT_TAG = {fam: ("%s_score_by_pair" % fam).encode() for fam in FAMILIES}


def c_call(lib, fam, base, gains=None, best_gain=None, count=False, **kw):
    """One raw call of an MSAC entry (count=True: of its count sibling, without the two outputs) with `base` behind every pointer."""
    import ctypes
    e = ENTRY[fam]
    a = {n: base for n in e["align"]}
    a["counts_in"] = 0
    a.update(e["scalars"])
    a.update(kw)
    args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in e["align"] else a[n] for n in e["order"]]
    args += [ctypes.c_void_p(base), 1 << 20, None]
    if count:
        return getattr(lib, "pats_%s_score_by_pair_f32" % fam)(*args)
    ptr = lambda v: ctypes.c_void_p(base if v is None else v) if (v is None or v) else None      # noqa: E731
    return getattr(lib, e["fn"])(*args, ptr(gains), ptr(best_gain))
