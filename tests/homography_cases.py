"""The per-pair homographies of include/pats_amd.h ("Per-pair homographies") restated in numpy: the four-draw sampler in exact integer
arithmetic, the two DLT rows of a match, float64 null vectors, the forward-transfer test in float64 with its undecided band and a
float32 emulation of it, the moments, the refit's denormalisation, and a seeded generator of planar scenes.  Shared by
tests/test_homography_cases_host.py (CPU) and tests/test_homography_gpu.py; written from the header's definition alone.

Definition (per pair; x = the float32 point after the optional normalisation, r = (r0, r1) of x_r):
    rows     A_i = [ -x_l^T, 0, r0 x_l^T ],  B_i = [ 0, -x_l^T, r1 x_l^T ]  for h = vec(H), x_r ~ H x_l
    sampler  the hypotheses' with four draws; pool m_h = n or max(4, (n (h + 1) + H - 1) / H)
    model    the unit null vector of the 8x9 matrix of a sample's rows, the component of largest magnitude positive
    test     a = H x_l, d0 = a0 - r0 a2, d1 = a1 - r1 a2;  inlier iff participates and a2^2 > 0 and d0^2 + d1^2 <= thr^2 a2^2
    moments  sum over the winner's inliers of A_i^T A_i + B_i^T B_i
    H_px     N_r^-1 H N_l rescaled, N = [[s0,0,-c0 s0],[0,s1,-c1 s1],[0,0,1]]
A (match, model) cell is DECIDED when the float64 d0^2 + d1^2 lies outside the relative band DELTA around thr^2 a2^2 - or when the
verdict does not depend on rounding at all."""
import numpy as np

import epipolar_cases as ec
import hypotheses_cases as hc

EPS32 = hc.EPS32
EPS64 = float(np.finfo(np.float64).eps)
DELTA = 1e-3            # relative half-width of the undecided band around thr^2 a2^2
MARGIN = hc.MARGIN      # 8 = 4 (a non-orthogonal method over LAPACK's SVD) x 2 (FMA, operation order): the 8-point solve's, not widened
MIN_INLIERS = 4
P_SWAP = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


# ---- the sampler ------------------------------------------------------------------------------------------------------------------
def pool(n, H, progressive):
    """m_h for h = 0 .. H-1 (int64); n >= 4."""
    h = np.arange(H, dtype=np.int64)
    if not progressive:
        return np.full(H, n, np.int64)
    return np.maximum(4, (np.int64(n) * (h + 1) + H - 1) // H)


def sample_idx(pair_seed, n, H, progressive=False):
    """-> [H,4] int32: the four draws of every hypothesis in draw order; all -1 for n < 4.  hypotheses_cases' mixer, four draws."""
    if n < 4:
        return np.full((H, 4), -1, np.int32)
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF                               # the 64 bits of the int64
    s_lo, s_hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    h = np.arange(H, dtype=np.uint64)
    k = hc.mix((hc.mix(hc.mix(s_lo) ^ s_hi) + h) & hc.M32)
    m = pool(n, H, progressive).astype(np.uint64)
    out = np.empty((H, 4), np.int64)
    for t in range(4):
        u = hc.mix((k + ((hc.GOLDEN * np.uint64(t + 1)) & hc.M32)) & hc.M32)
        j = ((u * (m - np.uint64(t))) >> np.uint64(32)).astype(np.int64)  # u < 2^32, m - t < 2^31: the product fits 64 bits
        prev = np.sort(out[:, :t], axis=1)
        for i in range(t):                                                # ascending: skip every earlier draw at or below j
            j = j + (prev[:, i] <= j)
        out[:, t] = j
    return out.astype(np.int32)


def sample_idx_slow(pair_seed, h, m):
    """One hypothesis from the definition's first form (the j-th index not drawn before), with Python integers."""
    def mix1(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF
    k = mix1(mix1(mix1(s & 0xFFFFFFFF) ^ (s >> 32)) + h)
    left, out = list(range(m)), []
    for t in range(4):
        u = mix1(k + 0x9E3779B9 * (t + 1))
        out.append(left.pop((u * (m - t)) >> 32))
    return out


# ---- rows, null vectors, the backward error -----------------------------------------------------------------------------------------
def match_rows(xl, xr):
    """xl, xr [...,2] float32 -> (A [...,9], B [...,9]) float64: the two rows of every match (exact products of float32)."""
    l = np.concatenate([np.asarray(xl, np.float64), np.ones(np.shape(xl)[:-1] + (1,))], -1)
    r0, r1 = np.asarray(xr, np.float64)[..., 0:1], np.asarray(xr, np.float64)[..., 1:2]
    z = np.zeros_like(l)
    return np.concatenate([-l, z, r0 * l], -1), np.concatenate([z, -l, r1 * l], -1)


def rows(xl, xr, idx):
    """idx [H,4] -> A [H,8,9] float64: rows 2t and 2t + 1 are A_i and B_i of draw t."""
    a, b = match_rows(xl[idx], xr[idx])
    return np.stack([a, b], 2).reshape(idx.shape[0], 8, 9)


def null64(A):
    """Float64 null vectors [H,9] of A [H,8,9]: the last right singular vector."""
    return np.linalg.svd(A)[2][:, 8, :]


def null32(A):
    """The same with numpy's float32 svd (LAPACK sgesdd): the baseline a float32 solve is measured against."""
    return np.linalg.svd(A.astype(np.float32))[2][:, 8, :]


ratio = hc.ratio        # |A e|_2 / (eps32 |A|_F) per hypothesis, e promoted to float64


def sign_rule(e):
    """e [...,9] (or [...,3,3]): the component of largest magnitude positive, the lowest index among equals."""
    f = np.asarray(e).reshape(-1, 9)
    big = f[np.arange(f.shape[0]), np.argmax(np.abs(f), axis=1)]
    return (f * np.where(big < 0, -1.0, 1.0)[:, None]).reshape(np.shape(e))


def reference(ml, mr, segs, seeds, H, progressive=False, norm=None):
    """Per pair a dict: idx [H,4] int32, A [H,8,9] float64 (None for n < 4), finite [H] bool (every sample coordinate finite),
    xl, xr, lo, n - the keys hypotheses_cases.check_models reads."""
    out = []
    for p, (lo, n) in enumerate(segs):
        with np.errstate(all="ignore"):
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        idx = sample_idx(seeds[p], n, H, progressive)
        A, fin = None, np.zeros(H, bool)
        if n >= 4:
            with np.errstate(all="ignore"):
                A = rows(xl, xr, idx)
            fin = np.isfinite(xl[idx]).all((1, 2)) & np.isfinite(xr[idx]).all((1, 2))
        out.append({"idx": idx, "A": A, "finite": fin, "xl": xl, "xr": xr, "lo": lo, "n": n})
    return out


check_models = hc.check_models      # zero or finite unit, zero where it must be, the sign rule, the bound: nothing 8-point in it


# ---- the test -----------------------------------------------------------------------------------------------------------------------
def _cells(xl, xr, Hm, dtype):
    """d0^2 + d1^2 and a2^2 [H,n] in `dtype`, every operation rounded to it (np.float32: the emulation, without FMA)."""
    Hm = np.asarray(Hm, np.float32).astype(dtype).reshape(-1, 3, 3)
    l0, l1 = xl[:, 0].astype(dtype)[None, :], xl[:, 1].astype(dtype)[None, :]
    r0, r1 = xr[:, 0].astype(dtype)[None, :], xr[:, 1].astype(dtype)[None, :]
    e = lambda i, j: Hm[:, i, j][:, None]                                        # noqa: E731
    with np.errstate(all="ignore"):
        a0 = e(0, 0) * l0 + e(0, 1) * l1 + e(0, 2)
        a1 = e(1, 0) * l0 + e(1, 1) * l1 + e(1, 2)
        a2 = e(2, 0) * l0 + e(2, 1) * l1 + e(2, 2)
        d0, d1 = a0 - r0 * a2, a1 - r1 * a2
        return d0 * d0 + d1 * d1, a2 * a2


def classify(xl, xr, part, Hm, thr, delta=DELTA):
    """-> (inlier64 [H,n] bool, decided [H,n] bool) of one pair."""
    H, n = np.asarray(Hm).reshape(-1, 3, 3).shape[0], xl.shape[0]
    thr = np.float32(thr)
    if not thr >= 0:                                                             # NaN or negative: no inliers, nothing to round
        return np.zeros((H, n), bool), np.ones((H, n), bool)
    s, w = _cells(xl, xr, Hm, np.float64)
    lim = np.float64(thr) ** 2 * w
    with np.errstate(invalid="ignore"):
        inl = part[None, :] & (w > 0) & (s <= lim)
        outside = (s < lim * (1 - delta)) | (s > lim * (1 + delta))
        certain = ~part[None, :] | np.isnan(s) | np.isnan(lim) | (w == 0)        # no rounding can turn these into inliers
    return inl, outside | certain


def emulate32(xl, xr, part, Hm, thr):
    """The same formula with every operation in np.float32 -> inlier [H,n] bool."""
    thr = np.float32(thr)
    H, n = np.asarray(Hm).reshape(-1, 3, 3).shape[0], xl.shape[0]
    if not thr >= 0:
        return np.zeros((H, n), bool)
    s, w = _cells(xl, xr, Hm, np.float32)
    with np.errstate(all="ignore"):
        lim = (thr * thr).astype(np.float32) * w
        return part[None, :] & (w > 0) & (s <= lim)


def verify_reference(ml, mr, segs, models, thr, norm=None, conf=None, min_conf=None, delta=DELTA):
    """Per pair a dict: inl [H,n] (float64 verdicts), decided [H,n], strict [H], loose [H], xl, xr, part, lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        part = ec.participates(xl, xr, None if conf is None else conf[lo:lo + n], min_conf)
        inl, dec = classify(xl, xr, part, models[p], thr[p], delta)
        strict = (inl & dec).sum(1)
        out.append({"inl": inl, "decided": dec, "strict": strict, "loose": strict + (~dec).sum(1), "xl": xl, "xr": xr, "part": part,
                    "lo": lo, "n": n})
    return out


def moments64(xl, xr, mask):
    """sum over mask of A_i^T A_i + B_i^T B_i -> M [9,9] float64, summed in extended precision: the reference's own rounding is
    then far below the float64 ordering differences the test allows."""
    a, b = match_rows(xl[mask], xr[mask])
    a, b = a.astype(np.longdouble), b.astype(np.longdouble)
    M = (a[:, :, None] * a[:, None, :]).sum(0) + (b[:, :, None] * b[:, None, :]).sum(0)
    return M.astype(np.float64)


# ---- the refit ------------------------------------------------------------------------------------------------------------------------
def norm_matrices(norm_row):
    """(N_l, N_r) float64 from one float32 row (c0_l, c1_l, s0_l, s1_l, c0_r, c1_r, s0_r, s1_r), widened exactly."""
    q = np.asarray(norm_row, np.float32).astype(np.float64)
    N = lambda c0, c1, s0, s1: np.array([[s0, 0.0, -c0 * s0], [0.0, s1, -c1 * s1], [0.0, 0.0, 1.0]])      # noqa: E731
    return N(*q[:4]), N(*q[4:])


def denormalise(Hm, norm_row=None):
    """H_px = N_r^-1 H N_l rescaled to Frobenius norm 1, the sign rule applied; H itself without norm."""
    Hm = np.asarray(Hm, np.float64).reshape(3, 3)
    if norm_row is None:
        return Hm
    Nl, Nr = norm_matrices(norm_row)
    G = np.linalg.solve(Nr, Hm @ Nl)
    return sign_rule(G / np.linalg.norm(G))


def swap(Hm):
    """P H P with the sign rule applied after the permutation."""
    return sign_rule(P_SWAP @ np.asarray(Hm, np.float64).reshape(3, 3) @ P_SWAP)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_scene(seed, n, outliers=0.4, noise=3e-4, thr=2e-3):
    """One pair looking at a plane: n left points uniform in +-0.6, H = R + t n^T / 2 (rotation angles N(0, 0.15), t N(0, 0.2),
    n = unit(0.1, -0.2, 1)), right points with N(0, noise) noise rounded to float32, the FIRST `outliers` share of them replaced by
    uniform outliers.  -> dict(ml, mr, H [3,3] float64 unit with the sign rule, good [n] bool, thr)."""
    rng = np.random.default_rng(seed)
    R = _rot(*rng.normal(scale=0.15, size=3))
    t = rng.normal(scale=0.2, size=3)
    nv = np.array([0.1, -0.2, 1.0])
    nv /= np.linalg.norm(nv)
    Ht = R + np.outer(t, nv) / 2
    xl = rng.uniform(-0.6, 0.6, (n, 2))
    y = np.concatenate([xl, np.ones((n, 1))], 1) @ Ht.T
    xr = y[:, :2] / y[:, 2:3] + rng.normal(scale=noise, size=(n, 2))
    bad = int(round(outliers * n))
    xr[:bad] = rng.uniform(-0.8, 0.8, (bad, 2))
    good = np.arange(n) >= bad
    return {"ml": xl.astype(np.float32), "mr": xr.astype(np.float32), "H": sign_rule(Ht / np.linalg.norm(Ht)), "good": good,
            "thr": np.float32(thr)}


def make_case(seed, n, H, outliers=0.4, thr=2e-3):
    """A scene with H float32 models: float64 null vectors of random 4-samples (the sign rule applied) and the true homography at a
    seeded index.  -> the scene's dict + models [H,3,3] float32, true."""
    c = make_scene(seed, n, outliers=outliers, thr=thr)
    rng = np.random.default_rng(seed + 7919)
    idx = np.stack([rng.choice(n, 4, replace=False) for _ in range(H)]) if n >= 4 else np.zeros((H, 4), np.int64)
    models = sign_rule(null64(rows(c["ml"], c["mr"], idx))) if n >= 4 else np.zeros((H, 9))
    true = int(rng.integers(0, H))
    models[true] = c["H"].reshape(9)
    c.update(models=models.reshape(H, 3, 3).astype(np.float32), true=true)
    return c


def make_pairs(lengths, seed, outliers=0.4):
    """Scenes concatenated -> (ml [cap,2], mr [cap,2], pair_off [pairs + 1] int64)."""
    scenes = [make_scene(seed + 17 * p, max(n, 1), outliers=outliers) for p, n in enumerate(lengths)]
    ml = np.concatenate([s["ml"][:n] for s, n in zip(scenes, lengths)] + [np.zeros((0, 2), np.float32)])
    mr = np.concatenate([s["mr"][:n] for s, n in zip(scenes, lengths)] + [np.zeros((0, 2), np.float32)])
    return ml, mr, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# the committed seeds of the verification: (seed, models, matches)
HOST_CASES = [(101, 96, 3000), (102, 257, 2049), (103, 64, 500), (104, 33, 4097), (105, 128, 1200), (106, 300, 65)]

# the tolerance cases: (scene seed, matches, hypotheses, pair_seed) - 2100 samples over three pairs of 600 matches
TOLERANCE_CASES = [(1, 600, 700, 1001), (2, 600, 700, 1002), (3, 600, 700, 1003)]


def tolerance_cases():
    """-> [(xl, xr, idx [H,4], A [H,8,9])] of TOLERANCE_CASES (non-progressive samples)."""
    out = []
    for seed, n, H, ps in TOLERANCE_CASES:
        c = make_scene(seed, n)
        idx = sample_idx(ps, n, H)
        out.append((c["ml"], c["mr"], idx, rows(c["ml"], c["mr"], idx)))
    return out


def baseline32():
    """b32: the largest backward-error ratio of numpy's float32 svd over the tolerance cases."""
    return max(float(ratio(A, null32(A)).max()) for _, _, _, A in tolerance_cases())


def host_figures(delta=DELTA):
    """The figures of HOST_CASES -> (largest undecided share, cells where the float32 emulation differs from float64 on a DECIDED
    cell, cells)."""
    worst, wrong, cells = 0.0, 0, 0
    for seed, H, n in HOST_CASES:
        c = make_case(seed, n, H)
        part = ec.participates(c["ml"], c["mr"])
        inl, dec = classify(c["ml"], c["mr"], part, c["models"], c["thr"], delta)
        emu = emulate32(c["ml"], c["mr"], part, c["models"], c["thr"])
        worst = max(worst, float((~dec).mean()))
        wrong += int(((emu != inl) & dec).sum())
        cells += inl.size
    return worst, wrong, cells


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------------
# per entry point: the argument order of the prototype (before workspace, workspace_bytes, stream), the pointers that must not be
# null, every pointer's alignment, the scalars of a valid call
ENTRY = {
    "hypotheses": {
        "fn": "pats_homography_hypotheses_by_pair_f32", "tag": b"homography_hypotheses_by_pair",
        "order": ("matches_l", "matches_r", "pair_off", "stride", "counts_in", "pairs", "cap", "H", "pair_seed", "norm", "progressive",
                  "models", "sample_idx"),
        "required": ("matches_l", "matches_r", "pair_seed", "models"),
        "align": {"matches_l": 8, "matches_r": 8, "pair_seed": 8, "models": 4, "norm": 4, "sample_idx": 4, "pair_off": 8, "counts_in": 8},
        "scalars": {"stride": 0, "pairs": 2, "cap": 100, "H": 8, "progressive": 0}},
    "score": {
        "fn": "pats_homography_score_by_pair_f32", "tag": b"homography_score_by_pair",
        "order": ("matches_l", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "models", "H", "thr", "norm",
                  "use_min_conf", "min_conf", "counts", "best", "best_count", "inlier", "moments"),
        "required": ("matches_l", "matches_r", "models", "thr", "counts", "best", "best_count", "inlier"),
        "align": {"matches_l": 8, "matches_r": 8, "models": 4, "thr": 4, "norm": 4, "conf": 4, "counts": 4, "best": 4, "pair_off": 8,
                  "counts_in": 8, "best_count": 8, "moments": 8, "inlier": 1},
        "scalars": {"stride": 0, "pairs": 2, "cap": 100, "H": 8, "use_min_conf": 0, "min_conf": 0.0}},
    "refit": {
        "fn": "pats_homography_refit_by_pair_f64", "tag": b"homography_refit_by_pair",
        "order": ("best_count", "moments", "models", "H", "best", "norm", "pairs", "swapped", "H_out", "H_px", "eig"),
        "required": ("best_count", "H_out", "eig"),
        "align": {"best_count": 8, "moments": 8, "H_out": 8, "H_px": 8, "eig": 8, "models": 4, "best": 4, "norm": 4},
        "scalars": {"H": 8, "pairs": 2, "swapped": 0}},
}


def c_call(lib, which, base, ws_bytes=1 << 20, **kw):
    """One raw call of an entry point with `base` behind every pointer (the ragged form), `kw` overriding arguments by name."""
    import ctypes
    e = ENTRY[which]
    a = {n: base for n in e["align"]}
    if "counts_in" in a:
        a["counts_in"] = 0
    a.update(e["scalars"])
    a.update(kw)
    args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in e["align"] else a[n] for n in e["order"]]
    return getattr(lib, e["fn"])(*args, ctypes.c_void_p(base), ws_bytes, None)


def refusals(lib, which, base):
    """Every refusal of the header's list -> [(keyword arguments of c_call(), the words the message must hold)]."""
    e = ENTRY[which]
    max_h = lib.pats_epipolar_max_h()
    segs = "pair_off" in e["align"]
    strided = {"pair_off": 0, "counts_in": base}
    out = [({name: 0}, (b"null", name.encode())) for name in e["required"]]
    for name, al in sorted(e["align"].items()):
        if al == 1:
            continue
        form = dict(strided, stride=10) if name == "counts_in" else {}
        out += [(dict(form, **{name: base + off}), (b"%d-byte aligned" % al, name.encode())) for off in ((1, 2, 3) if al == 4 else (1, 2, 4))]
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="),
                                           ({"H": max_h + 1}, b"max_h"))]
    if segs:
        out += [(dict(strided, pair_off=base, stride=10), (b"pair_off", b"counts_in")), ({"pair_off": 0}, (b"pair_off", b"counts_in"))]
        out += [(kw, (b"cap",)) for kw in ({"cap": -1}, {"cap": 2 ** 31 - 1}, {"cap": 2 ** 40})]
        out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                                {"stride": 1, "cap": 0})]
    if which == "hypotheses":
        out += [({"progressive": 2}, (b"progressive",)), ({"progressive": -1}, (b"progressive",))]
    if which == "score":
        out += [({"use_min_conf": 1, "min_conf": bad}, (b"min_conf",)) for bad in (float("nan"), -0.25, float("-inf"))]
        out += [({"use_min_conf": 1, "min_conf": 0.5, "conf": 0}, (b"min_conf", b"conf")),
                ({"pairs": 2 ** 31 - 1, "cap": 2 ** 31 - 2, "H": max_h}, (b"pairs",))]         # a grid of 2^31 workgroups or more
    if which == "refit":
        out += [({"swapped": 2}, (b"swapped",)), ({"swapped": -1}, (b"swapped",))]
        out += [(kw, (b"moments", b"models", b"best")) for kw in ({"moments": 0, "models": 0}, {"moments": 0, "best": 0},
                                                                   {"moments": 0, "models": 0, "best": 0})]
    return out


def check_refusals(lib, which, base):
    """Every refusal is refused with a message that names the entry point and the argument -> the number of cases."""
    cases = refusals(lib, which, base)
    for kw, words in cases:
        assert c_call(lib, which, base, **kw) != 0, (which, kw)
        msg = lib.pats_last_error()
        assert ENTRY[which]["tag"] in msg and all(w in msg for w in words), (which, kw, msg)
    return len(cases)
