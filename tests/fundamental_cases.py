"""The uncalibrated branch of include/pats_amd.h ("Per-pair 7-point hypotheses", "Per-pair fundamental matrices") restated in numpy:
the seven-draw sampler in exact integer arithmetic, the 7x9 constraint matrices from the float32 points, a float64 solver (SVD null
space, the binary cubic det(a F1 + b F2), np.roots), the three residuals the hypotheses' contract is written in, and the rank-2 refit
(eigh, SVD truncation, renormalise, sign rule) with its denormalisation and permutation.  Shared by
tests/test_fundamental_cases_host.py (CPU) and tests/test_fundamental_gpu.py; written from the header's definition alone - the device
takes another route (Householder null space, two charts of the projective line, bracketed Newton; Jacobi rotations for the refit).

Definition of the hypotheses (per pair p with n matches, sample h of H):
    pool      m_h = n (progressive == 0)  or  max(7, (n (h + 1) + H - 1) / H)
    sampler   the hypotheses' (tests/hypotheses_cases.py) with seven draws
    solutions A7 [7,9], row t = vec(x_r x_l^T) of draw t;  F1, F2 an orthonormal basis of its null space; every real (a : b) with
              det(a F1 + b F2) = 0; F = a F1 + b F2 with |F|_F = 1: at most 3
    models    [H,3,3,3] float32: the solutions found in the lowest slots, exact zeros behind; the component of largest magnitude
              positive;  all zero for n < 7 (samples -1) and for a sample with a non-finite coordinate
    contract  per non-zero model e (float64):  | |e| - 1 | <= 1e-5,  |A7 e|_2 <= B_epi eps32 |A7|_F,  |det F| <= B_det eps32"""
import numpy as np

import epipolar_cases as ec
import homography_cases as hm
import hypotheses_cases as hc
import pose_cases as pc

EPS32 = hc.EPS32
EPS64 = float(np.finfo(np.float64).eps)
MAX_MODELS = 3
MATCH_TOL = 1e-4        # a host solution is found when a device model of the sample has 1 - |<e_dev, e_host>| <= MATCH_TOL
DISTINCT_TOL = 1e-6     # two models of one sample are distinct when 1 - |<a, b>| > DISTINCT_TOL (the device drops within 2e-6)
MIN_INLIERS = 8
P_SWAP = hm.P_SWAP
sign_rule = hm.sign_rule


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def pool(n, H, progressive):
    """m_h for h = 0 .. H-1 (int64); n >= 7."""
    h = np.arange(H, dtype=np.int64)
    if not progressive:
        return np.full(H, n, np.int64)
    return np.maximum(7, (np.int64(n) * (h + 1) + H - 1) // H)


def sample_idx(pair_seed, n, H, progressive=False):
    """-> [H,7] int32: the seven draws of every sample in draw order; all -1 for n < 7."""
    if n < 7:
        return np.full((H, 7), -1, np.int32)
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF                               # the 64 bits of the int64
    s_lo, s_hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    h = np.arange(H, dtype=np.uint64)
    k = hc.mix((hc.mix(hc.mix(s_lo) ^ s_hi) + h) & hc.M32)
    m = pool(n, H, progressive).astype(np.uint64)
    out = np.empty((H, 7), np.int64)
    for t in range(7):
        u = hc.mix((k + ((hc.GOLDEN * np.uint64(t + 1)) & hc.M32)) & hc.M32)
        j = ((u * (m - np.uint64(t))) >> np.uint64(32)).astype(np.int64)  # u < 2^32, m - t < 2^31: the product fits 64 bits
        prev = np.sort(out[:, :t], axis=1)
        for i in range(t):                                                # ascending: skip every earlier draw at or below j
            j = j + (prev[:, i] <= j)
        out[:, t] = j
    return out.astype(np.int32)


def sample_idx_slow(pair_seed, h, m):
    """One sample from the definition's first form (the j-th index not drawn before), with Python integers."""
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
    for t in range(7):
        u = mix1(k + 0x9E3779B9 * (t + 1))
        out.append(left.pop((u * (m - t)) >> 32))
    return out


def constraint(xl, xr, idx):
    """xl, xr [n,2] float32 points, idx [H,7] -> A7 [H,7,9] float64: row t = vec(x_r x_l^T) of draw t (exact products)."""
    return hc.constraint(xl, xr, idx)


# ---- the float64 solver -----------------------------------------------------------------------------------------------------------
def cubic(F1, F2):
    """F1, F2 [S,3,3] -> c [S,4]: det(a F1 + b F2) = c0 a^3 + c1 a^2 b + c2 a b^2 + c3 b^3, from four values of the determinant."""
    d = lambda a, b: np.linalg.det(a * F1 + b * F2)                       # noqa: E731
    c0, c3 = d(1.0, 0.0), d(0.0, 1.0)
    p, m = d(1.0, 1.0), d(1.0, -1.0)                                     # c0 + c1 + c2 + c3,  c0 - c1 + c2 - c3
    c2 = (p + m) / 2 - c0
    c1 = (p - m) / 2 - c3
    return np.stack([c0, c1, c2, c3], 1)


def _unit_signed(e):
    e = e / np.linalg.norm(e, axis=1, keepdims=True)
    e = e[np.isfinite(e).all(1)]
    return e * np.sign(e[np.arange(e.shape[0]), np.argmax(np.abs(e), axis=1)])[:, None]


def solve64(A7, route="b/a"):
    """A7 [S,7,9] float64 -> per sample an array [k,9] (k <= 3) of the real unit solutions, the component of largest magnitude
    positive.  route "b/a": the roots t of c0 + c1 t + c2 t^2 + c3 t^3, F = F1 + t F2; route "a/b": the roots s of the reversed
    cubic, F = s F1 + F2.  A root at infinity of a route is a vanishing leading coefficient, which np.roots drops: generic samples
    have none."""
    S = A7.shape[0]
    N = np.linalg.svd(A7)[2][:, 7:, :].reshape(S, 2, 3, 3)
    c = cubic(N[:, 0], N[:, 1])
    out = []
    for s_ in range(S):
        k = c[s_] if route == "a/b" else c[s_, ::-1]                      # np.roots: the highest power first
        if not np.isfinite(k).all() or not k.any():
            out.append(np.zeros((0, 9)))
            continue
        w = np.roots(k)
        w = w[(w.imag == 0) & np.isfinite(w.real)].real
        ab = np.stack([w, np.ones_like(w)], 1) if route == "a/b" else np.stack([np.ones_like(w), w], 1)
        out.append(_unit_signed(ab @ N[s_].reshape(2, 9)))
    return out


# ---- the residuals ----------------------------------------------------------------------------------------------------------------
def epi_ratio(A7, e):
    """|A7 e|_2 / (eps32 |A7|_F); A7 [k,7,9], e [k,9] promoted to float64."""
    e = np.asarray(e).reshape(-1, 9).astype(np.float64)
    res = np.linalg.norm(np.einsum("ktj,kj->kt", A7, e), axis=1)
    return res / (EPS32 * np.linalg.norm(A7.reshape(A7.shape[0], -1), axis=1))


def det_ratio(e):
    """|det F| / eps32; e [k,9] promoted to float64."""
    return np.abs(np.linalg.det(np.asarray(e).reshape(-1, 3, 3).astype(np.float64))) / EPS32


def norm_error(e):
    """| |e| - 1 |; e [k,9] promoted to float64."""
    return np.abs(np.linalg.norm(np.asarray(e).reshape(-1, 9).astype(np.float64), axis=1) - 1)


def closeness(a, b):
    """1 - |<a_i, b_j>| for unit vectors a [i,9], b [j,9] -> [i,j] (float64)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 9), np.asarray(b, np.float64).reshape(-1, 9)
    return 1.0 - np.abs(a @ b.T)


def matches(dev, host, tol=MATCH_TOL):
    """dev [3,9] (zero slots allowed), host [k,9] of ONE sample -> [k] bool: host solution j has a device model within tol."""
    dev = np.asarray(dev).reshape(-1, 9)
    dev = dev[dev.any(1)]
    if host.shape[0] == 0:
        return np.zeros(0, bool)
    if dev.shape[0] == 0:
        return np.zeros(host.shape[0], bool)
    return (closeness(host, dev) <= tol).any(1)


def reference(ml, mr, segs, seeds, H, progressive=False, norm=None):
    """Per pair a dict: idx [H,7] int32, A [H,7,9] float64 (None for n < 7), finite [H] bool (every sample coordinate finite),
    xl, xr, lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        with np.errstate(all="ignore"):                                     # an infinite scale in norm is a case, not an accident
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        idx = sample_idx(seeds[p], n, H, progressive)
        A, fin = None, np.zeros(H, bool)
        if n >= 7:
            with np.errstate(all="ignore"):
                A = constraint(xl, xr, idx)
            fin = np.isfinite(xl[idx]).all((1, 2)) & np.isfinite(xr[idx]).all((1, 2))
        out.append({"idx": idx, "A": A, "finite": fin, "xl": xl, "xr": xr, "lo": lo, "n": n})
    return out


def check_models(models, ref, n_models=None, B_epi=None, B_det=None):
    """models [pairs,H,3,3,3] float32 against the contract's pointwise rules -> (the largest epipolar ratio, the largest determinant
    ratio) over the non-zero models (0.0 if there is none).  Asserts: finite; zero where it must be; compacted; n_models; unit norm;
    the sign rule; pairwise distinct; the bounds if given."""
    worst = [0.0, 0.0]
    for p, r in enumerate(ref):
        e = models[p].reshape(-1, MAX_MODELS, 9)
        assert np.isfinite(e).all(), "pair %d: a non-finite model" % p
        nz = e.any(2)                                                      # [H,3]
        assert not nz[~r["finite"]].any(), "pair %d: a model that must be zero is not" % p
        count = nz.sum(1)
        assert (nz == (np.arange(MAX_MODELS)[None, :] < count[:, None])).all(), "pair %d: the non-zero slots are not the lowest" % p
        if n_models is not None:
            assert np.array_equal(n_models[p], count.astype(np.int32)), "pair %d: n_models differs from the non-zero slots" % p
        if not nz.any():
            continue
        hh, ss = np.nonzero(nz)
        v = e[hh, ss]
        assert (norm_error(v) <= 1e-5).all(), "pair %d: |e| off 1 by %g" % (p, norm_error(v).max())
        big = np.argmax(np.abs(v), axis=1)                                 # np.argmax: the lowest index among equals
        assert (v[np.arange(v.shape[0]), big] > 0).all(), "pair %d: the sign rule" % p
        for h in np.nonzero(count > 1)[0]:
            c = closeness(e[h, :count[h]], e[h, :count[h]]) + 2 * np.eye(count[h])
            assert c.min() > DISTINCT_TOL, "pair %d sample %d: two models coincide" % (p, h)
        q_epi, q_det = epi_ratio(r["A"][hh], v), det_ratio(v)
        worst = [max(worst[0], float(q_epi.max())), max(worst[1], float(q_det.max()))]
        if B_epi is not None:
            assert q_epi.max() <= B_epi, "pair %d: epipolar residual %g eps32 |A7|_F > %g" % (p, q_epi.max(), B_epi)
        if B_det is not None:
            assert q_det.max() <= B_det, "pair %d: |det F| = %g eps32 > %g" % (p, q_det.max(), B_det)
    return tuple(worst)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# (make_case seed, matches, samples, pair_seed): 2100 non-progressive samples over three pairs of 600 matches
TOLERANCE_CASES = [(1, 600, 700, 1001), (2, 600, 700, 1002), (3, 600, 700, 1003)]
MARGIN = hc.MARGIN      # 8 = 4 (a non-LAPACK method) x 2 (FMA contraction, operation order): the hypotheses' argument, not widened
_CACHE = {}


def cases(exact):
    """-> [dict(ml, mr, idx [H,7], A [H,7,9], true [9] float64 unit, host: per sample [k,9])] of TOLERANCE_CASES - exact=True:
    outliers 0, noise 0 (exact geometry rounded to float32); exact=False: make_case's defaults (noise 5e-4, 40 % outliers).
    Computed once per process and shared: callers leave it unchanged."""
    if exact not in _CACHE:
        out = []
        for seed, n, H, ps in TOLERANCE_CASES:
            c = ec.make_case(seed, n, 1, outliers=0, noise=0) if exact else ec.make_case(seed, n, 1)
            idx = sample_idx(ps, n, H)
            A = constraint(c["ml"], c["mr"], idx)
            out.append({"ml": c["ml"], "mr": c["mr"], "idx": idx, "A": A, "true": c["models"][c["true"]].reshape(9).astype(np.float64),
                        "host": solve64(A)})
        _CACHE[exact] = out
    return _CACHE[exact]


def baselines():
    """(b_epi, b_det): the largest ratios of the float64 solver's models ROUNDED TO FLOAT32, over the exact and the noisy cases."""
    if "b" not in _CACHE:
        b = [0.0, 0.0]
        for exact in (True, False):
            for c in cases(exact):
                k = np.array([e.shape[0] for e in c["host"]])
                e32 = np.concatenate(c["host"]).astype(np.float32)
                b[0] = max(b[0], float(epi_ratio(np.repeat(c["A"], k, 0), e32).max()))
                b[1] = max(b[1], float(det_ratio(e32).max()))
        _CACHE["b"] = tuple(b)
    return _CACHE["b"]


def true_found(models, c, tol=MATCH_TOL):
    """models [H,3,9]: per sample, whether the case's true model is among them -> [H] bool."""
    m = np.asarray(models, np.float64).reshape(-1, MAX_MODELS, 9)
    return (1.0 - np.abs(m @ c["true"]) <= tol).any(1)


def host_models(c):
    """The float64 solutions of a case packed like the device's output -> [H,3,9] float64, zero slots behind."""
    out = np.zeros((len(c["host"]), MAX_MODELS, 9))
    for h, e in enumerate(c["host"]):
        out[h, :e.shape[0]] = e[:MAX_MODELS]
    return out


# ---- the refit ------------------------------------------------------------------------------------------------------------------------
def truncate(f):
    """f [9] -> (F [3,3] = U diag(s1, s2, 0) V^T of f as a 3x3 rescaled to |F|_F = 1 with the sign rule, sigma [3] descending)."""
    U, s, Vt = np.linalg.svd(np.asarray(f, np.float64).reshape(3, 3))
    F = (U[:, :2] * s[:2]) @ Vt[:2]
    return sign_rule(F / np.linalg.norm(F)), s


def refit64(M):
    """M [9,9] -> (F [3,3], eig [2], sigma [3], f [9]): eigh (the upper triangle read), the unit eigenvector of the smallest
    eigenvalue, its truncation."""
    M = np.triu(M) + np.triu(M, 1).T
    w, V = np.linalg.eigh(M)
    F, s = truncate(V[:, 0])
    return F, w[:2], s, V[:, 0]


def denormalise(F, norm_row=None):
    """F_px = N_r^T F N_l rescaled to Frobenius norm 1, the sign rule applied; F itself without norm."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    if norm_row is None:
        return F
    Nl, Nr = hm.norm_matrices(norm_row)
    G = Nr.T @ F @ Nl
    return sign_rule(G / np.linalg.norm(G))


def swap(F):
    """P F P with the sign rule applied after the permutation."""
    return sign_rule(P_SWAP @ np.asarray(F, np.float64).reshape(3, 3) @ P_SWAP)


def make_scene(seed, n, outliers=0.4, noise=5e-4):
    """pose_cases.make_scene's two-view pair (ml, mr, R, t, good [n] bool: the matches that follow the geometry) with its true model
    as F [3,3] float64 - unit, rank 2; an uncalibrated caller sees nothing else of it."""
    s = pc.make_scene(seed, n, outliers=outliers, noise=noise)
    s["F"] = pc.true_model(s).astype(np.float64)
    return s


def check_polish_refusals(lib, base):
    """polish_cases' table of refusals against the third family's entry point -> the number of cases."""
    import ctypes
    import polish_cases as pz
    cases_ = pz.refusals(lib, base)
    for kw, words in cases_:
        a = {n: base for n in pz.ALIGN}
        a["counts_in"] = 0
        a.update(pz.SCALARS)
        a.update(kw)
        args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in pz.ALIGN else a[n] for n in pz.ORDER]
        assert getattr(lib, POLISH[0])(*args, ctypes.c_void_p(base), 1 << 20, None) != 0, kw
        msg = lib.pats_last_error()
        assert POLISH[1] in msg and all(w in msg for w in words), (kw, msg)
    return len(cases_)


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------------
# per entry point: the argument order of the prototype (before workspace, workspace_bytes, stream), the pointers that must not be
# null, every pointer's alignment, the scalars of a valid call.  The polish entry point has polish_cases' table: its arguments are
# the other two families'.
ENTRY = {
    "hypotheses7": {
        "fn": "pats_epipolar_hypotheses7_by_pair_f32", "tag": b"epipolar_hypotheses7_by_pair",
        "order": ("matches_l", "matches_r", "pair_off", "stride", "counts_in", "pairs", "cap", "H", "pair_seed", "norm", "progressive",
                  "models", "sample_idx", "n_models"),
        "required": ("matches_l", "matches_r", "pair_seed", "models"),
        "align": {"matches_l": 8, "matches_r": 8, "pair_seed": 8, "models": 4, "norm": 4, "sample_idx": 4, "n_models": 4, "pair_off": 8,
                  "counts_in": 8},
        "scalars": {"stride": 0, "pairs": 2, "cap": 100, "H": 8, "progressive": 0}},
    "refit": {
        "fn": "pats_fundamental_refit_by_pair_f64", "tag": b"fundamental_refit_by_pair",
        "order": ("best_count", "moments", "models", "H", "best", "norm", "pairs", "swapped", "F", "F_px", "eig", "sigma", "f_refit"),
        "required": ("best_count", "F", "eig", "sigma"),
        "align": {"best_count": 8, "moments": 8, "F": 8, "F_px": 8, "eig": 8, "sigma": 8, "f_refit": 8, "models": 4, "best": 4, "norm": 4},
        "scalars": {"H": 8, "pairs": 2, "swapped": 0}},
}
POLISH = ("pats_fundamental_polish_by_pair_f32", b"fundamental_polish_by_pair")


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
    strided = {"pair_off": 0, "counts_in": base}
    out = [({name: 0}, (b"null", name.encode())) for name in e["required"]]
    for name, al in sorted(e["align"].items()):
        form = dict(strided, stride=10) if name == "counts_in" else {}
        out += [(dict(form, **{name: base + off}), (b"%d-byte aligned" % al, name.encode())) for off in ((1, 2, 3) if al == 4 else (1, 2, 4))]
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="),
                                           ({"H": max_h + 1}, b"max_h"))]
    if which == "hypotheses7":
        out += [(dict(strided, pair_off=base, stride=10), (b"pair_off", b"counts_in")), ({"pair_off": 0}, (b"pair_off", b"counts_in"))]
        out += [(kw, (b"cap",)) for kw in ({"cap": -1}, {"cap": 2 ** 31 - 1}, {"cap": 2 ** 40})]
        out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                                {"stride": 1, "cap": 0})]
        out += [({"progressive": 2}, (b"progressive",)), ({"progressive": -1}, (b"progressive",))]
        out += [({"H": max_h // 3 + 1}, (b"3 H", b"max_h")), ({"H": max_h}, (b"3 H", b"max_h"))]
        out += [({"pairs": 2 ** 31 - 1, "cap": 2 ** 31 - 2, "H": max_h // 3}, (b"pairs", b"grid"))]
    if which == "refit":
        out += [({"swapped": 2}, (b"swapped",)), ({"swapped": -1}, (b"swapped",))]
        out += [(kw, (b"moments", b"models", b"best")) for kw in ({"moments": 0, "models": 0}, {"moments": 0, "best": 0},
                                                                   {"moments": 0, "models": 0, "best": 0})]
    return out


def check_refusals(lib, which, base):
    """Every refusal is refused with a message that names the entry point and the argument -> the number of cases."""
    cases_ = refusals(lib, which, base)
    for kw, words in cases_:
        assert c_call(lib, which, base, **kw) != 0, (which, kw)
        msg = lib.pats_last_error()
        assert ENTRY[which]["tag"] in msg and all(w in msg for w in words), (which, kw, msg)
    return len(cases_)
