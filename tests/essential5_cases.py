"""The per-pair 5-point hypothesis generator of include/pats_amd.h ("Per-pair 5-point hypotheses") restated in numpy: the five-draw
sampler in exact integer arithmetic, the 5x9 constraint matrices from the float32 points, a float64 solver (SVD null space, the ten
cubic constraints, np.linalg.solve, the action matrix of multiplication by x, np.linalg.eig) and the three residuals the contract
is written in.  Shared by tests/test_essential5_cases_host.py (CPU) and tests/test_essential5_gpu.py; written from the header's
definition alone - the device takes another route to the roots (a 3x3 polynomial matrix in z, a Sturm chain).

Definition (per pair p with n matches, sample h of H):
    pool      m_h = n (progressive == 0)  or  max(5, (n (h + 1) + H - 1) / H)
    sampler   the hypotheses' (tests/hypotheses_cases.py) with five draws
    solutions A5 [5,9], row t = vec(x_r x_l^T) of draw t;  E with |E|_F = 1, A5 vec(E) = 0, 2 E E^T E - tr(E E^T) E = 0: at most 10
    models    [H,10,3,3] float32: the solutions found in the lowest slots, exact zeros behind; the component of largest magnitude
              positive;  all zero for n < 5 (samples -1), for a sample with a non-finite coordinate, for a degenerate sample
    contract  per non-zero model e (float64):  | |e| - 1 | <= 1e-5,  |A5 e|_2 <= B_epi eps32 |A5|_F,
              |2 E E^T E - tr(E E^T) E|_F <= B_ess eps32"""
import numpy as np

import epipolar_cases as ec
import hypotheses_cases as hc

EPS32 = hc.EPS32
MAX_MODELS = 10
MATCH_TOL = 1e-4        # a host solution is found when a device model of the sample has 1 - |<e_dev, e_host>| <= MATCH_TOL
DISTINCT_TOL = 1e-6     # two models of one sample are distinct when 1 - |<a, b>| > DISTINCT_TOL


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def pool(n, H, progressive):
    """m_h for h = 0 .. H-1 (int64); n >= 5."""
    h = np.arange(H, dtype=np.int64)
    if not progressive:
        return np.full(H, n, np.int64)
    return np.maximum(5, (np.int64(n) * (h + 1) + H - 1) // H)


def sample_idx(pair_seed, n, H, progressive=False):
    """-> [H,5] int32: the five draws of every sample in draw order; all -1 for n < 5."""
    if n < 5:
        return np.full((H, 5), -1, np.int32)
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF                               # the 64 bits of the int64
    s_lo, s_hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    h = np.arange(H, dtype=np.uint64)
    k = hc.mix((hc.mix(hc.mix(s_lo) ^ s_hi) + h) & hc.M32)
    m = pool(n, H, progressive).astype(np.uint64)
    out = np.empty((H, 5), np.int64)
    for t in range(5):
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
    for t in range(5):
        u = mix1(k + 0x9E3779B9 * (t + 1))
        out.append(left.pop((u * (m - t)) >> 32))
    return out


def constraint(xl, xr, idx):
    """xl, xr [n,2] float32 points, idx [H,5] -> A5 [H,5,9] float64: row t = vec(x_r x_l^T) of draw t (exact products)."""
    return hc.constraint(xl, xr, idx)


# ---- the float64 solver -----------------------------------------------------------------------------------------------------------
# polynomials in (x, y, z) of total degree <= 3 as arrays [..., 4, 4, 4] indexed by the exponents
def _pmul(a, b):
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape))
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - i - j):
                if not a[..., i, j, k].any():
                    continue
                out[..., i:, j:, k:] += a[..., i, j, k][..., None, None, None] * b[..., :4 - i, :4 - j, :4 - k]
    return out


CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# x times basis monomial i: ("c", row of CUBIC) or ("b", index in BASIS)
_TIMES_X = [("c", 0), ("c", 1), ("c", 2), ("c", 3), ("c", 4), ("c", 5), ("b", 0), ("b", 1), ("b", 2), ("b", 6)]


def cubics(N):
    """N [S,4,3,3]: the null-space basis X, Y, Z, W -> the ten cubic constraints [S,10,20], columns CUBIC then BASIS."""
    S = N.shape[0]
    E = np.zeros((S, 3, 3, 4, 4, 4))
    E[..., 1, 0, 0], E[..., 0, 1, 0], E[..., 0, 0, 1], E[..., 0, 0, 0] = N[:, 0], N[:, 1], N[:, 2], N[:, 3]
    rows = []
    det = sum(_pmul(E[:, 0, j], _pmul(E[:, 1, (j + 1) % 3], E[:, 2, (j + 2) % 3]) - _pmul(E[:, 1, (j + 2) % 3], E[:, 2, (j + 1) % 3]))
              for j in range(3))
    rows.append(det)
    G = [[sum(_pmul(E[:, i, k], E[:, j, k]) for k in range(3)) for j in range(3)] for i in range(3)]      # E E^T
    tr = G[0][0] + G[1][1] + G[2][2]
    for i in range(3):
        for j in range(3):
            rows.append(2 * sum(_pmul(G[i][k], E[:, k, j]) for k in range(3)) - _pmul(tr, E[:, i, j]))
    C = np.stack(rows, 1)                                                # [S,10,4,4,4]
    return np.stack([C[:, :, i, j, k] for i, j, k in CUBIC + BASIS], 2)


def solve64(A5):
    """A5 [S,5,9] float64 -> per sample an array [k,9] (k <= 10) of the real unit solutions, the component of largest magnitude
    positive.  A sample whose elimination is singular has none."""
    S = A5.shape[0]
    N = np.linalg.svd(A5)[2][:, 5:, :].reshape(S, 4, 3, 3)
    C = cubics(N)
    out = []
    for s_ in range(S):
        try:
            Bm = np.linalg.solve(C[s_, :, :10], C[s_, :, 10:])           # cubic monomial i = -Bm[i] . basis
        except np.linalg.LinAlgError:
            out.append(np.zeros((0, 9)))
            continue
        M = np.zeros((10, 10))
        for i, (kind, at) in enumerate(_TIMES_X):
            if kind == "c":
                M[i] = -Bm[at]
            else:
                M[i, at] = 1.0
        w, V = np.linalg.eig(M)
        real = (w.imag == 0) & np.isfinite(w.real)
        V = V[:, real].real
        V = V[:, np.abs(V[9]) > 0]
        xyz1 = V[6:10] / V[9]                                             # (x, y, z, 1) of every real solution
        e = np.einsum("vk,vij->kij", xyz1, N[s_]).reshape(-1, 9)
        e = e / np.linalg.norm(e, axis=1, keepdims=True)
        e = e[np.isfinite(e).all(1)]
        e = e * np.sign(e[np.arange(e.shape[0]), np.argmax(np.abs(e), axis=1)])[:, None]
        out.append(e)
    return out


# ---- the residuals ----------------------------------------------------------------------------------------------------------------
def epi_ratio(A5, e):
    """|A5 e|_2 / (eps32 |A5|_F); A5 [k,5,9], e [k,9] promoted to float64."""
    e = np.asarray(e).reshape(-1, 9).astype(np.float64)
    res = np.linalg.norm(np.einsum("ktj,kj->kt", A5, e), axis=1)
    return res / (EPS32 * np.linalg.norm(A5.reshape(A5.shape[0], -1), axis=1))


def ess_ratio(e):
    """|2 E E^T E - tr(E E^T) E|_F / eps32; e [k,9] promoted to float64."""
    E = np.asarray(e).reshape(-1, 3, 3).astype(np.float64)
    G = E @ E.transpose(0, 2, 1)
    R = 2 * G @ E - np.trace(G, axis1=1, axis2=2)[:, None, None] * E
    return np.linalg.norm(R.reshape(-1, 9), axis=1) / EPS32


def closeness(a, b):
    """1 - |<a_i, b_j>| for unit vectors a [i,9], b [j,9] -> [i,j] (float64)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 9), np.asarray(b, np.float64).reshape(-1, 9)
    return 1.0 - np.abs(a @ b.T)


def matches(dev, host, tol=MATCH_TOL):
    """dev [10,9] (zero slots allowed), host [k,9] of ONE sample -> [k] bool: host solution j has a device model within tol."""
    dev = np.asarray(dev).reshape(-1, 9)
    dev = dev[dev.any(1)]
    if host.shape[0] == 0:
        return np.zeros(0, bool)
    if dev.shape[0] == 0:
        return np.zeros(host.shape[0], bool)
    return (closeness(host, dev) <= tol).any(1)


def reference(ml, mr, segs, seeds, H, progressive=False, norm=None):
    """Per pair a dict: idx [H,5] int32, A [H,5,9] float64 (None for n < 5), finite [H] bool (every sample coordinate finite),
    xl, xr, lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        with np.errstate(all="ignore"):                                     # an infinite scale in norm is a case, not an accident
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        idx = sample_idx(seeds[p], n, H, progressive)
        A, fin = None, np.zeros(H, bool)
        if n >= 5:
            with np.errstate(all="ignore"):
                A = constraint(xl, xr, idx)
            fin = np.isfinite(xl[idx]).all((1, 2)) & np.isfinite(xr[idx]).all((1, 2))
        out.append({"idx": idx, "A": A, "finite": fin, "xl": xl, "xr": xr, "lo": lo, "n": n})
    return out


def check_models(models, ref, n_models=None, B_epi=None, B_ess=None):
    """models [pairs,H,10,3,3] float32 against the contract's pointwise rules -> (the largest epipolar ratio, the largest essential
    ratio) over the non-zero models (0.0 if there is none).  Asserts: finite; zero where it must be; compacted; n_models; unit norm;
    the sign rule; pairwise distinct; the bounds if given."""
    worst = [0.0, 0.0]
    for p, r in enumerate(ref):
        e = models[p].reshape(-1, MAX_MODELS, 9)
        assert np.isfinite(e).all(), "pair %d: a non-finite model" % p
        nz = e.any(2)                                                      # [H,10]
        assert not nz[~r["finite"]].any(), "pair %d: a model that must be zero is not" % p
        count = nz.sum(1)
        assert (nz == (np.arange(MAX_MODELS)[None, :] < count[:, None])).all(), "pair %d: the non-zero slots are not the lowest" % p
        if n_models is not None:
            assert np.array_equal(n_models[p], count.astype(np.int32)), "pair %d: n_models differs from the non-zero slots" % p
        if not nz.any():
            continue
        hh, ss = np.nonzero(nz)
        v = e[hh, ss]
        nrm = np.linalg.norm(v.astype(np.float64), axis=1)
        assert (np.abs(nrm - 1) <= 1e-5).all(), "pair %d: |e| off 1 by %g" % (p, np.abs(nrm - 1).max())
        big = np.argmax(np.abs(v), axis=1)                                 # np.argmax: the lowest index among equals
        assert (v[np.arange(v.shape[0]), big] > 0).all(), "pair %d: the sign rule" % p
        for h in np.nonzero(count > 1)[0]:
            c = closeness(e[h, :count[h]], e[h, :count[h]]) + 2 * np.eye(count[h])
            assert c.min() > DISTINCT_TOL, "pair %d sample %d: two models coincide" % (p, h)
        q_epi, q_ess = epi_ratio(r["A"][hh], v), ess_ratio(v)
        worst = [max(worst[0], float(q_epi.max())), max(worst[1], float(q_ess.max()))]
        if B_epi is not None:
            assert q_epi.max() <= B_epi, "pair %d: epipolar residual %g eps32 |A5|_F > %g" % (p, q_epi.max(), B_epi)
        if B_ess is not None:
            assert q_ess.max() <= B_ess, "pair %d: essential residual %g eps32 > %g" % (p, q_ess.max(), B_ess)
    return tuple(worst)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
# (make_case seed, matches, samples, pair_seed): 2100 non-progressive samples over three pairs of 600 matches
TOLERANCE_CASES = [(1, 600, 700, 1001), (2, 600, 700, 1002), (3, 600, 700, 1003)]
MARGIN = hc.MARGIN      # 8 = 4 (a non-LAPACK method) x 2 (FMA contraction, operation order): the hypotheses' argument, not widened
_CACHE = {}


def cases(exact):
    """-> [dict(ml, mr, idx [H,5], A [H,5,9], true [9] float64 unit, host: per sample [k,9])] of TOLERANCE_CASES - exact=True:
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
    """(b_epi, b_ess): the largest ratios of the float64 solver's models ROUNDED TO FLOAT32, over the exact and the noisy cases."""
    if "b" not in _CACHE:
        b = [0.0, 0.0]
        for exact in (True, False):
            for c in cases(exact):
                k = np.array([e.shape[0] for e in c["host"]])
                e32 = np.concatenate(c["host"]).astype(np.float32)
                b[0] = max(b[0], float(epi_ratio(np.repeat(c["A"], k, 0), e32).max()))
                b[1] = max(b[1], float(ess_ratio(e32).max()))
        _CACHE["b"] = tuple(b)
    return _CACHE["b"]


def true_found(models, c, tol=MATCH_TOL):
    """models [H,10,9]: per sample, whether the case's true E is among them -> [H] bool."""
    m = np.asarray(models, np.float64).reshape(-1, MAX_MODELS, 9)
    return (1.0 - np.abs(m @ c["true"]) <= tol).any(1)


def host_models(c):
    """The float64 solutions of a case packed like the device's output -> [H,10,9] float64, zero slots behind."""
    out = np.zeros((len(c["host"]), MAX_MODELS, 9))
    for h, e in enumerate(c["host"]):
        out[h, :e.shape[0]] = e[:MAX_MODELS]
    return out
