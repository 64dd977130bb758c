"""The per-pair hypothesis generator of include/pats_amd.h ("Per-pair hypotheses") restated in numpy: the counter-based sampler in
exact integer arithmetic, the 8x9 constraint matrices from the float32 points, float64 null vectors and the backward-error ratio
the contract is written in.  Shared by tests/test_hypotheses_cases_host.py (CPU) and tests/test_hypotheses_gpu.py; written from
the header's definition alone.

Definition (per pair p with n matches, hypothesis h of H):
    pool     m_h = n (progressive == 0)  or  max(8, (n (h + 1) + H - 1) / H)
    sampler  k = mix(mix(mix(s_lo) ^ s_hi) + h);  u_t = mix(k + 0x9e3779b9 (t + 1));  j_t = (u_t (m_h - t)) >> 32;  draw t = the
             j_t-th index of 0 .. m_h - 1 not drawn before  (uint32 arithmetic that wraps; s_lo, s_hi = the halves of pair_seed[p])
    model    A [8,9], row t = vec(x_r x_l^T) of draw t;  e with A e = 0, |e| = 1, the component of largest magnitude positive
    contract |A e|_2 <= B eps32 |A|_F with e promoted to float64, | |e| - 1 | <= 1e-5;  zero model for n < 8 (samples -1) and for a
             sample with a non-finite coordinate"""
import numpy as np

import epipolar_cases as ec

EPS32 = float(np.finfo(np.float32).eps)
M32 = np.uint64(0xFFFFFFFF)
GOLDEN = np.uint64(0x9E3779B9)


def mix(x):
    """x: uint64 array holding uint32 values -> the same, mixed.  Every product is reduced mod 2^32 (exact: 32 x 32 bits fit 64)."""
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def pool(n, H, progressive):
    """m_h for h = 0 .. H-1 (int64); n >= 8."""
    h = np.arange(H, dtype=np.int64)
    if not progressive:
        return np.full(H, n, np.int64)
    return np.maximum(8, (np.int64(n) * (h + 1) + H - 1) // H)


def sample_idx(pair_seed, n, H, progressive=False):
    """-> [H,8] int32: the eight draws of every hypothesis in draw order; all -1 for n < 8."""
    if n < 8:
        return np.full((H, 8), -1, np.int32)
    s = int(pair_seed) & 0xFFFFFFFFFFFFFFFF                               # the 64 bits of the int64
    s_lo, s_hi = np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)
    h = np.arange(H, dtype=np.uint64)
    k = mix((mix(mix(s_lo) ^ s_hi) + h) & M32)
    m = pool(n, H, progressive).astype(np.uint64)
    out = np.empty((H, 8), np.int64)
    for t in range(8):
        u = mix((k + ((GOLDEN * np.uint64(t + 1)) & M32)) & M32)
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
    for t in range(8):
        u = mix1(k + 0x9E3779B9 * (t + 1))
        out.append(left.pop((u * (m - t)) >> 32))
    return out


def constraint(xl, xr, idx):
    """xl, xr [n,2] float32 points, idx [H,8] -> A [H,8,9] float64: row t = vec(x_r x_l^T) of draw t (exact products of float32)."""
    l = np.concatenate([xl.astype(np.float64), np.ones((xl.shape[0], 1))], 1)[idx]
    r = np.concatenate([xr.astype(np.float64), np.ones((xr.shape[0], 1))], 1)[idx]
    return (r[..., :, None] * l[..., None, :]).reshape(idx.shape + (9,))


def null64(A):
    """Float64 null vectors [H,9] of A [H,8,9]: the last right singular vector."""
    return np.linalg.svd(A)[2][:, 8, :]


def null32(A):
    """The same with numpy's float32 svd (LAPACK sgesdd): the baseline a float32 solve is measured against."""
    return np.linalg.svd(A.astype(np.float32))[2][:, 8, :]


def ratio(A, e):
    """|A e|_2 / (eps32 |A|_F) per hypothesis, e promoted to float64."""
    e = np.asarray(e).reshape(A.shape[0], 9).astype(np.float64)
    res = np.linalg.norm(np.einsum("htk,hk->ht", A, e), axis=1)
    return res / (EPS32 * np.linalg.norm(A.reshape(A.shape[0], -1), axis=1))


def reference(ml, mr, segs, seeds, H, progressive=False, norm=None):
    """Per pair a dict: idx [H,8] int32, A [H,8,9] float64 (None for n < 8), finite [H] bool (every sample coordinate finite),
    xl, xr, lo, n."""
    out = []
    for p, (lo, n) in enumerate(segs):
        with np.errstate(all="ignore"):                                     # an infinite scale in norm is a case, not an accident
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], None if norm is None else norm[p])
        idx = sample_idx(seeds[p], n, H, progressive)
        A, fin = None, np.zeros(H, bool)
        if n >= 8:
            with np.errstate(all="ignore"):
                A = constraint(xl, xr, idx)
            fin = np.isfinite(xl[idx]).all((1, 2)) & np.isfinite(xr[idx]).all((1, 2))
        out.append({"idx": idx, "A": A, "finite": fin, "xl": xl, "xr": xr, "lo": lo, "n": n})
    return out


def check_models(models, ref, B=None):
    """models [pairs,H,3,3] float32 against the contract's pointwise rules -> the largest backward-error ratio over nonzero models
    (0.0 if there is none).  Asserts: zero or finite unit; zero where it must be; the sign rule; the bound B if given."""
    worst = 0.0
    for p, r in enumerate(ref):
        e = models[p].reshape(-1, 9)
        zero = ~e.any(1)
        assert np.isfinite(e).all(), "pair %d: a non-finite model" % p
        assert zero[~r["finite"]].all(), "pair %d: a model that must be zero is not" % p
        nz = ~zero
        if not nz.any():
            continue
        nrm = np.linalg.norm(e[nz].astype(np.float64), axis=1)
        assert (np.abs(nrm - 1) <= 1e-5).all(), "pair %d: |e| off 1 by %g" % (p, np.abs(nrm - 1).max())
        big = np.argmax(np.abs(e[nz]), axis=1)                             # np.argmax: the lowest index among equals
        assert (e[nz][np.arange(nz.sum()), big] > 0).all(), "pair %d: the sign rule" % p
        q = ratio(r["A"][nz], e[nz])
        worst = max(worst, float(q.max()))
        if B is not None:
            assert q.max() <= B, "pair %d: backward error %g eps32 |A|_F > %g" % (p, q.max(), B)
    return worst


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def make_pairs(lengths, seed, outliers=0.4):
    """Pairs made by epipolar_cases.make_case, concatenated -> (ml [cap,2], mr [cap,2], pair_off [pairs + 1] int64)."""
    cases = [ec.make_case(seed + 17 * p, max(n, 1), 1, outliers=outliers) for p, n in enumerate(lengths)]
    ml = np.concatenate([c["ml"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 2), np.float32)])
    mr = np.concatenate([c["mr"][:n] for c, n in zip(cases, lengths)] + [np.zeros((0, 2), np.float32)])
    return ml, mr, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# the tolerance cases: (make_case seed, matches, hypotheses, pair_seed) - 2100 samples over three pairs of 600 matches
TOLERANCE_CASES = [(1, 600, 700, 1001), (2, 600, 700, 1002), (3, 600, 700, 1003)]
MARGIN = 8.0            # B = MARGIN * b32: 4 (a non-orthogonal method over LAPACK's SVD) x 2 (FMA contraction, operation order)


def tolerance_cases():
    """-> [(xl, xr, idx [H,8], A [H,8,9])] of TOLERANCE_CASES (non-progressive samples)."""
    out = []
    for seed, n, H, ps in TOLERANCE_CASES:
        c = ec.make_case(seed, n, 1)
        idx = sample_idx(ps, n, H)
        out.append((c["ml"], c["mr"], idx, constraint(c["ml"], c["mr"], idx)))
    return out


def baseline32():
    """b32: the largest backward-error ratio of numpy's float32 svd over the tolerance cases."""
    return max(float(ratio(A, null32(A)).max()) for _, _, _, A in tolerance_cases())
