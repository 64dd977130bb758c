"""Inputs and the one comparison of tests/test_expand_edges_gpu.py (the patch-area expansion kernel, csrc/expand.hip,
against the CPU oracle); tests/test_expand_cases_host.py holds the generators to what the GPU tests rely on.

Numpy only apart from check_expand / raw_expand, which take the loaded `ops` module and import torch themselves.

The tie threshold is derived, not tuned.  A growth step compares strip sums of max(h, w) non-negative fp32 terms.  Any
summation order of k such terms is within (k - 1) * 2**-24 relative of the exact sum, the oracle's rounded double sum
within 2**-24; a decision compares two such sums (or one with lower_bound), so two implementations can only decide
differently where the oracle's own relative margin is at most max(h, w) * 2**-23.  Rows at or under it are "tie rows"."""
import ctypes

import numpy as np

ZERO_F = np.float32(1e-14)          # the project's "zero" (reference: 1e-14 appended / returned for no-match rows)
NAMES = ("whole_cost", "core_cost", "average_point", "x_scale", "y_scale", "bound")
# the gates the project already uses for these outputs (test_coarse_level, tools/fuzz_parity.py::op_expand)
GATES = {"whole_cost": dict(atol=3e-6, rtol=5e-5), "core_cost": dict(atol=3e-6, rtol=5e-4),
         "average_point": dict(atol=2e-4, rtol=2e-5), "x_scale": dict(atol=1e-5, rtol=5e-5),
         "y_scale": dict(atol=1e-5, rtol=5e-5)}
MAX_TIE_ROWS_PER_CALL = 2
MAX_TIE_SHARE = 1e-3


def tie_threshold(h, w):
    return max(h, w) * 2.0 ** -23


def blob_plan(rng, h, w, b, M=None, dust=0.15):
    """(P, Z, scalex, scaley): P [b, M, h*w + 1] float32, positive, rows sum to 1: a Gaussian blob of radius 0.7-3 cells round a
    random target cell per row over a 1e-5 floor, log-noise of 2 nats per entry, a dustbin entry that dominates on a share
    `dust` of the rows; Z = log(P) in float32 (the `input_is_log` input); scales independent, in exp(U(-1, 1))."""
    n = h * w
    M = n + 1 if M is None else M
    yy, xx = (np.arange(n) // w).astype(np.float64), (np.arange(n) % w).astype(np.float64)
    tgt = rng.integers(0, n, (b, M))
    rad = rng.uniform(0.7, 3.0, (b, M))
    d2 = (yy[None, None, :] - yy[tgt][..., None]) ** 2 + (xx[None, None, :] - xx[tgt][..., None]) ** 2
    logit = np.log(np.exp(-d2 / (2.0 * rad[..., None] ** 2)) + 1e-5) + 2.0 * rng.standard_normal((b, M, n))
    dusty = rng.random((b, M)) < dust
    total = np.log(np.exp(logit).sum(-1))
    # the dustbin entry: a twentieth of the row's real mass, or (dusty rows) so much that it exceeds every real entry
    dcol = np.where(dusty, logit.max(-1) + rng.uniform(0.5, 4.0, (b, M)), total + np.log(0.05) + rng.standard_normal((b, M)))
    full = np.concatenate([logit, dcol[..., None]], -1)
    full -= np.log(np.exp(full).sum(-1, keepdims=True))
    P = np.exp(full).astype(np.float32)
    Z = np.log(P.astype(np.float64)).astype(np.float32)
    sx = np.exp(rng.uniform(-1.0, 1.0, (b, n))).astype(np.float32)
    sy = np.exp(rng.uniform(-1.0, 1.0, (b, n))).astype(np.float32)
    return P, Z, sx, sy


def flat_plan(rng, h, w, b, M, value=2.0 ** -8):
    """(P, scalex, scaley, start): every entry of P [b, M, h*w + 1] is `value`, except one seeded real column per row raised
    to 2 * value (the row's start cell, returned as `start` [b, M]).  Every strip then holds equal dyadic cells, its fp32 sum is
    exact in any order, and every growth step is an exact tie decided by the reference's tie rules alone.
    Rows r with r % 7 == 3 carry 2 * value in a SECOND real column (first index wins the argmax; `start` is the smaller);
    rows with r % 7 == 5 carry 2 * value in the dustbin column too (the all-column argmax must stay on the real column)."""
    n = h * w
    P = np.full((b, M, n + 1), value, np.float32)
    start = rng.integers(0, n, (b, M))
    bi, ri = np.meshgrid(np.arange(b), np.arange(M), indexing="ij")
    P[bi, ri, start] = 2.0 * value
    second = (start + 1 + rng.integers(0, n - 1, (b, M))) % n if n > 1 else start
    two = (ri % 7 == 3)
    P[bi[two], ri[two], second[two]] = 2.0 * value
    start = np.where(two, np.minimum(start, second), start)
    dusteq = (ri % 7 == 5)
    P[bi[dusteq], ri[dusteq], n] = 2.0 * value
    sx = np.exp(rng.uniform(-1.0, 1.0, (b, n))).astype(np.float32)
    sy = np.exp(rng.uniform(-1.0, 1.0, (b, n))).astype(np.float32)
    return P, sx, sy, start


def force_argmax_column(P, rows, col, rng):
    """In place: the rows `rows` (indices into axis 1) of every problem get their maximum over ALL columns at `col`, strictly."""
    for r in rows:
        P[:, r, col] = P[:, r, :].max(-1) * np.float32(rng.uniform(1.5, 3.0))
    return P


def strip_cells(row, bound, h, w, d):
    """The cells (values, with the appended 1e-14 sentinel where the index leaves the grid) of strip d (0 up, 1 down, 2 left,
    3 right) next to the rectangle `bound` = (up, down, left, right), as Iterative_expand_matrix gathers them: `width` entries,
    the first bound_difference + 1 of them real indices, the others the 1e7 padding that overflows to the sentinel."""
    width = max(h, w)
    wh = h * w
    up, down, left, right = (int(v) for v in bound)
    ext = np.concatenate([np.asarray(row[:wh + 1], np.float32), [ZERO_F, ZERO_F]])
    out = []
    for k in range(width):
        if d < 2:
            base = float(k) if k <= right - left else 1e7
            f = base + (left + (up * width - width if d == 0 else down * width + width))
        else:
            base = float(k) if k <= down - up else 1e7
            f = base * width + (left + up * width - 1 if d == 2 else right + up * width + 1)
        s = int(f)
        if s < 0 or s > wh - 1:
            s = wh + 1
        out.append(ext[s])
    return np.asarray(out, np.float32)


def f32_sums(cells):
    """(forwards, backwards, pairwise) float32 sums of `cells`."""
    fw = np.float32(0)
    for v in cells:
        fw = np.float32(fw + v)
    bw = np.float32(0)
    for v in cells[::-1]:
        bw = np.float32(bw + v)
    lvl = [np.float32(v) for v in cells]
    while len(lvl) > 1:
        lvl = [np.float32(lvl[i] + lvl[i + 1]) if i + 1 < len(lvl) else lvl[i] for i in range(0, len(lvl), 2)]
    return fw, bw, lvl[0]


def oracle_stats(out, h, w):
    """What a plan exercises, from the oracle's outputs (with_margin=True): counts over all rows."""
    whole, bound, margin = out[0], out[5], out[6]
    width = max(h, w)
    height = h * w // width
    up, down, left, right = (bound[..., i] for i in range(4))
    thr = tie_threshold(h, w)
    grown = (down > up) | (right > left)
    return {"rows": int(whole.size), "tie_rows": int((margin[..., 0] <= thr).sum()),
            "elem_tie_rows": int((margin[..., 1] <= thr).sum()),
            "nomatch": int((whole == ZERO_F).sum()),
            "no_core": int((((down - up) <= 1) | ((right - left) <= 1)).sum()),
            "on_up": int((grown & (up == 0)).sum()), "on_down": int((grown & (down == height - 1)).sum()),
            "on_left": int((grown & (left == 0)).sum()), "on_right": int((grown & (right == width - 1)).sum()),
            "wrap_left": int((grown & (left == 0) & (up > 0)).sum()),
            "wrap_right": int((grown & (right == width - 1) & (down < height - 1)).sum()),
            "mean_area": float(((down - up + 1) * (right - left + 1)).mean()),
            "distinct": len({tuple(r) for r in bound.reshape(-1, 4).tolist()})}


# ---- GPU side ----------------------------------------------------------------------------------------------------------
def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_expand(ops, P, sx, sy, h, w, lim3, lower_bound, iter_num, is_log=False, lim_as_tensor=False, flag=True, count=None):
    """ops.Iterative_expand_matrix on device tensors; returns (six outputs, row_nomatch bool tensor or None)."""
    import torch
    b, M = P.shape[0], P.shape[1]
    positions, ranges = ops.Compute_positions_and_ranges(h, w, "cuda")
    lim = [0, h, 0, lim3]
    if lim_as_tensor:
        lim = torch.tensor(lim, dtype=torch.int64, device="cuda")
    rn = torch.full((b, M - 1), 2, dtype=torch.uint8, device="cuda") if flag else None
    got = ops.Iterative_expand_matrix(P, sx.reshape(b, -1, 1), sy.reshape(b, -1, 1), lim, ranges, positions,
                                      lower_bound=lower_bound, iter_num=iter_num, width=w, height=h, input_is_log=is_log,
                                      row_nomatch=rn, count=count)
    return got, rn


def check_expand(ops, oracle, P, sx, sy, h, w, lim3, lower_bound, iter_num, *, is_log, M, lim_as_tensor=False, exact=False):
    """The one comparison: the kernel and the oracle on the SAME input (`P` numpy [b, M, h*w + 1]; the log plan when `is_log`,
    the oracle then expands ops.exp(P) copied back - kernel and exp_kernel both call expf).  All six outputs and row_nomatch.
    `exact`: no tie exclusion at all (flat_plan: every sum is exact, every row must agree).
    Returns a dict: rows, tie_rows (excused bound differences are only possible there), elem_tie_rows, got (numpy outputs),
    want (oracle outputs incl. margin), flag."""
    P = np.ascontiguousarray(P, np.float32)
    b, Mp, N = P.shape
    assert Mp == M and N == h * w + 1, (P.shape, M, h, w)
    dP, dsx, dsy = cu(P), cu(sx), cu(sy)
    got, rn = gpu_expand(ops, dP, dsx, dsy, h, w, lim3, lower_bound, iter_num, is_log=is_log, lim_as_tensor=lim_as_tensor)
    lin = ops.exp(dP).cpu().numpy() if is_log else P
    want = oracle.iterative_expand(lin, sx, sy, lim3, h, w, lower_bound, iter_num, with_margin=True)
    got = [g.cpu().numpy() for g in got]
    what = "grid %dx%d b=%d M=%d lim3=%d lb=%g it=%d log=%d" % (h, w, b, M, lim3, lower_bound, iter_num, is_log)
    for g, wnt, name in zip(got, want, NAMES):
        assert g.shape == wnt.shape and g.dtype == wnt.dtype, (what, name, g.shape, g.dtype)

    flag = rn.cpu().numpy()
    want_flag = (P[:, :M - 1, :].argmax(-1) == N - 1).astype(np.uint8)      # numpy: first index on ties
    assert np.array_equal(flag, want_flag), "%s: row_nomatch differs in %d rows" % (what, int((flag != want_flag).sum()))

    thr = tie_threshold(h, w)
    margin = want[6]
    tie = np.zeros(margin.shape[:2], bool) if exact else margin[..., 0] <= thr
    elem_tie = np.zeros(margin.shape[:2], bool) if exact else margin[..., 1] <= thr
    diff = (got[5] != want[5]).any(-1)
    real = diff & ~tie
    if real.any():
        bi, ri = np.argwhere(real)[0]
        raise AssertionError("%s: bound differs in %d non-tie rows (of %d differing, %d rows); first [%d, %d]: kernel %s oracle %s "
                             "margin %.3g" % (what, int(real.sum()), int(diff.sum()), diff.size, bi, ri, got[5][bi, ri].tolist(),
                                              want[5][bi, ri].tolist(), float(margin[bi, ri, 0])))
    same = ~diff
    for i, name in enumerate(NAMES[:5]):
        rows = same & ~elem_tie if name == "whole_cost" else same
        g, wnt = got[i][rows], want[i][rows]
        bad = ~np.isclose(g, wnt, equal_nan=False, **GATES[name])
        if bad.any():
            k = np.argwhere(bad)[0]
            raise AssertionError("%s: %s differs on %d of %d entries (atol %g rtol %g); first: kernel %r oracle %r, max |d| %.3g"
                                 % (what, name, int(bad.sum()), bad.size, GATES[name]["atol"], GATES[name]["rtol"],
                                    g[tuple(k)], wnt[tuple(k)], float(np.nanmax(np.abs(g.astype(np.float64) - wnt)))))
    n_tie = int(tie.sum())
    assert n_tie <= MAX_TIE_ROWS_PER_CALL, "%s: %d tie rows in one call (cap %d)" % (what, n_tie, MAX_TIE_ROWS_PER_CALL)
    return {"rows": int(diff.size), "tie_rows": n_tie, "elem_tie_rows": int(elem_tie.sum()), "excused": int(diff.sum()),
            "got": got, "want": want, "flag": flag, "what": what}


SENT_BOUND, SENT_FLAG = -7, 2


def sentinel_outputs(b, m):
    """The six outputs and the flag bytes pre-filled: NaN for floats, -7 for bound, 2 for the flags."""
    import torch
    nan = float("nan")
    f = lambda *s: torch.full(s, nan, dtype=torch.float32, device="cuda")      # noqa: E731
    return [f(b, m), f(b, m), f(b, m, 2), f(b, m), f(b, m), torch.full((b, m, 4), SENT_BOUND, dtype=torch.int64, device="cuda"),
            torch.full((b, m), SENT_FLAG, dtype=torch.uint8, device="cuda")]


def raw_expand(ops, P, sx, sy, h, w, lim3, lower_bound, iter_num, outs, *, is_log=False, count=None):
    """The C entry points on caller-owned output buffers (`outs` of sentinel_outputs); raises what ops raises."""
    from pats_amd import _lib
    b, M, N = P.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731
    tail = [M, N, p(sx), p(sy), int(lim3), int(h), int(w), float(lower_bound), int(iter_num)] + [p(o) for o in outs] + [ops._stream()]
    if count is None:
        rc = _lib.lib().pats_iterative_expand_f32(p(P), int(is_log), b, *tail)
    else:
        rc = _lib.lib().pats_iterative_expand_counted_f32(p(P), int(is_log), b, p(count), *tail)
    _lib.check(rc, "Iterative_expand_matrix")


def untouched(outs, first_problem=0):
    """True when the outputs of every problem >= first_problem still hold their sentinel, bit for bit."""
    import torch
    fresh = sentinel_outputs(outs[0].shape[0], outs[0].shape[1])
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t    # noqa: E731  (NaN != NaN: compare the bits)
    return all(torch.equal(bits(o[first_problem:]), bits(f[first_problem:])) for o, f in zip(outs, fresh))
