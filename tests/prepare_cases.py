"""The image front end as include/pats_amd.h defines it ("Image front end"), restated in numpy from the header alone - the same
operations in the same order, one scalar rule at a time (the two integer passes run over whole arrays: int32 arithmetic has one
result in any order) - plus the seeded case generators.  No kernel, no library: the CPU tests hold this file to what can be known
without OpenCV (tests/test_prepare_cases_host.py) and to the reference's recorded intrinsics (tests/golden/prepare_intrinsics.npz),
the GPU tests hold the kernel to this file, bit for bit."""
import numpy as np

F64, F32 = np.float64, np.float32


# ---- the host half: target, window, canvas ----------------------------------------------------------------------------------------
def target_of(h0, w0, size):
    s = size / max(h0, w0)
    return int(w0 * s), int(h0 * s)                     # (w_t, h_t)


def window_of(h0, w0, w_t, h_t):
    """-> (y0, x0, h_c, w_c)"""
    if w0 / w_t < h0 / h_t:
        gap = int((h0 - w0 / w_t * h_t) / 2)
        return gap, 0, (h0 - gap) - gap, w0
    gap = int((w0 - h0 / h_t * w_t) / 2)
    return 0, gap, h0, (w0 - gap) - gap


def ceil32(v):
    return (v + 31) // 32 * 32


def canvas_of(targets, fixed=None):
    """targets = ((w_t, h_t) left, (w_t, h_t) right) of one pair -> (H, W)"""
    if fixed is not None:
        return tuple(fixed)
    return max(ceil32(t[1]) for t in targets), max(ceil32(t[0]) for t in targets)


# ---- the device half --------------------------------------------------------------------------------------------------------------
def axis_coefficients(sn, dn):
    """-> (s, t, a0, a1) int32 [dn]: the two taps and their weights of every destination sample."""
    inv = F64(dn) / F64(sn)
    scale = F64(1.0) / inv
    s_, t_, a0_, a1_ = (np.zeros(dn, np.int32) for _ in range(4))
    for d in range(dn):
        f = F32((F64(d) + F64(0.5)) * scale - F64(0.5))
        fl = np.floor(f)
        s = int(fl)
        f = F32(f - fl)
        if s < 0:
            s, f = 0, F32(0.0)
        if s >= sn - 1:
            s, f = sn - 1, F32(0.0)
        s_[d], t_[d] = s, min(s + 1, sn - 1)
        a0_[d] = int(np.rint(F32(F32(F32(1.0) - f) * F32(2048.0))))
        a1_[d] = int(np.rint(F32(f * F32(2048.0))))
    return s_, t_, a0_, a1_


def resize_u8(S, h_t, w_t):
    """The window S [h_c, w_c, 3] uint8 -> [h_t, w_t, 3] uint8."""
    S = np.asarray(S)
    assert S.dtype == np.uint8 and S.ndim == 3
    h_c, w_c = S.shape[:2]
    I = S.astype(np.int32)
    if w_c == 2 * w_t and h_c == 2 * h_t:
        return ((I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xs, xt, a0, a1 = axis_coefficients(w_c, w_t)
    ys, yt, b0, b1 = axis_coefficients(h_c, h_t)
    Hsum = I[:, xs, :] * a0[None, :, None] + I[:, xt, :] * a1[None, :, None]                   # [h_c, w_t, 3] int32
    out = (((b0[:, None, None] * (Hsum[ys] >> 4)) >> 16) + ((b1[:, None, None] * (Hsum[yt] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def prepare_u8(img, w_t, h_t, canvas, bgr=False):
    """One raw image [h0, w0, 3] uint8 -> its canvas [H, W, 3] uint8: window, resample, channel order, zero pad."""
    img = np.asarray(img)
    y0, x0, h_c, w_c = window_of(img.shape[0], img.shape[1], w_t, h_t)
    out = np.zeros((canvas[0], canvas[1], 3), np.uint8)
    r = resize_u8(img[y0:y0 + h_c, x0:x0 + w_c], h_t, w_t)
    out[:h_t, :w_t] = r[:, :, ::-1] if bgr else r
    return out


def resize_img_slices(h0, w0, w_new, h_new):
    """Resize_img's three lines of slicing (utils/utils.py:1123-1128) as Python slices of the rows and the columns."""
    if w0 / w_new < h0 / h_new:
        gap = int((h0 - w0 / w_new * h_new) / 2)
        return slice(gap, h0 - gap), slice(None)
    gap = int((w0 - h0 / h_new * w_new) / 2)
    return slice(None), slice(gap, w0 - gap)


# ---- intrinsics ---------------------------------------------------------------------------------------------------------------------
def ratio_and_add(h0, w0, w_t, h_t):
    w, h, wn, hn = F64(w0), F64(h0), F64(w_t), F64(h_t)
    h_w = hn / wn
    if w / wn < h / hn:
        return wn / w, (F64(0.0), (h - w * h_w) / F64(2.0))
    return hn / h, ((w - h / h_w) / F64(2.0), F64(0.0))


def intrinsics64(K, h0, w0, w_t, h_t, mode):
    K = np.asarray(K, F64)
    out = np.empty((3, 3), F64)
    if mode == "ratio":
        r, add = ratio_and_add(h0, w0, w_t, h_t)
        for i in range(3):
            for j in range(3):
                out[i, j] = r * K[i, j]
        out[2, 2] = F64(1.0)
        out[0, 2] = out[0, 2] - add[0] * r
        out[1, 2] = out[1, 2] - add[1] * r
        return out
    assert mode == "axes"
    d = (F64(1.0) / (F64(w0) / F64(w_t)), F64(1.0) / (F64(h0) / F64(h_t)), F64(1.0))
    for i in range(3):
        for j in range(3):
            out[i, j] = d[i] * K[i, j]                  # the matrix product with a diagonal matrix: the other terms are zeros
    return out


def norm32(Kl, Kr):
    """one pair -> [8] float32"""
    v = []
    for K in (Kl, Kr):
        v += [K[1, 2], K[0, 2], F64(1.0) / K[1, 1], F64(1.0) / K[0, 0]]
    return np.array(v, F64).astype(F32)


def thr32(Kl, Kr, threshold):
    return F32(F64(threshold) / np.mean([Kl[0, 0], Kr[1, 1], Kl[0, 0], Kr[1, 1]]))


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def image(seed, h, w, window=None):
    """A seeded uint8 [h, w, 3] image: a smooth ramp plus noise, values 0 .. 254.  With `window` (y0, x0, h_c, w_c) everything outside
    it is 255: a tap taken outside the window then shows in the output."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (yy[:, :, None] * 3 + xx[:, :, None] * 5 + np.arange(3)[None, None, :] * 40) % 200
    img = np.clip(base + rng.integers(-40, 55, (h, w, 3)), 0, 254).astype(np.uint8)
    if window is not None:
        y0, x0, h_c, w_c = window
        keep = img[y0:y0 + h_c, x0:x0 + w_c].copy()
        img[:] = 255
        img[y0:y0 + h_c, x0:x0 + w_c] = keep
    return img


# (h_c, w_c) -> (h_t, w_t): plain resamples of a whole window, both directions, from 2 x 2 to 480 x 640
RESIZE_CASES = [((2, 2), (9, 9)), ((5, 7), (11, 3)), ((1, 13), (4, 29)), ((13, 1), (29, 4)), ((9, 9), (2, 2)), ((48, 64), (33, 47)),
                ((64, 96), (32, 48)), ((64, 96), (40, 48)), ((3, 4097), (3, 1600)), ((37, 53), (111, 160)), ((480, 640), (300, 400)),
                ((240, 320), (480, 640))]
# raw (h0, w0) -> target (w_t, h_t): what each exercises
PLAN_CASES = {"gap_x": ((40, 64), (32, 32)), "gap_y": ((64, 40), (32, 32)), "odd_gap": ((45, 30), (20, 25)), "halving": ((64, 96), (48, 32)),
              "halving_x_only": ((65, 96), (48, 32)), "pad": ((48, 64), (47, 33)), "strip": ((3, 4097), (1600, 1)),
              "row": ((1, 13), (29, 4)), "column": ((13, 1), (4, 29)), "tiny_up": ((2, 2), (9, 9)), "mixed": ((5, 7), (3, 11))}
# the (w0, h0), (w_t, h_t) combinations of tests/golden/prepare_intrinsics.npz (tools/make_golden_prepare.py)
INTRINSIC_SIZES = [((1600, 1200), (1024, 768)), ((1200, 1600), (768, 1024)), ((1920, 1080), (1024, 576)), ((1000, 667), (1024, 683)),
                   ((640, 480), (640, 480)), ((1296, 968), (640, 478)), ((64, 40), (32, 32)), ((40, 64), (32, 32)), ((30, 45), (20, 25)),
                   ((4097, 3), (1600, 3)), ((1599, 1066), (1024, 682)), ((333, 500), (681, 1024))]


def intrinsic_K(i):
    rng = np.random.default_rng(7700 + i)
    (w0, h0), _ = INTRINSIC_SIZES[i]
    f = rng.uniform(0.6, 1.6) * max(w0, h0)
    return np.array([[f, 0.0, w0 / 2 + rng.uniform(-9, 9)], [0.0, f * rng.uniform(0.98, 1.02), h0 / 2 + rng.uniform(-9, 9)], [0.0, 0.0, 1.0]])


# the mixed batch: five pairs, four different source sizes, left and right of a pair with different canvases of their own, and grids
# whose stable sort is not the caller's order
MIXED_SIZES = [((120, 160), (90, 160)), ((40, 160), (40, 160)), ((160, 60), (160, 120)), ((160, 60), (160, 60)), ((75, 100), (60, 80))]
MIXED_SIZE = 96


def mixed_sources(seed=4100):
    return [(image(seed + 2 * p, *l), image(seed + 2 * p + 1, *r)) for p, (l, r) in enumerate(MIXED_SIZES)]
