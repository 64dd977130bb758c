"""CPU-only: the image front end's restatement (tests/prepare_cases.py) held to what can be known without OpenCV, the host half of the
product (ops.prepare_plan, ops.prepare_intrinsics and the norm / thr they lead to) held to the restatement and to the reference's
recorded intrinsics (tests/golden/prepare_intrinsics.npz), and the library's refusal of every bad argument without a GPU.
No kernel is launched here.  cv2 is not installed where this was written: nothing here claims parity with an OpenCV build."""
import ctypes

import numpy as np
import pytest
import torch

import prepare_cases as pc
from conftest import golden


@pytest.fixture(scope="module")
def ops():
    from pats_amd import build
    build.build()
    from pats_amd import ops
    return ops


def bilinear64(S, h_t, w_t):
    x = torch.from_numpy(np.ascontiguousarray(S)).double().permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(x, size=(h_t, w_t), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (1, 13), (13, 1), (9, 11), (48, 64)])
def test_identity_size_returns_the_source(shape):
    img = pc.image(11, *shape)
    assert np.array_equal(pc.resize_u8(img, *shape), img)


def test_constant_images_map_to_themselves():
    for v in range(256):
        c = np.full((7, 9, 3), v, np.uint8)
        for h_t, w_t in ((13, 5), (3, 20), (14, 18), (7, 9)):
            assert (pc.resize_u8(c, h_t, w_t) == v).all(), (v, h_t, w_t)


@pytest.mark.parametrize("src,dst", pc.RESIZE_CASES)
def test_within_one_grey_level_of_float64_bilinear(src, dst):
    img = pc.image(100 + src[0] + dst[1], *src)
    diff = np.abs(pc.resize_u8(img, *dst).astype(np.float64) - bilinear64(img, *dst)).max()
    print("resize %s -> %s: max |restatement - float64 bilinear| = %.4f" % (src, dst, diff))
    assert diff < 1.0


def test_exact_halving_is_the_rounded_mean():
    img = pc.image(12, 64, 96)
    mean = img.astype(np.float64).reshape(32, 2, 48, 2, 3).sum(axis=(1, 3)) / 4.0
    assert np.array_equal(pc.resize_u8(img, 32, 48), np.floor(mean + 0.5).astype(np.uint8))
    # a halving in one axis only stays bilinear: the mean of the two columns at full row weight where the rows coincide
    one = pc.resize_u8(img, 64, 48)
    xs, xt, a0, a1 = pc.axis_coefficients(96, 48)
    assert (xs == 2 * np.arange(48)).all() and (a0 == 1024).all() and (a1 == 1024).all()
    assert np.abs(one.astype(np.float64) - (img[:, 0::2].astype(np.float64) + img[:, 1::2]) / 2.0).max() <= 0.5


def test_axis_coefficients_at_the_edges():
    s, t, a0, a1 = pc.axis_coefficients(1, 5)                                       # a degenerate axis: one tap, full weight
    assert (s == 0).all() and (t == 0).all() and (a0 == 2048).all() and (a1 == 0).all()
    s, t, a0, a1 = pc.axis_coefficients(2, 9)                                       # upscaling: head and tail clamp
    assert s[0] == 0 and a0[0] == 2048 and s[-1] == 1 and t[-1] == 1 and a0[-1] == 2048 and a1[-1] == 0
    assert ((a0 + a1) == 2048).all()
    s, t, a0, a1 = pc.axis_coefficients(4097, 1600)
    assert s.max() <= 4096 and t.max() <= 4096 and (np.diff(s) > 0).all()


@pytest.mark.parametrize("name", sorted(pc.PLAN_CASES))
def test_windows_are_the_slices_resize_img_takes(name):
    (h0, w0), (w_t, h_t) = pc.PLAN_CASES[name]
    rows, cols = pc.resize_img_slices(h0, w0, w_t, h_t)
    idx = np.arange(h0 * w0).reshape(h0, w0)
    y0, x0, h_c, w_c = pc.window_of(h0, w0, w_t, h_t)
    assert np.array_equal(idx[rows, cols], idx[y0:y0 + h_c, x0:x0 + w_c])
    assert h_c >= 1 and w_c >= 1


def test_plan_cases_take_the_paths_they_are_named_after():
    w = {k: pc.window_of(h0, w0, w_t, h_t) for k, ((h0, w0), (w_t, h_t)) in pc.PLAN_CASES.items()}
    assert w["gap_x"][1] > 0 and w["gap_y"][0] > 0 and w["odd_gap"][2] % 2 == 1
    assert (w["halving"][2], w["halving"][3]) == (64, 96)
    assert w["halving_x_only"][3] == 2 * 48 and w["halving_x_only"][2] != 2 * 32
    assert w["row"][2] == 1 and w["column"][3] == 1 and w["strip"][3] == 4097


# ---- the product's host half ------------------------------------------------------------------------------------------------------------
def test_prepare_plan_is_the_restatement(ops):
    sizes = [((h0, w0), (h0, w0)) for (h0, w0), _ in pc.PLAN_CASES.values()]
    targets = [(t, t) for _, t in pc.PLAN_CASES.values()]
    pl = ops.prepare_plan(sizes, targets=targets)
    for p, ((h0, w0), (w_t, h_t)) in enumerate(pc.PLAN_CASES.values()):
        for side in range(2):
            got = tuple(int(getattr(pl, k)[p, side]) for k in ("y0", "x0", "h_c", "w_c", "h_t", "w_t", "h0", "w0"))
            assert got == pc.window_of(h0, w0, w_t, h_t) + (h_t, w_t, h0, w0)
        assert tuple(pl.canvas[p]) == pc.canvas_of(((w_t, h_t),) * 2)


def test_prepare_plan_reproduces_the_yfcc_canvases(ops):
    sizes = [((1200, 1600), (1600, 1200)), ((1066, 1599), (667, 1000)), ((768, 1024), (500, 333)), ((480, 640), (480, 640))]
    pl = ops.prepare_plan(sizes, size=1024)
    for p, pair in enumerate(sizes):
        dims = []
        for side, (h0, w0) in enumerate(pair):
            w_t, h_t = pc.target_of(h0, w0, 1024)
            assert (int(pl.w_t[p, side]), int(pl.h_t[p, side])) == (w_t, h_t) and max(w_t, h_t) in (1023, 1024)
            # yfcc.py:43-44: v // 32 * 32 + (1 - int(v % 32 == 0)) * 32
            dims.append((h_t // 32 * 32 + (1 - int(h_t % 32 == 0)) * 32, w_t // 32 * 32 + (1 - int(w_t % 32 == 0)) * 32))
        assert tuple(pl.canvas[p]) == (max(dims[0][0], dims[1][0]), max(dims[0][1], dims[1][1]))
    assert tuple(pl.canvas[0]) == (1024, 1024)
    # slots: grids sorted stably, offsets the prefix of the canvases in slot order
    order = sorted(range(len(sizes)), key=lambda i: pl.shapes[i])
    assert list(pl.caller_of) == order and [pl.slot_of[i] for i in order] == list(range(len(sizes)))
    off = 0
    for i in order:
        assert int(pl.dst[i]) == off and off % 3072 == 0
        off += int(pl.canvas[i, 0] * pl.canvas[i, 1] * 3)
    assert pl.elems == off


def test_prepare_plan_with_the_fixed_scannet_canvas(ops):
    sizes = [((968, 1296), (968, 1296)), ((480, 640), (968, 1296))]
    pl = ops.prepare_plan(sizes, size=640, canvas=(480, 640))
    assert (pl.canvas == np.array([480, 640])).all() and pl.shapes == [(15, 20)] * 2
    assert (int(pl.w_t[0, 0]), int(pl.h_t[0, 0])) == (640, 478)
    with pytest.raises(ValueError, match="does not fit"):
        ops.prepare_plan(sizes, size=640, canvas=(448, 640))
    with pytest.raises(ValueError):
        ops.prepare_plan(sizes, size=640, canvas=(480, 650))
    with pytest.raises(ValueError):
        ops.prepare_plan(sizes)
    with pytest.raises(ValueError):
        ops.prepare_plan(sizes, size=640, targets=(640, 480))


def test_intrinsics_equal_the_reference_record(ops):
    g = golden("prepare_intrinsics.npz")
    assert len(g["sizes"]) == len(pc.INTRINSIC_SIZES) >= 12
    branches = set()
    for i, (w0, h0, w_t, h_t) in enumerate(g["sizes"].tolist()):
        assert ((w0, h0), (w_t, h_t)) == pc.INTRINSIC_SIZES[i]
        K = pc.intrinsic_K(i)
        assert np.array_equal(K, g["K"][i])
        r, add = pc.ratio_and_add(h0, w0, w_t, h_t)
        assert r == g["ratio"][i] and np.array_equal(np.array(add), g["add_num"][i])
        branches.add("x" if add[0] != 0 else ("y" if add[1] != 0 else "none"))
        for mode, ref in (("ratio", g["K_ratio"][i]), ("axes", g["K_axes"][i])):
            assert np.array_equal(pc.intrinsics64(K, h0, w0, w_t, h_t, mode), ref), (i, mode)
            assert np.array_equal(ops.prepare_intrinsics(K, h0, w0, w_t, h_t, mode), ref), (i, mode)
    assert branches == {"x", "y", "none"}               # a float gap in either axis, and none


def test_norm_and_thr_are_the_restatement(ops):
    Kl = np.stack([pc.intrinsics64(pc.intrinsic_K(i), h0, w0, w_t, h_t, "ratio") for i, ((w0, h0), (w_t, h_t)) in enumerate(pc.INTRINSIC_SIZES)])
    Kr = np.roll(Kl, 1, axis=0)
    norm, thr = ops.prepare_norm(Kl, Kr), ops.prepare_thr(Kl, Kr, 0.5)
    assert norm.dtype == np.float32 and thr.dtype == np.float32 and norm.shape == (len(Kl), 8)
    for p in range(len(Kl)):
        assert np.array_equal(norm[p].view(np.uint32), pc.norm32(Kl[p], Kr[p]).view(np.uint32))
        assert np.float32(thr[p]).view(np.uint32) == pc.thr32(Kl[p], Kr[p], 0.5).view(np.uint32)


# ---- refusals without a GPU -------------------------------------------------------------------------------------------------------------
def _entry(ops, **kw):
    e = np.zeros(1, ops._PREPARE_IMAGE)
    v = dict(src=4096, dst=0, h0=40, w0=64, y0=0, x0=12, h_c=40, w_c=40, h_t=32, w_t=32, H=32, W=32, side=0, bgr=0)
    v.update(kw)
    for k, x in v.items():
        e[k] = x
    e["scale_x"] = kw.get("scale_x", 1.0 / (float(v["w_t"]) / float(v["w_c"]))) if v["w_t"] > 0 and v["w_c"] > 0 else 1.0
    e["scale_y"] = kw.get("scale_y", 1.0 / (float(v["h_t"]) / float(v["h_c"]))) if v["h_t"] > 0 and v["h_c"] > 0 else 1.0
    return e


BAD_ENTRIES = {"null src": dict(src=0), "window past the rows": dict(y0=1), "window past the columns": dict(x0=25),
               "negative window origin": dict(x0=-1, w_c=41), "empty window": dict(h_c=0), "target wider than the canvas": dict(w_t=33),
               "target taller than the canvas": dict(h_t=33), "empty target": dict(h_t=0), "canvas not a multiple of 32": dict(W=48),
               "zero canvas": dict(H=0), "canvas past the store": dict(dst=2 * 3072), "negative dst": dict(dst=-3072),
               "canvas off 16 bytes": dict(dst=8), "side": dict(side=2), "bgr": dict(bgr=2), "scale": dict(scale_x=1.5),
               "source above max_side": dict(h0=16385), "canvas above max_side": dict(W=16416)}


def test_the_library_refuses_bad_arguments_without_a_gpu(ops):
    from pats_amd import _lib
    lib = _lib.lib()
    assert ops.prepare_images_max_side() == 16384
    assert ops._PREPARE_IMAGE.itemsize == 80 and ops._PREPARE_IMAGE.fields["h0"][1] == 32
    P = ctypes.c_void_p

    def call(e, images=4096, left=4096, right=8192, n=1, elems=2 * 3072, dtype=3, host=True):
        return lib.pats_prepare_images_u8(P(e.ctypes.data) if host else None, P(images), n, P(left), elems, P(right), elems, dtype, None)

    good = _entry(ops)
    for what, kw in (("null images_host", dict(host=False)), ("null images", dict(images=0)), ("null left", dict(left=0)),
                     ("null right", dict(right=0)), ("left off 16 bytes", dict(left=4104)), ("unknown dtype", dict(dtype=4)),
                     ("negative dtype", dict(dtype=-1)), ("no images", dict(n=0)), ("too many images", dict(n=65536))):
        assert call(good, **kw) == 1, what
        assert b"prepare_images" in lib.pats_last_error(), what
    for what, kw in BAD_ENTRIES.items():
        assert call(_entry(ops, **kw)) == 1, what
        assert b"prepare_images: image 0" in lib.pats_last_error(), what


def test_ops_refuse_bad_sources_without_a_gpu(ops):
    pl = ops.prepare_plan([((40, 64), (40, 64))], targets=(32, 32))
    ok = torch.zeros(40, 64, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prepare_table([(ok, ok)], pl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prepare_images([(ok, ok)], pl, torch.zeros(3072, dtype=torch.uint8), torch.zeros(3072, dtype=torch.uint8))
    for bad, what in ((ok.float(), "uint8"), (torch.zeros(40, 64, 4, dtype=torch.uint8), "uint8"), (torch.zeros(40, 64, dtype=torch.uint8), "uint8"),
                      (torch.zeros(40, 3, 64, dtype=torch.uint8).permute(0, 2, 1), "contiguous"),
                      (torch.zeros(80, 64, 3, dtype=torch.uint8)[::2], "contiguous")):
        with pytest.raises(RuntimeError, match=what):
            ops.prepare_table([(bad, ok)], pl)
    with pytest.raises(RuntimeError):
        ops.prepare_table([(ok,)], pl)
    with pytest.raises(RuntimeError):
        ops.prepare_table([(ok, ok), (ok, ok)], pl)


def test_pack_raw_pairs_refuses_bad_arguments_without_a_gpu(ops):
    from pats_amd import batch
    img = torch.zeros(40, 64, 3, dtype=torch.uint8)
    K = np.eye(3)
    with pytest.raises(ValueError, match="does not fit"):
        batch.pack_raw_pairs([(img, img)], targets=(64, 40), canvas=(32, 64))
    with pytest.raises(ValueError, match="K must hold"):
        batch.pack_raw_pairs([(img, img)], targets=(32, 32), K=[(K, None)])
    with pytest.raises(ValueError, match="K must hold"):
        batch.pack_raw_pairs([(img, img), (img, img)], targets=(32, 32), K=[(K, K)])
    with pytest.raises(ValueError):
        batch.pack_raw_pairs([], size=64)
    with pytest.raises(ValueError, match="mode"):
        batch.pack_raw_pairs([(img, img)], targets=(32, 32), K=[(K, K)], intrinsics="both")
