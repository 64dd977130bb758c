"""The subdivision gather's crops on uint8 / float16 / bfloat16 images and in the fine backbone's format (ops.CropFormat,
pats_left_crops_typed / pats_tensor_resize_hwc_typed / pats_tensor_resize_typed).  The contract, checked with torch.equal:
  * fp32 crops of typed images are the float32 kernels' crops of images.float(), bit for bit (uniform, device-count and
    ragged batches, zero-padded borders and the images at the end of a ragged store included);
  * a formatted crop is the torch composition of the fp32 crop: permute (chw), .float(), (x - mean) / std, .to(dtype) -
    on the GPU and on the CPU;
  * out= buffers receive exactly the crops of separate allocations, and rows past the device-side count stay untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from pats_amd import synth

pytestmark = pytest.mark.gpu

HALF = (torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def ops():
    from pats_amd import build
    build.build()
    from pats_amd import ops as o
    return o


def images(n, H, W, dtype, seed):
    """seeded images: integers 0..255 for uint8 / float16, bf16-rounded normals (any sign, fractions) for bfloat16."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bfloat16:
        x = (torch.randn((n, H, W, 3), generator=g) * 300.0).to(torch.bfloat16)
    else:
        x = torch.randint(0, 256, (n, H, W, 3), generator=g).to(dtype)
    return x.cuda()


def cell_inputs(n, h, w, seed):
    """Compute_imgs inputs of n images on an h x w grid: points anywhere in and just around the image (crops that reach into the
    zero margin), scales 0.3..2.5, a third of the cells without a match."""
    rng = np.random.default_rng(seed)
    N = h * w
    ap = np.stack([rng.uniform(-1.0, h + 1.0, (n, N)), rng.uniform(-1.0, w + 1.0, (n, N))], -1).astype(np.float32)
    xs = rng.uniform(0.3, 2.5, (n, N)).astype(np.float32)
    ys = rng.uniform(0.3, 2.5, (n, N)).astype(np.float32)
    ifn = rng.random((n, N)) < 0.33
    cu = lambda a: torch.from_numpy(a).cuda()
    return cu(xs), cu(ys), cu(ap), cu(ifn)


def compose(c, fmt):
    """The reference's glue on fp32 HWC crops (second_layer.py:66-68): permute, .float(), Normalize, then the cast."""
    x = c.permute(0, 3, 1, 2) if fmt.layout == "chw" else c
    x = x.float()
    if fmt.normalize:
        shape = (1, 3, 1, 1) if fmt.layout == "chw" else (1, 1, 1, 3)
        x = (x - torch.tensor(fmt.mean, dtype=torch.float32, device=x.device).view(shape)) / \
            torch.tensor(fmt.std, dtype=torch.float32, device=x.device).view(shape)
    return x.to(fmt.dtype).contiguous()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


# ---- fp32 crops of typed images ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.uint8, torch.float16, torch.bfloat16])
def test_fp32_crops_of_typed_images_host_count(ops, dt):
    h, w = 15, 20
    l, r = images(2, 32 * h, 32 * w, dt, 11), images(2, 32 * h, 32 * w, dt, 12)
    inp = cell_inputs(2, h, w, 13)
    got = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h)
    want = ops.Compute_imgs_ex(*inp, l.float(), r.float(), width=w, height=h)
    K = want[1].shape[0]
    assert K > 0
    # new_left keeps left.dtype on this path, as it always did: today's fp32 crops .to(left.dtype), now written directly
    assert same(got[0], want[0].to(dt)) and same(got[0].float(), want[0])
    assert same(got[1], want[1])
    assert all(same(a, b) for a, b in zip(got[2:], want[2:]))


@pytest.mark.parametrize("dt", [torch.uint8, torch.float16, torch.bfloat16])
def test_fp32_crops_of_typed_images_device_count(ops, dt):
    h, w = 15, 20
    l, r = images(3, 32 * h, 32 * w, dt, 21), images(3, 32 * h, 32 * w, dt, 22)
    inp = cell_inputs(3, h, w, 23)
    got = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, known_count="device")
    want = ops.Compute_imgs_ex(*inp, l.float(), r.float(), width=w, height=h, known_count="device")
    K = int(want[7].item())
    assert same(got[7], want[7]) and same(got[6], want[6]) and 0 < K < 3 * h * w
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32
    assert same(got[0][:K], want[0][:K]) and same(got[1][:K], want[1][:K])


def _ragged(ops, dt, fmt=None, seed=31):
    from pats_amd import batch
    shapes = [(15, 20), (5, 6), (8, 10), (4, 12)]            # the last slot's image ends the store
    pairs = [(images(1, 32 * h, 32 * w, dt, seed + 2 * i)[0], images(1, 32 * h, 32 * w, dt, seed + 2 * i + 1)[0])
             for i, (h, w) in enumerate(shapes)]
    pk_t, pk_f = batch.pack_pairs(pairs, keep_dtype=True), batch.pack_pairs(pairs)
    assert pk_t.left.dtype == dt and pk_f.left.dtype == torch.float32 and same(pk_t.left.float(), pk_f.left)
    per = [cell_inputs(1, h, w, seed + 100 + i) for i, (h, w) in enumerate(pk_t.shapes)]
    inp = [torch.cat([p[k].reshape(-1) if k != 2 else p[k].reshape(-1, 2) for p in per]) for k in range(4)]
    got = ops.Compute_imgs_ragged(*inp, pk_t.left, pk_t.right, pk_t.table, crop_format=fmt)
    want = ops.Compute_imgs_ragged(*inp, pk_f.left, pk_f.right, pk_f.table)
    return got, want, int(want[7].item())


@pytest.mark.parametrize("dt", [torch.uint8, torch.float16, torch.bfloat16])
def test_fp32_crops_of_typed_images_ragged(ops, dt):
    got, want, K = _ragged(ops, dt)
    assert K > 0 and same(got[7], want[7])
    assert same(got[0][:K], want[0][:K]) and same(got[1][:K], want[1][:K])


# ---- output formats ---------------------------------------------------------------------------------------------------
FORMATS = [(d, lay, norm) for d in HALF for lay in ("hwc", "chw") for norm in (False, True)] + \
          [(torch.float32, "chw", False), (torch.float32, "chw", True), (torch.float32, "hwc", True)]


def _fmt(ops, d, lay, norm):
    return ops.CropFormat(d, lay, *((ops.CropFormat.BACKBONE_MEAN, ops.CropFormat.BACKBONE_STD) if norm else (None, None)))


@pytest.mark.parametrize("d, lay, norm", FORMATS)
@pytest.mark.parametrize("src", [torch.uint8, torch.float32])
def test_formats_equal_the_torch_composition(ops, d, lay, norm, src):
    h, w = 15, 20
    fmt = _fmt(ops, d, lay, norm)
    l = images(2, 32 * h, 32 * w, torch.uint8, 41).to(src)
    r = images(2, 32 * h, 32 * w, torch.uint8, 42).to(src)
    inp = cell_inputs(2, h, w, 43)
    base = ops.Compute_imgs_ex(*inp, l.float(), r.float(), width=w, height=h, known_count="device")
    got = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, known_count="device", crop_format=fmt)
    K = int(base[7].item())
    for side in (0, 1):
        assert got[side].dtype == d and tuple(got[side].shape) == fmt.shape(2 * h * w)
        c = base[side][:K]
        want_gpu, want_cpu = compose(c, fmt), compose(c.cpu(), fmt)
        assert same(got[side][:K], want_gpu), (side, fmt)
        assert same(got[side][:K], want_cpu), (side, fmt)
    # the host-count path and the ragged path write the same format
    got_h = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, crop_format=fmt)
    assert same(got_h[0], got[0][:K]) and same(got_h[1], got[1][:K])


@pytest.mark.parametrize("d", HALF)
def test_ragged_backbone_format(ops, d):
    from pats_amd import ops as o
    fmt = o.CropFormat.backbone(d)
    got, want, K = _ragged(ops, torch.uint8, fmt, seed=51)
    assert same(got[0][:K], compose(want[0][:K], fmt)) and same(got[1][:K], compose(want[1][:K], fmt))


def test_uint8_left_crops_written_as_uint8(ops):
    h, w = 15, 20
    l, r = images(2, 32 * h, 32 * w, torch.uint8, 61), images(2, 32 * h, 32 * w, torch.uint8, 62)
    inp = cell_inputs(2, h, w, 63)
    today = ops.Compute_imgs(*inp, l.float(), r.float(), width=w, height=h)[0].to(torch.uint8)   # the parent's new_left
    assert same(ops.Compute_imgs(*inp, l, r, width=w, height=h)[0], today)
    for lay in ("hwc", "chw"):
        fmt = ops.CropFormat(torch.uint8, lay)
        nl, nr = ops.Compute_imgs(*inp, l, r, width=w, height=h, crop_format=fmt)[:2]
        assert same(nl, today if lay == "hwc" else today.permute(0, 3, 1, 2).contiguous())
        base = ops.Compute_imgs(*inp, l.float(), r.float(), width=w, height=h)[1]
        assert same(nr, compose(base, ops.CropFormat(torch.float32, lay)))          # the right side stays float32
    with pytest.raises(RuntimeError, match="uint8 crops need uint8 images"):
        ops.Compute_imgs(*inp, l.half(), r.half(), width=w, height=h, crop_format=ops.CropFormat(torch.uint8))


# ---- out= ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [torch.bfloat16, torch.float32])
def test_out_views_of_one_stacked_buffer(ops, d):
    h, w = 15, 20
    fmt = ops.CropFormat.backbone(d)
    l, r = images(2, 32 * h, 32 * w, torch.uint8, 71), images(2, 32 * h, 32 * w, torch.uint8, 72)
    inp = cell_inputs(2, h, w, 73)
    cap = 2 * h * w
    sent = torch.tensor(-7.25, dtype=d)
    buf = torch.full((2, cap, 3, 96, 96), float(sent), dtype=d, device="cuda")
    sep = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, known_count="device", crop_format=fmt)
    got = ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, known_count="device", crop_format=fmt, out=(buf[0], buf[1]))
    K = int(sep[7].item())
    assert 0 < K < cap
    assert got[0].data_ptr() == buf[0].data_ptr() and got[1].data_ptr() == buf[1].data_ptr()
    assert same(buf[0][:K], sep[0][:K]) and same(buf[1][:K], sep[1][:K])
    assert bool((buf[:, K:] == sent.cuda()).all())              # rows past the device-side K_total: untouched
    stacked = buf.view(2 * cap, 3, 96, 96)
    assert same(stacked[cap:cap + K], sep[1][:K])
    # host-count path: the first K rows of a larger buffer
    buf2 = torch.full((2, cap, 3, 96, 96), float(sent), dtype=d, device="cuda")
    nl, nr = ops.Compute_imgs(*inp, l, r, width=w, height=h, crop_format=fmt, out=(buf2[0], buf2[1]))[:2]
    assert nl.shape[0] == K and same(nl, sep[0][:K]) and same(nr, sep[1][:K]) and bool((buf2[:, K:] == sent.cuda()).all())
    with pytest.raises(RuntimeError, match="out\\[0\\]"):
        ops.Compute_imgs_ex(*inp, l, r, width=w, height=h, known_count="device", crop_format=fmt,
                            out=(torch.empty((cap, 96, 96, 3), dtype=d, device="cuda"), None))


# ---- tensor_resize ------------------------------------------------------------------------------------------------------
def _ext():
    import importlib.machinery
    import importlib.util
    from pats_amd import build
    path = build.build_tensor_resize_ext()
    loader = importlib.machinery.ExtensionFileLoader("tensor_resize", path)
    spec = importlib.util.spec_from_file_location("tensor_resize", path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("d", HALF)
def test_tensor_resize_on_half_inputs(ops, d):
    g = golden("resize_small.npz")
    src, bound = torch.from_numpy(g["src"]).cuda().to(d), torch.from_numpy(g["bound"]).cuda()
    rng = np.random.default_rng(81)
    big = torch.from_numpy(rng.uniform(0, 255, (2, 3, 200, 240)).astype(np.float32)).cuda().to(d)
    y0 = rng.integers(0, 150, 64)
    x0 = rng.integers(0, 190, 64)
    b2 = torch.from_numpy(np.stack([y0, y0 + rng.integers(1, 50, 64), x0, x0 + rng.integers(0, 49, 64),
                                    rng.integers(0, 2, 64) * 10000 + np.arange(64)], 1).astype(np.int64)).cuda()
    ext = _ext()
    for s, b in ((src, bound), (big, b2)):
        want = ops.tensor_resize(s.float(), b)
        for fn in (ops.tensor_resize, ext.tensor_resize):
            got = fn(s, b)
            assert got.dtype == torch.float32 and same(got, want)
    empty = torch.zeros((0, 5), dtype=torch.int64, device="cuda")
    for fn in (ops.tensor_resize, ext.tensor_resize):
        e = fn(src, empty)
        assert e.shape == (0, 3, 96, 96) and e.dtype == torch.float32
        with pytest.raises(RuntimeError, match="float32"):
            fn(src.double(), bound)
        bad = torch.cat([bound, torch.tensor([[0, 0, 0, 4, 0]], dtype=torch.int64, device="cuda")])   # an empty crop
        with pytest.raises(RuntimeError, match="empty or outside"):
            fn(src, bad)
        with pytest.raises(RuntimeError, match="empty or outside"):
            fn(src.float(), bad)


# ---- batch --------------------------------------------------------------------------------------------------------------
def test_forward_pairs_with_uint8_images_and_the_backbone_format(ops):
    from pats_amd import batch
    from test_batch_gpu import _BatchNets

    class Rec(_BatchNets):
        def fine(self, rows, new_left, new_right):
            self.crops = (new_left.clone(), new_right.clone())
            # a backbone that widens the crops back: here the stand-in descriptors do not read them at all
            return super().fine(rows, new_left.float(), new_right.float())

    h, w = 15, 20
    nets = [synth.SynthNets(seed=synth.SEED + 40 + 1000 * i, h=h, w=w) for i in range(2)]
    lefts, rights = images(2, 32 * h, 32 * w, torch.uint8, 91), images(2, 32 * h, 32 * w, torch.uint8, 92)
    cap = batch.Capacities(2, h, w)
    fmt = ops.CropFormat.backbone(torch.bfloat16)
    ra, rb = Rec(nets), Rec(nets)
    a = batch.forward_pairs(lefts.float(), rights.float(), ra, cap)
    b = batch.forward_pairs(lefts, rights, rb, cap, crop_format=fmt)
    K = int(a["K_img"].sum().item())
    assert K > 0 and same(a["K_img"], b["K_img"])
    assert rb.crops[0].dtype == torch.bfloat16 and tuple(rb.crops[0].shape) == (2 * h * w, 3, 96, 96)
    assert same(rb.crops[0][:K], compose(ra.crops[0][:K], fmt)) and same(rb.crops[1][:K], compose(ra.crops[1][:K], fmt))
    M = int(a["M"].item())
    assert same(a["M"], b["M"]) and same(a["matches_l"][:M], b["matches_l"][:M]) and same(a["matches_r"][:M], b["matches_r"][:M])
    assert batch.split_by_pair(a, cap).__len__() == 2


# ---- a fresh process ----------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, torch
sys.path.insert(0, %(repo)r)
from pats_amd import ops
g = torch.Generator().manual_seed(5)
l = torch.randint(0, 256, (2, 480, 640, 3), generator=g).to(torch.uint8).cuda()
r = torch.randint(0, 256, (2, 480, 640, 3), generator=g).to(torch.uint8).cuda()
xs = (torch.rand((2, 300), generator=g) * 2 + 0.3).cuda(); ys = (torch.rand((2, 300), generator=g) * 2 + 0.3).cuda()
ap = torch.stack([torch.rand((2, 300), generator=g) * 17 - 1, torch.rand((2, 300), generator=g) * 22 - 1], -1).cuda()
ifn = (torch.rand((2, 300), generator=g) < 0.3).cuda()
fmt = ops.CropFormat.backbone(torch.bfloat16)
got = ops.Compute_imgs_ex(xs, ys, ap, ifn, l, r, known_count="device", crop_format=fmt)     # the first launches of the process
base = ops.Compute_imgs_ex(xs, ys, ap, ifn, l.float(), r.float(), known_count="device")
K = int(base[7].item())
ok = True
for s in (0, 1):
    c = base[s][:K].permute(0, 3, 1, 2).float()
    m = torch.tensor(fmt.mean, device="cuda").view(1, 3, 1, 1); v = torch.tensor(fmt.std, device="cuda").view(1, 3, 1, 1)
    ok = ok and torch.equal(got[s][:K], ((c - m) / v).to(torch.bfloat16))
t = ops.tensor_resize(l.permute(0, 3, 1, 2).contiguous().half(), base[5][:K].clone(), validate=False)
ok = ok and torch.equal(t, ops.tensor_resize(l.permute(0, 3, 1, 2).contiguous().float(), base[5][:K].clone(), validate=False))
print("FIRST_LAUNCH_OK" if ok and K > 0 else "FIRST_LAUNCH_BAD %%d" %% K)
"""


def test_typed_crops_exact_from_the_first_launch_of_a_process(ops):
    env = dict(os.environ)
    env.pop("PATS_CROPS_NT", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "FIRST_LAUNCH_OK" in r.stdout, r.stdout[-2000:]
