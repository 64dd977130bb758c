"""GPU: ops.prepare_images / batch.pack_raw_pairs against the definition of include/pats_amd.h ("Image front end") restated in numpy
(tests/prepare_cases.py) - every output bit-equal to the restatement.
    stores       views inside sentinel-filled buffers: the surroundings must not change, and every element of every canvas is written
                 (the views start out as sentinels too)
    sources      views at an odd offset inside buffers that hold 255, and 255 everywhere outside the crop window: a tap taken outside
                 the window shows as a wrong value, not as a fault
    tile edges   PREP_THREADS and PREP_LANE_BYTES are read from csrc/prepare.hip; canvases whose rows are one 32-px step below, at
                 and above a multiple of a workgroup's span of PREP_THREADS * PREP_LANE_BYTES bytes
Nothing here claims parity with an OpenCV build (see the header)."""
import os
import re

import numpy as np
import pytest
import torch

import prepare_cases as pc
from conftest import REPO

pytestmark = pytest.mark.gpu

PAD = 4096                                              # elements around a store view (a multiple of 16 bytes in every dtype)
SRC_PAD = 4099                                          # bytes around a source view: sources need no alignment
DTYPES = {"uint8": torch.uint8, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SENTINEL = {torch.uint8: 0xA5, torch.float32: -777.25, torch.float16: -777.0, torch.bfloat16: -776.0}


def _kernel_constant(name):
    src = open(os.path.join(REPO, "pats_amd", "csrc", "prepare.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


SPAN = _kernel_constant("PREP_THREADS") * _kernel_constant("PREP_LANE_BYTES")      # bytes of a canvas one workgroup writes


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def batch():
    from pats_amd import batch
    return batch


def source(img):
    """A raw image as a contiguous [h, w, 3] view at an odd offset inside a buffer of 255s."""
    img = np.ascontiguousarray(img)
    buf = torch.full((img.size + 2 * SRC_PAD,), 255, dtype=torch.uint8, device="cuda")
    view = buf[SRC_PAD:SRC_PAD + img.size].view(img.shape)
    view.copy_(torch.from_numpy(img))
    return view


def windowed_pair(seed, plan, p):
    """Pair p's two images (numpy) for a plan: seeded content inside the crop windows, 255 outside."""
    return tuple(pc.image(seed + s, int(plan.h0[p, s]), int(plan.w0[p, s]),
                          tuple(int(getattr(plan, k)[p, s]) for k in ("y0", "x0", "h_c", "w_c"))) for s in range(2))


def stores(elems, dtype):
    """-> (buffers, left view, right view): each view PAD elements inside its own sentinel-filled buffer, itself sentinels."""
    bufs = [torch.full((elems + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device="cuda") for _ in range(2)]
    return bufs, bufs[0][PAD:PAD + elems], bufs[1][PAD:PAD + elems]


def surroundings_unchanged(bufs, elems):
    for b in bufs:
        around = torch.cat([b[:PAD], b[PAD + elems:]])
        assert bool((around == SENTINEL[b.dtype]).all()), "elements around a store view changed"


def expected_stores(imgs, plan, bgr=False):
    """The restatement's two stores as uint8 numpy arrays."""
    out = [np.zeros(plan.elems, np.uint8), np.zeros(plan.elems, np.uint8)]
    for p, pr in enumerate(imgs):
        H, W = (int(v) for v in plan.canvas[p])
        for s in range(2):
            c = pc.prepare_u8(pr[s], int(plan.w_t[p, s]), int(plan.h_t[p, s]), (H, W), bgr)
            out[s][int(plan.dst[p]):int(plan.dst[p]) + H * W * 3] = c.ravel()
    return out


def assert_stores(got, want_u8):
    """A store of any dtype against uint8 expectations: 0 .. 255 is exact in all four, so equal values are equal bits."""
    want = torch.from_numpy(want_u8).cuda()
    if got.dtype == torch.uint8:
        bad = got != want
    else:
        bad = got.float() != want.float()
    n = int(bad.sum())
    if n:
        i = int(bad.nonzero()[0])
        raise AssertionError("%d of %d elements differ, first at %d: got %s, want %d" % (n, want.numel(), i, got[i].item(), int(want_u8[i])))


def run(ops, imgs, plan, dtype=torch.uint8, bgr=False):
    srcs = [(source(l), source(r)) for l, r in imgs]
    bufs, left, right = stores(plan.elems, dtype)
    ops.prepare_images(srcs, plan, left, right, bgr=bgr)
    torch.cuda.synchronize()
    surroundings_unchanged(bufs, plan.elems)
    return left, right


# ---- single pairs: the smallest shapes at which it can go wrong ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.PLAN_CASES))
def test_plan_cases(ops, name):
    (h0, w0), target = pc.PLAN_CASES[name]
    plan = ops.prepare_plan([((h0, w0), (h0, w0))], targets=target)
    imgs = [windowed_pair(300, plan, 0)]
    want = expected_stores(imgs, plan)
    left, right = run(ops, imgs, plan)
    assert_stores(left, want[0])
    assert_stores(right, want[1])
    if name == "pad":                                   # 33 x 47 on 64 x 64: 3 * w_t is no multiple of 16, a lane straddles image and pad
        c = left.view(64, 64, 3)
        assert tuple(plan.canvas[0]) == (64, 64) and (3 * 47) % 16 != 0
        assert bool((c[33:] == 0).all()) and bool((c[:, 47:] == 0).all()) and bool((c[:33, :47] != 0).any())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("step", [-1, 0, 1])
def test_rows_around_a_workgroup_span(ops, dtype, step):
    dt = DTYPES[dtype]
    esize = torch.empty((), dtype=dt).element_size()
    W_at = next(W for W in range(32, 1 << 16, 32) if (W * 3 * esize) % SPAN == 0)
    W = W_at + 32 * step
    assert W >= 64
    w_t, h_t = W - 5, 30                                 # one canvas row = W * 3 * esize bytes; 32 rows, the last two pad
    plan = ops.prepare_plan([((16, W // 2), (9, W // 3))], targets=(w_t, h_t))
    assert tuple(plan.canvas[0]) == (32, W)
    imgs = [windowed_pair(500 + step, plan, 0)]
    want = expected_stores(imgs, plan)
    left, right = run(ops, imgs, plan, dtype=dt)
    assert_stores(left, want[0])
    assert_stores(right, want[1])


# ---- the mixed batch -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ops):
    imgs = pc.mixed_sources()
    plan = ops.prepare_plan(pc.MIXED_SIZES, size=pc.MIXED_SIZE)
    return imgs, plan, expected_stores(imgs, plan)


def test_mixed_batch_is_what_it_is_meant_to_be(mixed):
    imgs, plan, _ = mixed
    assert len(imgs) == 5 and len({im.shape for pr in imgs for im in pr}) >= 4
    assert list(plan.caller_of) != sorted(plan.caller_of) and len(set(plan.shapes)) >= 3
    own = [[(pc.ceil32(int(plan.h_t[p, s])), pc.ceil32(int(plan.w_t[p, s]))) for s in range(2)] for p in range(5)]
    assert any(a != b for a, b in own)                  # a pair whose images would have different canvases: the maximum applies
    for p in range(5):
        assert tuple(plan.canvas[p]) == (max(own[p][0][0], own[p][1][0]), max(own[p][0][1], own[p][1][1]))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_mixed_batch_in_every_dtype(ops, mixed, dtype):
    imgs, plan, want = mixed
    left, right = run(ops, imgs, plan, dtype=DTYPES[dtype])
    assert_stores(left, want[0])
    assert_stores(right, want[1])


def test_mixed_batch_bgr(ops, mixed):
    imgs, plan, want = mixed
    swapped = expected_stores(imgs, plan, bgr=True)
    assert not np.array_equal(swapped[0], want[0])
    left, right = run(ops, imgs, plan, bgr=True)
    assert_stores(left, swapped[0])
    assert_stores(right, swapped[1])


def test_mixed_batch_on_a_fixed_canvas(ops, mixed):
    imgs = mixed[0]
    plan = ops.prepare_plan(pc.MIXED_SIZES, size=pc.MIXED_SIZE, canvas=(96, 128))
    assert plan.shapes == [(3, 4)] * 5 and list(plan.caller_of) == list(range(5))
    want = expected_stores(imgs, plan)
    left, right = run(ops, imgs, plan, dtype=torch.float16)
    assert_stores(left, want[0])
    assert_stores(right, want[1])


def test_two_calls_give_the_same_bits(ops, mixed):
    imgs, plan, _ = mixed
    a = run(ops, imgs, plan, dtype=torch.bfloat16)
    b = run(ops, imgs, plan, dtype=torch.bfloat16)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))


def test_graph_capture_replays_to_the_same_bits(ops, mixed):
    imgs, plan, want = mixed
    srcs = [(source(l), source(r)) for l, r in imgs]
    table = ops.prepare_table(srcs, plan)               # made before the capture: the captured call allocates and uploads nothing
    bufs, left, right = stores(plan.elems, torch.uint8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.prepare_images(srcs, plan, left, right, table=table)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert_stores(left, want[0])
    g = torch.cuda.CUDAGraph()                          # one kernel node: no parallel branches
    with torch.cuda.graph(g, stream=s):
        ops.prepare_images(srcs, plan, left, right, table=table)
    for b in bufs:
        b.fill_(SENTINEL[torch.uint8])
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    surroundings_unchanged(bufs, plan.elems)
    assert_stores(left, want[0])
    assert_stores(right, want[1])
    del g


# ---- the pack --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "bfloat16"])
def test_pack_raw_pairs_equals_pack_pairs_of_the_restated_images(ops, batch, mixed, dtype):
    imgs, plan, _ = mixed
    dt = DTYPES[dtype]
    pk = batch.pack_raw_pairs([(source(l), source(r)) for l, r in imgs], size=pc.MIXED_SIZE, dtype=dt)
    prepared = []
    for p, pr in enumerate(imgs):
        canvas = tuple(int(v) for v in plan.canvas[p])
        prepared.append(tuple(torch.from_numpy(pc.prepare_u8(pr[s], int(plan.w_t[p, s]), int(plan.h_t[p, s]), canvas)).cuda().to(dt)
                              for s in range(2)))
    ref = batch.pack_pairs(prepared, keep_dtype=True)
    assert pk.shapes == ref.shapes and pk.slot_of == ref.slot_of and pk.caller_of == ref.caller_of
    assert pk.left.dtype == dt and pk.left.shape == ref.left.shape
    bits = torch.uint8 if dt == torch.uint8 else torch.int16
    assert torch.equal(pk.left.view(bits), ref.left.view(bits)) and torch.equal(pk.right.view(bits), ref.right.view(bits))
    for name in ("shape_host", "cell_base_host", "img_base_host"):
        assert np.array_equal(getattr(pk.table, name), getattr(ref.table, name)), name
    for name in ("shape", "cell_base", "img_base"):
        assert torch.equal(getattr(pk.table, name), getattr(ref.table, name)), name
    assert (pk.table.pairs, pk.table.cells, pk.table.hmax) == (ref.table.pairs, ref.table.cells, ref.table.hmax)
    assert len(pk.groups) == len(ref.groups) >= 3
    for a, b in zip(pk.groups, ref.groups):
        assert a[:4] == b[:4] and a[4].shape == b[4].shape
        assert torch.equal(a[4].view(bits), b[4].view(bits)) and torch.equal(a[5].view(bits), b[5].view(bits))
        assert a[4].data_ptr() == pk.left.data_ptr() + int(pk.table.img_base_host[a[0]]) * pk.left.element_size()
    assert pk.norm is None and pk.thr is None and pk.K_left is None
    for k in ("h_t", "w_t", "y0", "x0", "h_c", "w_c"):
        assert np.array_equal(getattr(pk.plan, k), getattr(plan, k))


def _mixed_K():
    out = []
    for p, pr in enumerate(pc.MIXED_SIZES):
        rng = np.random.default_rng(8800 + p)
        Ks = []
        for h0, w0 in pr:
            f = rng.uniform(0.8, 1.4) * max(h0, w0)
            Ks.append(np.array([[f, 0.0, w0 / 2 + rng.uniform(-3, 3)], [0.0, f * rng.uniform(0.98, 1.02), h0 / 2 + rng.uniform(-3, 3)],
                                [0.0, 0.0, 1.0]]))
        out.append(tuple(Ks))
    return out


@pytest.mark.parametrize("mode", ["ratio", "axes"])
def test_norm_and_thr(ops, batch, mixed, mode):
    imgs, plan, _ = mixed
    K = _mixed_K()
    pk = batch.pack_raw_pairs([(source(l), source(r)) for l, r in imgs], size=pc.MIXED_SIZE, K=K, intrinsics=mode, threshold=0.5)
    sides = []
    for s in range(2):
        sides.append(np.stack([pc.intrinsics64(K[p][s], int(plan.h0[p, s]), int(plan.w0[p, s]), int(plan.w_t[p, s]), int(plan.h_t[p, s]), mode)
                               for p in range(5)]))
    assert np.array_equal(pk.K_left, sides[0]) and np.array_equal(pk.K_right, sides[1]) and pk.K_left.dtype == np.float64
    norm = np.stack([pc.norm32(sides[0][p], sides[1][p]) for p in range(5)])
    thr = np.array([pc.thr32(sides[0][p], sides[1][p], 0.5) for p in range(5)], np.float32)
    assert pk.norm.is_cuda and pk.norm.dtype == torch.float32 and pk.thr.is_cuda and pk.thr.dtype == torch.float32
    assert np.array_equal(pk.norm.cpu().numpy().view(np.uint32), norm.view(np.uint32))
    assert np.array_equal(pk.thr.cpu().numpy().view(np.uint32), thr.view(np.uint32))

    # a handful of synthetic matches per pair, in pixels of the prepared images, (row, column) order as the pipeline emits them: a
    # planted two-view scene plus outliers.  The verification counts the same inliers with pk.norm as with a norm built by hand
    n, rng = 24, np.random.default_rng(8900)
    ml, mr, models = np.zeros((5, n, 2), np.float32), np.zeros((5, n, 2), np.float32), np.zeros((5, 3, 3, 3), np.float32)
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for p in range(5):
        ang, axis = 0.2, np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
        A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A
        t = np.array([1.0, 0.1, 0.05])
        X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 8, n)], 1)
        Y = X @ R.T + t
        for pts, Kp, dst in ((X, sides[0][p], ml), (Y, sides[1][p], mr)):
            xn, yn = pts[:, 0] / pts[:, 2], pts[:, 1] / pts[:, 2]
            dst[p, :, 0], dst[p, :, 1] = yn * Kp[1, 1] + Kp[1, 2], xn * Kp[0, 0] + Kp[0, 2]
        mr[p, 18:] += rng.uniform(5, 20, (n - 18, 2)).astype(np.float32)            # six outliers
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        M = swap @ E @ swap                                                        # the model of the (row, column, 1) points
        models[p, 1] = M / np.linalg.norm(M)
        models[p, 0] = rng.normal(size=(3, 3))
        models[p, 2] = np.eye(3)
    cu = lambda a: torch.from_numpy(a).cuda()
    counts = torch.full((5,), n, dtype=torch.int64, device="cuda")
    by_hand = np.zeros((5, 8), np.float32)
    for p in range(5):
        for s in range(2):
            Kp = sides[s][p]
            by_hand[p, 4 * s:4 * s + 4] = (Kp[1, 2], Kp[0, 2], 1.0 / Kp[1, 1], 1.0 / Kp[0, 0])
    res = [ops.epipolar_score_by_pair(cu(ml), cu(mr), cu(models), pk.thr * 0.01, stride=n, counts=counts, norm=nm)
           for nm in (pk.norm, cu(by_hand))]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][3], res[1][3])
    got = res[0][0].cpu().numpy()
    assert (got[:, 1] >= 18).all() and (got[:, 1] < n).all() and (res[0][1].cpu().numpy() == 1).all()
