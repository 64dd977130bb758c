"""-m gpu: the point-tiled NCHW third-level gather (third_desc_kernel: a tile of consecutive points per workgroup, outputs staged in
LDS and written as linear spans).  Every output - both descriptor tensors, p_s and p_t - must equal, bit for bit, the per-point
kernel (ops.set_third_gather("point")), the channels-last gather and, where the reference's indices stay inside the tensors,
the CPU oracle: sorted rows of many sizes, tiles that straddle rows, unsorted / repeated rows, a repeated point, point counts
that are not a multiple of the tile, device-side counts (nothing past the count is written), the clamp / wrap paths at the
borders and the first / last image, misaligned outputs, and the golden fixtures."""
import numpy as np
import pytest
import torch

from conftest import golden
from pats_amd import synth

pytestmark = pytest.mark.gpu

M = 52


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    assert o.set_third_gather("tile") == "tile"          # the default
    return o


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cl(a):
    return cu(a).contiguous(memory_format=torch.channels_last)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def call(ops, d, fmt=cu, **kw):
    return ops.third_descriptors(fmt(d["ff0"]), fmt(d["ff1"]), cu(d["mk0"]), cu(d["mk1"]), cu(d["b_ids"]), cu(d["kenc"]),
                                 cu(d["rubbish"]), **kw)


def point_kernel(ops, d, **kw):
    prev = ops.set_third_gather("point")
    try:
        out = call(ops, d, **kw)
        torch.cuda.synchronize()
        return out
    finally:
        ops.set_third_gather(prev)


def check(ops, oracle, d, with_oracle=True):
    """tiled NCHW == per-point NCHW == channels-last (== oracle): every output, bit for bit."""
    got = call(ops, d)
    for name, ref in (("point", point_kernel(ops, d)), ("channels_last", call(ops, d, fmt=cl))):
        for i, (a, b) in enumerate(zip(got, ref)):
            assert same(a, b), "output %d differs from the %s kernel" % (i, name)
    if with_oracle:
        want = oracle.third_descriptors(d["ff0"], d["ff1"], d["mk0"], d["mk1"], d["b_ids"], d["kenc"], d["rubbish"])
        for a, w in zip(got, want):
            a = a.cpu().numpy()
            assert a.shape == w.shape
            np.testing.assert_array_equal(a.view(np.uint32 if w.dtype == np.float32 else w.dtype),
                                          w.view(np.uint32 if w.dtype == np.float32 else w.dtype))
    return got


def maps(rng, B):
    ff0, ff1 = rng.standard_normal((2, B, 128, M, M)).astype(np.float32)
    rub = rng.standard_normal((B, 128, 144)).astype(np.float32)
    rub[0, :5, :] = -0.0
    return {"ff0": ff0, "ff1": ff1, "kenc": rng.standard_normal((128, 64)).astype(np.float32), "rubbish": rub}


def row_points(rng, rows, inner=True):
    """Points in the scan order of third_inputs_kernel: per fine row (b), k distinct source cells in increasing order."""
    mk0, b_ids = [], []
    for b, k in rows:
        lo, hi = (1, 11) if inner else (0, 12)
        cells = np.sort(rng.choice((hi - lo) ** 2, size=k, replace=False))
        y, x = lo + cells // (hi - lo), lo + cells % (hi - lo)
        mk0 += [[8 * xx + 4, 8 * yy + 4] for xx, yy in zip(x, y)]
        b_ids += [b] * k
    P = len(b_ids)
    mk1 = (rng.integers(-8, 209, size=(P, 2)) * 0.5).astype(np.float32)        # -4.0 .. 104.0: clamped to [0, 96]
    return np.asarray(mk0, np.float32), mk1, np.asarray(b_ids, np.int64)


def test_sorted_rows_of_many_sizes(ops, oracle):
    """rows of 1, 2, 5, 17 and 144 points (the whole 12 x 12 grid, border ring included): tiles straddle every row boundary"""
    rng = np.random.default_rng(71)
    d = maps(rng, 7)
    rows = [(1, 1), (2, 2), (3, 5), (4, 17), (5, 144)]
    d["mk0"], d["mk1"], d["b_ids"] = row_points(rng, rows[:4])
    m5, k5, b5 = row_points(rng, rows[4:], inner=False)
    d["mk0"], d["mk1"], d["b_ids"] = (np.concatenate([d["mk0"], m5]), np.concatenate([d["mk1"], k5]),
                                     np.concatenate([d["b_ids"], b5]))
    assert d["b_ids"].size == 169
    check(ops, oracle, d)


def test_rows_in_reverse_and_ones(ops, oracle):
    rng = np.random.default_rng(72)
    d = maps(rng, 6)
    d["mk0"], d["mk1"], d["b_ids"] = row_points(rng, [(4, 17), (3, 1), (2, 5), (1, 1), (2, 2), (4, 1), (3, 9)])
    check(ops, oracle, d)


def test_unsorted_and_repeated_rows(ops, oracle):
    rng = np.random.default_rng(73)
    d = maps(rng, 5)
    P = 203
    d["mk0"] = (rng.integers(1, 11, size=(P, 2)) * 8 + 4).astype(np.float32)
    d["mk1"] = (rng.integers(-8, 209, size=(P, 2)) * 0.5).astype(np.float32)
    d["b_ids"] = rng.integers(1, 4, size=P).astype(np.int64)
    check(ops, oracle, d)


def test_the_same_point_repeated(ops, oracle):
    rng = np.random.default_rng(74)
    d = maps(rng, 3)
    P = 37
    d["mk0"] = np.tile(np.array([[44, 60]], np.float32), (P, 1))
    d["mk1"] = np.tile(np.array([[50.5, 13.0]], np.float32), (P, 1))
    d["b_ids"] = np.ones(P, np.int64)
    got = check(ops, oracle, d)
    assert all(torch.equal(got[0][i], got[0][0]) and torch.equal(got[1][i], got[1][0]) for i in range(P))


@pytest.mark.parametrize("P", [1, 2, 3, 5, 7, 9, 13, 31, 65])
def test_point_counts_not_a_multiple_of_the_tile(ops, oracle, P):
    rng = np.random.default_rng(75 + P)
    d = maps(rng, 4)
    d["mk0"] = (rng.integers(1, 11, size=(P, 2)) * 8 + 4).astype(np.float32)
    d["mk1"] = (rng.integers(0, 193, size=(P, 2)) * 0.5).astype(np.float32)
    d["b_ids"] = np.sort(rng.integers(1, 3, size=P)).astype(np.int64)
    check(ops, oracle, d)


@pytest.mark.parametrize("count", [0, 1, 6, 77, 202, 203])
def test_counted_launch_writes_nothing_past_the_count(ops, oracle, count):
    rng = np.random.default_rng(80)
    d = maps(rng, 5)
    P = 203
    d["mk0"], d["mk1"], d["b_ids"] = row_points(rng, [(1, 40), (2, 63), (3, 100)])
    assert d["b_ids"].size == P
    full = call(ops, d)
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
    for fn in (lambda **kw: call(ops, d, **kw), lambda **kw: point_kernel(ops, d, **kw)):
        out = (torch.full((P, 128, 65), 7.0, device="cuda"), torch.full((P, 128, 65), -3.0, device="cuda"))
        o0, o1, ps, pt = fn(count=cnt, out=out)
        assert o0.data_ptr() == out[0].data_ptr() and o1.data_ptr() == out[1].data_ptr()
        assert same(o0[:count], full[0][:count]) and same(o1[:count], full[1][:count])
        assert same(ps[:count], full[2][:count]) and same(pt[:count], full[3][:count])
        assert bool((o0[count:] == 7.0).all()) and bool((o1[count:] == -3.0).all())


def test_clamp_and_wrap_paths_and_the_outer_images(ops, oracle):
    """right-side points at 0 and 96 (and beyond: clamped), left cells on the border ring (windows wrap into the neighbouring
    row / image), rows 0 and B - 1 of the map tensor (indices leave the tensor: clamped - the oracle, like torch.gather, would
    raise there, so those points are checked against the other two kernels only)"""
    rng = np.random.default_rng(81)
    B = 5
    d = maps(rng, B)
    ring = [[4, 4], [92, 92], [4, 92], [92, 4], [4, 44], [92, 60], [28, 4], [76, 92]]
    right = [[0, 0], [96, 96], [0, 96], [96, 0], [-3, 120], [100, -1], [0, 48], [96, 50]]
    mk0, mk1, b_ids = [], [], []
    for b in range(B):
        for r0 in ring:
            for r1 in right[:5]:
                mk0.append(r0)
                mk1.append(r1)
                b_ids.append(b)
    d["mk0"], d["mk1"], d["b_ids"] = np.asarray(mk0, np.float32), np.asarray(mk1, np.float32), np.asarray(b_ids, np.int64)
    check(ops, oracle, d, with_oracle=False)
    inner = (d["b_ids"] > 0) & (d["b_ids"] < B - 1)
    e = {k: (v[inner] if k in ("mk0", "mk1", "b_ids") else v) for k, v in d.items()}
    check(ops, oracle, e)
    # interior windows of the first and the last image: inside the tensor, the oracle applies
    mk0, mk1, b_ids = row_points(rng, [(0, 21), (B - 1, 19)])
    mk1 = np.clip(mk1, 8, 88)
    e = dict(d, mk0=mk0, mk1=mk1, b_ids=b_ids)
    check(ops, oracle, e)
    # b_ids outside [0, B): both NCHW kernels and the channels-last one clamp alike
    e = dict(d, b_ids=np.where(np.arange(d["b_ids"].size) % 3 == 0, -1, d["b_ids"] + 1).astype(np.int64))
    check(ops, oracle, e, with_oracle=False)


def test_misaligned_outputs_take_the_per_point_kernel(ops, oracle):
    """outputs that are not 16-byte aligned cannot take the linear float4 spans: same bits through the per-point kernel"""
    rng = np.random.default_rng(82)
    d = maps(rng, 4)
    d["mk0"], d["mk1"], d["b_ids"] = row_points(rng, [(1, 11), (2, 6)])
    P = d["b_ids"].size
    n = P * 128 * 65
    buf0, buf1 = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 3, device="cuda")
    out = (buf0[1:].view(P, 128, 65), buf1[3:].view(P, 128, 65))
    got = call(ops, d, out=out)
    want = call(ops, d)
    assert all(same(a, b) for a, b in zip(got, want))
    assert float(buf0[0]) == 0.0 and float(buf1[:3].abs().sum()) == 0.0


@pytest.mark.parametrize("name,make", [("third_desc.npz", synth.third_maps), ("third_desc_ring.npz", synth.third_maps_ring)])
def test_golden_fixtures(ops, oracle, name, make):
    d = make()
    d["kenc"] = d["kenc"].reshape(128, 64)
    g = golden(name)
    o0, o1, ps, pt = check(ops, oracle, d, with_oracle=(name == "third_desc.npz"))
    assert np.array_equal(ps.cpu().numpy(), g["p_s"]) and np.array_equal(pt.cpu().numpy(), g["p_t"])
    np.testing.assert_array_equal(o0.cpu().numpy()[:, ::4, :], g["out0"])
    np.testing.assert_array_equal(o1.cpu().numpy()[:, ::4, :], g["out1"])


def test_bench_shaped_step_inputs(ops, oracle):
    """several thousand points in rows of the bench's sizes (about 5.5 per row), on a capacity larger than the count"""
    rng = np.random.default_rng(83)
    B = 40
    d = maps(rng, B)
    sizes = rng.integers(1, 14, size=B - 2)
    d["mk0"], d["mk1"], d["b_ids"] = row_points(rng, [(b + 1, int(k)) for b, k in enumerate(sizes)])
    check(ops, oracle, d)
    P = d["b_ids"].size
    cnt = torch.tensor([P - 5], dtype=torch.int64, device="cuda")
    full = call(ops, d)
    out = (torch.full((P, 128, 65), 1.5, device="cuda"), torch.full((P, 128, 65), 1.5, device="cuda"))
    o0, o1, _, _ = call(ops, d, count=cnt, out=out)
    assert same(o0[:P - 5], full[0][:P - 5]) and same(o1[:P - 5], full[1][:P - 5])
    assert bool((o0[P - 5:] == 1.5).all()) and bool((o1[P - 5:] == 1.5).all())


def test_set_third_gather_refuses_unknown_modes(ops):
    with pytest.raises(ValueError):
        ops.set_third_gather("rows")
    assert ops.set_third_gather("tile") == "tile"
