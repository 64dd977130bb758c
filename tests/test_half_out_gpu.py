"""-m gpu: float16 / bfloat16 OUTPUT of the descriptor gathers (ops.fine_descriptors / ops.third_descriptors with out_dtype or
a half `out`).  The one rule: every output element is the float32 value the float32-output call writes, rounded once to the
output type, to nearest even.  The yardstick is therefore always the EXISTING float32-output call on the same inputs followed by
torch.Tensor.to(dtype); outputs are compared as raw 16-bit integers, NaN positions as a mask (payloads are not compared).  No
tolerance anywhere in this file."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from pats_amd import synth
from test_half_out_host import specials_for

pytestmark = pytest.mark.gpu

OUTS = [torch.float16, torch.bfloat16]
MAPS = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["nchw", "channels_last"]
NODES = [0, 63, 64, 127, 128, 143]        # the lane-group (64, 128) and tile-pass (32 g + 8 w) edges of the fine kernels
SENTINEL = 0x7B7B


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


def lay(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t.contiguous()


def raw(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(got, want):
    """bit-equal, except that a NaN is compared as 'a NaN'"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    ng, nw = torch.isnan(got), torch.isnan(want)
    if not torch.equal(ng, nw):
        return False
    z = torch.zeros((), dtype=raw(got).dtype, device=got.device)
    return torch.equal(torch.where(ng, z, raw(got)), torch.where(nw, z, raw(want)))


def sentinel(shape, dt):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(dt)


def is_sentinel(t):
    return bool((raw(t) == SENTINEL).all())


def cnt(n):
    return torch.tensor([n], dtype=torch.int64, device="cuda")


# ---- inputs and their float32-output references: built once per (shape, map type, layout), never modified --------------------------
@functools.lru_cache(maxsize=None)
def fine_case(B, mdt, layout, planted=True):
    """maps in `mdt` / `layout`, title, rubbish, and the float32-output descriptors.  planted: the special values sit in map 2
    (no pooling: they reach the store exactly) at NODES of its first and last channel, in every second dustbin feature and
    in the title."""
    from pats_amd import ops
    gen = torch.Generator(device="cpu")
    gen.manual_seed(synth.SEED + 400 + B)
    f0, f1, f2 = (torch.randn(s, generator=gen) for s in ((2 * B, 64, 48, 48), (2 * B, 64, 24, 24), (2 * B, 128, 12, 12)))
    title, rub = torch.randn((B, 8), generator=gen), torch.randn((B, 264), generator=gen)
    if planted:
        sp = specials_for(mdt)
        slot = 0
        for n in range(2 * B):
            for ch in (0, 127):
                for k in NODES:
                    f2[n, ch, k // 12, k % 12] = sp[slot % sp.numel()]
                    slot += 1
        assert slot >= sp.numel()
        every = specials_for(torch.float32)                    # title / rubbish are float32 whatever the maps are
        for b in range(B):
            rub[b, ::2] = every[(torch.arange(132) + 5 * b) % every.numel()]
            title[b] = every[(torch.arange(8) + 8 * b + 14) % every.numel()]      # b = 0: ..., inf, -inf, NaN, 0
    maps = [lay(m.to(mdt).cuda(), layout) for m in (f0, f1, f2)]
    title, rub = title.cuda(), rub.cuda()
    ref = ops.fine_descriptors(maps, title, rub)
    assert ref.dtype == torch.float32
    return maps, title, rub, ref


def ring_points(P):
    g = golden("third_desc_ring.npz")                          # rounded points on the border ring: the clamps and the wraps
    mk0 = np.concatenate([[[0, 0], [96, 96]], g["p_s"]]).astype(np.float32)[:P]
    mk1 = np.concatenate([[[96, 96], [0, 0]], g["p_t"]]).astype(np.float32)[:P]
    return torch.from_numpy(mk0).cuda(), torch.from_numpy(mk1).cuda(), (torch.arange(P) % 2).cuda()


@functools.lru_cache(maxsize=None)
def third_case(P, mdt, layout, planted=True):
    """B = 2 maps with the special values sprinkled in, kenc = 0 (map values reach the store exactly), dustbin features with
    the special values too, points of the border ring; and the float32-output call's results."""
    from pats_amd import ops
    B = 2
    gen = torch.Generator(device="cpu")
    gen.manual_seed(synth.SEED + 420 + P)
    ff = [torch.randn((B, 128, 52, 52), generator=gen) for _ in range(2)]
    rub = torch.randn((B, 128, 144), generator=gen)
    kenc = torch.zeros((128, 64)) if planted else 0.1 * torch.randn((128, 64), generator=gen)
    if planted:
        sp, every = specials_for(mdt), specials_for(torch.float32)
        for i in range(2):
            use = torch.rand(ff[i].shape, generator=gen) < 0.05
            ff[i] = torch.where(use, sp[torch.randint(0, sp.numel(), ff[i].shape, generator=gen)], ff[i])
        use = torch.rand(rub.shape, generator=gen) < 0.2
        rub = torch.where(use, every[torch.randint(0, every.numel(), rub.shape, generator=gen)], rub)
    f0, f1 = (lay(f.to(mdt).cuda(), layout) for f in ff)
    mk0, mk1, b_ids = ring_points(P)
    args = (f0, f1, mk0, mk1, b_ids, kenc.cuda(), rub.cuda())
    ref = ops.third_descriptors(*args)
    return args, ref


def check_specials_reached(ref, ot):
    """the float32 reference holds NaNs, infinities and elements the output type rounds"""
    fin = ref[torch.isfinite(ref)]
    assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any()) and bool((fin.to(ot).float() != fin).any())


# ---- fine level ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ot", OUTS)
@pytest.mark.parametrize("mdt", MAPS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B", [1, 3])
def test_fine_descriptors_half_output(ops, ot, mdt, layout, B):
    maps, title, rub, ref = fine_case(B, mdt, layout)
    check_specials_reached(ref, ot)
    planted = ref[:, :, [136, 263]][:, :, :, NODES]
    assert bool(torch.isnan(planted).any()) and bool(torch.isinf(planted).any()) and bool((planted == 0).any())
    assert bool(torch.isnan(ref[..., 144]).any()) and bool(torch.isnan(ref[:, :, :8, :144]).any())      # dustbin column, title rows
    want = ref.to(ot)
    got = ops.fine_descriptors(maps, title, rub, out_dtype=ot)
    assert got.dtype == ot and same(got, want)
    out = sentinel((2, B, 264, 145), ot)                        # a given `out` decides the type
    res = ops.fine_descriptors(maps, title, rub, out=out)
    assert res.data_ptr() == out.data_ptr() and same(out, want)
    assert same(ops.fine_descriptors(maps, title, rub, out=sentinel((2, B, 264, 145), ot), out_dtype=ot), want)


@pytest.mark.parametrize("ot", OUTS)
@pytest.mark.parametrize("mdt", MAPS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fine_descriptors_half_output_at_an_odd_element_offset(ops, ot, mdt, layout):
    """NCHW stores need the element size only; the channels-last copy needs 16 bytes and says so."""
    maps, title, rub, ref = fine_case(1, mdt, layout)
    buf = sentinel((2 * 264 * 145 + 2,), ot)
    out = buf[1:-1].view(2, 1, 264, 145)
    assert out.data_ptr() % 4 == 2
    if layout == "nchw":
        ops.fine_descriptors(maps, title, rub, out=out)
        assert same(out, ref.to(ot)) and is_sentinel(buf[:1]) and is_sentinel(buf[-1:])
    else:
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ops.fine_descriptors(maps, title, rub, out=out)
        assert is_sentinel(buf)


# ---- third level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ot", OUTS)
@pytest.mark.parametrize("mdt", MAPS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("P", [1, 8, 9, 17])
def test_third_descriptors_half_output(ops, ot, mdt, layout, P):
    args, ref = third_case(P, mdt, layout)
    if P >= 8:
        check_specials_reached(ref[0], ot)
        check_specials_reached(ref[1], ot)
        assert bool(torch.isnan(ref[0][..., 64]).any())        # the dustbin column
    want = (ref[0].to(ot), ref[1].to(ot))

    def check(got):
        assert got[0].dtype == ot and got[1].dtype == ot
        assert same(got[0], want[0]) and same(got[1], want[1])
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    check(ops.third_descriptors(*args, out_dtype=ot))
    prev = ops.set_third_gather("point")                        # the per-point kernel selected for the float32 output as well
    try:
        check(ops.third_descriptors(*args, out_dtype=ot))
    finally:
        ops.set_third_gather(prev)
    out = (sentinel((P, 128, 65), ot), sentinel((P, 128, 65), ot))
    got = ops.third_descriptors(*args, out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    check(got)
    if layout == "nchw":                                        # outputs at 2 mod 4 bytes: slices of larger buffers
        bufs = [sentinel((P * 128 * 65 + 2,), ot) for _ in range(2)]
        outs = tuple(b[1:-1].view(P, 128, 65) for b in bufs)
        assert all(o.data_ptr() % 4 == 2 for o in outs)
        check(ops.third_descriptors(*args, out=outs))
        assert all(is_sentinel(b[:1]) and is_sentinel(b[-1:]) for b in bufs)


# ---- counted launches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ot", OUTS)
@pytest.mark.parametrize("mdt", MAPS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_counted_launches_leave_rows_past_the_count_untouched(ops, ot, mdt, layout):
    maps, title, rub, ref = fine_case(3, mdt, layout)
    out = sentinel((2, 3, 264, 145), ot)
    ops.fine_descriptors(maps, title, rub, out=out, count=cnt(2))
    assert same(out[:, :2], ref[:, :2].to(ot)) and is_sentinel(out[:, 2:])
    args, ref3 = third_case(17, mdt, layout)
    outs = (sentinel((17, 128, 65), ot), sentinel((17, 128, 65), ot))
    ps32, pt32 = ops.third_descriptors(*args, count=cnt(9))[2:]
    _, _, ps, pt = ops.third_descriptors(*args, count=cnt(9), out=outs)
    for o, r in zip(outs, ref3):
        assert same(o[:9], r[:9].to(ot)) and is_sentinel(o[9:])
    assert torch.equal(ps[:9], ps32[:9]) and torch.equal(pt[:9], pt32[:9])
    assert torch.equal(ps[:9], ref3[2][:9]) and torch.equal(pt[:9], ref3[3][:9])


# ---- float32 output: untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdt", MAPS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_float32_output_is_the_call_without_the_argument(ops, mdt, layout):
    maps, title, rub, ref = fine_case(3, mdt, layout)
    assert same(ops.fine_descriptors(maps, title, rub, out_dtype=torch.float32), ref)
    out = torch.full((2, 3, 264, 145), float("nan"), device="cuda")
    assert same(ops.fine_descriptors(maps, title, rub, out=out), ref)
    assert same(ops.fine_descriptors(maps, title, rub, out=out, out_dtype=torch.float32), ref)
    args, ref3 = third_case(17, mdt, layout)
    got = ops.third_descriptors(*args, out_dtype=torch.float32)
    assert same(got[0], ref3[0]) and same(got[1], ref3[1]) and torch.equal(got[2], ref3[2]) and torch.equal(got[3], ref3[3])
    outs = (torch.full((17, 128, 65), float("nan"), device="cuda"), torch.full((17, 128, 65), float("nan"), device="cuda"))
    ops.third_descriptors(*args, out=outs)
    assert same(outs[0], ref3[0]) and same(outs[1], ref3[1])


# ---- the chain: half descriptors straight into the typed cost builds -----------------------------------------------------------------
@pytest.mark.parametrize("ot", OUTS)
@pytest.mark.parametrize("mdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cost_ot_and_third_level_on_half_gather_outputs(ops, ot, mdt, layout):
    maps, title, rub, ref = fine_case(3, mdt, layout, planted=False)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 440)
    ns = (torch.rand((3, 1, 144), device="cuda", generator=gen) + 0.5).contiguous()
    one = torch.ones(1, device="cuda")
    desc = ops.fine_descriptors(maps, title, rub, out_dtype=ot)
    conv = ref.to(ot)
    for kw in ({}, {"count": cnt(2)}):
        got = ops.cost_ot(desc[0], desc[1], 2, one, ns, 100, bias_k=2.0, return_flags=True, **kw)
        want = ops.cost_ot(conv[0], conv[1], 2, one, ns, 100, bias_k=2.0, return_flags=True, **kw)
        live = 2 if kw else 3
        assert bool(torch.isfinite(got[0][:live]).all())
        assert same(got[0][:live], want[0][:live]) and torch.equal(got[1][:live], want[1][:live])
    args, ref3 = third_case(17, mdt, layout, planted=False)
    t0, t1, ps, pt = ops.third_descriptors(*args, out_dtype=ot)
    scale = (torch.rand((17, 1, 64), device="cuda", generator=gen) + 0.5).contiguous()
    got = ops.third_level(t0, t1, scale, ps, pt)
    want = ops.third_level(ref3[0].to(ot), ref3[1].to(ot), scale, ref3[2], ref3[3])
    assert len(got) == len(want) == 4 and all(same(g, w) if g.is_floating_point() else torch.equal(g, w) for g, w in zip(got, want))
    assert bool(torch.isfinite(got[1]).all())


# ---- a whole throughput step: the callbacks emit bf16 straight from the gathers -----------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_forward_pairs_with_bf16_descriptors_straight_from_the_gathers(ops, layout):
    from pats_amd import batch
    from benchlib.nets import BenchNets
    g = golden("pipeline_outdoor.npz")                          # the one-pair batch and grid of tests/test_batch_gpu.py
    h, w = int(g["h"]), int(g["w"])
    bf = torch.bfloat16

    class Nets(BenchNets):
        """BenchNets whose gathers write bf16 buffers (emit), or float32 buffers that a .to(bfloat16) pass converts"""
        emit = True

        def fine(self, rows, new_left, new_right):
            buf = self.hdesc if self.emit else self.desc[0]
            self.ops.fine_descriptors([self.m0, self.m1, self.m2], self.title, self.rubbish, out=buf, count=rows.chunk_base[-1:])
            d = buf if self.emit else buf.to(bf)
            self.seen.append(d.dtype)
            return d[0], d[1], self.sx, self.sy, self.ns2

        def third(self, rows, mk0, mk1, b_ids, P_dev):
            outs = (self.h0, self.h1) if self.emit else (self.t0[0], self.t1[0])
            t0, t1, ps, pt = self.ops.third_descriptors(self.ff0, self.ff1, mk0, mk1, b_ids, self.kenc, self.rubbish3, count=P_dev,
                                                        out=outs)
            if not self.emit:
                t0, t1 = t0.to(bf), t1.to(bf)
            self.seen.append(t0.dtype)
            return t0, t1, self.scale3, ps, pt
    cap = batch.Capacities(1, h, w, if_local=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 450)
    nets = Nets(ops, torch.device("cuda"), gen, cap, h, w, channels_last=layout == "channels_last")
    nets.hdesc = torch.zeros_like(nets.desc[0], dtype=bf)
    nets.h0, nets.h1 = torch.zeros_like(nets.t0[0], dtype=bf), torch.zeros_like(nets.t1[0], dtype=bf)
    for t in (nets.desc[0], nets.t0[0], nets.t1[0]):
        t.zero_()
    res = []
    for emit in (True, False):
        nets.emit, nets.seen = emit, []
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, if_outdoor=True, merge_new=True)
        assert nets.seen and set(nets.seen) == {bf}
        M = int(out["M"].item())
        res.append({"M": M, "P": int(out["P"].item()), "status": int(out["status"].item()), "ml": out["matches_l"][:M].clone(),
                    "mr": out["matches_r"][:M].clone(), "row": out["match_row"][:M].clone()})
    got, want = res
    assert got["M"] == want["M"] > 0 and got["P"] == want["P"] > 0 and got["status"] == want["status"]
    for k in ("ml", "mr", "row"):
        assert torch.equal(got[k], want[k]), k
