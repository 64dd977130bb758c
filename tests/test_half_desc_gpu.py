"""-m gpu: float16 / bfloat16 DESCRIPTORS in the cost builds and the descriptor -> plan entry points (ops.cost, ops.cost_ot,
ops.third_level).  Every element is widened to fp32 exactly at the load and everything behind the load is the fp32 code in
its order, so every output must equal the same call on desc.float(), bit for bit - with and without a device-side count,
in both solver modes, through the in-kernel fp32 redo tile and the guard-trip re-solves, and over whole throughput steps.
The only tolerance in here is the one the fp32 cost build is already held to against the oracle on random descriptors
(tests/test_determinism_gpu.py: atol=2e-5, rtol=1e-5).

Run as a script (`python tests/test_half_desc_gpu.py <case>`) this file is the child process of the two fresh-process
tests below."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from pats_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


def cu(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dt is None else t.to(dt)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def all_same(got, want, eq=same_bits):
    got, want = (got if isinstance(got, tuple) else (got,)), (want if isinstance(want, tuple) else (want,))
    return len(got) == len(want) and all(eq(g, w) for g, w in zip(got, want))


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda") if dtype == torch.float32 else torch.full(shape, 0xEE, dtype=dtype, device="cuda")


def fine_set(dt, B=6, seed=synth.SEED + 1):
    inp = synth.fine_inputs(seed=seed, B=B)
    return cu(inp["d0"], dt), cu(inp["d1"], dt), (cu(inp["scale_x"]) * cu(inp["scale_y"])).contiguous()


def third_set(dt, P=32, seed=synth.SEED + 2):
    inp = synth.third_inputs(seed=seed, P=P)
    return cu(inp["d0"], dt), cu(inp["d1"], dt), cu(inp["scale"]), cu(inp["p_s"]), cu(inp["p_t"])


# ---- ops.cost ----------------------------------------------------------------------------------------------------------------
def _cost_case(case, dt):
    if case == "generic":            # no dedicated shape: several tiles with ragged edges, a ragged last k-chunk (40 = 2 x 16 + 8)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(synth.SEED + 300)
        return (torch.randn((3, 40, 161), device="cuda", generator=gen).to(dt), torch.randn((3, 40, 97), device="cuda", generator=gen).to(dt))
    inp = {"coarse_301": synth.coarse_inputs, "fine_145": synth.fine_inputs, "third_65": synth.third_inputs}[case]()
    return cu(inp["d0"], dt), cu(inp["d1"], dt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("case", ["coarse_301", "fine_145", "third_65", "generic"])
def test_cost_on_half_descriptors(ops, dt, case):
    d0, d1 = _cost_case(case, dt)
    got = ops.cost(d0, d1)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert same_bits(got, ops.cost(d0.float(), d1.float()))
    out = torch.empty_like(got)
    assert ops.cost(d0, d1, out=out).data_ptr() == out.data_ptr() and same_bits(out, got)


@pytest.mark.parametrize("dt", HALF)
def test_cost_on_half_randn_descriptors_against_the_oracle(ops, oracle, dt):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 301)
    d0 = torch.randn((8, 264, 145), device="cuda", generator=gen).to(dt)
    d1 = torch.randn((8, 264, 145), device="cuda", generator=gen).to(dt)
    got = ops.cost(d0, d1).cpu().numpy()
    want = oracle.cost(d0.float().cpu().numpy(), d1.float().cpu().numpy())
    print("max |cost - oracle| = %g (|oracle| <= %g)" % (np.abs(got - want).max(), np.abs(want).max()))
    np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-5)


# ---- ops.cost_ot -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("hw", [(15, 20), (24, 32)])          # 301 x 301 (resident solver), 769 x 769 (streaming solver)
def test_cost_ot_variant_1_on_half_descriptors(ops, dt, hw):
    inp = synth.coarse_inputs(h=hw[0], w=hw[1])
    d0, d1, ns, alpha = cu(inp["d0"], dt), cu(inp["d1"], dt), cu(inp["ns"]), float(inp["alpha"])
    got = ops.cost_ot(d0, d1, 1, alpha, ns, 100)
    n = hw[0] * hw[1]
    assert got.shape == (1, n + 1, n + 1) and bool(torch.isfinite(got).all())
    assert same_bits(got, ops.cost_ot(d0.float(), d1.float(), 1, alpha, ns, 100))


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("flags", [False, True])
@pytest.mark.parametrize("bias_k", [2.0, 3.0])
def test_cost_ot_variant_2_on_half_descriptors(ops, dt, flags, bias_k):
    d0, d1, ns = fine_set(dt)
    one = torch.tensor(1.0, device="cuda")
    got = ops.cost_ot(d0, d1, 2, one, ns, 100, bias_k=bias_k, return_flags=flags)
    want = ops.cost_ot(d0.float(), d1.float(), 2, one, ns, 100, bias_k=bias_k, return_flags=flags)
    assert all_same(got, want)
    Z = got[0] if flags else got
    assert Z.shape == (6, 145, 145) and bool(torch.isfinite(Z).all())
    if flags:
        assert got[1].dtype == torch.bool and 0 < int(got[1].sum()) < got[1].numel()


@pytest.mark.parametrize("dt", HALF)
def test_cost_ot_65_wide_on_half_descriptors(ops, dt):
    """variant 2 at 65 x 65: the one-wave cost build + solve (sinkhorn65_kernel), with and without the column flags."""
    d0, d1, scale, _, _ = third_set(dt)
    for flags in (False, True):
        got = ops.cost_ot(d0, d1, 2, 1.0, scale, 100, return_flags=flags)
        assert all_same(got, ops.cost_ot(d0.float(), d1.float(), 2, 1.0, scale, 100, return_flags=flags))


# ---- ops.third_level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("outdoor", [True, False])
@pytest.mark.parametrize("plan", [False, True])
def test_third_level_on_half_descriptors(ops, dt, outdoor, plan):
    d0, d1, scale, ps, pt = third_set(dt)
    got = ops.third_level(d0, d1, scale, ps, pt, outdoor=outdoor, return_plan=plan)
    want = ops.third_level(d0.float(), d1.float(), scale, ps, pt, outdoor=outdoor, return_plan=plan)
    assert len(got) == (5 if plan else 4) and all_same(got, want)
    assert bool(torch.isfinite(got[1]).all()) and 0 < int(got[3].sum()) < got[3].numel()


# ---- counted launches --------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 23, 37, 50]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("count", COUNTS)
def test_counted_fine_cost_ot_on_half_descriptors(ops, dt, count):
    """The C entry itself, so that Z and the flags are buffers this test pre-fills: rows past the count must stay untouched."""
    from pats_amd.ops import _L, _check, _ptr, _stream, _workspace, _MAP_DTYPES
    cap = 37
    d0, d1, ns = fine_set(dt, B=cap, seed=synth.SEED + 310)
    one = torch.ones(1, device="cuda")
    full_Z, full_f = ops.cost_ot(d0, d1, 2, one, ns, 100, bias_k=2.0, return_flags=True)
    Z, fl = nan_like((cap, 145, 145)), nan_like((cap, 144), torch.uint8)
    nb = _L().pats_cost_ot_workspace_bytes(cap, 264, 145, 145, 2)
    ws = _workspace(nb, d0.device)
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
    _check(_L().pats_cost_ot_typed(_ptr(d0), _ptr(d1), _MAP_DTYPES[dt], cap, _ptr(cnt), 264, 145, 145, 2, _ptr(one), _ptr(ns), 100, 2.0,
                                   _ptr(Z), _ptr(fl), _ptr(ws), nb, _stream()), "cost_ot_typed")
    live = min(count, cap)
    assert same_bits(Z[:live], full_Z[:live]) and torch.equal(fl[:live].bool(), full_f[:live])
    assert bool(torch.isnan(Z[live:]).all()) and bool((fl[live:] == 0xEE).all())
    # and through ops (its own outputs): the live rows
    Zo, fo = ops.cost_ot(d0, d1, 2, one, ns, 100, bias_k=2.0, return_flags=True, count=cnt)
    assert same_bits(Zo[:live], full_Z[:live]) and torch.equal(fo[:live], full_f[:live])
    want = ops.cost_ot(d0.float(), d1.float(), 2, one, ns, 100, bias_k=2.0, return_flags=True, count=cnt)
    assert same_bits(Zo[:live], want[0][:live]) and torch.equal(fo[:live], want[1][:live])


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("count", COUNTS)
def test_counted_third_level_on_half_descriptors(ops, dt, count):
    cap = 37
    d0, d1, scale, ps, pt = third_set(dt, P=cap, seed=synth.SEED + 311)
    full = ops.third_level(d0, d1, scale, ps, pt)
    out = (nan_like((cap, 16, 2)), nan_like((cap, 16, 2)), nan_like((cap * 16, 2)), nan_like((cap, 16), torch.uint8))
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
    got = ops.third_level(d0, d1, scale, ps, pt, count=cnt, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    live = min(count, cap)
    m0, m1, label, ifm = out
    assert same_bits(m0[:live], full[0][:live]) and same_bits(m1[:live], full[1][:live])
    assert same_bits(label[:16 * live], full[2][:16 * live]) and torch.equal(ifm[:live].bool(), full[3][:live])
    assert bool(torch.isnan(m0[live:]).all()) and bool(torch.isnan(m1[live:]).all()) and bool(torch.isnan(label[16 * live:]).all())
    assert bool((ifm[live:] == 0xEE).all())
    ref = ops.third_level(d0.float(), d1.float(), scale, ps, pt, count=cnt)
    assert all(same_bits(g[:n], r[:n]) for g, r, n in zip((m0, m1, label), ref[:3], (live, live, 16 * live)))
    assert torch.equal(ifm[:live].bool(), ref[3][:live])


# ---- range: beyond fp16's split range (the in-kernel fp32 redo tile), inf, NaN, signed zeros, half subnormals ---------------------
def _wild(d, dt, gen, big=None, nonfinite=True):
    """d with, per problem: one column of huge entries (default: close to the type's largest), +-0 and half subnormals sprinkled
    in and - nonfinite - an inf and a NaN in one column."""
    fi = torch.finfo(dt)
    big = big if big is not None else (60000.0 if dt == torch.float16 else 3e38)
    sub = fi.tiny * fi.eps
    d = d.clone()
    B, D, n = d.shape
    d[:, :, 3] = torch.where(torch.rand((B, D), device="cuda", generator=gen) < 0.5, big, -big).to(dt)[:, :] * (torch.arange(D, device="cuda") % 7 == 0).to(dt)
    if nonfinite:
        d[:, 5, 7] = float("inf")
        d[:, 6, 7] = float("nan")
    sprinkle = torch.tensor([0.0, -0.0, sub, -sub, 3 * sub, fi.tiny - sub], device="cuda").to(dt)
    pick = torch.randint(0, sprinkle.numel(), d.shape, device="cuda", generator=gen)
    use = torch.rand(d.shape, device="cuda", generator=gen) < 0.05
    use[:, :, 3] = False
    use[:, 5:7, 7] = False
    return torch.where(use, sprinkle[pick], d)


@pytest.mark.parametrize("dt", HALF)
def test_range_and_special_values_in_half_descriptors(ops, dt):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 320)
    # cost: a generic shape and the fine shape; the huge column sends its tiles to the fp32 redo
    for shape0, shape1 in (((3, 40, 161), (3, 40, 97)), ((4, 264, 145), (4, 264, 145))):
        d0 = _wild(torch.randn(shape0, device="cuda", generator=gen).to(dt), dt, gen)
        d1 = _wild(torch.randn(shape1, device="cuda", generator=gen).to(dt), dt, gen)
        got, want = ops.cost(d0, d1), ops.cost(d0.float(), d1.float())
        assert same_bits(got, want)
        assert bool(torch.isnan(got).any()) and bool(torch.isfinite(got).any())
        if dt == torch.float16:      # 60 000 x 60 000 products stay finite in fp32 only through the fp32 redo
            assert float(got[torch.isfinite(got)].abs().max()) > 1e6
    # fine-level cost + OT and the third level on such descriptors: finite but far outside the split's range (fp32 redo tile,
    # scores the linear solve's guard gives up on -> the re-solves), then with the inf / NaN column as well
    one = torch.ones(1, device="cuda")
    f0, f1, ns = fine_set(dt, B=4, seed=synth.SEED + 321)
    t0, t1, scale, ps, pt = third_set(dt, P=24, seed=synth.SEED + 322)
    for nonfinite in (False, True):
        kw = {"big": 6000.0, "nonfinite": nonfinite}
        d0, d1 = _wild(f0, dt, gen, **kw), _wild(f1, dt, gen, **kw)
        ops.sinkhorn_fallbacks(reset=True)
        got = ops.cost_ot(d0, d1, 2, one, ns, 100, bias_k=2.0, return_flags=True)
        trips = ops.sinkhorn_fallbacks(reset=True)
        assert all_same(got, ops.cost_ot(d0.float(), d1.float(), 2, one, ns, 100, bias_k=2.0, return_flags=True))
        assert trips > 0, "the fine level's guard must trip on these scores"
        ops.sinkhorn_fallbacks(reset=True)
        w0, w1 = _wild(t0, dt, gen, **kw), _wild(t1, dt, gen, **kw)
        for plan in (False, True):
            got = ops.third_level(w0, w1, scale, ps, pt, return_plan=plan)
            assert all_same(got, ops.third_level(w0.float(), w1.float(), scale, ps, pt, return_plan=plan))
        assert ops.sinkhorn_fallbacks(reset=True) > 0, "the third level's guard must trip on these scores"


@pytest.mark.parametrize("dt", HALF)
def test_third_level_redo_walk_reads_half_descriptors(ops, dt):
    """More problems than the 6144 workgroups of the two re-solve walks, built as tests/test_third_redo_walk_gpu.py builds its
    launches (a base set of 96 problems, 32 of them amplified until the linear solve's guard trips, gathered by an index
    vector): the stabilised kernel and the log-domain scan kernel both rebuild their cost from the half descriptors."""
    from test_third_redo_walk_gpu import AMPS, K, NWILD
    P = 6144 + 700
    inp = synth.third_inputs(seed=synth.SEED + 64, P=K)
    d0, d1 = inp["d0"].copy(), inp["d1"].copy()
    d0[:NWILD] *= AMPS[:, None, None]
    d1[:NWILD] *= AMPS[:, None, None]
    rng = np.random.default_rng(9)
    idx = rng.integers(NWILD, K, P)
    idx[rng.choice(P, 900, replace=False)] = rng.integers(0, NWILD, 900)      # wild problems on every lane of the walk
    idx[6144:6144 + 64] = np.arange(64) % NWILD                               # and beyond the first W problems
    sel = cu(idx.astype(np.int64))
    base = (cu(d0, dt), cu(d1, dt), cu(inp["scale"]), cu(inp["p_s"]), cu(inp["p_t"]))
    h0, h1, scale, ps, pt = (torch.index_select(t, 0, sel) for t in base)
    ops.sinkhorn_fallbacks(reset=True)
    got = ops.third_level(h0, h1, scale, ps, pt)
    trips = ops.sinkhorn_fallbacks(reset=True)
    want = ops.third_level(h0.float(), h1.float(), scale, ps, pt)
    trips32 = ops.sinkhorn_fallbacks(reset=True)
    print("guard trips: %d (half), %d (float32) of %d problems" % (trips, trips32, P))
    assert trips == trips32 >= 100, "the launch must send problems through both re-solve kernels"
    assert all_same(got, want)
    assert bool(torch.isfinite(got[1]).all()) and set(torch.unique(got[3].to(torch.uint8)).tolist()) <= {0, 1}
    cnt = torch.tensor([6144 + 300], dtype=torch.int64, device="cuda")         # the counted form: flagged problems on both sides
    out = (nan_like((P, 16, 2)), nan_like((P, 16, 2)), nan_like((P * 16, 2)), nan_like((P, 16), torch.uint8))
    ops.third_level(h0, h1, scale, ps, pt, count=cnt, out=out)
    live = 6144 + 300
    assert same_bits(out[1][:live], got[1][:live]) and torch.equal(out[3][:live].bool(), got[3][:live])
    assert bool(torch.isnan(out[1][live:]).all()) and bool((out[3][live:] == 0xEE).all())


# ---- solver modes, PATS_COST_F32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
def test_log_domain_solver_mode_on_half_descriptors(ops, dt):
    d0, d1, ns = fine_set(dt)
    t0, t1, scale, ps, pt = third_set(dt)
    one = torch.ones(1, device="cuda")
    prev = ops.set_sinkhorn_mode("log")
    try:
        got_f = ops.cost_ot(d0, d1, 2, one, ns, 100, bias_k=2.0, return_flags=True)
        want_f = ops.cost_ot(d0.float(), d1.float(), 2, one, ns, 100, bias_k=2.0, return_flags=True)
        got_t = ops.third_level(t0, t1, scale, ps, pt)
        want_t = ops.third_level(t0.float(), t1.float(), scale, ps, pt)
    finally:
        ops.set_sinkhorn_mode(prev)
    assert all_same(got_f, want_f) and all_same(got_t, want_t)


def _child(case, env=None, timeout=600):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]


def test_cost_f32_switch_on_half_descriptors_in_a_fresh_process():
    """PATS_COST_F32=1 (read once per process): every contraction on the fp32 MFMA, for every element type."""
    lines = _child("cost_f32", {"PATS_COST_F32": "1"})
    assert lines == ["RESULT cost_f32 float16 True True", "RESULT cost_f32 bfloat16 True True"], lines


def test_typed_launches_identical_from_the_first_launch_of_a_process():
    """The first launches of a process are the typed fine-level cost build and the typed third level: launch 0 equals
    launch 1 and the float32 call, bit for bit."""
    lines = _child("first_launch")
    assert lines == ["RESULT first_launch cost True True", "RESULT first_launch third True True"], lines


# ---- fallbacks -------------------------------------------------------------------------------------------------------------------
def _odd(t):
    """a copy of t in a view at an odd element offset"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("dt", HALF)
def test_mixed_dtypes_odd_offsets_and_half_small_operands(ops, dt):
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 330)
    ints = lambda shape: torch.randint(-4, 5, shape, device="cuda", generator=gen).float()      # noqa: E731  exact in both half types
    one = torch.ones(1, device="cuda")
    # one fp16 and one bf16 set in the same call; a half and a float32 set
    a, b = ints((3, 264, 145)), ints((3, 264, 145))
    ns = (torch.rand((3, 1, 144), device="cuda", generator=gen) + 0.5).contiguous()
    want = ops.cost_ot(a, b, 2, one, ns, 100, bias_k=2.0, return_flags=True)
    assert same_bits(ops.cost(a.to(dt), b.to(other)), ops.cost(a, b))
    assert all_same(ops.cost_ot(a.to(dt), b.to(other), 2, one, ns, 100, bias_k=2.0, return_flags=True), want)
    assert all_same(ops.cost_ot(a.to(dt), b, 2, one, ns, 100, bias_k=2.0, return_flags=True), want)
    t0, t1, scale, ps, pt = third_set(torch.float32, P=16)
    t0, t1 = ints(t0.shape), ints(t1.shape)
    want3 = ops.third_level(t0, t1, scale, ps, pt)
    assert all_same(ops.third_level(t0.to(other), t1.to(dt), scale, ps, pt), want3)
    # a half view at an odd element offset: the kernels' loads need the element size only
    d0, d1, ns = fine_set(dt)
    want = ops.cost_ot(d0.float(), d1.float(), 2, one, ns, 100, bias_k=2.0, return_flags=True)
    assert all_same(ops.cost_ot(_odd(d0), d1, 2, one, ns, 100, bias_k=2.0, return_flags=True), want)
    assert all_same(ops.cost_ot(d0, _odd(d1), 2, one, ns, 100, bias_k=2.0, return_flags=True), want)
    assert same_bits(ops.cost(_odd(d0), _odd(d1)), ops.cost(d0.float(), d1.float()))
    h0, h1, scale, ps, pt = third_set(dt)
    want3 = ops.third_level(h0.float(), h1.float(), scale, ps, pt)
    assert all_same(ops.third_level(_odd(h0), h1, scale, ps, pt), want3)
    assert all_same(ops.third_level(h0, _odd(h1), scale, ps, pt), want3)
    c0, c1 = _cost_case("third_65", dt)
    assert same_bits(ops.cost(_odd(c0), _odd(c1)), ops.cost(c0.float(), c1.float()))
    # half scale / ns / alpha / one: widened by ops
    assert all_same(ops.third_level(h0, h1, scale.to(dt), ps, pt), ops.third_level(h0.float(), h1.float(), scale.to(dt).float(), ps, pt))
    assert all_same(ops.cost_ot(d0, d1, 2, one.to(dt), ns.to(dt), 100, bias_k=2.0, return_flags=True),
                    ops.cost_ot(d0.float(), d1.float(), 2, one, ns.to(dt).float(), 100, bias_k=2.0, return_flags=True))
    inp = synth.coarse_inputs()
    m0, m1, nsc = cu(inp["d0"], dt), cu(inp["d1"], dt), cu(inp["ns"])
    alpha = torch.tensor(0.25, device="cuda").to(dt)
    assert same_bits(ops.cost_ot(m0, m1, 1, alpha, nsc.to(dt), 100), ops.cost_ot(m0.float(), m1.float(), 1, alpha.float(), nsc.to(dt).float(), 100))


def test_other_descriptor_dtypes_raise(ops):
    d = torch.zeros((1, 32, 40), device="cuda")
    for dt in (torch.float64, torch.int32, torch.uint8):
        with pytest.raises(RuntimeError, match=str(dt).replace("torch.", "")):
            ops.cost(d.to(dt), d)
        with pytest.raises(RuntimeError, match=str(dt).replace("torch.", "")):
            ops.cost_ot(d, d.to(dt), 1, 0.5, torch.ones((1, 1, 40), device="cuda"), 10)


# ---- whole steps: nets whose callbacks return bf16 descriptors against the same nets returning bf16.float() -----------------------
def _half_nets(base_cls, widen):
    """base_cls with the two descriptor tensors of every callback rounded to bfloat16 - handed on as they are, or (widen) as
    the .float() copies a caller had to make before the typed entry points."""
    def cast(t):
        h = t.to(torch.bfloat16)
        return h.float() if widen else h

    class N(base_cls):
        def coarse(self, *a, **k):
            r = super().coarse(*a, **k)
            return (cast(r[0]), cast(r[1])) + tuple(r[2:])

        def fine(self, *a, **k):
            r = super().fine(*a, **k)
            return (cast(r[0]), cast(r[1])) + tuple(r[2:])

        def third(self, *a, **k):
            r = super().third(*a, **k)
            return (cast(r[0]), cast(r[1])) + tuple(r[2:])
    return N


def _step_result(out, cap, batch):
    M = int(out["M"].item())
    off = batch.group_by_pair(out, cap)[2]
    return {"M": M, "P": int(out["P"].item()), "status": int(out["status"].item()), "ml": out["matches_l"][:M].clone(),
            "mr": out["matches_r"][:M].clone(), "row": out["match_row"][:M].clone(), "off": off.clone()}


def _same_steps(got, want):
    assert got["M"] == want["M"] > 0 and got["P"] == want["P"] > 0 and got["status"] == want["status"]
    for k in ("ml", "mr", "row", "off"):
        assert torch.equal(got[k], want[k]), k


def test_forward_pairs_on_bf16_descriptors(ops):
    from pats_amd import batch
    from benchlib.nets import BenchNets
    pairs, h, w = 4, 6, 8
    cap = batch.Capacities(pairs, h, w, if_local=True)
    res = []
    for widen in (False, True):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(synth.SEED + 340)
        nets = _half_nets(BenchNets, widen)(ops, torch.device("cuda"), gen, cap, h, w)
        seen = nets.coarse(nets.lefts, nets.rights)[0].dtype
        assert seen == (torch.float32 if widen else torch.bfloat16)
        out = batch.forward_pairs(nets.lefts, nets.rights, nets, cap, if_outdoor=True, merge_new=True)
        assert out["stages"]["f0"].dtype == seen and out["stages"]["feat0"].dtype == seen
        res.append(_step_result(out, cap, batch))
    _same_steps(*res)


def test_forward_pairs_mixed_on_bf16_descriptors(ops):
    from pats_amd import batch
    from test_mixed_batch_gpu import _MixedNets

    class Nets(_MixedNets):
        """_MixedNets with third-level descriptors that are not all zero: drawn per capacity slot from a fixed seed"""
        def third(self, rows, mk0, mk1, b_ids, P_dev):
            cap_ = mk0.shape[0]
            g = torch.Generator(device="cuda")
            g.manual_seed(synth.SEED + 341)
            base = torch.randn((cap_, 128, 65), device="cuda", generator=g)
            return (3.0 * base + torch.randn((cap_, 128, 65), device="cuda", generator=g),
                    3.0 * base + torch.randn((cap_, 128, 65), device="cuda", generator=g), torch.ones((cap_, 1, 64), device="cuda"))
    nets = [synth.SynthNets(seed=41, h=6, w=8), synth.SynthNets(seed=42, h=5, w=7), synth.SynthNets(seed=43, h=6, w=8)]
    imgs = [tuple(cu(x) for x in n.images()) for n in nets]
    pack = batch.pack_pairs(imgs)
    cap = batch.MixedCapacities([(n.h, n.w) for n in nets], if_local=True)
    res = []
    for widen in (False, True):
        out = batch.forward_pairs_mixed(pack, _half_nets(Nets, widen)(nets, pack), cap, if_outdoor=True, merge_new=True)
        res.append(_step_result(out, cap, batch))
    _same_steps(*res)


def test_pipeline_forward_path_on_bf16_descriptors(ops):
    from conftest import golden
    from pats_amd import pipeline
    from test_gpu_parity import _CudaNets
    gd = golden("pipeline_outdoor.npz")
    n = synth.SynthNets(seed=int(gd["seed"]), h=int(gd["h"]), w=int(gd["w"]))
    left, right = [cu(x) for x in n.images()]
    got = pipeline.forward_path(left, right, _half_nets(_CudaNets, False)(n), if_local=True)
    want = pipeline.forward_path(left, right, _half_nets(_CudaNets, True)(n), if_local=True)
    assert got["matches_l"].shape[0] > 0
    assert torch.equal(got["matches_l"], want["matches_l"]) and torch.equal(got["matches_r"], want["matches_r"])


# ---- child processes ---------------------------------------------------------------------------------------------------------------
def _main(case):
    from pats_amd import ops
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED + 350)
    if case == "cost_f32":
        for dt in HALF:
            d0 = torch.randn((5, 264, 145), device="cuda", generator=gen).to(dt)
            d1 = torch.randn((5, 264, 145), device="cuda", generator=gen).to(dt)
            g0, g1 = torch.randn((2, 40, 161), device="cuda", generator=gen).to(dt), torch.randn((2, 40, 97), device="cuda", generator=gen).to(dt)
            print("RESULT cost_f32", str(dt).replace("torch.", ""), same_bits(ops.cost(d0, d1), ops.cost(d0.float(), d1.float())),
                  same_bits(ops.cost(g0, g1), ops.cost(g0.float(), g1.float())))
    elif case == "first_launch":
        B, P = 4096, 32768
        d0 = torch.randn((B, 264, 145), device="cuda", generator=gen).to(torch.bfloat16)
        d1 = (d0.float() + 0.3 * torch.randn((B, 264, 145), device="cuda", generator=gen)).to(torch.bfloat16)
        first = ops.cost(d0, d1)                         # launch 0 of this process
        second = ops.cost(d0, d1)
        ref = ops.cost(d0.float(), d1.float())
        print("RESULT first_launch cost", same_bits(first, second), same_bits(first, ref))
        del first, second, ref, d0, d1
        base = 3.0 * torch.randn((P, 128, 65), device="cuda", generator=gen)
        t0 = (base + 0.9 * torch.randn((P, 128, 65), device="cuda", generator=gen)).to(torch.float16)
        t1 = (base + 0.9 * torch.randn((P, 128, 65), device="cuda", generator=gen)).to(torch.float16)
        del base
        scale = (torch.rand((P, 1, 64), device="cuda", generator=gen) + 0.5).contiguous()
        ps = torch.randint(1, 23, (P, 2), device="cuda", generator=gen) * 4
        pt = torch.randint(0, 25, (P, 2), device="cuda", generator=gen) * 4
        first = ops.third_level(t0, t1, scale, ps, pt)   # the first typed third-level launch of this process
        second = ops.third_level(t0, t1, scale, ps, pt)
        ref = ops.third_level(t0.float(), t1.float(), scale, ps, pt)
        print("RESULT first_launch third", all_same(first, second), all_same(first, ref))
    else:
        raise SystemExit("unknown case %r" % case)


if __name__ == "__main__":
    _main(sys.argv[1])
