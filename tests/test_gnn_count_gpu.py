"""-m gpu: the GNN layers over a capacity with the row count on the device - ops.attentional_gnn(count=...) and
ops.attentional_propagation(count=, count_off=), which throughput mode runs on both levels (the fine stack [rows, 264, 145],
the third level's layers [P, 128, 65]).  Every case fills the padding rows (at or past the count) with NaN, +-inf, +-1e30 and
values beyond the fp16 range of the split operands, and starts `out` as a sentinel bit pattern.  With k = clamp(count - count_off,
0, b):
  * rows < k equal, bit for bit, the uncounted call on the first k rows (problems are independent; the fine stack's packing of
    both sets' live problems into one index space moves a column to another tile, not its arithmetic), and the oracle on the
    first and last live row of each set;
  * rows >= k are +0.0 at the fine level and keep the sentinel at the third level - also after an overflow in a live row has
    sent the call to the gated composition, which runs over the whole capacity;
  * under set_gnn_redo('deferred') the padding never raises the overflow flag."""
import ctypes

import numpy as np
import pytest
import torch

from pats_amd import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EEDF00D           # a finite float (~8.6e18) whose bits tell "untouched" from "zeroed"
HOSTILE = (float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 7.0e4, -3.0e5)     # 7 entries: every channel and token meets each
SPIKE = 3.0e4                   # beyond the fp16 range of the split operands (x * 2^6 > 65504)
FINE_NAMES = ["cross", "self", "cross"]
THIRD_NAMES = ["self", "cross"] * 5                       # the third level's stack (benchlib/nets.py)
STACK_TOL = dict(atol=1e-4, rtol=2e-4)                    # the GNN stack parity tests' gates
SPIKE_TOL = dict(atol=2e-2, rtol=2e-4)                    # test_fine_level_gnn_stack_beyond_the_fp16_range: outputs of magnitude 3e4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    assert o.set_gnn_redo("inline") == "inline"           # the default
    return o


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def dev_count(c):
    return torch.tensor([c], dtype=torch.int64, device="cuda")


def bits(t):
    return t.view(torch.int32)


def sentinel_like(t):
    return torch.full(t.shape, SENTINEL, dtype=torch.int32, device=t.device).view(torch.float32)


def live_rows(count, count_off, b):
    return max(0, min(count - count_off, b))


def padded(clean, k):
    """A copy of `clean` whose rows >= k hold the hostile pattern."""
    t = clean.clone()
    if k < t.shape[0]:
        pad = t[k:]
        vals = torch.tensor(HOSTILE, dtype=torch.float32, device=t.device)
        pad.copy_(vals[torch.arange(pad.numel(), device=t.device) % len(HOSTILE)].view(pad.shape))
    return t


def assert_same(got, want, what):
    """Bit-identical; on failure the first row that differs."""
    assert got.shape == want.shape, what
    bad = (bits(got) != bits(want)).reshape(got.shape[0], -1).any(1).nonzero()
    if bad.numel():
        r = int(bad[0])
        raise AssertionError("%s: live row %d of %d differs from the uncounted call (max |d| %.3g)"
                             % (what, r, got.shape[0], float((got[r] - want[r]).abs().max())))


def assert_rows_hold(t, k, pattern, what):
    """Rows k.. of t hold the 32-bit pattern (0: +0.0) in every element."""
    if k >= t.shape[0]:
        return
    bad = (bits(t[k:]) != pattern).reshape(t.shape[0] - k, -1).any(1).nonzero()
    assert bad.numel() == 0, "%s: row %d past the count does not hold %#x" % (what, k + int(bad[0]), pattern)


def oracle_stack(oracle, ps, names, r0, r1):
    for p, name in zip(ps, names):
        y0, y1 = (r1, r0) if name == "cross" else (r0, r1)
        r0, r1 = oracle.attentional_propagation(r0, y0, p, residual=r0), oracle.attentional_propagation(r1, y1, p, residual=r1)
    return r0, r1


def oracle_rows(oracle, ps, names, x0, x1, rows):
    """{row: (set 0, set 1)}: the oracle's stack on the given rows (a cross layer couples row i of one set with row i of the other
    only, so a subset of rows is a stack of its own)."""
    rows = sorted(rows)
    r0, r1 = oracle_stack(oracle, ps, names, host(x0[rows]), host(x1[rows]))
    return {r: (r0[i], r1[i]) for i, r in enumerate(rows)}


def assert_oracle(g0, g1, ref, rows, tol, what):
    for r in sorted(set(rows)):
        np.testing.assert_allclose(host(g0[r]), ref[r][0], err_msg="%s: set 0, row %d" % (what, r), **tol)
        np.testing.assert_allclose(host(g1[r]), ref[r][1], err_msg="%s: set 1, row %d" % (what, r), **tol)


def counted_stack(ops, layers, names, x0, x1, k, count):
    """attentional_gnn over the capacity: padding rows hostile, out a sentinel."""
    d0, d1 = padded(x0, k), padded(x1, k)
    out = (sentinel_like(d0), sentinel_like(d1))
    g = ops.attentional_gnn(d0, d1, layers, names, count=dev_count(count), out=out)
    assert g[0].data_ptr() == out[0].data_ptr() and g[1].data_ptr() == out[1].data_ptr()
    return out


def counted_layer(ops, P, x, s, r, k, count, count_off):
    """attentional_propagation over the capacity (s is x: a self layer; r is x: AttentionalGNN's residual)."""
    xd = padded(x, k)
    sd = xd if s is x else padded(s, k)
    rd = xd if r is x else (None if r is None else padded(r, k))
    out = sentinel_like(xd)
    got = ops.attentional_propagation(xd, sd, P, residual=rd, count=dev_count(count), count_off=count_off, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out


def uncounted_prefix(ops, P, x, s, r, k):
    xs = x[:k]
    return ops.attentional_propagation(xs, xs if s is x else s[:k], P, residual=xs if r is x else (None if r is None else r[:k]))


# ---- the fine level: the packed stack (pats_attentional_gnn_packed_f32) and the single layer --------------------------------------
@pytest.fixture(scope="module")
def fine(ops):
    ps = [synth.gnn_params(seed=1500 + i, C=264) for i in range(3)]
    a = synth.gnn_inputs(seed=1510, b=37, C=264, n=145)
    r = synth.gnn_inputs(seed=1511, b=37, C=264, n=145)["x"]
    return dict(ps=ps, P=[ops.PropagationParams(p) for p in ps], x0=cu(a["x"]), x1=cu(a["source"]), r=cu(r))


# 145 tokens a problem: set 1's live problems start at column 145 k of the packed space, inside a 64-column tile unless 64 | 145 k
FINE_COUNTS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 36, 37, 38, 10 ** 9]


@pytest.fixture(scope="module")
def fine_oracle(oracle, fine):
    b = fine["x0"].shape[0]
    rows = {r for c in FINE_COUNTS if min(c, b) > 0 for r in (0, min(c, b) - 1)}
    return oracle_rows(oracle, fine["ps"], FINE_NAMES, fine["x0"], fine["x1"], rows)


@pytest.mark.parametrize("count", FINE_COUNTS)
def test_fine_stack_counted(ops, fine, fine_oracle, count):
    x0, x1 = fine["x0"], fine["x1"]
    k = live_rows(count, 0, x0.shape[0])
    g0, g1 = counted_stack(ops, fine["P"], FINE_NAMES, x0, x1, k, count)
    what = "fine stack, count %d" % count
    assert_rows_hold(g0, k, 0, what + ", set 0")
    assert_rows_hold(g1, k, 0, what + ", set 1")
    if k:
        w0, w1 = ops.attentional_gnn(x0[:k], x1[:k], fine["P"], FINE_NAMES)
        assert_same(g0[:k], w0, what + ", set 0")
        assert_same(g1[:k], w1, what + ", set 1")
        assert_oracle(g0, g1, fine_oracle, (0, k - 1), STACK_TOL, what)


BLOCK_COUNTS = [4000, 4095, 4096, 4097, 4141]


@pytest.fixture(scope="module")
def fine_big(ops, oracle, fine):
    assert ops.GNN_STACK_ROWS == 4096
    b = ops.GNN_STACK_ROWS + 45
    g = torch.Generator(device="cuda")
    g.manual_seed(1520)
    x0 = torch.randn((b, 264, 145), device="cuda", generator=g)
    x1 = torch.randn((b, 264, 145), device="cuda", generator=g)
    rows = {r for c in BLOCK_COUNTS for r in (4095, 4096, c - 1) if r < c}
    return x0, x1, oracle_rows(oracle, fine["ps"], FINE_NAMES, x0, x1, rows)


@pytest.mark.parametrize("count", BLOCK_COUNTS)
def test_fine_stack_counted_across_a_block(ops, fine, fine_big, count):
    """The stack runs in blocks of GNN_STACK_ROWS rows with live_off = the block's first row: count=4000 leaves the second block
    nothing to compute, 4097 one row."""
    x0, x1, ref = fine_big
    k = live_rows(count, 0, x0.shape[0])
    g0, g1 = counted_stack(ops, fine["P"], FINE_NAMES, x0, x1, k, count)
    what = "fine stack of %d rows, count %d" % (x0.shape[0], count)
    assert_rows_hold(g0, k, 0, what + ", set 0")
    assert_rows_hold(g1, k, 0, what + ", set 1")
    w0, w1 = ops.attentional_gnn(x0[:k], x1[:k], fine["P"], FINE_NAMES)
    assert_same(g0[:k], w0, what + ", set 0")
    assert_same(g1[:k], w1, what + ", set 1")
    assert_oracle(g0, g1, ref, [r for r in (4095, 4096, k - 1) if r < k], STACK_TOL, what)


def fine_layer_operands(fine, residual):
    """(x, source, residual) of a fine-level layer: the self layer with its own x as the residual, or a distinct source with no
    residual / with a residual that is neither (the conversion out adds that one)."""
    x = fine["x0"]
    if residual == "x":
        return x, x, x
    return x, fine["x1"], None if residual == "none" else fine["r"]


@pytest.mark.parametrize("count_off", [0, 5])
@pytest.mark.parametrize("residual", ["x", "none", "add"])
def test_fine_single_layer_counted(ops, oracle, fine, residual, count_off):
    """pats_attentional_propagation_packed_counted_f32 at the fine level's shape: the one-kernel layer between the conversions in
    and out; rows past the count are zeros whatever the residual."""
    p, P = fine["ps"][0], fine["P"][0]
    x, s, r = fine_layer_operands(fine, residual)
    b = x.shape[0]
    counts = [count_off + j for j in (0, 1, 8, 9, 17, 36, 37, 38)] + [10 ** 9] + ([count_off - 2] if count_off else [])
    ks = [live_rows(c, count_off, b) for c in counts]
    rows = sorted({q for k in ks if k for q in (0, k - 1)})
    want = oracle.attentional_propagation(host(x[rows]), host(s[rows]), p, residual=None if r is None else host(r[rows]))
    for count, k in zip(counts, ks):
        what = "fine layer, residual %s, count %d - %d" % (residual, count, count_off)
        got = counted_layer(ops, P, x, s, r, k, count, count_off)
        assert_rows_hold(got, k, 0, what)
        if k:
            assert_same(got[:k], uncounted_prefix(ops, P, x, s, r, k), what)
            for q in (0, k - 1):
                np.testing.assert_allclose(host(got[q]), want[rows.index(q)], err_msg="%s: row %d" % (what, q), **STACK_TOL)


# ---- the third level: the fused one-kernel layer (gnn_fused.hip) through the layer-by-layer path ------------------------------------
@pytest.fixture(scope="module")
def third(ops):
    ps = [synth.gnn_params(seed=1600 + i, C=128) for i in range(10)]
    a = synth.gnn_inputs(seed=1610, b=41, C=128, n=65)
    return dict(ps=ps, P=[ops.PropagationParams(p) for p in ps], x0=cu(a["x"]), x1=cu(a["source"]))


THIRD_COUNTS = [0, 1, 40, 41, 50]


@pytest.fixture(scope="module")
def third_oracle(oracle, third):
    b = third["x0"].shape[0]
    rows = {r for c in THIRD_COUNTS if min(c, b) > 0 for r in (0, min(c, b) - 1)}
    return oracle_rows(oracle, third["ps"], THIRD_NAMES, third["x0"], third["x1"], rows)


@pytest.mark.parametrize("count", THIRD_COUNTS)
def test_third_stack_counted(ops, third, third_oracle, count):
    x0, x1 = third["x0"], third["x1"]
    k = live_rows(count, 0, x0.shape[0])
    g0, g1 = counted_stack(ops, third["P"], THIRD_NAMES, x0, x1, k, count)
    what = "third-level stack, count %d" % count
    assert_rows_hold(g0, k, SENTINEL, what + ", set 0")
    assert_rows_hold(g1, k, SENTINEL, what + ", set 1")
    if k:
        w0, w1 = ops.attentional_gnn(x0[:k], x1[:k], third["P"], THIRD_NAMES)
        assert_same(g0[:k], w0, what + ", set 0")
        assert_same(g1[:k], w1, what + ", set 1")
        assert_oracle(g0, g1, third_oracle, (0, k - 1), STACK_TOL, what)


@pytest.mark.parametrize("count_off", [0, 3])
def test_third_single_layer_counted(ops, oracle, third, count_off):
    p, P = third["ps"][1], third["P"][1]
    x, s = third["x0"], third["x1"]
    b = x.shape[0]
    counts = [count_off + c for c in THIRD_COUNTS] + ([count_off - 2] if count_off else [])
    ks = [live_rows(c, count_off, b) for c in counts]
    rows = sorted({q for k in ks if k for q in (0, k - 1)})
    want = oracle.attentional_propagation(host(x[rows]), host(s[rows]), p, residual=host(x[rows]))
    for count, k in zip(counts, ks):
        what = "third-level layer, count %d - %d" % (count, count_off)
        got = counted_layer(ops, P, x, s, x, k, count, count_off)
        assert_rows_hold(got, k, SENTINEL, what)
        if k:
            assert_same(got[:k], uncounted_prefix(ops, P, x, s, x, k), what)
            for q in (0, k - 1):
                np.testing.assert_allclose(host(got[q]), want[rows.index(q)], err_msg="%s: row %d" % (what, q), **STACK_TOL)


LAYER_COUNTS = [32000, 32768, 32769, 32868]


@pytest.fixture(scope="module")
def third_big(ops, oracle, third):
    assert ops.GNN_LAYER_ROWS == 32768
    b = ops.GNN_LAYER_ROWS + 100
    g = torch.Generator(device="cuda")
    g.manual_seed(1620)
    x0 = torch.randn((b, 128, 65), device="cuda", generator=g)
    x1 = torch.randn((b, 128, 65), device="cuda", generator=g)
    rows = {r for c in LAYER_COUNTS for r in (32767, 32768, c - 1) if r < c}
    return x0, x1, oracle_rows(oracle, third["ps"], THIRD_NAMES, x0, x1, rows)


@pytest.mark.parametrize("count", LAYER_COUNTS)
def test_third_stack_counted_across_a_block(ops, third, third_big, count):
    """The layer-by-layer path runs in blocks of GNN_LAYER_ROWS rows with count_off = the block's first row."""
    x0, x1, ref = third_big
    k = live_rows(count, 0, x0.shape[0])
    g0, g1 = counted_stack(ops, third["P"], THIRD_NAMES, x0, x1, k, count)
    what = "third-level stack of %d rows, count %d" % (x0.shape[0], count)
    assert_rows_hold(g0, k, SENTINEL, what + ", set 0")
    assert_rows_hold(g1, k, SENTINEL, what + ", set 1")
    w0, w1 = ops.attentional_gnn(x0[:k], x1[:k], third["P"], THIRD_NAMES)
    assert_same(g0[:k], w0, what + ", set 0")
    assert_same(g1[:k], w1, what + ", set 1")
    assert_oracle(g0, g1, ref, [r for r in (32767, 32768, k - 1) if r < k], STACK_TOL, what)


# ---- an activation beyond the fp16 range together with a count ------------------------------------------------------------------
OVERFLOW_KINDS = ["fine_stack", "fine_layer", "third_layer", "third_stack"]


def overflow_case(fine, third, kind):
    """One counted entry point as (run(ops, x0, x1, k, count) -> outputs, uncounted(ops, x0, x1, k) -> outputs,
    reference(oracle, x0, x1, rows) -> {row: outputs}, the bits of rows past the count, count_off, its data)."""
    if kind in ("fine_stack", "third_stack"):
        d = fine if kind == "fine_stack" else third
        names = FINE_NAMES if kind == "fine_stack" else THIRD_NAMES[:2]
        layers, ps = d["P"][:len(names)], d["ps"][:len(names)]
        return (lambda ops, x0, x1, k, c: counted_stack(ops, layers, names, x0, x1, k, c),
                lambda ops, x0, x1, k: ops.attentional_gnn(x0[:k], x1[:k], layers, names),
                lambda oracle, x0, x1, rows: oracle_rows(oracle, ps, names, x0, x1, rows),
                0 if kind == "fine_stack" else SENTINEL, 0, d)
    d = fine if kind == "fine_layer" else third
    p, P, off = d["ps"][0], d["P"][0], (5 if kind == "fine_layer" else 3)
    extra = d["r"] if kind == "fine_layer" else None         # the fine layer with a residual of its own (the conversion out adds it)

    def reference(oracle, x0, x1, rows):
        res = extra if extra is not None else x0
        y = oracle.attentional_propagation(host(x0[rows]), host(x1[rows]), p, residual=host(res[rows]))
        return {q: (y[i],) for i, q in enumerate(rows)}
    return (lambda ops, x0, x1, k, c: (counted_layer(ops, P, x0, x1, extra if extra is not None else x0, k, c, off),),
            lambda ops, x0, x1, k: (uncounted_prefix(ops, P, x0, x1, extra if extra is not None else x0, k),),
            reference, 0 if kind == "fine_layer" else SENTINEL, off, d)


@pytest.mark.parametrize("kind", OVERFLOW_KINDS)
def test_overflow_in_a_live_row_keeps_the_count_contract(ops, oracle, fine, third, kind):
    """A spike in the last live row of set 0: deferred mode raises the flag (the spike does overflow); inline mode redoes the call
    in the gated composition over the whole capacity - live rows finite and right, rows past the count still zeros (fine level) or
    untouched (third level)."""
    run, uncounted, reference, pad, off, d = overflow_case(fine, third, kind)
    k = 17 if kind.startswith("fine") else 40
    count = k + off
    x0, x1 = d["x0"].clone(), d["x1"]
    x0[k - 1, 7, 33] = SPIKE
    prev = ops.set_gnn_redo("deferred")
    try:
        ops.gnn_overflows(reset=True)
        run(ops, x0, x1, k, count)
        assert ops.gnn_overflows(reset=True), "%s: the spike in a live row did not raise the overflow flag" % kind
    finally:
        assert ops.set_gnn_redo(prev) == "deferred"
    got = run(ops, x0, x1, k, count)
    clean = uncounted(ops, d["x0"], x1, k)
    want = reference(oracle, x0, x1, [0, k - 1])
    for i, g in enumerate(got):
        what = "%s, spike in row %d, count %d - %d, output %d" % (kind, k - 1, count, off, i)
        assert torch.isfinite(g[:k]).all(), what
        assert_rows_hold(g, k, pad, what)
        np.testing.assert_allclose(host(g[0]), want[0][i], err_msg=what + ": row 0", **STACK_TOL)
        np.testing.assert_allclose(host(g[k - 1]), want[k - 1][i], err_msg=what + ": the spiked row", **SPIKE_TOL)
        # the rows the spike does not reach: the composition's arithmetic against the one-kernel layer's
        np.testing.assert_allclose(host(g[:k - 1]), host(clean[i][:k - 1]), err_msg=what, **STACK_TOL)


@pytest.mark.parametrize("kind", OVERFLOW_KINDS)
def test_deferred_spike_in_a_padding_row_leaves_the_flag_down(ops, fine, third, kind):
    """Deferred mode, a spike in the first padding row (besides the hostile pattern): no layer reads it - the flag stays down and
    the live rows are the clean run's bits."""
    run, uncounted, _, pad, off, d = overflow_case(fine, third, kind)
    k = 17 if kind.startswith("fine") else 40
    count = k + off
    x0, x1 = d["x0"].clone(), d["x1"]
    clean = uncounted(ops, x0, x1, k)
    x0[k, 7, 33] = SPIKE
    prev = ops.set_gnn_redo("deferred")
    try:
        ops.gnn_overflows(reset=True)
        got = run(ops, x0, x1, k, count)
        raised = ops.gnn_overflows(reset=True)
    finally:
        assert ops.set_gnn_redo(prev) == "deferred"
    assert not raised, "%s: the padding rows raised the overflow flag" % kind
    for i, g in enumerate(got):
        what = "%s deferred, count %d - %d, output %d" % (kind, count, off, i)
        assert_same(g[:k], clean[i], what)
        assert_rows_hold(g, k, pad, what)


# ---- what the count does not cover -------------------------------------------------------------------------------------------------
def test_bn_train_with_a_count_is_refused(ops, fine, third):
    """Batch statistics over a capacity would take in the padding rows: the combination is refused before anything is launched
    (ops and the C-ABI) instead of the count being ignored."""
    x0, x1 = padded(third["x0"], 20), padded(third["x1"], 20)
    out = (sentinel_like(x0), sentinel_like(x1))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="bn_train.*count"):
        ops.attentional_propagation(x0, x1, third["P"][0], bn_train=True, count=dev_count(20), out=out[0])
    with pytest.raises(RuntimeError, match="bn_train.*count"):
        ops.attentional_gnn(x0, x1, third["P"][:2], THIRD_NAMES[:2], bn_train=True, count=dev_count(20), out=out)
    f0, f1 = padded(fine["x0"], 9), padded(fine["x1"], 9)
    fout = (sentinel_like(f0), sentinel_like(f1))
    with pytest.raises(RuntimeError, match="bn_train.*count"):
        ops.attentional_gnn(f0, f1, fine["P"], FINE_NAMES, bn_train=True, count=dev_count(9), out=fout)
    # the C entry point on its own
    P = third["P"][0]
    b, C, n = x0.shape
    nb = ops._L().pats_attentional_propagation_workspace_bytes(b, C, n, n)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    w = P.struct(True)
    cnt = dev_count(20)
    rc = ops._L().pats_attentional_propagation_packed_counted_f32(ops._ptr(x0), ops._ptr(x1), b, ops._ptr(cnt), 0, C, 4, n, n,
                                                                  ctypes.byref(w), ops._ptr(P.packed(4)), 1, float(P.eps), ops._ptr(x0),
                                                                  ops._ptr(out[0]), ops._ptr(ws), nb, ops._stream())
    assert rc != 0 and "bn_train" in ops._L().pats_last_error().decode()
    torch.cuda.synchronize()
    for t, name in ((out[0], "set 0"), (out[1], "set 1"), (fout[0], "fine set 0"), (fout[1], "fine set 1")):
        assert_rows_hold(t, 0, SENTINEL, "refused call, " + name)


def test_count_at_a_shape_without_a_one_kernel_layer(ops, oracle):
    """[2, 448, 300] (the coarse level's width) has no one-kernel layer: the count is ignored there, every row is computed.  Only the
    live row is pinned down, against the oracle."""
    ps = [synth.gnn_params(seed=1700 + i, C=448) for i in range(2)]
    P = [ops.PropagationParams(p) for p in ps]
    a = synth.gnn_inputs(seed=1710, b=2, C=448, n=300)
    x0, x1 = padded(cu(a["x"]), 1), padded(cu(a["source"]), 1)
    y = ops.attentional_propagation(x0, x1, P[0], residual=x0, count=dev_count(1))
    want = oracle.attentional_propagation(a["x"][:1], a["source"][:1], ps[0], residual=a["x"][:1])
    np.testing.assert_allclose(host(y[:1]), want, **STACK_TOL)
    g0, g1 = ops.attentional_gnn(x0, x1, P, ["self", "cross"], count=dev_count(1))
    r0, r1 = oracle_stack(oracle, ps, ["self", "cross"], a["x"][:1], a["source"][:1])
    np.testing.assert_allclose(host(g0[:1]), r0, **STACK_TOL)
    np.testing.assert_allclose(host(g1[:1]), r1, **STACK_TOL)
