"""-m gpu: the GNN layers' three fp16-split attention cores on peaked and long-tailed softmax rows, on the case table of
tests/attention_cases.py (tests/test_attention_cases_host.py holds the table, the split model and the CPU oracle to the same gate):

* the third level's fused layer (csrc/gnn_fused.hip) through ops.attentional_propagation at [b, 128, 65];
* gnn_fine_attn_kernel (csrc/gnn_fine.hip) through ops.attentional_propagation at [b, 264, 145], source = another tensor and
  source = x, and through a two-layer ops.attentional_gnn stack whose second layer has the designed rows;
* attention145_kernel (csrc/attention145.hip) through ops.attentional_propagation at the corners of its box;
* attention65_kernel through ops.attention(return_prob=False) on the fused layer's q, k, v (measured, like the general kernel).

Every other layer test of the suite shows these kernels near-uniform rows (every probability above both thresholds of the
probabilities' fp16 split, attention_cases.P_HI / P_LO); here one key dominates, the tail sits below one threshold or the other, a
row crosses both, the top is a near-tie, or ONE designed key carries the whole row - which puts a whole value on a misplaced key
slot where a near-uniform row puts 1 / 145 of one.

Gate, with V = max(1, max|v|) and E32 the fp32 formula's own error on the case: |out - ref64| <= max(2e-5 V, 4 E32) + 1e-5 |ref64|.
All calls run under ops.set_gnn_redo('deferred') and assert that no overflow flag rose: in inline mode a raised flag hands the
launch to the fp32 composition and the test would measure that.  Each test prints its largest error as a share of the gate and,
for information, the general fp32 kernel's on the same q, k, v (pytest -rA); docs/parity.md, "Attention cores on non-uniform
softmax rows", holds the table and what four deliberately wrong builds do to these tests."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import attention_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


@contextlib.contextmanager
def deferred(ops):
    prev = ops.set_gnn_redo("deferred")
    try:
        ops.gnn_overflows(reset=True)
        yield
    finally:
        ops.set_gnn_redo(prev)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


_PARAMS = {}


def params_of(ops, c):
    if c.name not in _PARAMS:
        _PARAMS.clear()                               # (one case's weights at a time)
        _PARAMS[c.name] = [ops.PropagationParams(p) for p in c.layers]
    return _PARAMS[c.name]


def launch(ops, c, x, source):
    """The layer entry point that reaches the case's kernel -> the outputs, one per side."""
    P = params_of(ops, c)
    if c.mode == "stack":
        return list(ops.attentional_gnn(x, source, P, c.names))
    return [ops.attentional_propagation(x, x if c.mode == "self" else source, P[0])]


def run_twice(ops, fn, inputs):
    """fn() twice under the deferred protocol: no flag, finite outputs, equal bits, inputs untouched -> float64 outputs."""
    before = [t.clone() for t in inputs]
    with deferred(ops):
        first = fn()
        assert not ops.gnn_overflows(reset=True), "the overflow flag rose: the case left the fp16 range"
        second = fn()
        assert not ops.gnn_overflows(reset=True)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert bool(torch.isfinite(a).all()), "non-finite output"
        assert torch.equal(bits(a), bits(b)), "two launches differ"
    for t, b in zip(inputs, before):
        assert torch.equal(bits(t), bits(b)), "an input was written"
    return [a.cpu().numpy().astype(np.float64) for a in first]


def general_error(ops, s):
    """For information: the general fp32 kernel (ops.attention with the probabilities returned) on the same q, k, v."""
    out, _ = ops.attention(cu(s.q), cu(s.k), cu(s.v), return_prob=True)
    return float(np.abs(out.cpu().numpy().astype(np.float64) - s.att).max())


def report(name, what, err, gate, extra=""):
    sh = np.abs(err) / gate
    at = int(sh.argmax())
    print("%s: %s largest error = %.3f of the gate (|d| = %.2e of %.2e there; largest |d| anywhere %.2e)%s"
          % (name, what, float(sh.max()), float(np.abs(err).flat[at]), float(np.broadcast_to(gate, err.shape).flat[at]),
             float(np.abs(err).max()), extra))
    return float(sh.max())


def check_selector(c, s, out):
    """Every query returns the value of its designed key: |out - v[:, pi(i)]| <= 2e-5 V."""
    got = out.reshape(c.b, c.dim, ac.HEADS, c.n)
    worst = 0.0
    for (bi, h), info in s.infos.items():
        want = s.v[bi, :, h][:, info["pi"]].astype(np.float64)
        worst = max(worst, float(np.abs(got[bi, :, h] - want).max()))
    print("%s: selector, largest |out - v[:, pi(i)]| = %.2e = %.3f of 2e-5 V" % (c.name, worst, worst / (ac.FLOOR * s.V)))
    assert worst <= ac.FLOOR * s.V


def layer_case(ops, name):
    c = ac.case(name)
    x, source = cu(c.x), cu(c.source)
    outs = run_twice(ops, lambda: launch(ops, c, x, source), [x, source])
    worst = 0.0
    for j, (s, out) in enumerate(zip(c.sides, outs)):
        assert out.shape == s.ref.shape
        worst = max(worst, report(name, "side %d," % j, out - s.ref, s.gate(), "; general fp32 kernel |d| = %.2e" % general_error(ops, s)))
        if c.family == "selector" and c.mode != "stack":
            check_selector(c, s, out)
    assert worst <= 1.0, "%s: %.3f of the gate" % (name, worst)


@pytest.mark.parametrize("name", ac.names_of("fused"))
def test_fused_layer_core(ops, name):
    layer_case(ops, name)


@pytest.mark.parametrize("name", ac.names_of("fine"))
def test_fine_attn_core(ops, name):
    layer_case(ops, name)


@pytest.mark.parametrize("name", ac.names_of("a145"))
def test_attention145_core(ops, name):
    layer_case(ops, name)


@pytest.mark.parametrize("name", ac.names_of("fused"))
def test_attention65_on_the_same_rows(ops, name):
    c = ac.case(name)
    s = c.sides[0]
    q, k, v = cu(s.q), cu(s.k), cu(s.v)
    out, = run_twice(ops, lambda: [ops.attention(q, k, v, return_prob=False)[0]], [q, k, v])
    worst = report(name, "attention65_kernel,", out - s.att, s.gate(s.att), "; general fp32 kernel |d| = %.2e" % general_error(ops, s))
    if c.family == "selector":
        check_selector(c, s, out)
    assert worst <= 1.0, "%s: %.3f of the gate" % (name, worst)
