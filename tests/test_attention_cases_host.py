"""Host side (-m "not gpu", oracle only): tests/attention_cases.py is held to what tests/test_attention_edges_gpu.py relies on.
The float64 references agree with the CPU oracle (oracle.attention, oracle.attentional_propagation) within the GPU tests' own
gate; every family realises the softmax profile it promises, counted against the two thresholds of the probabilities' fp16 split;
the fp32 evaluation's error E32 stays below 5e-6 outside the large-magnitude family, so the gate there is its 2e-5 floor; the
split model's two predictions are printed per case (pytest -rA) and the 'keep' one - subnormal halves take part - passes every
gate: the cases ask no more than the arithmetic can give."""
import numpy as np
import pytest

import attention_cases as ac


def share(err, gate):
    return float((np.abs(err) / gate).max())


def sides_of(name):
    return ac.case(name).sides


# ---- the references against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.NAMES)
def test_references_agree_with_the_oracle(oracle, name):
    c = ac.case(name)
    worst = 0.0
    for s in c.sides:
        out, _ = oracle.attention(s.q, s.k, s.v, with_prob=False)
        worst = max(worst, share(out - s.att, s.gate(s.att)))
    if c.mode == "stack":
        d0, d1 = c.x, c.source
        for p, nm in zip(c.layers, c.names):
            s0, s1 = (d1, d0) if nm == "cross" else (d0, d1)
            d0, d1 = (oracle.attentional_propagation(d0, s0, p, residual=d0), oracle.attentional_propagation(d1, s1, p, residual=d1))
        outs = [d0, d1]
    else:
        outs = [oracle.attentional_propagation(c.x, c.source, c.layers[0])]
    for s, o in zip(c.sides, outs):
        worst = max(worst, share(o - s.ref, s.gate()))
    print("%s: the oracle's largest error = %.3f of the gate" % (name, worst))
    assert worst <= 1.0


def test_readout_layer_returns_its_attention():
    """The layer reference of a read-out layer is its attention reference but for BatchNorm's 1 / sqrt(1 + eps)."""
    for name in ("fused_graded", "fine_self_tail_hi_b1"):
        c = ac.case(name)
        s = c.sides[0]
        assert np.abs(s.ref * np.sqrt(1.0 + ac.EPS) - s.att.reshape(s.ref.shape)).max() <= 1e-12 * s.V


# ---- every family realises its profile --------------------------------------------------------------------------------------------
def rows_of(name):
    """(probabilities [m], scores-in-nats deviation, info, query index) of every row of the active heads of a case's first side."""
    s = sides_of(name)[0]
    for (bi, h), info in s.infos.items():
        for i in range(s.prob.shape[2]):
            yield s.prob[bi, h, i], info, i


@pytest.mark.parametrize("name", ac.NAMES)
def test_family_realises_its_profile(name):
    c = ac.case(name)
    fam, m = c.family, c.m
    stds = []
    for p, info, i in rows_of(name):
        lo, mid = p < ac.P_HI, (p >= ac.P_HI) & (p < ac.P_LO)
        n_lo, n_mid, n_up = int(lo.sum()), int(mid.sum()), int((p >= ac.P_LO).sum())
        if fam == "selector":
            assert p[info["pi"][i]] > 1.0 - 1e-6 and n_lo == m - 1
        elif fam == "tail_hi":
            d = info["dom"][i][0]
            rest = np.delete(p, d)
            assert p[d] > 0.9998 and n_lo == m - 1 and rest.min() >= 2e-7 and rest.max() <= 9e-7
        elif fam == "tail_lo":
            d = info["dom"][i][0]
            rest = np.delete(p, d)
            assert p[d] > 0.4 and n_mid == m - 1 and n_up == 1 and rest.min() >= 1e-3 and rest.max() <= 3.8e-3
            assert 0.05 <= p[mid].sum() <= 0.6
        elif fam == "graded":
            assert min(n_lo, n_mid, n_up) >= 5 and p.min() <= 3e-9 and 0.05 <= p.max() <= 0.2
            assert abs(np.log10(p.max() / p.min()) - 8.0) < 0.1
        elif fam in ("ties2", "tiesk"):
            kk = 2 if fam == "ties2" else 5
            d = info["dom"][i]
            assert len(d) == kk and np.all(np.abs(p[d] - 1.0 / kk) <= 1e-3 / kk) and n_lo == m - kk
            assert np.log(p[d].max() / p[d].min()) <= 1e-3 and np.delete(p, d).max() < 1e-9
        else:
            stds.append(np.log(p).std())
    if stds:
        want = ac.RANDOM_STD[fam]
        assert 0.7 * want <= np.mean(stds) <= 1.3 * want, np.mean(stds)
        if fam == "uniform":                   # today's regime: every probability above both thresholds... at 65 keys; at 145 all
            pmin = min(p.min() for p, _, _ in rows_of(name))          # above the hi threshold by three orders
            assert pmin > 1e-3


@pytest.mark.parametrize("kernel", ["fused", "fine", "a145"])
def test_selector_covers_every_key_slot(kernel):
    """pi hits key 0 and key m - 1, and every key of every shape is selected by some query of some problem."""
    for name in ac.names_of(kernel):
        c = ac.case(name)
        if c.family != "selector":
            continue
        hit = np.zeros(c.m, bool)
        for info in c.sides[0].infos.values():
            assert len(set(info["pi"])) == min(c.n, c.m) or c.n > c.m
            hit[info["pi"]] = True
        assert hit.all() and hit[0] and hit[c.m - 1], name
        first = c.sides[0].infos[0, c.active[0]]["pi"]
        assert np.array_equal(first, ((7 if c.m % 7 else 11) * np.arange(c.n) + 3) % c.m)


def test_stack_second_layer_keeps_the_family():
    """The first layer of a stack case moves the descriptors so little that the second layer's rows are the family's."""
    for name, (lo, hi) in (("fine_stack_tail_hi_b1", (2e-7, 9e-7)), ("fine_stack_tail_lo_b5", (1e-3, 3.8e-3))):
        s = sides_of(name)[0]
        srt = np.sort(s.prob, -1)
        assert srt[..., :-1].min() >= lo and srt[..., :-1].max() <= hi, (name, srt[..., :-1].min(), srt[..., :-1].max())


# ---- ranges and E32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.NAMES)
def test_ranges_and_e32(name):
    c = ac.case(name)
    assert c.b <= 8
    for x in (c.x, c.source):                          # exact in the fp16 hi + lo operands, inside the range no flag rises in
        assert np.array_equal(ac.bits20(x), x.astype(np.float64)) and np.abs(x).max() < 1023 / 2
    for j, s in enumerate(c.sides):
        assert max(np.abs(s.q).max(), np.abs(s.k).max(), np.abs(s.v).max()) < 1023 / 2
        if c.family != "large" and j == 0:
            sc = np.matmul(s.q.astype(np.float64).transpose(0, 2, 3, 1), s.k.astype(np.float64).transpose(0, 2, 1, 3)) / np.sqrt(c.dim)
            assert np.abs(sc).max() <= 40.0
            assert s.E32 < 5e-6, s.E32


# ---- the split model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.NAMES)
def test_split_model_keep_passes_every_gate(name):
    for j, s in enumerate(sides_of(name)):
        g = s.gate(s.att)
        got = {(fl, sh): share(ac.split_model(s.q, s.k, s.v, fl, sh) - s.att, g) for fl in (False, True) for sh in (6, 14)}
        print("%s side %d: split model, largest error as a share of the gate: 2^6 keep %.3f flush %.3f | 2^14 keep %.3f flush %.3f"
              % (name, j, got[False, 6], got[True, 6], got[False, 14], got[True, 14]))
        assert got[False, 6] <= 1.0 and got[False, 14] <= 1.0
