"""GPU: ops.epipolar_hypotheses_by_pair / batch.hypothesize_by_pair against the definition of include/pats_amd.h restated in numpy
(tests/hypotheses_cases.py):
    sample_idx   equals the restatement bit for bit (integer arithmetic: nothing to round)
    models       exactly zero where the definition says so (n < 8, a non-finite sample coordinate), otherwise finite with
                 | |e| - 1 | <= 1e-5, the component of largest magnitude positive, and - the accuracy contract - a backward error
                 |A e|_2 <= B eps32 |A|_F with B = MARGIN * b32, b32 = what numpy's float32 svd reaches on the same samples in the
                 same run.  Measured: b32 = 0.155, the device 0.19 (B = 1.24); docs/parity.md records both
Every output lies inside a larger sentinel-filled buffer and every input list in a larger NaN-filled one: the call must define every
byte of the views, none around them, and read no row beyond cap (a NaN row in a sample would zero a model that must not be zero)."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import hypotheses_cases as hc

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I = -777.25, -123456


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bound():
    """B = MARGIN * b32, the baseline measured in this run on the tolerance cases (shared, computed once)."""
    b32 = hc.baseline32()
    assert np.isfinite(b32) and b32 > 0
    return hc.MARGIN * b32, b32


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_lists(ml, mr):
    """The lists as views of longer buffers whose rows beyond cap are NaN."""
    out = []
    for a in (ml, mr):
        buf = torch.full((a.shape[0] + PAD, 2), float("nan"), dtype=torch.float32, device="cuda")
        buf[:a.shape[0]] = cu(a)
        out.append(buf[:a.shape[0]])
    return out


def run(ops, ml, mr, H, seeds, samples=True, **kw):
    """One call on fresh sentinel buffers -> (models, sample_idx) as numpy arrays (the surroundings checked)."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs = len(seeds)
    bm = torch.full((pairs * H * 9 + 2 * PAD,), SENT_F, dtype=torch.float32, device="cuda")
    bi = torch.full((pairs * H * 8 + 2 * PAD,), SENT_I, dtype=torch.int32, device="cuda")
    vm, vi = bm[PAD:-PAD].view(pairs, H, 3, 3), bi[PAD:-PAD].view(pairs, H, 8)
    gl, gr = guarded_lists(ml, mr)
    got = ops.epipolar_hypotheses_by_pair(gl, gr, H, cu(np.asarray(seeds, np.int64)), return_samples=samples,
                                          out=(vm, vi) if samples else vm, **d)
    torch.cuda.synchronize()
    if samples:
        assert len(got) == 2 and got[0].data_ptr() == vm.data_ptr() and got[1].data_ptr() == vi.data_ptr()
    else:
        assert got.data_ptr() == vm.data_ptr() and bool((bi == SENT_I).all())
    assert bool((torch.cat([bm[:PAD], bm[-PAD:]]) == SENT_F).all()) and bool((torch.cat([bi[:PAD], bi[-PAD:]]) == SENT_I).all()), \
        "bytes around an output view changed"
    return vm.cpu().numpy(), vi.cpu().numpy()


def check(got, ref, B=None, nonzero=True):
    """Both outputs against the restatement; -> the largest backward-error ratio."""
    models, idx = got
    assert models.dtype == np.float32 and idx.dtype == np.int32
    for p, r in enumerate(ref):
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        if r["n"] < 8:
            assert not models[p].any() and (idx[p] == -1).all()
        elif nonzero:                                                     # a generic sample: zero ONLY where the definition says so
            assert np.array_equal(models[p].reshape(-1, 9).any(1), r["finite"]), "pair %d: a zero model on a finite sample" % p
    return hc.check_models(models, ref, B)


NORM = np.array([[0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3]], np.float32)


def norm_for(pairs):
    return np.ascontiguousarray(NORM * np.linspace(0.9, 1.1, pairs, dtype=np.float32)[:, None])


# ---- 1. exactness and edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_ragged_lengths_around_eight_and_hypothesis_counts_around_the_workgroup(ops, bound, H):
    lengths = [0, 7, 8, 9, 600, 64]
    ml, mr, off = hc.make_pairs(lengths, seed=100 + H)
    ml, mr = np.concatenate([ml, ml[:23]]), np.concatenate([mr, mr[:23]])              # rows inside cap behind the last segment
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    seeds = [5000 + H + 3 * p for p in range(len(lengths))]
    for norm in (None, norm_for(len(lengths))):
        for progressive in (False, True):
            got = run(ops, ml, mr, H, seeds, pair_off=off, norm=norm, progressive=progressive)
            check(got, hc.reference(ml, mr, segs, seeds, H, progressive, norm), B=bound[0])
    only = run(ops, ml, mr, H, seeds, samples=False, pair_off=off)                     # sample_idx is optional
    both = run(ops, ml, mr, H, seeds, pair_off=off)
    assert np.array_equal(only[0].view(np.int32), both[0].view(np.int32))


def test_strided_segments_and_clamped_counts(ops, bound):
    stride, counts = 16, np.array([8, 16, 3, 20], np.int64)                             # 20 is clamped to 16
    ml, mr, _ = hc.make_pairs([stride] * 4 + [9], seed=200)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 8), (16, 16), (32, 3), (48, 16)]
    seeds = [1, 2, 3, 4]
    for norm in (None, norm_for(4)):
        for progressive in (False, True):
            got = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts, norm=norm, progressive=progressive)
            check(got, hc.reference(ml, mr, segs, seeds, 65, progressive, norm), B=bound[0])
    # the same rows in the ragged form: the same bits
    off = np.array([0, 8], np.int64)
    a = run(ops, ml, mr, 65, seeds[:1], pair_off=off)
    b = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    assert np.array_equal(a[0][0].view(np.int32), b[0][0].view(np.int32)) and np.array_equal(a[1][0], b[1][0])
    # top-K shaped inputs [pairs,K,2] are taken as the flat lists they are
    c = ops.epipolar_hypotheses_by_pair(cu(ml[:64].reshape(4, 16, 2)), cu(mr[:64].reshape(4, 16, 2)), 65, cu(np.asarray(seeds, np.int64)),
                                        stride=stride, counts=cu(counts))
    assert np.array_equal(c.cpu().numpy().view(np.int32), run(ops, ml[:64], mr[:64], 65, seeds, stride=stride, counts=counts)[0].view(np.int32))


def test_stale_offsets_are_clamped(ops, bound):
    ml, mr, _ = hc.make_pairs([300], seed=300)
    cap = ml.shape[0]
    for bad in (np.array([-50, 120, 40, cap + 100000], np.int64),                       # negative, descending (empty), past cap
                np.array([cap + 5, cap + 9, 2 ** 40, -2 ** 40], np.int64)):
        segs = ec.segments(3, cap, pair_off=bad)
        got = run(ops, ml, mr, 40, [7, 8, 9], pair_off=bad)
        check(got, hc.reference(ml, mr, segs, [7, 8, 9], 40), B=bound[0])
    assert ec.segments(3, cap, pair_off=np.array([-50, 120, 40, cap + 100000])) == [(0, 120), (120, 0), (40, cap - 40)]
    longer = np.array([0, 100, 300, 12345, -1, 7], np.int64)                            # a longer buffer that starts with the offsets
    got = run(ops, ml, mr, 9, [1, 2], pair_off=longer, pairs=2)
    check(got, hc.reference(ml, mr, [(0, 100), (100, 200)], [1, 2], 9), B=bound[0])


def test_empty_arrays_define_every_output(ops):
    z2 = np.zeros((0, 2), np.float32)
    m, i = run(ops, z2, z2, 70, [1, 2], pair_off=np.zeros(3, np.int64))
    assert not m.any() and (i == -1).all()


# ---- 2. awkward geometry ------------------------------------------------------------------------------------------------------
def test_sideways_translation_has_a_zero_last_component(ops, bound):
    """R = I, t = (1, 0, 0), no noise: E = [t]_x = e7 - e5 (up to scale) has e[8] = 0 - a solver that pins e[8] = 1 cannot find it."""
    rng = np.random.default_rng(41)
    n, H = 200, 256
    Z = rng.uniform(3.0, 8.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.6, 0.6, n) * Z, Z], 1)
    ml = (X[:, :2] / Z[:, None]).astype(np.float32)
    mr = ml.copy()
    mr[:, 0] = ((X[:, 0] + 1.0) / Z).astype(np.float32)                                 # y is the same float32 on both sides
    got = run(ops, ml, mr, H, [99], pair_off=np.array([0, n], np.int64))
    ref = hc.reference(ml, mr, [(0, n)], [99], H)
    worst = check(got, ref, B=bound[0])
    e = got[0][0].reshape(H, 9).astype(np.float64)
    true = np.zeros(9)
    true[5], true[7] = -np.sqrt(0.5), np.sqrt(0.5)
    err = np.minimum(np.abs(e - true).max(1), np.abs(e + true).max(1))
    print("sideways translation: worst backward error %.3f eps32 |A|_F, median distance to E %.2e, median |e[8]| %.2e"
          % (worst, np.median(err), np.median(np.abs(e[:, 8]))))
    assert np.median(err) < 1e-4 and np.median(np.abs(e[:, 8])) < 1e-4


def test_eight_identical_matches_give_zero_or_finite_unit_models(ops):
    ml, mr, _ = hc.make_pairs([1, 30], seed=400)
    ml, mr = np.concatenate([np.repeat(ml[:1], 8, 0), ml[1:]]), np.concatenate([np.repeat(mr[:1], 8, 0), mr[1:]])
    segs = [(0, 8), (8, 30)]
    got = run(ops, ml, mr, 70, [11, 12], pair_off=np.array([0, 8, 38], np.int64))
    check(got, hc.reference(ml, mr, segs, [11, 12], 70), nonzero=False)                 # zero or finite unit, the sign rule
    assert got[0][1].reshape(70, 9).any(1).all()                                        # the neighbour is unaffected


def test_a_nan_coordinate_zeroes_exactly_the_samples_that_hold_it(ops, bound):
    ml, mr, off = hc.make_pairs([40, 40], seed=500)
    ml[5, 1], mr[40 + 17, 0] = np.nan, np.inf
    H = 200
    got = run(ops, ml, mr, H, [21, 22], pair_off=off)
    ref = hc.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H)
    check(got, ref, B=bound[0])                                                         # zero iff not finite (nonzero=True)
    for p, row in ((0, 5), (1, 17)):
        hit = (got[1][p] == row).any(1)
        assert 10 < hit.sum() < H - 10 and np.array_equal(~got[0][p].reshape(H, 9).any(1), hit)
    norm = norm_for(2)
    norm[1, 6] = np.inf                                                                 # a non-finite x after norm: the whole pair
    got = run(ops, ml, mr, H, [21, 22], pair_off=off, norm=norm)
    check(got, hc.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H, norm=norm), B=bound[0])
    assert not got[0][1].any() and (got[1][1] >= 0).all()


# ---- 3. tolerance -------------------------------------------------------------------------------------------------------------
def test_backward_error_against_eight_times_the_float32_svd(ops, bound):
    B, b32 = bound
    cases = hc.tolerance_cases()
    ml, mr = np.concatenate([c[0] for c in cases]), np.concatenate([c[1] for c in cases])
    H = hc.TOLERANCE_CASES[0][2]
    seeds = [c[3] for c in hc.TOLERANCE_CASES]
    off = np.concatenate([[0], np.cumsum([c[1] for c in hc.TOLERANCE_CASES])]).astype(np.int64)
    got = run(ops, ml, mr, H, seeds, pair_off=off)
    ref = hc.reference(ml, mr, ec.segments(3, ml.shape[0], pair_off=off), seeds, H)
    assert all(np.array_equal(r["idx"], c[2]) for r, c in zip(ref, cases))              # the samples b32 was measured on
    worst = check(got, ref)
    print("backward error over %d samples: device %.4f, b32 %.4f, B = %.1f * b32 = %.4f" % (3 * H, worst, b32, hc.MARGIN, B))
    assert worst <= B


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_are_byte_identical_and_the_seed_matters(ops):
    ml, mr, off = hc.make_pairs([600, 64, 9], seed=600)
    a = run(ops, ml, mr, 257, [1, 2, 3], pair_off=off, progressive=True)
    b = run(ops, ml, mr, 257, [1, 2, 3], pair_off=off, progressive=True)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    c = run(ops, ml, mr, 257, [1, 2 + 2 ** 32, 3], pair_off=off, progressive=True)     # the high half of the seed counts
    assert np.array_equal(a[1][0], c[1][0]) and np.array_equal(a[1][2], c[1][2]) and not np.array_equal(a[1][1], c[1][1])
    assert np.array_equal(a[0][0].view(np.int32), c[0][0].view(np.int32))


# ---- 5. through the batch path ------------------------------------------------------------------------------------------------
def test_hypothesize_then_verify_finds_the_true_model():
    from pats_amd import batch
    H, thr = 512, np.float32(2e-3)
    cases = [ec.make_case(seed, 600, 4, outliers=0.3) for seed in (11, 12, 13, 14)]
    ml, mr = np.concatenate([c["ml"] for c in cases]), np.concatenate([c["mr"] for c in cases])
    cap = batch.Capacities(4, 5, 6)
    summary = np.array([0, 600, 1200, 1800, 2400, 2400, 0, 0], np.int64)                # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:5]), "summary": ds}
    models, idx = batch.hypothesize_by_pair(out, cap, H, seed=2024, on="all", progressive=False, samples=True)
    assert out["hypotheses"][0] is models and tuple(models.shape) == (4, H, 3, 3) and tuple(idx.shape) == (4, H, 8)
    ver = batch.verify_by_pair(out, cap, models, cu(np.full(4, thr, np.float32)))
    idx_h, best_count = idx.cpu().numpy(), ver[2].cpu().numpy()
    for p, c in enumerate(cases):
        assert np.array_equal(idx_h[p], hc.sample_idx(2024 + p, 600, H))                # pair_seed = seed + p
        xl, xr = ec.points32(c["ml"], c["mr"])
        part = ec.participates(xl, xr)
        inl, dec = ec.classify(xl, xr, part, c["models"][c["true"]], thr)
        true_count = int((inl & dec).sum())
        e64 = hc.null64(hc.constraint(xl, xr, idx_h[p]))                                # the device's samples, solved on the host
        inl, dec = ec.classify(xl, xr, part, e64.astype(np.float32).reshape(H, 3, 3), thr)
        host_best = int((inl & dec).sum(1).max())
        print("pair %d: true model %d strict inliers, best of %d host-solved samples %d, device best_count %d"
              % (p, true_count, H, host_best, best_count[p]))
        assert true_count > 300 and host_best >= 0.9 * true_count, "an unlucky sample, not the solver: change the seed"
        assert best_count[p] >= 0.9 * true_count


def test_mixed_pack_hypotheses_follow_the_callers_pair():
    from pats_amd import batch, ops
    from test_confidence_gpu import _small_batch
    _, cap, out, _ = _small_batch(True)
    K, H, seed = 50, 37, 31337
    norm = np.tile(np.array([160, 120, 1 / 200.0, 1 / 200.0, 160, 120, 1 / 200.0, 1 / 200.0], np.float32), (cap.pairs, 1))
    norm[:, 0] += np.arange(cap.pairs)                                                  # distinct per pair: a wrong permutation shows
    dn = cu(norm)
    top = batch.topk_by_pair(out, cap, K)
    before = [t.clone() for t in list(out["topk"]) + list(out["by_pair"])]
    models, idx = batch.hypothesize_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)          # on="topk", progressive
    slot = out["caller_of"]
    assert slot != list(range(cap.pairs))
    for i in range(cap.pairs):
        s_ = slot.index(i)
        hand = ops.epipolar_hypotheses_by_pair(top[0][s_], top[1][s_], H, cu(np.array([seed + i], np.int64)), stride=K,
                                               counts=top[4][s_:s_ + 1], norm=dn[i:i + 1], progressive=True, return_samples=True)
        assert torch.equal(models[i].view(torch.int32), hand[0][0].view(torch.int32)) and torch.equal(idx[i], hand[1][0])
        assert int(top[4][s_]) >= 8 and bool(models[i].reshape(H, 9).any(1).all())
    ver = batch.verify_by_pair(out, cap, models, cu(np.full(cap.pairs, 0.05, np.float32)), norm=dn, on="topk")
    assert int(ver[2].min()) >= 8                                                       # a model fits its own eight matches
    again = batch.hypothesize_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)
    assert torch.equal(again[0].view(torch.int32), models.view(torch.int32)) and torch.equal(again[1], idx)
    other = batch.hypothesize_by_pair(out, cap, H, seed=seed + 1, norm=dn, samples=True)
    assert not torch.equal(other[1], idx)
    full = batch.hypothesize_by_pair(out, cap, H, seed=seed, norm=dn, on="all")         # progressive defaults to False here
    assert tuple(full.shape) == (cap.pairs, H, 3, 3) and out["hypotheses"] is full
    same = lambda a, b: torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)  # noqa: E731
    assert all(same(a, b) for a, b in zip(list(out["topk"]) + list(out["by_pair"]), before))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    import test_hypotheses_host as th
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.zeros(4096, dtype=torch.float32, device="cuda")                        # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    th.A16 = base
    try:
        for kw, words in th.refusals(lib, base=base):
            th.refused(lib, kw, words)
    finally:
        th.A16 = 0x7f0000001000
    torch.cuda.synchronize()
    assert not live.any()                                                               # nothing ran: nothing was written
    ml = torch.zeros((20, 2), device="cuda")
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 10, 20], device="cuda")
    for kw, word in (({"H": 0}, "H = 0"), ({"H": ops.epipolar_max_h() + 1}, "H ="), ({"norm": torch.zeros((3, 8), device="cuda")}, "norm"),
                     ({"out": torch.zeros((2, 4, 3, 3), device="cuda").double()}, "models"),
                     ({"out": (torch.zeros((2, 4, 3, 3), device="cuda"),), "return_samples": True}, "out must be")):
        with pytest.raises(RuntimeError, match=word):
            ops.epipolar_hypotheses_by_pair(ml, ml, kw.pop("H", 4), seed, pair_off=off, **kw)
    with pytest.raises(RuntimeError, match="seed must hold one int64 per pair"):
        ops.epipolar_hypotheses_by_pair(ml, ml, 4, seed[:1], pair_off=off)
