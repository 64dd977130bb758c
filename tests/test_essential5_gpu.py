"""GPU: ops.epipolar_hypotheses5_by_pair / batch.hypothesize5_by_pair against the definition of include/pats_amd.h restated in numpy
(tests/essential5_cases.py):
    sample_idx   equals the restatement bit for bit (integer arithmetic: nothing to round)
    models       all ten slots exactly zero where the definition says so (n < 5, a non-finite sample coordinate); the non-zero slots
                 the lowest of their sample, n_models their count; each finite with | |e| - 1 | <= 1e-5, the component of largest
                 magnitude positive, pairwise distinct, and - the accuracy contract - |A5 e|_2 <= B_epi eps32 |A5|_F and
                 |2 E E^T E - tr(E E^T) E|_F <= B_ess eps32 with B = MARGIN * b, b = what the float64 numpy solver's models, rounded
                 to float32, reach on the tolerance and noisy cases in the same run
    completeness on the exact cases the true E is among the device's models in at least 99 % of the samples; on exact and noisy cases
                 at most 1 % of the float64 solver's solutions have no device model within 1 - |<.,.>| <= 1e-4
docs/parity.md records the measured ratios and shares.  Every output lies inside a larger sentinel-filled buffer and every input list
in a larger NaN-filled one: the call must define every byte of the views, none around them, and read no row beyond cap."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import essential5_cases as e5
import hypotheses_cases as hc

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I = -777.25, -123456


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bounds():
    """(B_epi, B_ess) = MARGIN * the baselines measured in this run (shared, computed once)."""
    b_epi, b_ess = e5.baselines()
    assert np.isfinite(b_epi) and b_epi > 0 and np.isfinite(b_ess) and b_ess > 0
    return e5.MARGIN * b_epi, e5.MARGIN * b_ess


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


def run(ops, ml, mr, H, seeds, samples=True, counts_out=True, **kw):
    """One call on fresh sentinel buffers -> (models [pairs,H,10,3,3], sample_idx, n_models) as numpy arrays (the surroundings
    checked; an output that was not asked for must stay untouched and comes back as None)."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs = len(seeds)
    bm = torch.full((pairs * H * 90 + 2 * PAD,), SENT_F, dtype=torch.float32, device="cuda")
    bi = torch.full((pairs * H * 5 + 2 * PAD,), SENT_I, dtype=torch.int32, device="cuda")
    bn = torch.full((pairs * H + 2 * PAD,), SENT_I, dtype=torch.int32, device="cuda")
    vm, vi, vn = bm[PAD:-PAD].view(pairs, H, 10, 3, 3), bi[PAD:-PAD].view(pairs, H, 5), bn[PAD:-PAD].view(pairs, H)
    dest = (vm,) + ((vi,) if samples else ()) + ((vn,) if counts_out else ())
    gl, gr = guarded_lists(ml, mr)
    got = ops.epipolar_hypotheses5_by_pair(gl, gr, H, cu(np.asarray(seeds, np.int64)), return_samples=samples, return_counts=counts_out,
                                           out=dest if len(dest) > 1 else vm, **d)
    torch.cuda.synchronize()
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(dest) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    assert samples or bool((bi == SENT_I).all())
    assert counts_out or bool((bn == SENT_I).all())
    for buf, sent in ((bm, SENT_F), (bi, SENT_I), (bn, SENT_I)):
        assert bool((torch.cat([buf[:PAD], buf[-PAD:]]) == sent).all()), "bytes around an output view changed"
    return vm.cpu().numpy(), vi.cpu().numpy() if samples else None, vn.cpu().numpy() if counts_out else None


def check(got, ref, bounds=None, solved=True):
    """All three outputs against the restatement -> (the largest epipolar ratio, the largest essential ratio)."""
    models, idx, nm = got
    assert models.dtype == np.float32 and idx.dtype == np.int32 and nm.dtype == np.int32
    for p, r in enumerate(ref):
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        if r["n"] < 5:
            assert not models[p].any() and (idx[p] == -1).all() and not nm[p].any()
        elif solved and r["n"] >= 64 and r["finite"].any():               # generic samples: most of them have real solutions
            assert (nm[p][r["finite"]] > 0).mean() > 0.9, "pair %d: too many finite samples without a model" % p
    assert nm.max() <= 10
    B = bounds or (None, None)
    return e5.check_models(models, ref, n_models=nm, B_epi=B[0], B_ess=B[1])


NORM = np.array([[0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3]], np.float32)


def norm_for(pairs):
    return np.ascontiguousarray(NORM * np.linspace(0.9, 1.1, pairs, dtype=np.float32)[:, None])


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1. exactness and edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_ragged_lengths_around_five_and_sample_counts_around_the_workgroup(ops, bounds, H):
    lengths = [0, 4, 5, 6, 600, 64]
    ml, mr, off = hc.make_pairs(lengths, seed=100 + H)
    ml, mr = np.concatenate([ml, ml[:23]]), np.concatenate([mr, mr[:23]])              # rows inside cap behind the last segment
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    seeds = [5000 + H + 3 * p for p in range(len(lengths))]
    for norm in (None, norm_for(len(lengths))):
        for progressive in (False, True):
            got = run(ops, ml, mr, H, seeds, pair_off=off, norm=norm, progressive=progressive)
            check(got, e5.reference(ml, mr, segs, seeds, H, progressive, norm), bounds, solved=H >= 63)
    both = run(ops, ml, mr, H, seeds, pair_off=off)
    for samples, counts_out in ((False, False), (True, False), (False, True)):         # sample_idx and n_models are optional
        only = run(ops, ml, mr, H, seeds, samples=samples, counts_out=counts_out, pair_off=off)
        assert same_bits(only[0], both[0])
        assert (only[1] is None or np.array_equal(only[1], both[1])) and (only[2] is None or np.array_equal(only[2], both[2]))


def test_strided_segments_and_clamped_counts(ops, bounds):
    stride, counts = 16, np.array([5, 16, 3, 20], np.int64)                             # 20 is clamped to 16
    ml, mr, _ = hc.make_pairs([stride] * 4 + [9], seed=200)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 5), (16, 16), (32, 3), (48, 16)]
    seeds = [1, 2, 3, 4]
    for norm in (None, norm_for(4)):
        for progressive in (False, True):
            got = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts, norm=norm, progressive=progressive)
            check(got, e5.reference(ml, mr, segs, seeds, 65, progressive, norm), bounds, solved=False)
    # the same rows in the ragged form: the same bits; and two identical calls
    off = np.array([0, 5], np.int64)
    a = run(ops, ml, mr, 65, seeds[:1], pair_off=off)
    b = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    c = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    assert same_bits(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[2][0], b[2][0])
    assert same_bits(b[0], c[0]) and np.array_equal(b[1], c[1]) and np.array_equal(b[2], c[2])
    assert b[2][1].max() >= 2                                                           # models were compared, not zeros alone
    # top-K shaped inputs [pairs,K,2] are taken as the flat lists they are
    d = ops.epipolar_hypotheses5_by_pair(cu(ml[:64].reshape(4, 16, 2)), cu(mr[:64].reshape(4, 16, 2)), 65, cu(np.asarray(seeds, np.int64)),
                                         stride=stride, counts=cu(counts))
    assert tuple(d.shape) == (4, 65, 10, 3, 3)
    assert same_bits(d.cpu().numpy(), run(ops, ml[:64], mr[:64], 65, seeds, stride=stride, counts=counts)[0])


def test_empty_arrays_define_every_output(ops):
    z2 = np.zeros((0, 2), np.float32)
    m, i, n = run(ops, z2, z2, 70, [1, 2], pair_off=np.zeros(3, np.int64))
    assert not m.any() and (i == -1).all() and not n.any()


def test_a_nan_coordinate_zeroes_exactly_the_samples_that_hold_it(ops, bounds):
    ml, mr, off = hc.make_pairs([40, 40], seed=500)
    clean = run(ops, ml, mr, 200, [21, 22], pair_off=off)
    ml[5, 1], mr[40 + 17, 0] = np.nan, np.inf
    H = 200
    got = run(ops, ml, mr, H, [21, 22], pair_off=off)
    ref = e5.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H)
    check(got, ref, bounds)
    for p, row in ((0, 5), (1, 17)):
        hit = (got[1][p] == row).any(1)
        assert 5 < hit.sum() < H - 5 and not got[0][p][hit].any() and not got[2][p][hit].any()
        assert same_bits(got[0][p][~hit], clean[0][p][~hit]) and np.array_equal(got[2][p][~hit], clean[2][p][~hit])    # nothing else
        assert np.array_equal(got[1][p], clean[1][p])                                   # sample_idx is still written
    norm = norm_for(2)
    norm[1, 6] = np.inf                                                                 # a non-finite x after norm: the whole pair
    got = run(ops, ml, mr, H, [21, 22], pair_off=off, norm=norm)
    check(got, e5.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H, norm=norm), bounds)
    assert not got[0][1].any() and (got[1][1] >= 0).all()


def test_five_identical_matches_give_zeros_or_models_that_meet_the_contract(ops, bounds):
    ml, mr, _ = hc.make_pairs([1, 30], seed=400)
    ml, mr = np.concatenate([np.repeat(ml[:1], 5, 0), ml[1:]]), np.concatenate([np.repeat(mr[:1], 5, 0), mr[1:]])
    segs = [(0, 5), (5, 30)]
    got = run(ops, ml, mr, 70, [11, 12], pair_off=np.array([0, 5, 35], np.int64))      # the call returns
    check(got, e5.reference(ml, mr, segs, [11, 12], 70), bounds, solved=False)          # finite; zero or within the contract
    assert (got[2][1] > 0).mean() > 0.9                                                 # the neighbour is unaffected


# ---- 2. the contract and the completeness shares ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_cases(ops):
    """The exact and the noisy cases through the device, once: {exact: (models [3,H,10,3,3], sample_idx, n_models)}."""
    out = {}
    H = e5.TOLERANCE_CASES[0][2]
    seeds = [c[3] for c in e5.TOLERANCE_CASES]
    off = np.concatenate([[0], np.cumsum([c[1] for c in e5.TOLERANCE_CASES])]).astype(np.int64)
    for exact in (True, False):
        cs = e5.cases(exact)
        ml, mr = np.concatenate([c["ml"] for c in cs]), np.concatenate([c["mr"] for c in cs])
        got = run(ops, ml, mr, H, seeds, pair_off=off)
        assert all(np.array_equal(got[1][p], c["idx"]) for p, c in enumerate(cs))       # the samples the host solved
        out[exact] = got
    return out


@pytest.mark.parametrize("exact", [True, False])
def test_pointwise_contract_against_eight_times_the_rounded_float64_solver(device_cases, bounds, exact):
    cs = e5.cases(exact)
    H = cs[0]["idx"].shape[0]
    ref = [{"idx": c["idx"], "A": c["A"], "finite": np.ones(H, bool), "n": 600} for c in cs]
    b_epi, b_ess = e5.baselines()
    w_epi, w_ess = check(device_cases[exact], ref)
    print("%s cases, %d models: epipolar ratio device %.4f, b_epi %.4f, B_epi %.4f; essential ratio device %.4f, b_ess %.4f, B_ess %.4f"
          % ("exact" if exact else "noisy", int(device_cases[exact][2].sum()), w_epi, b_epi, bounds[0], w_ess, b_ess, bounds[1]))
    assert w_epi <= bounds[0] and w_ess <= bounds[1]


def test_the_true_essential_matrix_is_among_the_models_of_the_exact_cases(device_cases):
    found = total = 0
    for p, c in enumerate(e5.cases(True)):
        f = e5.true_found(device_cases[True][0][p], c)
        found, total = found + int(f.sum()), total + f.size
    print("the true E among the device's models: %d/%d samples" % (found, total))
    assert found >= 0.99 * total


@pytest.mark.parametrize("exact", [True, False])
def test_at_most_one_percent_of_the_float64_solutions_lack_a_device_match(device_cases, exact):
    missed = total = 0
    for p, c in enumerate(e5.cases(exact)):
        dev = device_cases[exact][0][p].reshape(-1, 10, 9)
        for h, host in enumerate(c["host"]):
            m = e5.matches(dev[h], host)
            missed, total = missed + int((~m).sum()), total + m.size
    nm = device_cases[exact][2]
    print("%s cases: %d of %d float64 solutions without a device match; models per sample: mean %.2f, histogram %s"
          % ("exact" if exact else "noisy", missed, total, nm.mean(), np.bincount(nm.reshape(-1), minlength=11).tolist()))
    assert nm.max() <= 10 and missed <= 0.01 * total


# ---- 3. through the batch path ------------------------------------------------------------------------------------------------
def test_hypothesize5_then_verify_reaches_the_true_models_inliers():
    from pats_amd import batch
    H, thr = 128, np.float32(2e-3)
    cases = [ec.make_case(seed, 600, 4, outliers=0.4, noise=0) for seed in (11, 12)]
    ml, mr = np.concatenate([c["ml"] for c in cases]), np.concatenate([c["mr"] for c in cases])
    cap = batch.Capacities(2, 5, 6)
    summary = np.array([0, 600, 1200, 1200, 0, 0], np.int64)                            # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:3]), "summary": ds}
    models, idx = batch.hypothesize5_by_pair(out, cap, H, seed=2024, on="all", progressive=False, samples=True)
    assert out["hypotheses5"][0] is models and "hypotheses" not in out
    assert tuple(models.shape) == (2, 10 * H, 3, 3) and tuple(idx.shape) == (2, H, 5)
    ver = batch.verify_by_pair(out, cap, models, cu(np.full(2, thr, np.float32)))        # the view goes straight in
    idx_h, best_count = idx.cpu().numpy(), ver[2].cpu().numpy()
    for p, c in enumerate(cases):
        assert np.array_equal(idx_h[p], e5.sample_idx(2024 + p, 600, H))                # pair_seed = seed + p
        xl, xr = ec.points32(c["ml"], c["mr"])
        inl, dec = ec.classify(xl, xr, ec.participates(xl, xr), c["models"][c["true"]], thr)
        strict = int((inl & dec).sum())                                                 # the true E's inliers outside the undecided band
        print("pair %d: true model %d decided inliers, device best_count %d" % (p, strict, best_count[p]))
        assert strict > 300 and best_count[p] >= strict


def test_batch_results_follow_the_callers_pair():
    from pats_amd import batch, ops
    from test_confidence_gpu import _small_batch
    K, H, seed = 50, 37, 31337
    for mixed in (False, True):
        _, cap, out, _ = _small_batch(mixed)
        norm = np.tile(np.array([160, 120, 1 / 200.0, 1 / 200.0, 160, 120, 1 / 200.0, 1 / 200.0], np.float32), (cap.pairs, 1))
        norm[:, 0] += np.arange(cap.pairs)                                              # distinct per pair: a wrong permutation shows
        dn = cu(norm)
        top = batch.topk_by_pair(out, cap, K)
        models, idx = batch.hypothesize5_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)     # on="topk", progressive
        slot = out["caller_of"] if mixed else list(range(cap.pairs))
        assert not mixed or slot != list(range(cap.pairs))
        for i in range(cap.pairs):
            s_ = slot.index(i)
            hand = ops.epipolar_hypotheses5_by_pair(top[0][s_], top[1][s_], H, cu(np.array([seed + i], np.int64)), stride=K,
                                                    counts=top[4][s_:s_ + 1], norm=dn[i:i + 1], progressive=True, return_samples=True)
            assert torch.equal(models[i].view(torch.int32), hand[0][0].reshape(10 * H, 3, 3).view(torch.int32)) and torch.equal(idx[i], hand[1][0])
            assert int(top[4][s_]) >= 5 and bool(models[i].reshape(10 * H, 9).any(1).any())
        ver = batch.verify_by_pair(out, cap, models, cu(np.full(cap.pairs, 0.05, np.float32)), norm=dn, on="topk")
        assert tuple(ver[0].shape) == (cap.pairs, 10 * H) and int(ver[2].min()) >= 5   # a model fits its own five matches
        again = batch.hypothesize5_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)
        assert torch.equal(again[0].view(torch.int32), models.view(torch.int32)) and torch.equal(again[1], idx)
        full = batch.hypothesize5_by_pair(out, cap, H, seed=seed, norm=dn, on="all")    # progressive defaults to False here
        assert tuple(full.shape) == (cap.pairs, 10 * H, 3, 3) and out["hypotheses5"] is full and "hypotheses" not in out


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    import test_essential5_host as th
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
    for kw, word in (({"H": 0}, "H = 0"), ({"H": ops.epipolar_max_h() // 10 + 1}, "H ="), ({"norm": torch.zeros((3, 8), device="cuda")}, "norm"),
                     ({"out": torch.zeros((2, 4, 10, 3, 3), device="cuda").double()}, "models"),
                     ({"out": (torch.zeros((2, 4, 10, 3, 3), device="cuda"),), "return_counts": True}, "out must be")):
        with pytest.raises(RuntimeError, match=word):
            ops.epipolar_hypotheses5_by_pair(ml, ml, kw.pop("H", 4), seed, pair_off=off, **kw)
    with pytest.raises(RuntimeError, match="seed must hold one int64 per pair"):
        ops.epipolar_hypotheses5_by_pair(ml, ml, 4, seed[:1], pair_off=off)
