"""GPU: the uncalibrated branch - ops.epipolar_hypotheses7_by_pair, ops.fundamental_refit_by_pair, ops.fundamental_polish_by_pair and
their batch functions - against the definitions of include/pats_amd.h restated in numpy (tests/fundamental_cases.py):
    sample_idx   equals the restatement bit for bit (integer arithmetic: nothing to round)
    models       all three slots exactly zero where the definition says so (n < 7, a non-finite sample coordinate); the non-zero
                 slots the lowest of their sample, n_models their count; each finite with | |e| - 1 | <= 1e-5, the component of
                 largest magnitude positive, pairwise distinct, and - the accuracy contract - |A7 e|_2 <= B_epi eps32 |A7|_F and
                 |det F| <= B_det eps32 with B = MARGIN * b, b = what the float64 numpy solver's models, rounded to float32, reach on
                 the tolerance and noisy cases in the same run
    completeness on the exact cases the true model is among the device's models in at least 99 % of the samples; on exact and noisy
                 cases at most 1 % of the float64 solver's solutions have no device model within 1 - |<.,.>| <= 1e-4
    refit        unit norm, rank 2 and the sign rule to 64 eps64; F against numpy's truncated SVD of the device's own f_refit within
                 Wedin's bound 64 eps64 / (sigma2 - sigma3); sigma, eig, the eigen-residual, F_px and the permutation
    polish       all six outputs equal, bit for bit, the chain score (H = 1, moments) -> fundamental refit -> cast, round for round
docs/parity.md records the measured ratios and shares.  Every output lies inside a larger sentinel-filled buffer and every input list
in a larger NaN-filled one: the call must define every byte of the views, none around them, and read no row beyond cap."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import fundamental_cases as fc
import hypotheses_cases as hc
import pose_cases as pc

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0x5A
E64 = 64 * fc.EPS64


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def bounds():
    """(B_epi, B_det) = MARGIN * the baselines measured in this run (shared, computed once)."""
    b_epi, b_det = fc.baselines()
    assert np.isfinite(b_epi) and b_epi > 0 and np.isfinite(b_det) and b_det > 0
    return fc.MARGIN * b_epi, fc.MARGIN * b_det


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a, fill=float("nan")):
    """a as a view of a longer buffer whose rows beyond it hold `fill`."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.shape[0] + PAD,) + a.shape[1:], fill, dtype=cu(a[:0]).dtype, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


def views_of(shapes):
    """Sentinel-filled buffers with a view each -> (views, check: the bytes around every view are untouched)."""
    bufs, views = [], []
    for shape, dt, sent in shapes:
        b = torch.full((int(np.prod(shape)) + 2 * PAD,), sent, dtype=dt, device="cuda")
        bufs.append((b, sent))
        views.append(b[PAD:b.numel() - PAD].view(shape))

    def check():
        for b, sent in bufs:
            assert bool((torch.cat([b[:PAD], b[b.numel() - PAD:]]) == sent).all()), "bytes around an output view changed"
    return views, check, bufs


def dev_kw(kw):
    return {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


# ---- the hypotheses ---------------------------------------------------------------------------------------------------------------
def run(ops, ml, mr, H, seeds, samples=True, counts_out=True, **kw):
    """One call on fresh sentinel buffers -> (models [pairs,H,3,3,3], sample_idx, n_models) as numpy arrays (the surroundings
    checked; an output that was not asked for must stay untouched and comes back as None)."""
    pairs = len(seeds)
    (vm, vi, vn), chk, bufs = views_of([((pairs, H, 3, 3, 3), torch.float32, SENT_F), ((pairs, H, 7), torch.int32, SENT_I),
                                        ((pairs, H), torch.int32, SENT_I)])
    dest = (vm,) + ((vi,) if samples else ()) + ((vn,) if counts_out else ())
    got = ops.epipolar_hypotheses7_by_pair(guarded(ml), guarded(mr), H, cu(np.asarray(seeds, np.int64)), return_samples=samples,
                                           return_counts=counts_out, out=dest if len(dest) > 1 else vm, **dev_kw(kw))
    torch.cuda.synchronize()
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(dest) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    assert samples or bool((bufs[1][0] == SENT_I).all())
    assert counts_out or bool((bufs[2][0] == SENT_I).all())
    chk()
    return vm.cpu().numpy(), vi.cpu().numpy() if samples else None, vn.cpu().numpy() if counts_out else None


def check(got, ref, bounds=None, solved=True):
    """All three outputs against the restatement -> (the largest epipolar ratio, the largest determinant ratio)."""
    models, idx, nm = got
    assert models.dtype == np.float32 and idx.dtype == np.int32 and nm.dtype == np.int32
    for p, r in enumerate(ref):
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        if r["n"] < 7:
            assert not models[p].any() and (idx[p] == -1).all() and not nm[p].any()
        elif solved and r["n"] >= 64 and r["finite"].any():               # a real cubic has a real root: every generic sample is solved
            assert (nm[p][r["finite"]] > 0).all(), "pair %d: a finite sample without a model" % p
    assert nm.max() <= 3
    B = bounds or (None, None)
    return fc.check_models(models, ref, n_models=nm, B_epi=B[0], B_det=B[1])


NORM = np.array([[0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3]], np.float32)


def norm_for(pairs):
    return np.ascontiguousarray(NORM * np.linspace(0.9, 1.1, pairs, dtype=np.float32)[:, None])


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_ragged_lengths_around_seven_and_sample_counts_around_the_workgroup(ops, bounds, H):
    lengths = [0, 6, 7, 8, 600, 64]
    ml, mr, off = hc.make_pairs(lengths, seed=100 + H)
    ml, mr = np.concatenate([ml, ml[:23]]), np.concatenate([mr, mr[:23]])              # rows inside cap behind the last segment
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    seeds = [5000 + H + 3 * p for p in range(len(lengths))]
    for norm in (None, norm_for(len(lengths))):
        for progressive in (False, True):
            got = run(ops, ml, mr, H, seeds, pair_off=off, norm=norm, progressive=progressive)
            check(got, fc.reference(ml, mr, segs, seeds, H, progressive, norm), bounds)
    both = run(ops, ml, mr, H, seeds, pair_off=off)
    for samples, counts_out in ((False, False), (True, False), (False, True)):         # sample_idx and n_models are optional
        only = run(ops, ml, mr, H, seeds, samples=samples, counts_out=counts_out, pair_off=off)
        assert same_bits(only[0], both[0])
        assert (only[1] is None or np.array_equal(only[1], both[1])) and (only[2] is None or np.array_equal(only[2], both[2]))
    other = run(ops, ml, mr, H, [s + 1 for s in seeds], pair_off=off)                   # another seed: other draws
    assert not np.array_equal(other[1][4], both[1][4]) and np.array_equal(other[1][0], both[1][0])


def test_strided_segments_and_clamped_counts(ops, bounds):
    stride, counts = 16, np.array([7, 16, 3, 20], np.int64)                             # 20 is clamped to 16
    ml, mr, _ = hc.make_pairs([stride] * 4 + [9], seed=200)
    segs = ec.segments(4, ml.shape[0], stride=stride, counts=counts)
    assert segs == [(0, 7), (16, 16), (32, 3), (48, 16)]
    seeds = [1, 2, 3, 4]
    for norm in (None, norm_for(4)):
        for progressive in (False, True):
            got = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts, norm=norm, progressive=progressive)
            check(got, fc.reference(ml, mr, segs, seeds, 65, progressive, norm), bounds, solved=False)
    # the same rows in the ragged form: the same bits; and two identical calls
    off = np.array([0, 7], np.int64)
    a = run(ops, ml, mr, 65, seeds[:1], pair_off=off)
    b = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    c = run(ops, ml, mr, 65, seeds, stride=stride, counts=counts)
    assert same_bits(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[2][0], b[2][0])
    assert same_bits(b[0], c[0]) and np.array_equal(b[1], c[1]) and np.array_equal(b[2], c[2])
    assert b[2][1].min() >= 1 and b[2][1].max() == 3                                    # models were compared, not zeros alone
    # top-K shaped inputs [pairs,K,2] are taken as the flat lists they are
    d = ops.epipolar_hypotheses7_by_pair(cu(ml[:64].reshape(4, 16, 2)), cu(mr[:64].reshape(4, 16, 2)), 65, cu(np.asarray(seeds, np.int64)),
                                         stride=stride, counts=cu(counts))
    assert tuple(d.shape) == (4, 65, 3, 3, 3)
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
    ref = fc.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H)
    check(got, ref, bounds)
    for p, row in ((0, 5), (1, 17)):
        hit = (got[1][p] == row).any(1)
        assert 5 < hit.sum() < H - 5 and not got[0][p][hit].any() and not got[2][p][hit].any()
        assert same_bits(got[0][p][~hit], clean[0][p][~hit]) and np.array_equal(got[2][p][~hit], clean[2][p][~hit])    # nothing else
        assert np.array_equal(got[1][p], clean[1][p])                                   # sample_idx is still written
    norm = norm_for(2)
    norm[1, 6] = np.inf                                                                 # a non-finite x after norm: the whole pair
    got = run(ops, ml, mr, H, [21, 22], pair_off=off, norm=norm)
    check(got, fc.reference(ml, mr, [(0, 40), (40, 40)], [21, 22], H, norm=norm), bounds)
    assert not got[0][1].any() and (got[1][1] >= 0).all()


def test_seven_identical_matches_give_zeros_or_finite_unit_models(ops):
    ml, mr, _ = hc.make_pairs([1, 30], seed=400)
    ml, mr = np.concatenate([np.repeat(ml[:1], 7, 0), ml[1:]]), np.concatenate([np.repeat(mr[:1], 7, 0), mr[1:]])
    segs = [(0, 7), (7, 30)]
    got = run(ops, ml, mr, 70, [11, 12], pair_off=np.array([0, 7, 37], np.int64))      # the call returns
    ref = fc.reference(ml, mr, segs, [11, 12], 70)
    check(got, ref, None, solved=False)                                                 # finite; zero or unit, signed, distinct
    assert (got[2][1] > 0).all()                                                        # the neighbour is unaffected


@pytest.fixture(scope="module")
def device_cases(ops):
    """The exact and the noisy cases through the device, once: {exact: (models [3,H,3,3,3], sample_idx, n_models)}."""
    out = {}
    H = fc.TOLERANCE_CASES[0][2]
    seeds = [c[3] for c in fc.TOLERANCE_CASES]
    off = np.concatenate([[0], np.cumsum([c[1] for c in fc.TOLERANCE_CASES])]).astype(np.int64)
    for exact in (True, False):
        cs = fc.cases(exact)
        ml, mr = np.concatenate([c["ml"] for c in cs]), np.concatenate([c["mr"] for c in cs])
        got = run(ops, ml, mr, H, seeds, pair_off=off)
        assert all(np.array_equal(got[1][p], c["idx"]) for p, c in enumerate(cs))       # the samples the host solved
        out[exact] = got
    return out


@pytest.mark.parametrize("exact", [True, False])
def test_pointwise_contract_against_eight_times_the_rounded_float64_solver(device_cases, bounds, exact):
    cs = fc.cases(exact)
    H = cs[0]["idx"].shape[0]
    ref = [{"idx": c["idx"], "A": c["A"], "finite": np.ones(H, bool), "n": 600} for c in cs]
    b_epi, b_det = fc.baselines()
    w_epi, w_det = check(device_cases[exact], ref)
    print("%s cases, %d models: epipolar ratio device %.4f, b_epi %.4f, B_epi %.4f; determinant ratio device %.4f, b_det %.4f, B_det %.4f"
          % ("exact" if exact else "noisy", int(device_cases[exact][2].sum()), w_epi, b_epi, bounds[0], w_det, b_det, bounds[1]))
    assert w_epi <= bounds[0] and w_det <= bounds[1]


def test_the_true_model_is_among_the_models_of_the_exact_cases(device_cases):
    found = total = 0
    for p, c in enumerate(fc.cases(True)):
        f = fc.true_found(device_cases[True][0][p], c)
        found, total = found + int(f.sum()), total + f.size
    print("the true model among the device's models: %d/%d samples" % (found, total))
    assert found >= 0.99 * total


@pytest.mark.parametrize("exact", [True, False])
def test_at_most_one_percent_of_the_float64_solutions_lack_a_device_match(device_cases, exact):
    missed = total = 0
    for p, c in enumerate(fc.cases(exact)):
        dev = device_cases[exact][0][p].reshape(-1, 3, 9)
        for h, host in enumerate(c["host"]):
            m = fc.matches(dev[h], host)
            missed, total = missed + int((~m).sum()), total + m.size
    nm = device_cases[exact][2]
    print("%s cases: %d of %d float64 solutions without a device match; models per sample: mean %.2f, histogram %s"
          % ("exact" if exact else "noisy", missed, total, nm.mean(), np.bincount(nm.reshape(-1), minlength=4).tolist()))
    assert nm.max() <= 3 and missed <= 0.01 * total


# ---- the refit --------------------------------------------------------------------------------------------------------------------
REFIT_NAMES = ("F", "eig", "sigma", "F_px", "f_refit")


def run_refit(ops, bc, **kw):
    pairs = len(bc)
    views, chk, _ = views_of([((pairs, 3, 3), torch.float64, SENT_F), ((pairs, 2), torch.float64, SENT_F), ((pairs, 3), torch.float64, SENT_F),
                              ((pairs, 3, 3), torch.float64, SENT_F), ((pairs, 9), torch.float64, SENT_F)])
    got = ops.fundamental_refit_by_pair(cu(np.asarray(bc, np.int64)), return_pixel=True, return_refit=True, out=tuple(views), **dev_kw(kw))
    torch.cuda.synchronize()
    assert len(got) == 5 and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    chk()
    out = {n: v.cpu().numpy() for n, v in zip(REFIT_NAMES, views)}
    assert all(np.isfinite(v).all() and not (v == SENT_F).any() for v in out.values())  # no NaN in any output, ever
    return out


SCENE_SIZES = (20, 65, 500, 1200, 3000, 4097)


@pytest.fixture(scope="module")
def refit_scenes():
    """Six pairs of 20 .. 4097 matches with their float64 moments over the true matches, with and without norm.  With norm the
    stored coordinates are x / s + c: the normalised points are the scene's again, to rounding."""
    out = {}
    for key, norm in (("plain", None), ("norm", norm_for(6))):
        scenes = [fc.make_scene(201 + i, n) for i, n in enumerate(SCENE_SIZES)]
        M, stored = [], []
        for i, s in enumerate(scenes):
            ml, mr = s["ml"], s["mr"]
            if norm is not None:
                ml = (ml / norm[i, 2:4] + norm[i, 0:2]).astype(np.float32)
                mr = (mr / norm[i, 6:8] + norm[i, 4:6]).astype(np.float32)
            xl, xr = ec.points32(ml, mr, None if norm is None else norm[i])
            M.append(ec.moments64(xl, xr, s["good"])[0])
            stored.append((ml, mr))
        out[key] = (scenes, np.stack(M), norm, stored)
    return out


@pytest.mark.parametrize("key", ["plain", "norm"])
def test_refit_is_the_rank_two_truncation_of_the_smallest_eigenvector(ops, refit_scenes, key):
    scenes, M, norm, stored = refit_scenes[key]
    bc = [int(s["good"].sum()) for s in scenes]
    nk = {} if norm is None else {"norm": norm}
    out = run_refit(ops, bc, moments=M, **nk)
    b64 = max(pc.residual(m, pc.refit64(m)[0]) for m in M)
    for p, (s, m) in enumerate(zip(scenes, M)):
        F, f, sig, eig = out["F"][p], out["f_refit"][p], out["sigma"][p], out["eig"][p]
        assert abs(np.linalg.norm(F) - 1) <= E64 and abs(np.linalg.det(F)) <= E64
        assert np.array_equal(fc.sign_rule(F), F)
        # the refit: the eigen-residual contract of the homography and pose refits
        fro = np.linalg.norm(m)
        w = pc.refit64(m)[1]
        assert abs(np.linalg.norm(f) - 1) <= E64 and pc.residual(m, f) <= fc.MARGIN * b64
        tol = fc.MARGIN * b64 * fc.EPS64 * fro
        assert f @ m @ f <= w[0] + tol and eig[0] <= eig[1] and eig[0] >= -tol
        assert np.abs(eig - w[:2]).max() <= E64 * fro
        # the truncation: numpy's, of the device's own f_refit.  Wedin: the truncated SVDs of two matrices E64 apart differ by at most
        # E64 / (sigma2 - sigma3)
        T, s_np = fc.truncate(f)
        gap = s_np[1] - s_np[2]
        print("pair %d (%s): sigma %s, gap %.3g, |F - T|_max %.3g" % (p, key, s_np.tolist(), gap, np.abs(F - T).max()))
        assert np.abs(sig - s_np).max() <= E64 and sig[0] >= sig[1] >= sig[2] >= 0
        assert np.abs(F - T).max() <= E64 / gap
        if norm is None:
            assert np.array_equal(out["F_px"][p], F)
        else:
            assert np.abs(out["F_px"][p] - fc.denormalise(F, norm[p])).max() <= E64   # numpy's N_r^T F N_l from the kernel's own F
        if bc[p] >= 100:                                                  # ... which is the scene's geometry on the stored points
            ml, mr = (a[s["good"]].astype(np.float64) for a in stored[p])
            l, r = np.c_[ml, np.ones(len(ml))], np.c_[mr, np.ones(len(mr))]
            alg = np.abs(np.einsum("ni,ij,nj->n", r, out["F_px"][p], l))
            assert np.sqrt((alg ** 2).mean()) < 2e-3                      # the scene's noise is 5e-4 per coordinate
            assert fc.closeness(F.reshape(1, 9), s["F"].reshape(1, 9))[0, 0] < 1e-3
    # swapped: P F P of the swapped=0 call with the sign rule
    sw = run_refit(ops, bc, moments=M, swapped=True, **nk)
    for p in range(len(scenes)):
        assert np.array_equal(sw["F"][p], fc.swap(out["F"][p])) and np.array_equal(sw["F_px"][p], fc.swap(out["F_px"][p]))
    assert all(sw[n].tobytes() == out[n].tobytes() for n in ("eig", "sigma", "f_refit"))
    again = run_refit(ops, bc, moments=M, **nk)
    assert all(again[n].tobytes() == out[n].tobytes() for n in REFIT_NAMES)
    # F_px and f_refit are optional: the same bits without them
    lone = ops.fundamental_refit_by_pair(cu(np.asarray(bc, np.int64)), moments=cu(M), **dev_kw(nk))
    assert len(lone) == 3 and all(lone[k].cpu().numpy().tobytes() == out[n].tobytes() for k, n in enumerate(REFIT_NAMES[:3]))


def test_refit_without_a_model_writes_zeros_and_the_winning_model_is_promoted(ops, refit_scenes):
    scenes, M, _, _ = refit_scenes["plain"]
    M = M.copy()
    M[1, 3, 7] = np.nan                                                   # in the upper triangle, which is what is read
    M[2, 0, 0] = np.inf
    bc = [7, 500, 500, 8, 0, -5]
    out = run_refit(ops, bc, moments=M, norm=norm_for(6))
    for p in (0, 1, 2, 4, 5):
        assert not any(out[n][p].any() for n in REFIT_NAMES), p
    assert abs(np.linalg.norm(out["F"][3]) - 1) <= E64 and abs(np.linalg.norm(out["F_px"][3]) - 1) <= E64
    lower = M.copy()
    lower[3, 8, 0] = np.nan                                               # the lower triangle is not read
    assert run_refit(ops, bc, moments=lower, norm=norm_for(6))["F"][3].tobytes() == out["F"][3].tobytes()
    bad_norm = norm_for(6)
    bad_norm[3, 6] = 0.0                                                  # a zero scale: F stays, N_r is singular and F_px is no model
    z = run_refit(ops, bc, moments=M, norm=bad_norm)
    assert z["F"][3].tobytes() == out["F"][3].tobytes() and not z["F_px"][3].any()
    # without moments: models[p, best[p]] promoted and truncated, eig 0; the zero model and a rank-1 model are no model
    models = np.stack([ec.make_case(700 + p, 50, 5)["models"] for p in range(4)])
    models[2] = 0.0
    models[3, 0] = np.outer([1, 2, 3], [0.1, 0.2, -0.3]).astype(np.float32)
    best = np.array([1, 9, 0, 0], np.int32)                               # 9 is clamped to H - 1 = 4
    got = run_refit(ops, [10, 10, 10, 10], models=models, best=best)
    for p, h in ((0, 1), (1, 4)):
        T, s_np = fc.truncate(models[p, h].astype(np.float64).reshape(9))
        assert np.array_equal(got["f_refit"][p], models[p, h].astype(np.float64).reshape(9))
        assert np.abs(got["F"][p] - T).max() <= E64 / (s_np[1] - s_np[2]) and np.abs(got["sigma"][p] - s_np).max() <= E64
    assert not got["F"][2].any() and not got["sigma"][2].any() and not got["eig"].any() and np.array_equal(got["F_px"], got["F"])
    assert not got["F"][3].any() or abs(np.linalg.det(got["F"][3])) <= E64      # rank 1 up to rounding: zeros or a finite rank-2 F


# ---- the local optimisation ----------------------------------------------------------------------------------------------------
POLISH_NAMES = ("model", "best_count", "inlier", "moments", "best_round", "counts")


def run_polish(ops, ml, mr, models, thr, best, rounds, **kw):
    """One fused call on fresh sentinel buffers -> dict of numpy arrays (the surroundings checked, every byte defined, all finite)."""
    pairs, cap = models.shape[0], ml.shape[0]
    views, chk, _ = views_of([((pairs, 3, 3), torch.float32, SENT_F), ((pairs,), torch.int64, SENT_I), ((cap,), torch.uint8, SENT_B),
                              ((pairs, 9, 9), torch.float64, SENT_F), ((pairs,), torch.int32, SENT_I),
                              ((pairs, rounds + 1), torch.int32, SENT_I)])
    got = ops.fundamental_polish_by_pair(guarded(ml), guarded(mr), cu(models), cu(thr), best=None if best is None else cu(best),
                                         rounds=rounds, out=tuple(views), **dev_kw(kw))
    torch.cuda.synchronize()
    assert len(got) == 6 and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    chk()
    out = {n: v.cpu().numpy() for n, v in zip(POLISH_NAMES, views)}
    assert np.isfinite(out["model"]).all() and np.isfinite(out["moments"]).all()
    assert not (out["model"] == np.float32(SENT_F)).any() and not (out["moments"] == SENT_F).any()
    assert set(np.unique(out["inlier"]).tolist()) <= {0, 1}
    return out


def chain(ops, ml, mr, models, thr, best, rounds, segs, **kw):
    """The oracle: the existing verification and the fundamental refit, one call per link, the best picked on the host."""
    d = dev_kw(kw)
    pairs, H = models.shape[0], models.shape[1]
    h = np.zeros(pairs, np.int64) if best is None else np.clip(best.astype(np.int64), 0, H - 1)
    dml, dmr, dthr = cu(ml), cu(mr), cu(thr)
    m = cu(models[np.arange(pairs), h].reshape(pairs, 1, 3, 3))
    links = []
    for r in range(rounds + 1):
        _, _, bc, inl, mom = ops.epipolar_score_by_pair(dml, dmr, m, dthr, moments=True, **d)
        links.append((m.cpu().numpy().reshape(pairs, 3, 3), bc.cpu().numpy(), inl.cpu().numpy(), mom.cpu().numpy()))
        if r < rounds:
            m = ops.fundamental_refit_by_pair(bc, moments=mom, norm=d.get("norm"))[0].float().reshape(pairs, 1, 3, 3)
    counts = np.stack([l[1] for l in links], 1).astype(np.int32)
    b = np.argmax(counts, 1).astype(np.int32)                              # the lowest round with the largest count
    out = {"model": np.stack([links[b[p]][0][p] for p in range(pairs)]), "best_count": counts[np.arange(pairs), b].astype(np.int64),
           "moments": np.stack([links[b[p]][3][p] for p in range(pairs)]), "best_round": b, "counts": counts,
           "inlier": np.zeros(ml.shape[0], np.uint8)}
    for p, (lo, n) in enumerate(segs):
        out["inlier"][lo:lo + n] = links[b[p]][2][lo:lo + n]
    return out


def minimal_pairs(lengths, seed0):
    """Pairs of the given lengths, each with a noisy 8-point model of its true matches at index best[p] of 3 models."""
    import polish_cases as pz
    rng = np.random.default_rng(seed0)
    pairs = len(lengths)
    cs = [pz.make_pair("epipolar", seed0 + 31 * p, max(n, 64)) for p, n in enumerate(lengths)]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ml = np.concatenate([c["ml"][:n] for c, n in zip(cs, lengths)])
    mr = np.concatenate([c["mr"][:n] for c, n in zip(cs, lengths)])
    models = rng.normal(size=(pairs, 3, 3, 3)).astype(np.float32)
    models /= np.linalg.norm(models.reshape(pairs, 3, 9), axis=2).reshape(pairs, 3, 1, 1)
    best = rng.integers(0, 3, pairs).astype(np.int32)
    for p, c in enumerate(cs):
        models[p, best[p]] = c["model"]
    return ml, mr, off, [(int(off[p]), int(lengths[p])) for p in range(pairs)], models, best


@pytest.mark.parametrize("rounds", [1, 2, 4])
def test_the_fused_walk_equals_the_chain_of_score_and_fundamental_refit(ops, rounds):
    lengths = [600, 5, 8193, 600]                                         # staged, n < 8, the unstaged walk, a NaN thr
    ml, mr, off, segs, models, best = minimal_pairs(lengths, 40 + rounds)
    thr = np.array([2e-3, 2e-3, 2e-3, np.nan], np.float32)
    for norm in (None, norm_for(4)):
        kw = {"pair_off": off} if norm is None else {"pair_off": off, "norm": norm}
        got = run_polish(ops, ml, mr, models, thr, best, rounds, **kw)
        want = chain(ops, ml, mr, models, thr, best, rounds, segs, **kw)
        for n in POLISH_NAMES:
            assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape and got[n].tobytes() == want[n].tobytes(), n
        for p, (lo, n) in enumerate(segs):
            assert int(got["inlier"][lo:lo + n].sum()) == got["best_count"][p]
        print("rounds %d norm %s: counts %s best_round %s" % (rounds, norm is not None, got["counts"].tolist(), got["best_round"].tolist()))
        assert got["best_count"][3] == 0 and got["best_count"][1] <= 5
        if norm is None:
            assert (got["best_round"][[0, 2]] > 0).all() and (got["best_count"][[0, 2]] > got["counts"][[0, 2], 0]).all()     # it helped
            for p in (0, 2):                                              # a rank-2 unit matrix rounded to float32: |cof|_F <= 1/2
                assert abs(np.linalg.det(got["model"][p].astype(np.float64))) <= fc.EPS32


def _handed_over(ml, mr, lengths, caller_of=None):
    """A result dict as the batch path leaves it after group_by_pair, from plain lists."""
    from pats_amd import batch
    pairs = len(lengths)
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([[0], np.cumsum(lengths), [sum(lengths), 0, 0]]).astype(np.int64)          # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if caller_of is not None:
        out["caller_of"] = caller_of
    return batch, cap, out


@pytest.mark.parametrize("mixed", [False, True])
def test_polish_f_then_fundamental_through_batch_equals_the_hand_written_rounds(ops, mixed):
    import polish_cases as pz
    pairs, n, rounds = 4, 600, 3
    cs = [pz.make_pair("epipolar", seed, n) for seed in (1, 4, 26, 13)]                     # the CALLER's order
    caller_of = [2, 0, 3, 1] if mixed else [0, 1, 2, 3]                                     # slot s holds the caller's pair caller_of[s]
    norm = norm_for(pairs)                                                                  # stored = x / s + c: normalised, the scene's again
    ml = np.concatenate([(cs[i]["ml"] / norm[i, 2:4] + norm[i, 0:2]).astype(np.float32) for i in caller_of])
    mr = np.concatenate([(cs[i]["mr"] / norm[i, 6:8] + norm[i, 4:6]).astype(np.float32) for i in caller_of])
    slot_of = [caller_of.index(i) for i in range(pairs)]
    models = np.zeros((pairs, 2, 3, 3), np.float32)                                         # a zero model and the minimal-sample one
    models[:, 1] = np.stack([c["model"] for c in cs])
    dmodels = cu(models)
    dthr = cu(np.array([pz.THR, pz.THR * 1.5, pz.THR, pz.THR * 0.75], np.float32))          # per pair, in the caller's order
    dn = cu(norm)

    def fresh():
        return _handed_over(ml, mr, [n] * pairs, caller_of if mixed else None)

    batch, cap, hand = fresh()
    with pytest.raises(ValueError, match="first"):
        batch.polish_f_by_pair(hand, cap, dthr)
    with pytest.raises(ValueError, match="first"):
        batch.fundamental_by_pair(hand, cap)
    # the hand-written rounds of the documents, the best kept on the host
    ver = batch.verify_by_pair(hand, cap, dmodels, dthr, norm=dn, moments=True)
    counts, fits = [], []
    for r in range(rounds + 1):
        counts.append(ver[2].cpu().numpy()[slot_of])                                        # slot order -> the caller's
        res = batch.fundamental_by_pair(hand, cap, norm=dn, swapped=True, pixel=True)
        assert len(res) == 4 and hand["fundamental"] is res
        fits.append([t.cpu().numpy() for t in res])
        if r < rounds:
            plain = batch.fundamental_by_pair(hand, cap, norm=dn)
            assert len(plain) == 3
            ver = batch.verify_by_pair(hand, cap, plain[0].float().reshape(pairs, 1, 3, 3), dthr, norm=dn, moments=True)
    counts = np.stack(counts, 1)
    b = np.argmax(counts, 1)

    _, _, out = fresh()
    batch.verify_by_pair(out, cap, dmodels, dthr, norm=dn, moments=True)
    new = batch.polish_f_by_pair(out, cap, dthr, rounds=rounds, norm=dn)
    assert out["verified"] is new and len(new) == 5 and tuple(new[0].shape) == (pairs, 1) and not new[1].any()
    assert "polished" not in out
    model, best_round, pcounts = out["polished_f"]
    assert torch.equal(out["verified_models"], model[:, None]) and torch.equal(new[0][:, 0].long(), new[2])
    assert np.array_equal(pcounts.cpu().numpy()[slot_of], counts) and np.array_equal(best_round.cpu().numpy()[slot_of], b)
    res = batch.fundamental_by_pair(out, cap, norm=dn, swapped=True, pixel=True)
    for i in range(pairs):
        for k in range(4):
            assert res[k][i].cpu().numpy().tobytes() == fits[b[i]][k][i].tobytes(), (i, k)
    print(counts.tolist(), b.tolist())
    assert (b > 0).any()
    # without moments the winning model is the refit's source
    _, _, nom = fresh()
    batch.verify_by_pair(nom, cap, dmodels, dthr, norm=dn)
    F = batch.fundamental_by_pair(nom, cap, norm=dn)[0].cpu().numpy()
    for i in range(pairs):
        assert np.abs(F[i] - fc.truncate(models[i, 1].astype(np.float64).reshape(9))[0]).max() < 1e-12


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_hypothesize7_verify_polish_fundamental_end_to_end():
    H, thr = 256, np.float32(2e-3)
    scenes = [fc.make_scene(seed, 600, outliers=0.4, noise=0) for seed in (11, 12)]
    ml, mr = np.concatenate([s["ml"] for s in scenes]), np.concatenate([s["mr"] for s in scenes])
    batch, cap, out = _handed_over(ml, mr, [600, 600])
    dthr = cu(np.full(2, thr, np.float32))
    models, idx = batch.hypothesize7_by_pair(out, cap, H, seed=2024, on="all", progressive=False, samples=True)
    assert out["hypotheses7"][0] is models and "hypotheses" not in out and "hypotheses5" not in out
    assert tuple(models.shape) == (2, H, 3, 3, 3) and tuple(idx.shape) == (2, H, 7)
    flat = models.reshape(2, -1, 3, 3)
    ver = batch.verify_by_pair(out, cap, flat, dthr, moments=True)
    verified = ver[2].cpu().numpy().copy()
    new = batch.polish_f_by_pair(out, cap, dthr, rounds=4)
    F, eig, sigma, F_px = batch.fundamental_by_pair(out, cap, swapped=False, pixel=True)
    F, idx_h, polished = F.cpu().numpy(), idx.cpu().numpy(), new[2].cpu().numpy()
    inl = new[3].cpu().numpy().astype(bool)
    for p, s in enumerate(scenes):
        assert np.array_equal(idx_h[p], fc.sample_idx(2024 + p, 600, H))                # pair_seed = seed + p
        xl, xr = ec.points32(s["ml"], s["mr"])
        true_inl, dec = ec.classify(xl, xr, ec.participates(xl, xr), s["F"].astype(np.float32)[None], thr)
        strict = true_inl[0] & dec[0] & s["good"]                                       # the planted inliers outside the undecided band
        print("pair %d: planted %d, verified %d, polished %d, |det F| %.3g" % (p, strict.sum(), verified[p], polished[p],
                                                                               abs(np.linalg.det(F[p]))))
        assert strict.sum() > 300 and polished[p] >= verified[p] >= 7
        assert (inl[600 * p:600 * (p + 1)] | ~strict).all()                             # the inlier set contains the planted inliers
        assert abs(np.linalg.norm(F[p]) - 1) <= E64 and abs(np.linalg.det(F[p])) <= E64
    assert torch.equal(F_px, torch.from_numpy(F).cuda())                                # no norm: F_px is F
    # the reference's stopping rule on the same models: the usual tuple, nothing to change in the adaptive kernels
    _, _, ad = _handed_over(ml, mr, [600, 600])
    res = batch.verify_adaptive_by_pair(ad, cap, flat, dthr, 1 - 1e-5, 7, models_per_sample=3, round_models=192, moments=True)
    assert len(res) == 7 and len(ad["verified"]) == 5 and tuple(ad["verified"][0].shape) == (2, 3 * H)
    used = res[5].cpu().numpy()
    assert (used % 192 == 0).all() and (used > 0).all() and (used <= 3 * H).all()
    assert (res[2].cpu().numpy() >= 7).all() and (res[2].cpu().numpy() <= verified).all()
    Fa = batch.fundamental_by_pair(ad, cap)[0].cpu().numpy()
    assert all(abs(np.linalg.det(Fa[p])) <= E64 for p in range(2))


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
        models, idx = batch.hypothesize7_by_pair(out, cap, H, seed=seed, norm=dn, samples=True)     # on="topk", progressive
        slot = out["caller_of"] if mixed else list(range(cap.pairs))
        for i in range(cap.pairs):
            s_ = slot.index(i)
            hand = ops.epipolar_hypotheses7_by_pair(top[0][s_], top[1][s_], H, cu(np.array([seed + i], np.int64)), stride=K,
                                                    counts=top[4][s_:s_ + 1], norm=dn[i:i + 1], progressive=True, return_samples=True)
            assert torch.equal(models[i].view(torch.int32), hand[0][0].view(torch.int32)) and torch.equal(idx[i], hand[1][0])
            assert int(top[4][s_]) >= 7 and bool(models[i].reshape(3 * H, 9).any(1).any())
        dthr = cu(np.full(cap.pairs, 0.05, np.float32))
        ver = batch.verify_by_pair(out, cap, models.reshape(cap.pairs, -1, 3, 3), dthr, norm=dn, on="topk", moments=True)
        assert tuple(ver[0].shape) == (cap.pairs, 3 * H) and int(ver[2].min()) >= 7   # a model fits its own seven matches
        batch.polish_f_by_pair(out, cap, dthr, norm=dn)
        res = batch.fundamental_by_pair(out, cap, norm=dn, swapped=True, pixel=True)
        assert all(bool(torch.isfinite(t).all()) for t in res) and tuple(res[3].shape) == (cap.pairs, 3, 3)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.zeros(4096, dtype=torch.float32, device="cuda")                        # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    assert fc.check_refusals(lib, "hypotheses7", base) > 50 and fc.check_refusals(lib, "refit", base) > 40
    assert fc.check_polish_refusals(lib, base) > 70
    torch.cuda.synchronize()
    assert not live.any()                                                               # nothing ran: nothing was written
    ml = torch.zeros((20, 2), device="cuda")
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 10, 20], device="cuda")
    for kw, word in (({"H": 0}, "H = 0"), ({"H": ops.epipolar_max_h() // 3 + 1}, "H ="), ({"norm": torch.zeros((3, 8), device="cuda")}, "norm"),
                     ({"out": torch.zeros((2, 4, 3, 3, 3), device="cuda").double()}, "models"),
                     ({"out": (torch.zeros((2, 4, 3, 3, 3), device="cuda"),), "return_counts": True}, "out must be")):
        with pytest.raises(RuntimeError, match=word):
            ops.epipolar_hypotheses7_by_pair(ml, ml, kw.pop("H", 4), seed, pair_off=off, **kw)
    with pytest.raises(RuntimeError, match="seed must hold one int64 per pair"):
        ops.epipolar_hypotheses7_by_pair(ml, ml, 4, seed[:1], pair_off=off)
    bc = torch.full((2,), 100, dtype=torch.int64, device="cuda")
    mom = torch.eye(9, dtype=torch.float64, device="cuda").repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="moments must be"):
        ops.fundamental_refit_by_pair(bc, moments=mom[:1])
    with pytest.raises(RuntimeError, match="norm"):
        ops.fundamental_refit_by_pair(bc, moments=mom, norm=torch.zeros((3, 8), device="cuda"))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.fundamental_refit_by_pair(bc, moments=mom, out=(mom,))
    with pytest.raises(RuntimeError, match="give moments, or models and best"):
        ops.fundamental_refit_by_pair(bc)
