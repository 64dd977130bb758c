"""CPU-only: the restatement of tests/absolute_polish_cases.py holds on its own - it converges on the noisy generator (so that the GPU
test's accuracy factor can never be met by a weak case), its Jacobian is the derivative of the projection, the degenerate inputs
end where the definition says - and the new entry point exists in every layer and refuses bad arguments before any launch."""
import ctypes

import numpy as np
import pytest

import absolute_cases as ac
import absolute_polish_cases as pc

F32 = np.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def walks():
    """The twelve noisy cases walked once: [(case, walk)]."""
    out = []
    for seed in pc.SEEDS:
        c = pc.noisy_pair(seed)
        models, best = pc.ransac_models(c, pair_seed=seed)
        out.append((c, pc.walk(c["X"], c["xr"], ac.participates(c["X"], c["xr"]), models[best], pc.THR, 4, 3)))
    return out


def test_the_restatement_converges_on_the_noisy_cases(walks):
    worst = 0.0
    for seed, (c, w) in zip(pc.SEEDS, walks):
        d0, db = pc.model_distance(w["models"][0], c), pc.model_distance(w["model"], c)
        print("seed %d: support %s, best round %d, pose_distance %.3g -> %.3g (%.3f)" % (seed, w["counts"].tolist(), w["best_round"], d0, db, db / d0))
        worst = max(worst, db / d0)
        assert db <= 0.6 * d0
        assert w["best_count"] >= w["counts"][0] and w["best_count"] == w["counts"].max() == w["mask"].sum()
        R = w["model"][:, :3].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * pc.EPS32
    print("the largest ratio: %.3f" % worst)


def test_the_best_rule_and_the_padding(walks):
    assert pc.pick([5, 7, 7, 6], [1.0, 3.0, 2.0, 0.1]) == 2
    assert pc.pick([5, 5, 5], [1.0, 1.0, 0.5]) == 2 and pc.pick([5, 5, 5], [1.0, 1.0, 1.0]) == 0
    assert pc.pick([5, 5], [1.0, NAN]) == 0 and pc.pick([5, 6], [1.0, NAN]) == 1
    for c, w in walks:
        assert w["best_round"] == pc.pick(w["counts"], w["cost"])
        for r in range(1, 5):
            if pc.same_bits(w["models"][r], w["models"][r - 1]):             # a repeated model: everything behind it repeats
                assert (w["counts"][r:] == w["counts"][r - 1]).all() and (w["cost"][r:] == w["cost"][r - 1]).all()


def test_jacobian_against_central_differences():
    c = ac.make_pair(7, 40)
    m = np.concatenate([c["R"], c["t"][:, None]], 1)
    m[:, 3] += 0.01                                                           # off the optimum: e is not zero
    e, J = pc.residual_jacobian(m, c["X"], c["xr"])
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        plus = np.concatenate([pc.exp_so3(d[:3]) @ m[:, :3], (pc.exp_so3(d[:3]) @ m[:, 3] + d[3:])[:, None]], 1)
        minus = np.concatenate([pc.exp_so3(-d[:3]) @ m[:, :3], (pc.exp_so3(-d[:3]) @ m[:, 3] - d[3:])[:, None]], 1)
        num = (pc.residual_jacobian(plus, c["X"], c["xr"])[0] - pc.residual_jacobian(minus, c["X"], c["xr"])[0]) / (2 * h)
        assert np.abs(num - J[:, :, k]).max() <= 1e-8 * max(1.0, np.abs(J[:, :, k]).max()), k
    # the update is a rotation, and w = 0 is the identity
    E = pc.exp_so3(np.array([0.3, -0.2, 0.5]))
    assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(E) - 1) <= 1e-15
    assert np.array_equal(pc.exp_so3(np.zeros(3)), np.eye(3))
    assert np.abs(E - ac.rodrigues(np.array([0.3, -0.2, 0.5]))).max() <= 1e-15


def test_ordered_sum_is_a_sum():
    rng = np.random.default_rng(2)
    for n in (1, 63, 512, 513, 1300):
        terms, mask = rng.normal(size=(n, 3)), rng.random(n) < 0.7
        got = pc.ordered_sum(terms, mask)
        assert np.abs(got - terms[mask].sum(0)).max() <= 1e-12
    assert not pc.ordered_sum(np.full((5, 2), NAN), np.zeros(5, bool)).any()   # what the mask leaves out is not read


def test_degenerate_inputs():
    # noise-free: the refit from the truth rounded to float32 moves by the rounding, its last step by nothing
    c = ac.make_pair(3, 120)
    X, xr = c["X"], c["xr"]
    part = ac.participates(X, xr)
    m0 = np.concatenate([c["R"], c["t"][:, None]], 1).astype(F32)
    cnt, mask = pc.support(X, xr, part, m0, 1e-3)
    assert cnt == 120
    m1, d = pc.refit(m0, X, xr, mask, cnt, 3)
    assert d is not None and np.abs(d).max() < 1e-12
    assert np.abs(m1.astype(np.float64) - m0).max() <= 4e-7
    # fewer than four inliers: no refit
    few = mask & (np.cumsum(mask) <= 3)
    out, d = pc.refit(m0, X, xr, few, 3, 3)
    assert d is None and out is not None and pc.same_bits(out, m0)
    w = pc.walk(X[:3], xr[:3], part[:3], m0, 1e-3, 4, 3)
    assert w["counts"].tolist() == [3] * 5 and w["best_round"] == 0 and pc.same_bits(w["model"], m0) and len(set(w["cost"].tolist())) == 1
    # coincident points: the normal matrix has rank 2 and the pivot rule trips
    Xc, xc = np.repeat(X[:1], 8, 0), np.repeat(xr[:1], 8, 0)
    A, b, _ = pc.unpack(pc.sums(m0.astype(np.float64), Xc, xc, np.ones(8, bool)))
    assert pc.solve(A, b) is None
    out, d = pc.refit(m0, Xc, xc, np.ones(8, bool), 8, 3)
    assert d is None and pc.same_bits(out, m0)
    # a NaN or negative threshold, an empty segment: zeros, the input model
    for thr, n in ((NAN, 120), (-1.0, 120), (1e-3, 0)):
        w = pc.walk(X[:n], xr[:n], part[:n], m0, thr, 3, 3)
        assert not w["counts"].any() and not w["cost"].any() and w["best_round"] == 0 and pc.same_bits(w["model"], m0) and not w["mask"].any()


# ---- the layers -------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_exists_in_every_layer_and_refuses_bad_arguments():
    import os
    from pats_amd import _lib, batch, build, ops
    build.build()
    lib = _lib.lib()
    name = "pats_absolute_polish_by_pair_f32"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "pats_amd.h")).read()
    assert name + "(" in header and "Per-pair absolute local optimisation" in header
    assert hasattr(ops, "absolute_polish_by_pair") and hasattr(batch, "polish_abs_by_pair")
    fn = lib.pats_absolute_polish_by_pair_f32
    # refused before any launch: no GPU is touched
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)

    def call(points=a, mr=a, conf=None, pair_off=a, stride=0, counts_in=None, pairs=1, cap=0, models=a, M=1, thr=a, norm=None, use=0,
             min_conf=0.0, best=a, rounds=4, steps=3, model=a, best_count=a, inlier=a, best_round=a, counts=a, cost=a):
        return fn(points, mr, conf, pair_off, stride, counts_in, pairs, cap, models, M, thr, norm, use, min_conf, best, rounds, steps, model,
                  best_count, inlier, best_round, counts, cost, None)

    for arg in ("points", "mr", "models", "thr", "model", "best_count", "inlier", "best_round", "counts", "cost"):
        assert call(**{arg: None}) == 1, arg
        msg = lib.pats_last_error()
        assert msg.startswith(b"absolute_polish_by_pair: null ") and (b"matches_r" if arg == "mr" else arg.encode()) in msg, msg
    for arg, off in (("points", 2), ("mr", 4), ("models", 2), ("thr", 2), ("model", 2), ("best_count", 4), ("best_round", 2), ("counts", 2),
                     ("cost", 4), ("conf", 2), ("norm", 2), ("pair_off", 4), ("best", 2)):
        assert call(**{arg: a + off}) == 1, arg
        msg = lib.pats_last_error()
        assert msg.startswith(b"absolute_polish_by_pair: ") and b"aligned" in msg, msg
    for kw, word in (({"rounds": 0}, b"rounds = 0"), ({"rounds": 17}, b"rounds = 17"), ({"steps": 0}, b"steps = 0"), ({"steps": 9}, b"steps = 9"),
                     ({"best": None, "M": 2}, b"null best needs M == 1"), ({"M": 0}, b"H = 0"), ({"pairs": 0}, b"pairs"),
                     ({"cap": 2 ** 31}, b"cap"), ({"counts_in": a, "stride": 4}, b"exactly one"), ({"use": 1, "min_conf": 0.5}, b"min_conf needs conf"),
                     ({"use": 1, "conf": a, "min_conf": -1.0}, b"min_conf = -1")):
        assert call(**kw) == 1, kw
        msg = lib.pats_last_error()
        assert msg.startswith(b"absolute_polish_by_pair: ") and word in msg, msg
    cap = batch.Capacities(2, 15, 20)
    with pytest.raises(ValueError, match="polish_abs_by_pair: run verify_abs_by_pair first"):
        batch.polish_abs_by_pair({"lifted": ()}, cap, None)


def test_ops_refuses_cpu_wrong_type_wrong_shape_and_strided_tensors():
    import torch
    from pats_amd import ops
    X, mr, off = torch.zeros(8, 3), torch.zeros(8, 2), torch.tensor([0, 8])
    models, thr = torch.zeros(1, 1, 3, 4), torch.zeros(1)
    with pytest.raises(RuntimeError, match="points is on cpu"):
        ops.absolute_polish_by_pair(X, mr, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: models must be float32"):
        ops.absolute_polish_by_pair(X, mr, models.double(), thr, pair_off=off)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: best must be int32"):
        ops.absolute_polish_by_pair(X, mr, models, thr, best=torch.zeros(1, dtype=torch.int64), pair_off=off)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: points must be contiguous"):
        ops.absolute_polish_by_pair(torch.zeros(3, 8).t(), mr, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: give either pair_off, or stride and counts"):
        ops.absolute_polish_by_pair(X, mr, models, thr)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: rounds = 17"):
        ops.absolute_polish_by_pair(X, mr, models, thr, pair_off=off, rounds=17)
    with pytest.raises(RuntimeError, match="absolute_polish_by_pair: steps = 0"):
        ops.absolute_polish_by_pair(X, mr, models, thr, pair_off=off, steps=0)
