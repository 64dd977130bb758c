"""GPU: the local optimisation of the absolute-pose branch - ops.absolute_polish_by_pair and batch.polish_abs_by_pair - against the
definition of include/pats_amd.h ("Per-pair absolute local optimisation") restated in float64 numpy (tests/absolute_polish_cases.py):
    one round     counts[:, 0], the round-0 masks and cost[:, 0] are the restatement's; the model is the restatement's m_1 - or m_0 by
                  the best rule - within the float32 cast of two float64 results that differ by summation order
    any rounds    the outputs are consistent with one another and with the float32 emulation of the device's own model; R is
                  orthonormal; the support never falls below round 0's
    accuracy      the distance to the true pose is at most 4 x the restatement's on the same input
    determinism, a segment too long to stage, the confidence gate, and the chain through batch on a mixed pack and on a top-K
docs/parity.md records the measured margins.  Every output lies inside a larger sentinel-filled buffer and every input list in a
larger NaN-filled one: a call must define every byte of its views, none around them, and read no row beyond cap.

Measured (MI355X): see docs/parity.md, "Per-pair absolute local optimisation"."""
import numpy as np
import pytest
import torch

import absolute_cases as ac
import absolute_polish_cases as pc
import epipolar_cases as ec

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0xAB
F32 = np.float32
NAN = float("nan")
EPS32 = pc.EPS32
ABS_STAGE = 6144                                                              # csrc/absolute.hip: the matches a workgroup keeps in LDS
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 300, 511, 512, 513]
TAIL = 23                                                                     # rows inside cap behind the last segment


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a):
    """A list as the view of a longer buffer whose rows beyond cap are NaN."""
    buf = torch.full((a.shape[0] + PAD,) + tuple(a.shape[1:]), NAN, dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


class Sentinel:
    """Output views inside sentinel-filled buffers; check() asserts that nothing around them changed."""

    def __init__(self):
        self.bufs = []

    def view(self, shape, dtype):
        sent = {torch.float32: SENT_F, torch.float64: SENT_F, torch.int32: SENT_I, torch.int64: SENT_I, torch.uint8: SENT_B}[dtype]
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device="cuda")
        self.bufs.append((buf, sent))
        return buf[PAD:PAD + n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, sent in self.bufs:
            assert bool((torch.cat([buf[:PAD], buf[-PAD:]]) == sent).all()), "bytes around an output view changed"


def run_polish(ops, X, mr, models, thr, rounds, steps, **kw):
    """-> (model, best_count, inlier, best_round, counts, cost) as numpy, from sentinel-guarded destinations."""
    d = {k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    pairs, cap = models.shape[0], X.shape[0]
    s = Sentinel()
    dest = (s.view((pairs, 3, 4), torch.float32), s.view((pairs,), torch.int64), s.view((cap,), torch.uint8), s.view((pairs,), torch.int32),
            s.view((pairs, rounds + 1), torch.int32), s.view((pairs, rounds + 1), torch.float64))
    if "conf" in d:
        d["conf"] = guarded(kw["conf"])
    got = ops.absolute_polish_by_pair(guarded(X), guarded(mr), cu(models), cu(thr), rounds=rounds, steps=steps, out=dest, **d)
    s.check()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, dest))
    return tuple(t.cpu().numpy() for t in dest)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_tensor(a, b):
    """Equal bit for bit (the invalid lifts' NaN rows too)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def check_consistent(got, X, mr, segs, thr, m0, norm=None, conf=None, min_conf=None):
    """What holds between the six outputs of any call, whatever the number of rounds."""
    model, best_count, inlier, best_round, counts, cost = got
    covered = np.zeros(X.shape[0], bool)
    for p, (lo, n) in enumerate(segs):
        x, r = X[lo:lo + n], ac.right32(mr[lo:lo + n], None if norm is None else norm[p])
        part = ac.participates(x, r, None if conf is None else conf[lo:lo + n], min_conf)
        c, mask = pc.support(x, r, part, model[p], thr[p])
        assert np.array_equal(inlier[lo:lo + n].astype(bool), mask) and best_count[p] == c == inlier[lo:lo + n].sum(), p
        assert counts[p, best_round[p]] == best_count[p] and best_count[p] >= counts[p, 0] and best_count[p] == counts[p].max(), p
        assert best_round[p] == pc.pick(counts[p], cost[p]), p
        if best_round[p] == 0:
            assert pc.same_bits(model[p], m0[p]), p
        for q in range(1, counts.shape[1]):                                   # a repeated model: everything behind it repeats
            if counts[p, q] == counts[p, q - 1] and same_bits(cost[p, q:q + 1], cost[p, q - 1:q]):
                assert (counts[p, q:] == counts[p, q]).all() and same_bits(cost[p, q:], np.full_like(cost[p, q:], cost[p, q])), p
        assert (cost[p][counts[p] == 0] == 0).all() and (cost[p] >= 0).all()
        covered[lo:lo + n] = True
    assert not inlier[~covered].any()


# ---- 1. one round against the restatement ---------------------------------------------------------------------------------------
def ragged_case(lengths, seed):
    """Noisy pairs of the given lengths (the short ones clean, so that four and five matches are a support of four and five) ->
    (X, mr, pair_off, m0 [pairs,3,4]: the truth moved by a small rigid motion, rounded to float32)."""
    Xs, rs, m0 = [], [], []
    for p, n in enumerate(lengths):
        c = pc.noisy_pair(seed + 17 * p, max(n, 1), **({} if n > 5 else {"outliers": 0.0, "holes": 0.0}))
        rng = np.random.default_rng(seed + 1000 + p)
        E = ac.rodrigues(3e-4 * rng.normal(size=3))
        m0.append(np.concatenate([E @ c["R"], (E @ c["t"] + 3e-4 * rng.normal(size=3))[:, None]], 1))
        Xs.append(c["X"][:n])
        rs.append(c["xr"][:n])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(Xs), np.concatenate(rs), off, np.stack(m0).astype(F32)


def check_one_round(got, ref, m0, steps, tag):
    """rounds = 1: the device against the restatement's walk -> the largest model difference in units of eps32 max(1, |entry|)."""
    model, best_count, inlier, best_round, counts, cost = got
    worst, refits, worst_cost = 0.0, 0, 0.0
    for p, r in enumerate(ref):
        assert counts[p, 0] == r["counts"][0], "%s pair %d: c_0" % (tag, p)
        worst_cost = max(worst_cost, abs(cost[p, 0] - r["cost"][0]) / r["cost"][0] if r["cost"][0] > 0 else 0.0)
        assert abs(cost[p, 0] - r["cost"][0]) <= 1e-12 * abs(r["cost"][0]), "%s pair %d: S_0 = %r against %r" % (tag, p, cost[p, 0], r["cost"][0])
        assert best_round[p] == pc.pick(counts[p], cost[p])
        seg = slice(r["lo"], r["lo"] + r["n"])
        if pc.same_bits(r["models"][1], r["models"][0]):                      # "no refit": the walk ends at round 0
            assert counts[p, 1] == counts[p, 0] and cost[p, 1] == cost[p, 0] and best_round[p] == 0, "%s pair %d" % (tag, p)
        if best_round[p] == 0:
            assert pc.same_bits(model[p], r["models"][0]) and np.array_equal(inlier[seg].astype(bool), r["masks"][0]), "%s pair %d" % (tag, p)
        else:
            refits += 1
            d = np.abs(model[p].astype(np.float64) - r["models"][1]) / np.maximum(1.0, np.abs(r["models"][1]))
            worst = max(worst, float(d.max()) / EPS32)
            assert d.max() <= 2 * EPS32, "%s pair %d: the model differs from the restatement's m_1 by %.3g eps32" % (tag, p, d.max() / EPS32)
    print("%s, steps = %d: %d pairs refitted, the largest |model - m_1| = %.3f eps32 max(1, |entry|), the largest |S_0 - restatement's| = %.3g S_0" %
          (tag, steps, refits, worst, worst_cost))
    return refits


@pytest.mark.parametrize("steps", [1, 3])
def test_one_round_equals_the_restatement(ops, steps):
    pairs = len(LENGTHS)
    X, mr, off, m0 = ragged_case(LENGTHS, 900)
    X, mr = np.concatenate([X, X[:TAIL]]), np.concatenate([mr, mr[:TAIL]])
    thr = np.full(pairs, 3e-3, F32)
    thr[7] = NAN
    models = np.stack([np.zeros_like(m0), m0], 1)                             # the winner is model 1; model 0 is the zero model
    best = np.ones(pairs, np.int32)
    best[9] = 7                                                               # out of range: clamped to M - 1 = 1
    best[10] = -3                                                             # clamped to 0: the zero model has no inlier
    m_in = m0.copy()
    m_in[10] = 0
    # the ragged form
    segs = ec.segments(pairs, X.shape[0], pair_off=off)
    got = run_polish(ops, X, mr, models, thr, 1, steps, pair_off=off, best=best)
    ref = pc.walk_reference(X, mr, segs, m_in, thr, 1, steps)
    assert check_one_round(got, ref, m_in, steps, "ragged") >= 6
    check_consistent(got, X, mr, segs, thr, m_in)
    assert not got[4][7].any() and not got[5][7].any() and not got[4][10].any() and got[3][10] == 0 and pc.same_bits(got[0][10], m_in[10])
    assert got[4][1, 0] == 1 and got[4][2, 0] == 3 and got[4][3, 0] >= 4 and got[4][4, 0] >= 4 and got[3][1] == 0 and got[3][2] == 0     # three inliers: no refit; four: one
    # round 0's support is the verification's, bit for bit
    s = ops.absolute_score_by_pair(cu(X), cu(mr), cu(m_in[:, None]), cu(thr), pair_off=cu(off))
    assert np.array_equal(s[0].cpu().numpy()[:, 0], got[4][:, 0])
    for p, r in enumerate(ref):
        assert np.array_equal(s[3].cpu().numpy()[r["lo"]:r["lo"] + r["n"]].astype(bool), r["masks"][0])
    # the strided form: the same pairs in rows of `stride`, one count short of its row, one beyond it (clamped)
    stride = max(LENGTHS) + 5
    Xs, rs = np.full((pairs * stride + TAIL, 3), NAN, F32), np.full((pairs * stride + TAIL, 2), NAN, F32)
    for p, n in enumerate(LENGTHS):
        Xs[p * stride:p * stride + n], rs[p * stride:p * stride + n] = X[off[p]:off[p] + n], mr[off[p]:off[p] + n]
    cnt = np.array(LENGTHS, np.int64)
    cnt[8] = 299
    cnt[11] = stride + 9
    segs_s = ec.segments(pairs, Xs.shape[0], stride=stride, counts=cnt)
    got_s = run_polish(ops, Xs, rs, models, thr, 1, steps, stride=stride, counts=cnt, best=best)
    ref_s = pc.walk_reference(Xs, rs, segs_s, m_in, thr, 1, steps)
    check_one_round(got_s, ref_s, m_in, steps, "strided")
    check_consistent(got_s, Xs, rs, segs_s, thr, m_in)
    same = [p for p in range(pairs) if p not in (8, 11)]                      # the same segment at the same indices: the same bits
    for k in (0, 1, 3, 4, 5):
        assert same_bits(got_s[k][same], got[k][same]), k


# ---- 2. - 4. the twelve noisy cases: self-consistency, accuracy, determinism --------------------------------------------------------
@pytest.fixture(scope="module")
def noisy():
    """The twelve cases of the host test in one ragged call, and the restatement's walk (T = 4, G = 3) - computed once, not changed."""
    cases = [pc.noisy_pair(seed) for seed in pc.SEEDS]
    win = [pc.ransac_models(c, pair_seed=seed) for c, seed in zip(cases, pc.SEEDS)]
    m0 = np.stack([m[b] for m, b in win])
    n = cases[0]["X"].shape[0]
    X, mr = np.concatenate([c["X"] for c in cases] + [cases[0]["X"][:TAIL]]), np.concatenate([c["xr"] for c in cases] + [cases[0]["xr"][:TAIL]])
    off = (np.arange(len(cases) + 1) * n).astype(np.int64)
    thr = np.full(len(cases), pc.THR, F32)
    segs = ec.segments(len(cases), X.shape[0], pair_off=off)
    return {"cases": cases, "m0": m0, "X": X, "mr": mr, "off": off, "thr": thr, "segs": segs,
            "ref": pc.walk_reference(X, mr, segs, m0, thr, 4, 3)}


@pytest.mark.parametrize("rounds", [4, 16])
def test_outputs_are_consistent_at_any_number_of_rounds(ops, noisy, rounds):
    q = noisy
    got = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], rounds, 3, pair_off=q["off"])
    check_consistent(got, q["X"], q["mr"], q["segs"], q["thr"], q["m0"])
    model, best_count, inlier, best_round, counts, cost = got
    RtR = np.einsum("pki,pkj->pij", model[:, :, :3].astype(np.float64), model[:, :, :3].astype(np.float64))
    dev = np.abs(RtR - np.eye(3)).max()
    print("rounds = %d: |R^T R - I|_max = %.3f eps32, best rounds %s, support %s -> %s" %
          (rounds, dev / EPS32, best_round.tolist(), counts[:, 0].tolist(), best_count.tolist()))
    assert dev <= 4 * EPS32
    assert (best_count > counts[:, 0]).sum() >= 10                            # the cases gain support (the host test: the restatement does on all)
    if rounds == 16:
        short = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"])
        assert np.array_equal(counts[:, :5], short[4]) and same_bits(np.ascontiguousarray(cost[:, :5]), short[5])    # the walk does not depend on T
        ended = [(counts[p, 15] == counts[p, 16]) and cost[p, 15] == cost[p, 16] for p in range(len(q["cases"]))]
        assert sum(ended) >= 3                                                # walks that reach a repeated model: the padding is exercised


def test_accuracy_against_the_restatement(ops, noisy):
    q = noisy
    got = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"])
    worst = 0.0
    for p, (c, r) in enumerate(zip(q["cases"], q["ref"])):
        d_dev, d_ref, d_0 = pc.model_distance(got[0][p], c), pc.model_distance(r["model"], c), pc.model_distance(q["m0"][p], c)
        # 4 x the restatement on the same input: 2 for the operation order, 2 for a float32 rounding per round (test_absolute_gpu.py's
        # factor for a chain against its float64 restatement); the floor is float32's step at |t|
        tol = 4 * max(d_ref, EPS32 * np.linalg.norm(c["t"]))
        worst = max(worst, d_dev / tol * 4)
        print("pair %d: pose_distance %.3g -> %.3g (restatement %.3g), support %d -> %d (restatement %d)" %
              (p, d_0, d_dev, d_ref, got[4][p, 0], got[1][p], r["best_count"]))
        assert d_dev <= tol
        assert got[4][p, 0] == r["counts"][0] and abs(got[5][p, 0] - r["cost"][0]) <= 1e-12 * r["cost"][0]
    print("accuracy: the largest pose_distance(device) / pose_distance(restatement) = %.3f (bound 4)" % worst)


def test_two_calls_give_the_same_bits(ops, noisy):
    q = noisy
    a = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"])
    b = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"])
    assert all(same_bits(x, y) for x, y in zip(a, b))


# ---- 5. a segment too long to stage -----------------------------------------------------------------------------------------------
def test_walks_a_segment_too_long_to_stage(ops):
    X, mr, off, m0 = ragged_case([ABS_STAGE + 1, 200], 950)
    thr = np.full(2, 3e-3, F32)
    segs = ec.segments(2, X.shape[0], pair_off=off)
    one = run_polish(ops, X, mr, m0[:, None], thr, 1, 3, pair_off=off)
    ref = pc.walk_reference(X, mr, segs, m0, thr, 1, 3)
    assert check_one_round(one, ref, m0, 3, "long") == 2
    check_consistent(one, X, mr, segs, thr, m0)
    two = run_polish(ops, X, mr, m0[:, None], thr, 2, 3, pair_off=off)
    check_consistent(two, X, mr, segs, thr, m0)
    assert np.array_equal(two[4][:, :2], one[4]) and same_bits(np.ascontiguousarray(two[5][:, :2]), one[5])
    assert one[1][0] > 3000
    # the short pair alone walks as it did beside the long one: the same values
    lo = int(off[1])
    alone = run_polish(ops, X[lo:], mr[lo:], m0[1:, None], thr[1:], 2, 3, pair_off=np.array([0, 200], np.int64))
    assert all(same_bits(np.ascontiguousarray(a[1:] if k != 2 else a[lo:]), b) for k, (a, b) in enumerate(zip(two, alone)))


# ---- 6. the confidence gate ----------------------------------------------------------------------------------------------------------
def test_confidence_gate_removes_exactly_the_gated_matches(ops, noisy):
    q = noisy
    rng = np.random.default_rng(5)
    conf = rng.random(q["X"].shape[0]).astype(F32)
    conf[::13] = NAN
    gated = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"], conf=conf, min_conf=0.3)
    check_consistent(gated, q["X"], q["mr"], q["segs"], q["thr"], q["m0"], conf=conf, min_conf=0.3)
    Xn = q["X"].copy()
    Xn[~(conf >= F32(0.3))] = NAN                                              # the gated matches take no part: the same walk
    plain = run_polish(ops, Xn, q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"])
    assert all(same_bits(a, b) for a, b in zip(gated, plain))
    assert not gated[2][~(conf >= F32(0.3))].any()
    free = run_polish(ops, q["X"], q["mr"], q["m0"][:, None], q["thr"], 4, 3, pair_off=q["off"], conf=conf)     # no min_conf: conf is not read
    assert (free[4][:, 0] > gated[4][:, 0]).all()


# ---- 7. the chain through batch ----------------------------------------------------------------------------------------------------
FOCAL = 60.0
PIXEL_NOISE = 0.15


def render_depth(h, w, seed):
    """A plane with a box on it, seen from the left camera at the origin: depth per pixel (i = y, j = x)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    y, x = (i - h / 2) / FOCAL, (j - w / 2) / FOCAL
    plane = 4.0 / (1.0 + 0.3 * x + 0.2 * y)
    box = (np.abs(i - h * rng.uniform(0.3, 0.7)) < h / 6) & (np.abs(j - w * rng.uniform(0.3, 0.7)) < w / 6)
    return np.where(box, 2.5, plane).astype(F32)


def chain_case(shapes, n, seed):
    """Per pair (the CALLER's order): a depth map, n left pixels, the right pixels under a known metric pose with PIXEL_NOISE pixels
    of noise (30 % outliers), 15 % of the matches on depth holes; everything in the hand-over's (y, x) order -> list of dicts."""
    P = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]])
    out = []
    for p, (h, w) in enumerate(shapes):
        rng = np.random.default_rng(seed + p)
        depth = render_depth(h, w, seed + 10 * p)
        ml = np.stack([rng.uniform(0, h - 1, n), rng.uniform(0, w - 1, n)], 1).astype(F32)
        hole = rng.random(n) < 0.15
        depth[np.rint(ml[hole, 0]).astype(int), np.rint(ml[hole, 1]).astype(int)] = 0.0
        norm = np.array([h / 2, w / 2, 1 / FOCAL, 1 / FOCAL] * 2, F32)
        X, ok = ac.lift32(ml, depth, norm[:4])
        R, t = ac.rodrigues(0.15 * rng.normal(size=3)), 0.4 * rng.normal(size=3)       # the reference's (x, y) frame
        Y = np.where(ok[:, None], X, 1.0).astype(np.float64) @ (P @ R @ P).T + P @ t
        mr = np.stack([Y[:, 0] / Y[:, 2] * FOCAL + h / 2, Y[:, 1] / Y[:, 2] * FOCAL + w / 2], 1)
        mr += rng.normal(scale=PIXEL_NOISE, size=mr.shape)
        bad = rng.random(n) < 0.3
        mr[bad] = np.stack([rng.uniform(0, h, int(bad.sum())), rng.uniform(0, w, int(bad.sum()))], 1)
        out.append({"depth": depth, "ml": ml, "mr": mr.astype(F32), "norm": norm, "R": R, "t": t})
    return out


@pytest.mark.parametrize("on", ["all", "topk"])
def test_chain_through_batch(ops, on):
    from pats_amd import batch
    shapes, n, H, seed = [(40, 56), (48, 64), (40, 56)], 200, 64, 5
    pairs = len(shapes)
    cases = chain_case(shapes, n, 700)
    mixed = on == "all"
    caller_of = [1, 0, 2] if mixed else [0, 1, 2]                             # slot s holds the caller's pair caller_of[s]
    cap = batch.Capacities(pairs, 5, 6)
    ml = np.concatenate([cases[i]["ml"] for i in caller_of])
    mr = np.concatenate([cases[i]["mr"] for i in caller_of])
    summary = np.concatenate([np.arange(pairs + 1) * n, [pairs * n, 0, 0]]).astype(np.int64)
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if mixed:
        out["caller_of"] = caller_of
    else:                                                                     # the same rows as a top-K result
        out["topk"] = (dl.view(pairs, n, 2), dr.view(pairs, n, 2), torch.ones(pairs, n, device="cuda"),
                       torch.arange(n, dtype=torch.int32, device="cuda").repeat(pairs, 1), cu(np.full(pairs, n, np.int64)))
    norm = cu(np.stack([c["norm"] for c in cases]))
    thr_np = np.array([0.5 / FOCAL, 0.6 / FOCAL, 0.55 / FOCAL], F32)          # per pair: a wrong permutation shows
    thr = cu(thr_np)
    depths = [cu(c["depth"]) for c in cases]
    T1 = np.tile(np.eye(4), (pairs, 1, 1))
    for i, c in enumerate(cases):
        T1[i, :3, :3], T1[i, :3, 3] = c["R"], c["t"]
    with pytest.raises(ValueError, match="polish_abs_by_pair: run verify_abs_by_pair first"):
        batch.polish_abs_by_pair(out, cap, thr, norm=norm)
    # the other branches first: they must come through untouched
    E = np.stack([ac.pose_from_model(np.concatenate([c["R"], c["t"][:, None]], 1), False)[0] for c in cases]).astype(F32)
    batch.verify_by_pair(out, cap, cu(E.reshape(pairs, 1, 3, 3)), thr, norm=norm, on=on, moments=True)
    batch.pose_by_pair(out, cap, norm=norm, swapped=True)
    batch.verify_h_by_pair(out, cap, cu(np.tile(np.eye(3, dtype=F32), (pairs, 1, 1, 1))), thr, norm=norm, on=on)
    lifted = batch.lift_by_pair(out, cap, depths, norm, on=on)
    kept = {k: [t.clone() for t in out[k] if isinstance(t, torch.Tensor)] for k in ("pose", "verified", "verified_h", "lifted")}
    held = {k: out[k] for k in kept}
    models = batch.hypothesize_p3p_by_pair(out, cap, H, seed=seed, norm=norm, progressive=False)
    with pytest.raises(ValueError, match="polish_abs_by_pair: run verify_abs_by_pair first"):
        batch.polish_abs_by_pair(out, cap, thr, norm=norm)
    ver = batch.verify_abs_by_pair(out, cap, models, thr, norm=norm)
    slot_models, slot_best, before_count = out["verified_abs_models"], ver[1], ver[2].clone()
    batch.pose_abs_by_pair(out, cap, swapped=True)
    err_before = batch.pose_error_by_pair(batch.pose_branch(out, "absolute"), cap, cu(T1))[2].cpu().numpy()

    pol = batch.polish_abs_by_pair(out, cap, thr, rounds=4, steps=3, norm=norm)
    assert out["verified_abs"] is pol and len(pol) == 4 and out["verified_abs_on"] == on and len(out["polished_abs"]) == 4
    pose = batch.pose_abs_by_pair(out, cap, swapped=True)
    view = batch.pose_branch(out, "absolute")
    err_after = batch.pose_error_by_pair(view, cap, cu(T1))[2].cpu().numpy()
    torch.cuda.synchronize()

    for k in kept:                                                            # bit-unchanged, and the same objects
        assert out[k] is held[k] and all(same_tensor(a, b) for a, b in zip([t for t in out[k] if isinstance(t, torch.Tensor)], kept[k])), k
    # the polished tuple, in SLOT order: what the ops call gives on the slots' own rows, thresholds and norms
    idx = torch.tensor(caller_of, device="cuda")
    seg = {"stride": n, "counts": out["topk"][4]} if not mixed else {"pair_off": ds[:pairs + 1]}
    want = ops.absolute_polish_by_pair(lifted[0], dr, slot_models, thr.index_select(0, idx), best=slot_best, rounds=4, steps=3,
                                       norm=norm.index_select(0, idx), **seg)
    model, best_round, counts, cost = out["polished_abs"]
    assert torch.equal(model, want[0]) and torch.equal(pol[2], want[1]) and torch.equal(pol[3], want[2])
    assert torch.equal(best_round, want[3]) and torch.equal(counts, want[4]) and torch.equal(cost, want[5])
    assert torch.equal(pol[0], want[1].to(torch.int32)[:, None]) and not bool(pol[1].any()) and pol[1].dtype == torch.int32
    assert out["verified_abs_models"].shape == (pairs, 1, 3, 4) and torch.equal(out["verified_abs_models"][:, 0], model)
    assert bool((pol[2] >= before_count).all()) and bool((pol[2] > before_count).any())
    assert view["verified"] is pol and view["pose"] is pose
    # the pose in the CALLER's order: the polished model of the pair's slot, widened, in the reference's frame
    P = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1]])
    m = model.cpu().numpy().astype(np.float64)
    for i, c in enumerate(cases):
        s_ = caller_of.index(i)
        assert np.array_equal(pose[1][i].cpu().numpy(), P @ m[s_][:, :3] @ P) and np.array_equal(pose[2][i].cpu().numpy(), P @ m[s_][:, 3])
        assert int(pose[3][i]) == int(pol[2][s_])
        print("%s pair %d: err %.4f -> %.4f degrees, support %d -> %d, best round %d" %
              (on, i, err_before[i], err_after[i], int(before_count[s_]), int(pol[2][s_]), int(best_round[s_])))
        assert err_after[i] <= err_before[i]
