"""GPU: the per-pair MSAC scoring - ops.{epipolar,homography}_score_msac_by_pair and batch.verify{,_h}_msac_by_pair - against
the definition of include/pats_amd.h ("Per-pair MSAC scoring") restated in numpy (tests/msac_cases.py):
    gains        |gains / 2^20 - G64| <= S per model: G64 the float64 gain, S the summed per-cell bound of a float32 evaluation
                 (eps = 8 * 2^-24 from an analysis of plain float32, tests/test_msac_cases_host.py caps S at 4 on the committed
                 cases).  The test prints the largest |gains / 2^20 - G64| / S it met; docs/parity.md ("MSAC scoring") records it
    counts       array-equal to the count entry's on the same inputs
    winner       best the lowest index of the largest of the device's own gains, best_gain and best_count that model's, inlier and
                 moments bit-equal to the count entry called with the winner as the pair's only model, and the float64 gain of
                 the winner within the two bounds of the float64 maximum
    disagreement on the committed seeds the MSAC entry returns the true model (1) where the count entry returns the perturbed one (0)
    placement    a pair's gains do not depend on where its segment lies or in which form it is given; two calls give identical bits
Every output lies inside a larger sentinel-filled buffer: a call defines every byte of the views and none around them."""
import numpy as np
import pytest
import torch

import epipolar_cases as ec
import homography_cases as hm
import msac_cases as mc

pytestmark = pytest.mark.gpu

PAD = 64
SENT = {torch.int32: -123456, torch.int64: -123456, torch.uint8: 0xA5, torch.float64: -777.25}
T, C = 2048, 256        # the score kernel's match tile (EPI_THREADS * EPI_R) and model chunk (EPI_CHUNK): asserted against the source
NORM = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)
LENGTHS = ([1], [T - 1, 0, T], [T + 1, 0, 2 * T + 1], [1, 0, 63], [64, 0, 65])
HS = (1, 64, 65, C - 1, C, C + 1)


def test_the_tile_constants_are_the_kernels():
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "pats_amd", "csrc", "epipolar.hip")).read()
    k = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))       # noqa: E731
    assert k("EPI_THREADS") * k("EPI_R") == T and k("EPI_CHUNK") == C


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    assert ops.msac_gain_one() == mc.ONE
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def views_of(shapes):
    """Sentinel-filled buffers -> (views, check): check() asserts that the PAD elements around every view kept the sentinel."""
    views, whole = [], []
    for shape, dt in shapes:
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENT[dt], dtype=dt, device="cuda")
        whole.append(buf)
        views.append(buf[PAD:PAD + n].view(shape))

    def check():
        for buf in whole:
            assert bool((torch.cat([buf[:PAD], buf[-PAD:]]) == SENT[buf.dtype]).all()), "bytes around an output view changed"
    return tuple(views), check


def guarded(a):
    """A list as a view of a longer buffer whose rows beyond cap are NaN: a read past cap would show in the gains."""
    buf = torch.full((a.shape[0] + PAD, 2), float("nan"), dtype=torch.float32, device="cuda")
    buf[:a.shape[0]] = cu(a)
    return buf[:a.shape[0]]


def run(ops, family, ml, mr, models, thr, msac=True, moments=True, **kw):
    """-> dict of numpy arrays: counts, best, best_count, inlier[, moments][, gains, best_gain]."""
    pairs, H = models.shape[0], models.shape[1]
    names = ["counts", "best", "best_count", "inlier"] + (["moments"] if moments else []) + (["gains", "best_gain"] if msac else [])
    shape = {"counts": ((pairs, H), torch.int32), "best": ((pairs,), torch.int32), "best_count": ((pairs,), torch.int64),
             "inlier": ((ml.shape[0],), torch.uint8), "moments": ((pairs, 9, 9), torch.float64), "gains": ((pairs, H), torch.int64),
             "best_gain": ((pairs,), torch.int64)}
    views, chk = views_of([shape[n] for n in names])
    fn = getattr(ops, "%s_score%s_by_pair" % (family, "_msac" if msac else ""))
    got = fn(guarded(ml), guarded(mr), cu(models), cu(np.asarray(thr, np.float32)), moments=moments, out=views,
             **{k: (cu(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert len(got) == len(names) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    chk()
    return {n: v.cpu().numpy() for n, v in zip(names, views)}


def same_bits(a, b, names=None):
    for n in names or a:
        assert a[n].tobytes() == b[n].tobytes(), n


def make_pairs(family, lengths, Hmax, seed, thrs=(1e-2, 2e-3, 5e-4)):
    """Seeded pairs concatenated -> (ml, mr, pair_off, models [pairs,Hmax,3,3], thr [pairs]); the true model sits at index 0 of the
    odd pairs and at its seeded index of the even ones."""
    mls, mrs, models, thr = [], [], [], []
    for p, n in enumerate(lengths):
        c = mc.make_case(family, seed + 31 * p, max(n, 8), Hmax, thrs[p % len(thrs)])
        m = c["models"].copy()
        if p % 2:
            m[[0, c["true"]]] = m[[c["true"], 0]]
        mls.append(c["ml"][:n]); mrs.append(c["mr"][:n]); models.append(m); thr.append(c["thr"])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return np.concatenate(mls), np.concatenate(mrs), off, np.stack(models), np.asarray(thr, np.float32)


def check_msac(family, ops, ml, mr, models, thr, ref, segs, stats, **kw):
    """One MSAC call against the restatement `ref` (of these models) and against the count entry -> the MSAC call's outputs."""
    got = run(ops, family, ml, mr, models, thr, **kw)
    cnt = run(ops, family, ml, mr, models, thr, msac=False, **kw)
    assert got["gains"].dtype == np.int64 and got["best_gain"].dtype == np.int64 and got["best"].dtype == np.int32
    assert np.array_equal(got["counts"], cnt["counts"]), "counts differ from the count entry's"
    pairs, H = models.shape[:2]
    covered = np.zeros(ml.shape[0], bool)
    for p, (r, (lo, n)) in enumerate(zip(ref, segs)):
        covered[lo:lo + n] = True
        g = got["gains"][p] / mc.ONE
        G64, S = r["G64"][:H], r["S"][:H]
        err = np.abs(g - G64)
        assert np.all(err <= S), "pair %d: gains outside the bound by %g" % (p, float((err - S).max()))
        if (S > 0).any():
            stats.append(float((err[S > 0] / S[S > 0]).max()))
        b = int(got["best"][p])
        assert b == int(np.argmax(got["gains"][p])), "pair %d: best is not the lowest index of the largest gain" % p
        assert got["best_gain"][p] == got["gains"][p, b] and got["best_count"][p] == got["counts"][p, b]
        assert G64[b] >= G64.max() - S[b] - S[int(np.argmax(G64))], "pair %d: the winner's float64 gain is not the maximum's" % p
        assert got["inlier"][lo:lo + n].sum() == got["best_count"][p]
    assert set(np.unique(got["inlier"])) <= {0, 1} and not got["inlier"][~covered].any()
    # the mask kernel of today on the MSAC winner: the count entry with that one model
    winner = models[np.arange(pairs), got["best"]][:, None]
    one = run(ops, family, ml, mr, winner, thr, msac=False, **kw)
    same_bits(got, one, ["inlier", "moments", "best_count"])
    return got


# ---- 1. the sandwich and self-consistency ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_gains_lie_within_the_bound_and_the_outputs_agree_with_each_other(ops, family, lengths):
    ml, mr, off, models, thr = make_pairs(family, lengths, C + 1, 900 + len(lengths) + lengths[0])
    segs = ec.segments(len(lengths), ml.shape[0], pair_off=off)
    ref = mc.reference(family, ml, mr, segs, models, thr)                        # once, for the C + 1 models: a model's gain is its own
    stats = []
    for H in HS:
        got = check_msac(family, ops, ml, mr, np.ascontiguousarray(models[:, :H]), thr, ref, segs, stats, pair_off=off)
        for p, n in enumerate(lengths):
            if n == 0:
                assert not got["gains"][p].any() and got["best"][p] == 0 and got["best_gain"][p] == 0 and got["best_count"][p] == 0
    if max(lengths) >= 64:
        assert max(r["G64"].max() for r in ref) > 10                              # the cases have something to rank
    print("%s %s: the largest |gains / 2^20 - G64| / S = %.4f, the largest S = %.3f"
          % (family, lengths, max(stats) if stats else 0.0, max(float(r["S"].max()) for r in ref)))


# ---- 2. the committed disagreement seeds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_msac_picks_the_true_model_where_the_count_picks_the_perturbed_one(ops, family):
    cs = [mc.disagreement_case(family, seed, n) for seed, n in mc.DISAGREEMENTS[family]]
    lens = [c["ml"].shape[0] for c in cs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ml, mr = np.concatenate([c["ml"] for c in cs]), np.concatenate([c["mr"] for c in cs])
    models, thr = np.stack([c["models"] for c in cs]), np.asarray([c["thr"] for c in cs], np.float32)
    segs = ec.segments(len(cs), ml.shape[0], pair_off=off)
    ref = mc.reference(family, ml, mr, segs, models, thr)
    got = check_msac(family, ops, ml, mr, models, thr, ref, segs, [], pair_off=off)
    cnt = run(ops, family, ml, mr, models, thr, msac=False, pair_off=off)
    print(family, "counts", got["counts"].tolist(), "gains / 2^20", np.round(got["gains"] / mc.ONE, 2).tolist())
    assert got["best"].tolist() == [1] * len(cs) and cnt["best"].tolist() == [0] * len(cs)
    assert (got["best_count"] < cnt["best_count"]).all()


# ---- 3. placement independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_a_pairs_gains_do_not_depend_on_where_its_segment_lies(ops, family):
    n, H = T + 5, 65
    ml, mr, off, models, thr = make_pairs(family, [300, 77, n], H, 4100)
    lo = int(off[2])
    alone = run(ops, family, ml[lo:], mr[lo:], models[2:], thr[2:], pair_off=np.array([0, n], np.int64))
    ragged = run(ops, family, ml, mr, models, thr, pair_off=off)
    again = run(ops, family, ml, mr, models, thr, pair_off=off)
    same_bits(ragged, again)
    stride = n + 11                                                               # the strided form: slack rows behind every pair, a tail
    sl, sr = np.full((3 * stride + 5, 2), 0.25, np.float32), np.full((3 * stride + 5, 2), -0.5, np.float32)
    for p in range(3):
        k = int(off[p + 1] - off[p])
        sl[p * stride:p * stride + k], sr[p * stride:p * stride + k] = ml[off[p]:off[p + 1]], mr[off[p]:off[p + 1]]
    strided = run(ops, family, sl, sr, models, thr, stride=stride, counts=np.diff(off))
    for name in ("gains", "counts", "best", "best_gain", "best_count", "moments"):
        assert np.array_equal(alone[name][0], ragged[name][2]), name
        assert np.array_equal(ragged[name], strided[name]), name
    assert alone["gains"][0].max() > 100 * mc.ONE
    assert np.array_equal(alone["inlier"], ragged["inlier"][lo:])
    for p in range(3):                                                            # slack rows and the tail: defined, zero
        k = int(off[p + 1] - off[p])
        assert np.array_equal(strided["inlier"][p * stride:p * stride + k], ragged["inlier"][off[p]:off[p + 1]])
        assert not strided["inlier"][p * stride + k:(p + 1) * stride].any()
    assert not strided["inlier"][3 * stride:].any()


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_norm_gate_non_finite_rows_and_zero_models(ops, family):
    lengths, H = [700, 130], 70
    ml, mr, off, models, thr = make_pairs(family, lengths, H, 5200)
    models[:, 40:] = 0                                                            # zero models pad H
    segs = ec.segments(2, ml.shape[0], pair_off=off)
    # norm: raw points that normalise to the case's - against the pre-normalised points, bit for bit
    norm = np.stack([NORM, NORM + np.array([0.01, 0, 0, 0, 0, -0.01, 0, 0], np.float32)])
    rawl, rawr = ml.copy(), mr.copy()
    for p, (lo, n) in enumerate(segs):
        rawl[lo:lo + n] = ml[lo:lo + n] / norm[p, 2:4] + norm[p, 0:2]
        rawr[lo:lo + n] = mr[lo:lo + n] / norm[p, 6:8] + norm[p, 4:6]
    pre = [ec.points32(rawl[lo:lo + n], rawr[lo:lo + n], norm[p]) for p, (lo, n) in enumerate(segs)]
    prel, prer = np.concatenate([a for a, _ in pre]), np.concatenate([b for _, b in pre])
    ref = mc.reference(family, rawl, rawr, segs, models, thr, norm=norm)
    stats = []
    a = check_msac(family, ops, rawl, rawr, models, thr, ref, segs, stats, pair_off=off, norm=norm)
    b = run(ops, family, prel, prer, models, thr, pair_off=off)
    same_bits(a, b)
    assert not a["gains"][:, 40:].any() and (a["best"] < 40).all() and a["gains"].max() > 10 * mc.ONE
    # the gate and non-finite coordinates: gated rows behave like rows that are not there
    conf = np.random.default_rng(3).uniform(0, 1, ml.shape[0]).astype(np.float32)
    conf[5] = np.nan
    bad = ml.copy()
    bad[11, 0], bad[12, 1] = np.inf, np.nan
    ref = mc.reference(family, bad, mr, segs, models, thr, conf=conf, min_conf=0.5)
    g = check_msac(family, ops, bad, mr, models, thr, ref, segs, stats, pair_off=off, conf=conf, min_conf=0.5)
    holes = bad.copy()
    holes[~(conf >= 0.5)] = np.nan
    h = run(ops, family, holes, mr, models, thr, pair_off=off)
    same_bits(g, h)
    assert not g["inlier"][[5, 11, 12]].any() and not g["inlier"][~(conf >= 0.5)].any()


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_bad_thresholds_empty_pairs_and_cap_zero(ops, family):
    lengths = [300, 300, 300, 0, 300]
    ml, mr, off, models, thr = make_pairs(family, lengths, 66, 6100)
    thr = np.array([np.nan, -1e-3, 0.0, 2e-3, 2e-3], np.float32)
    segs = ec.segments(5, ml.shape[0], pair_off=off)
    ref = mc.reference(family, ml, mr, segs, models, thr)
    got = check_msac(family, ops, ml, mr, models, thr, ref, segs, [], pair_off=off)
    for p in (0, 1, 3):                                                           # NaN, negative, empty: nothing
        assert not got["gains"][p].any() and not got["counts"][p].any() and not got["moments"][p].any()
        assert got["best"][p] == 0 and got["best_gain"][p] == 0 and got["best_count"][p] == 0
        assert not got["inlier"][off[p]:off[p + 1]].any()
    assert got["gains"][4].max() > 10 * mc.ONE
    # cap == 0: every output defined
    z = np.zeros((0, 2), np.float32)
    got = run(ops, family, z, z, models[:2], thr[3:], pair_off=np.zeros(3, np.int64))
    for name in ("gains", "counts", "best", "best_gain", "best_count", "moments"):
        assert not got[name].any(), name


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_corrupt_offsets_stay_inside_the_arrays_and_every_byte_is_defined(ops, family):
    ml, mr, off, models, thr = make_pairs(family, [200, 150, 100], 9, 7300)
    cap = ml.shape[0]
    corrupt = np.array([-50, 180, 120, 10 ** 12], np.int64)                        # clamped: (0, 180), (180, 0), (120, cap - 120)
    segs = ec.segments(3, cap, pair_off=corrupt)
    assert segs == [(0, 180), (180, 0), (120, cap - 120)]
    got = run(ops, family, ml, mr, models, thr, pair_off=corrupt)
    for p in (0, 2):                                                              # each pair alone with its clamped segment
        lo, n = segs[p]
        one = run(ops, family, ml[lo:lo + n], mr[lo:lo + n], models[p:p + 1], thr[p:p + 1], pair_off=np.array([0, n], np.int64))
        for name in ("gains", "counts", "best", "best_gain", "best_count", "moments"):
            assert np.array_equal(got[name][p], one[name][0]), (p, name)
    assert not got["gains"][1].any()
    for name, v in got.items():                                                   # sentinel-filled outputs, fully overwritten
        if name == "inlier":
            assert set(np.unique(v)) <= {0, 1}
        elif v.dtype != np.float64:
            assert not (v == -123456).any(), name
        else:
            assert not (v == -777.25).any(), name


def test_refusals_with_a_real_allocation_behind_the_pointers_launch_nothing():
    from pats_amd import _lib
    lib = _lib.lib()
    live = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    base = live.data_ptr()
    for family in mc.FAMILIES:
        for kw, words in hm.refusals(lib, "score", base):
            assert mc.c_call(lib, family, base, **kw) != 0, kw
            msg = lib.pats_last_error()
            assert mc.ENTRY[family]["tag"] in msg and all(w in msg for w in words), (kw, msg)
        for name in ("gains", "best_gain"):
            for bad in (0, base + 4):
                assert mc.c_call(lib, family, base, **{name: bad}) != 0 and name.encode() in lib.pats_last_error()
    torch.cuda.synchronize()
    assert not live.any()                                                         # nothing ran: nothing was written


# ---- 5. through the batch path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_verify_with_msac_through_batch_feeds_the_later_stages_unchanged(ops, family, mixed):
    from pats_amd import batch
    cs = [mc.disagreement_case(family, seed, n) for seed, n in mc.DISAGREEMENTS[family]]      # the CALLER's order
    pairs = len(cs)
    caller_of = [2, 0, 3, 1][:pairs] if mixed else list(range(pairs))                       # slot s holds the caller's pair caller_of[s]
    lens = [cs[i]["ml"].shape[0] for i in caller_of]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ml, mr = np.concatenate([cs[i]["ml"] for i in caller_of]), np.concatenate([cs[i]["mr"] for i in caller_of])
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([off, [int(off[-1]), 0, 0]]).astype(np.int64)                  # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)

    def fresh():
        out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
        if mixed:
            out["caller_of"] = caller_of
        return out

    dmodels = cu(np.stack([c["models"] for c in cs]))
    dthr = cu(np.asarray([c["thr"] for c in cs], np.float32))
    verify, verify_msac = ((batch.verify_by_pair, batch.verify_msac_by_pair) if family == "epipolar" else
                           (batch.verify_h_by_pair, batch.verify_h_msac_by_pair))
    key = "verified" if family == "epipolar" else "verified_h"
    count, msac = fresh(), fresh()
    verify(count, cap, dmodels, dthr, moments=True)
    res = verify_msac(msac, cap, dmodels, dthr, moments=True)
    assert key + "_gain" not in count and key + "_score" not in count
    assert len(res) == 7 and len(msac[key]) == 5 and msac[key + "_score"] == "msac" and msac[key + "_on"] == "all"
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(msac[key], count[key]))
    gains, best_gain = msac[key + "_gain"]
    assert tuple(gains.shape) == (pairs, 4) and gains.dtype == torch.int64 and tuple(best_gain.shape) == (pairs,)
    assert torch.equal(msac[key][0], count[key][0])
    assert msac[key][1].tolist() == [1] * pairs and count[key][1].tolist() == [0] * pairs  # slot order; the same in every slot
    slot_of = [caller_of.index(i) for i in range(pairs)]
    direct = [run(ops, family, c["ml"], c["mr"], c["models"][None], [c["thr"]], pair_off=np.array([0, c["ml"].shape[0]], np.int64)) for c in cs]
    for i in range(pairs):                                                                   # the caller's pair i sits in slot slot_of[i]
        assert np.array_equal(gains[slot_of[i]].cpu().numpy(), direct[i]["gains"][0])
    if family == "epipolar":
        sv = batch.split_verified_by_pair(msac, cap)
        for i in range(pairs):
            assert tuple(sv[i][0].shape) == (cs[i]["ml"].shape[0], 2) and np.array_equal(sv[i][0].cpu().numpy(), cs[i]["ml"])
            assert np.array_equal(sv[i][2].cpu().numpy().astype(np.uint8), direct[i]["inlier"]) and int(sv[i][3]) == 1
        pose = batch.pose_by_pair(msac, cap)
        assert tuple(pose[0].shape) == (pairs, 3, 3) and bool(torch.isfinite(pose[1]).all())
        new = batch.polish_by_pair(msac, cap, dthr, rounds=2)
        assert msac[key] is new and len(new) == 5
        assert (new[2].cpu().numpy()[slot_of] >= np.array([d["best_count"][0] for d in direct])).all()
    else:
        Hm = batch.homography_by_pair(msac, cap)
        assert tuple(Hm[0].shape) == (pairs, 3, 3) and bool(torch.isfinite(Hm[0]).all())
        new = batch.polish_h_by_pair(msac, cap, dthr, rounds=2)
        assert msac[key] is new and len(new) == 5
    # a count verification on the same result leaves no stale gains behind
    verify(msac, cap, dmodels, dthr)
    assert key + "_gain" not in msac and key + "_score" not in msac and len(msac[key]) == 4
