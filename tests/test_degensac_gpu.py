"""GPU: the plane-and-parallax (DEGENSAC) stage - ops.plane_parallax_hypotheses_by_pair, ops.plane_parallax_select_by_pair and
batch.degensac_by_pair - against the definitions of include/pats_amd.h restated in numpy (tests/degensac_cases.py):
    pool, sample_idx  equal the restatement exactly, as integers, -1 rows included (the scenes keep every match a relative 1e-3 away
                      from the pool boundary: tests/test_degensac_cases_host.py)
    models            zero exactly where the restatement's are; each non-zero one with | |F| - 1 | <= 1e-6, the sign rule, within
                      4 eps32 per entry of the float64 restatement from the same sample_idx where |e| >= 1e-3 |l_1| |l_2| (float64
                      arithmetic, one rounding to float32 of entries below 1, the normalisation), and |x'^T F x| < 1e-5 on the two
                      sampled matches and on every match of the plane
    end to end        scene A: the 7-point chain's winner explains the plane and little else (count_before < 0.9 of the true
                      inliers); after degensac_by_pair the pair is replaced, its support holds every true inlier, and
                      fundamental_by_pair's F puts every true inlier within thr.  Scene B: nothing is replaced and nothing changes
    edges             pools of 0, 1 and 2, n < 2, no matches, no plane, non-finite coordinates, a pool longer than pool_max, H around
                      the workgroup, both segment forms, a mixed pack, samples=False, determinism, ties
Every output lies inside a larger sentinel-filled buffer: the call must define every byte of the views and none around them."""
import numpy as np
import pytest
import torch

import degensac_cases as dc
import epipolar_cases as ec
import fundamental_cases as fc

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I, SENT_B = -777.25, -123456, 0x5A
EPS32 = dc.EPS32


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def run(ops, ml, mr, H, seeds, models_h, best_h, thr, samples=True, **kw):
    """One call on fresh sentinel buffers -> (models [pairs,H,9], pool [pairs], sample_idx [pairs,H,2] or None) as numpy arrays."""
    pairs = len(seeds)
    (vm, vp, vi), chk, bufs = views_of([((pairs, H, 3, 3), torch.float32, SENT_F), ((pairs,), torch.int32, SENT_I),
                                        ((pairs, H, 2), torch.int32, SENT_I)])
    got = ops.plane_parallax_hypotheses_by_pair(cu(ml), cu(mr), H, cu(np.asarray(seeds, np.int64)), cu(np.asarray(models_h, np.float32)),
                                                cu(np.asarray(best_h, np.int32)), cu(np.asarray(thr, np.float32)), return_samples=samples,
                                                out=(vm, vp, vi) if samples else (vm, vp), **dev_kw(kw))
    torch.cuda.synchronize()
    assert len(got) == (3 if samples else 2) and got[0].data_ptr() == vm.data_ptr() and got[1].data_ptr() == vp.data_ptr()
    assert samples or bool((bufs[2][0] == SENT_I).all())
    chk()
    models = vm.cpu().numpy().reshape(pairs, H, 9)
    assert np.isfinite(models).all() and not (models == np.float32(SENT_F)).any()      # never a NaN, every byte defined
    return models, vp.cpu().numpy(), vi.cpu().numpy() if samples else None


def check(got, ref, labels=None):
    """The three outputs against the restatement -> the number of models compared entry by entry."""
    models, pool, idx = got
    compared = 0
    for p, r in enumerate(ref):
        assert pool[p] == r["pool"], "pair %d: pool %d, the restatement %d" % (p, pool[p], r["pool"])
        assert np.array_equal(idx[p], r["idx"]), "pair %d: sample_idx differs from the restatement" % p
        live = models[p].any(1)
        assert np.array_equal(live, r["F"].any(1)), "pair %d: a zero model where the restatement has one, or the reverse" % p
        if not live.any():
            continue
        F = models[p][live].astype(np.float64)
        assert np.abs(np.linalg.norm(F, axis=1) - 1).max() <= 1e-6
        assert np.array_equal(fc.sign_rule(models[p][live]), models[p][live])
        well = r["cond"][live] >= 1e-3
        diff = np.abs(F - r["F"][live])[well]
        assert diff.size == 0 or diff.max() <= 4 * EPS32, "pair %d: %g eps32 from the float64 restatement" % (p, diff.max() / EPS32)
        compared += int(well.sum())
        alg = dc.algebraic(F, r["xl"], r["xr"])
        at = r["idx"][live]
        assert np.abs(alg[np.arange(len(at))[:, None], at]).max() < 1e-5
        if labels is not None and labels[p] is not None:
            assert np.abs(alg[:, labels[p] == dc.LABEL_PLANE]).max() < 1e-5
    return compared


def all_scenes():
    """The six scenes as one batch with the plane in slot 1 of 2 (slot 0 is another matrix) -> (sc, ml, mr, off, segs, norm, models_h)."""
    sc = dc.scenes("A") + dc.scenes("B")
    ml, mr, off, segs, norm = dc.packed(sc)
    models_h = np.stack([np.stack([np.eye(3) * 0.5 + 0.01, s["H"]]) for s in sc]).astype(np.float32)
    return sc, ml, mr, off, segs, norm, models_h


@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_pool_sampler_and_solver_equal_the_restatement_around_the_workgroup(ops, H):
    sc, ml, mr, off, segs, norm, models_h = all_scenes()
    pairs = len(sc)
    seeds = [900 + H + 7 * p for p in range(pairs)]
    best_h = [1, 1, 9, 1, 1, 1]                                            # 9 is clamped to Mh - 1 = 1
    thr = np.full(pairs, dc.THR, np.float32)
    got = run(ops, ml, mr, H, seeds, models_h, best_h, thr, pair_off=off, norm=norm)
    ref = dc.reference(ml, mr, segs, seeds, H, models_h, best_h, thr, norm=norm)
    labels = [s["label"] if s["kind"] == "A" else None for s in sc]
    compared = check(got, ref, labels)
    assert compared >= 0.75 * pairs * H - 1 and all(r["pool"] >= 40 for r in ref)
    # sample_idx is optional: the same bits without it; and two calls give the same bits
    lone = run(ops, ml, mr, H, seeds, models_h, best_h, thr, samples=False, pair_off=off, norm=norm)
    again = run(ops, ml, mr, H, seeds, models_h, best_h, thr, pair_off=off, norm=norm)
    for other in (lone, again):
        assert other[0].tobytes() == got[0].tobytes() and np.array_equal(other[1], got[1])
    assert np.array_equal(again[2], got[2])
    # the strided form of the same rows: the same bits
    stride = max(n for _, n in segs)
    sl, sr = (np.full((pairs * stride + 5, 2), np.nan, np.float32) for _ in range(2))
    for p, (lo, n) in enumerate(segs):
        sl[p * stride:p * stride + n], sr[p * stride:p * stride + n] = ml[lo:lo + n], mr[lo:lo + n]
    counts = np.array([n for _, n in segs], np.int64)
    strided = run(ops, sl, sr, H, seeds, models_h, best_h, thr, stride=stride, counts=counts, norm=norm)
    assert strided[0].tobytes() == got[0].tobytes() and np.array_equal(strided[1], got[1]) and np.array_equal(strided[2], got[2])
    # a larger parallax asks for more: no pool grows, scene B's (errors of every size against its slot-1 matrix) shrink
    wide = run(ops, ml, mr, H, seeds, models_h, best_h, thr, pair_off=off, norm=norm, parallax=40.0)
    assert (wide[1] <= got[1]).all() and (wide[1][3:] < got[1][3:]).all()


def edge_batch():
    """Pairs cut from scene A's third pair: pools of 0, 1 and 2, n = 1, n = 0, no plane, non-finite coordinates."""
    s = dc.scenes("A")[2]
    plane, off = np.flatnonzero(s["label"] == dc.LABEL_PLANE), np.flatnonzero(s["label"] == dc.LABEL_OFF)
    full = np.arange(len(s["ml"]))
    rows = [plane, np.sort(np.concatenate([plane, off[:1]])), np.sort(np.concatenate([plane, off[:2]])), off[:1], full[:0], full, full]
    ml, mr = np.concatenate([s["ml"][r] for r in rows]), np.concatenate([s["mr"][r] for r in rows])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    lo = int(offs[6])
    ml[lo + off[3], 1] = np.nan                                            # inside the pool: it leaves it
    mr[lo + off[5], 0] = np.inf
    mr[lo + plane[4], 1] = np.nan                                          # outside the pool: nothing changes for it
    pairs = len(rows)
    models_h = np.repeat(s["H"].astype(np.float32)[None, None], pairs, 0)
    models_h[5] = 0.0                                                      # no plane
    norm = np.repeat(s["norm"][None], pairs, 0)
    return s, rows, ml, mr, offs, [(int(offs[p]), len(rows[p])) for p in range(pairs)], norm, models_h


def test_small_pools_short_pairs_no_plane_and_non_finite_coordinates(ops):
    s, rows, ml, mr, off, segs, norm, models_h = edge_batch()
    pairs, H = len(rows), 70
    seeds, best_h, thr = list(range(31, 31 + pairs)), [0] * pairs, np.full(pairs, dc.THR, np.float32)
    got = run(ops, ml, mr, H, seeds, models_h, best_h, thr, pair_off=off, norm=norm)
    ref = dc.reference(ml, mr, segs, seeds, H, models_h, best_h, thr, norm=norm)
    check(got, ref)
    models, pool, idx = got
    n_off = int((s["label"] != dc.LABEL_PLANE).sum())
    assert pool.tolist() == [0, 1, 2, 1, 0, len(s["ml"]), n_off - 2]      # against the zero matrix a2^2 == 0: every finite match
    for p in (0, 1, 3, 4, 5):                                              # pools of 0 and 1, n = 1, n = 0, no plane
        assert not models[p].any() and (idx[p] == -1).all(), p
    a, b = (int(v) for v in ref[2]["members"])
    assert models[2].any(1).all() and set(map(tuple, idx[2].tolist())) == {(a, b), (b, a)}      # a pool of two: both orders, one model
    assert models[6].any(1).sum() >= H - 2
    # a NaN threshold compares false: nothing is off the plane; an infinite coordinate of the plane leaves nothing finite to store
    nan_thr = thr.copy()
    nan_thr[6] = np.nan
    bad_h = models_h.copy()
    bad_h[2, 0, 1, 1] = np.inf
    got = run(ops, ml, mr, H, seeds, bad_h, best_h, nan_thr, pair_off=off, norm=norm)
    assert got[1][6] == 0 and not got[0][6].any() and not got[0][2].any()
    # empty lists: every output is defined
    z2 = np.zeros((0, 2), np.float32)
    m0, p0, i0 = run(ops, z2, z2, 5, [1, 2], models_h[:2], [0, 0], thr[:2], pair_off=np.zeros(3, np.int64))
    assert not m0.any() and not p0.any() and (i0 == -1).all()


def test_a_pool_longer_than_the_list_keeps_its_first_members(ops):
    pool_max = ops.plane_parallax_pool_max()
    assert pool_max == 8192
    n, lead, H = pool_max + 300, 50, 257
    rng = np.random.default_rng(5)
    xl = rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
    xr = xl + np.float32(0.125)                                            # far off the identity's plane ...
    xr[:lead] = xl[:lead]                                                  # ... but for the first rows, which lie on it
    stride = n + 7
    ml, mr = np.zeros((2 * stride, 2), np.float32), np.zeros((2 * stride, 2), np.float32)
    ml[:n], mr[:n] = xl, xr
    ml[stride:stride + 40], mr[stride:stride + 40] = xl[30:70], xr[30:70]
    counts = np.array([n, 40], np.int64)
    models_h = np.repeat(np.eye(3, dtype=np.float32)[None, None], 2, 0)
    thr = np.full(2, dc.THR, np.float32)
    got = run(ops, ml, mr, H, [77, 78], models_h, [0, 0], thr, stride=stride, counts=counts)
    ref = dc.reference(ml, mr, [(0, n), (stride, 40)], [77, 78], H, models_h, [0, 0], thr, pool_max=pool_max)
    check(got, ref)
    assert got[1].tolist() == [n - lead, 20]                               # the size before clamping
    assert got[2][0].min() >= lead and lead + pool_max - 500 < got[2][0].max() < lead + pool_max


# ---- the hand-over ----------------------------------------------------------------------------------------------------------------
SELECT_NAMES = ("model", "best_count", "inlier", "moments", "replaced", "overlap")


def run_select(ops, ml, mr, thr, models_h, best_h, standing, candidate, moments=True, **kw):
    pairs, cap = len(thr), ml.shape[0]
    shapes = [((pairs, 3, 3), torch.float32, SENT_F), ((pairs,), torch.int64, SENT_I), ((cap,), torch.uint8, SENT_B),
              ((pairs, 9, 9), torch.float64, SENT_F), ((pairs,), torch.uint8, SENT_B), ((pairs,), torch.int32, SENT_I)]
    if not moments:
        del shapes[3]
    views, chk, _ = views_of(shapes)
    side = lambda t: tuple(cu(a) for a in (t if moments else t[:4]))       # noqa: E731
    got = ops.plane_parallax_select_by_pair(cu(ml), cu(mr), cu(thr), cu(models_h), cu(np.asarray(best_h, np.int32)), side(standing),
                                            side(candidate), out=tuple(views), **dev_kw(kw))
    torch.cuda.synchronize()
    assert len(got) == len(views) and all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
    chk()
    names = [n for n in SELECT_NAMES if moments or n != "moments"]
    return {n: v.cpu().numpy() for n, v in zip(names, views)}


def test_the_hand_over_keeps_the_standing_verification_on_a_tie_and_counts_the_overlap(ops):
    s, rows, ml, mr, off, segs, norm, models_h = edge_batch()
    pairs, cap = len(rows), ml.shape[0] + 9                                # rows inside cap behind the last segment
    ml, mr = np.concatenate([ml, ml[:9]]), np.concatenate([mr, mr[:9]])
    rng = np.random.default_rng(8)
    thr = np.full(pairs, dc.THR, np.float32)
    thr[1] = np.nan                                                        # no plane inliers: overlap 0
    sides = []
    for Hx in (3, 5):
        models = rng.normal(size=(pairs, Hx, 3, 3)).astype(np.float32)
        sides.append([models, rng.integers(-1, Hx + 2, pairs).astype(np.int32), None, (rng.random(cap) < 0.6).astype(np.uint8),
                      rng.normal(size=(pairs, 9, 9))])
    sides[0][2] = np.array([5, 5, 0, 1, 0, 40, 7], np.int64)
    sides[1][2] = np.array([5, 6, 0, 0, 0, 90, 8], np.int64)               # a tie, +1, both zero, -1, an empty pair, more, +1
    sides[0][3][int(off[6]):int(off[7])] *= 3                              # any non-zero byte is an inlier; the output is 0 / 1
    want_replaced = np.array([0, 1, 0, 0, 0, 1, 1], np.uint8)
    for moments in (True, False):
        got = run_select(ops, ml, mr, thr, models_h, [0] * pairs, sides[0], sides[1], moments=moments, pair_off=off, norm=norm)
        assert np.array_equal(got["replaced"], want_replaced)
        for p, (lo, n) in enumerate(segs):
            kept = sides[int(want_replaced[p])]
            Hx = kept[0].shape[1]
            assert got["best_count"][p] == kept[2][p]
            assert got["model"][p].tobytes() == kept[0][p, min(max(int(kept[1][p]), 0), Hx - 1)].tobytes()
            assert np.array_equal(got["inlier"][lo:lo + n], (kept[3][lo:lo + n] != 0).astype(np.uint8))
            if moments:
                assert got["moments"][p].tobytes() == kept[4][p].tobytes()
            # the overlap: the standing inliers the plane explains at thr - exact, the scene's margins are wide
            xl, xr = ec.points32(ml[lo:lo + n], mr[lo:lo + n], norm[p])
            on = ec.participates(xl, xr) & ~dc.pool_test32(xl, xr, models_h[p, 0], thr[p], 1.0) if n else np.zeros(0, bool)
            want = int((on & (sides[0][3][lo:lo + n] != 0)).sum()) if thr[p] >= 0 and models_h[p].any() else 0
            assert got["overlap"][p] == want, (p, got["overlap"][p], want)
        assert not got["inlier"][segs[-1][0] + segs[-1][1]:].any()         # the rows behind the last segment
        assert got["overlap"][0] > 50 and got["overlap"][1] == 0 and got["overlap"][5] == 0
    once, again = (run_select(ops, ml, mr, thr, models_h, [0] * pairs, sides[0], sides[1], pair_off=off, norm=norm) for _ in range(2))
    assert all(once[n].tobytes() == again[n].tobytes() for n in SELECT_NAMES)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def handed_over(sc, caller_of=None):
    """A result dict as the batch path leaves it after group_by_pair, from the scenes in SLOT order."""
    from pats_amd import batch
    order = list(range(len(sc))) if caller_of is None else caller_of
    ml, mr = np.concatenate([sc[i]["ml"] for i in order]), np.concatenate([sc[i]["mr"] for i in order])
    lengths = [len(sc[i]["ml"]) for i in order]
    pairs = len(sc)
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([[0], np.cumsum(lengths), [sum(lengths), 0, 0]]).astype(np.int64)          # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds}
    if caller_of is not None:
        out["caller_of"] = caller_of
    return batch, cap, out


def front(batch, cap, out, sc, plane=True, H7=dc.H7):
    """The worked loop up to the stage: hypothesize7 -> verify -> hypothesize_h -> verify_h -> polish_h -> (norm, thr)."""
    pairs = len(sc)
    dn, dthr = cu(np.stack([s["norm"] for s in sc])), cu(np.full(pairs, dc.THR, np.float32))
    h7 = batch.hypothesize7_by_pair(out, cap, H7, seed=dc.SEED7, norm=dn, on="all").reshape(pairs, -1, 3, 3)
    batch.verify_by_pair(out, cap, h7, dthr, norm=dn, on="all", moments=True)
    if plane:
        hh = batch.hypothesize_h_by_pair(out, cap, 64, seed=dc.SEED7, norm=dn, on="all")
        batch.verify_h_by_pair(out, cap, hh, dthr, norm=dn, on="all", moments=True)
        batch.polish_h_by_pair(out, cap, dthr, norm=dn)
    return dn, dthr


def state(out):
    ver = out["verified"]
    win = out["verified_models"][torch.arange(ver[1].numel(), device="cuda"), ver[1].long().clamp(0, out["verified_models"].shape[1] - 1)]
    return {"best_count": ver[2].cpu().numpy().copy(), "inlier": ver[3].cpu().numpy().copy(), "moments": ver[4].cpu().numpy().copy(),
            "model": win.cpu().numpy().copy()}


def test_scene_a_end_to_end_the_degenerate_winner_is_replaced_by_the_scenes_geometry():
    """The test that fails without the stage: the 7-point winner explains the plane; the result must explain the scene."""
    sc = dc.scenes("A")
    batch, cap, out = handed_over(sc)
    with pytest.raises(ValueError, match="verify_by_pair"):
        batch.degensac_by_pair(out, cap, dc.H_PP, None)
    dn, dthr = front(batch, cap, out, sc, plane=False)
    with pytest.raises(ValueError, match="verify_h_by_pair"):
        batch.degensac_by_pair(out, cap, dc.H_PP, dthr, norm=dn, on="all")
    batch, cap, out = handed_over(sc)
    dn, dthr = front(batch, cap, out, sc)
    with pytest.raises(ValueError, match="not aligned"):
        batch.degensac_by_pair(dict(out, topk=None), cap, dc.H_PP, dthr, norm=dn, on="topk")
    keys = set(out)
    untouched = {k: out[k] for k in ("verified_h", "verified_h_models", "polished_h", "hypotheses7", "hypotheses_h", "by_pair", "summary")}
    res = batch.degensac_by_pair(out, cap, dc.H_PP, dthr, seed=dc.SEED_PP, norm=dn, on="all", samples=True)
    assert out["degensac"] is res and len(res) == 6 and set(out) == keys | {"degensac"}
    assert all(out[k] is v for k, v in untouched.items()) and out["verified_on"] == "all"
    replaced, overlap, pool, before, count_pp, idx = (t.cpu().numpy() for t in res)
    ver = out["verified"]
    assert len(ver) == 5 and tuple(ver[0].shape) == (3, 1) and not ver[1].any() and torch.equal(ver[0][:, 0].long(), ver[2])
    assert tuple(out["verified_models"].shape) == (3, 1, 3, 3) and tuple(idx.shape) == (3, dc.H_PP, 2)
    best_count, inl = ver[2].cpu().numpy(), ver[3].cpu().numpy().astype(bool)
    batch.polish_f_by_pair(out, cap, dthr, norm=dn)
    F = batch.fundamental_by_pair(out, cap, norm=dn)[0].cpu().numpy()
    lo = 0
    for p, s in enumerate(sc):
        n, true = len(s["ml"]), int(s["true"].sum())
        worst = dc.sampson64(F[p].reshape(1, 9), s["xl"], s["xr"])[0][s["true"]].max()
        print("pair %d: true %d, count_before %d, count_pp %d, kept %d, pool %d, overlap %d, worst true Sampson %.3g thr"
              % (p, true, before[p], count_pp[p], best_count[p], pool[p], overlap[p], worst / float(dc.THR)))
        assert before[p] < 0.9 * true                                      # what the generator promised of the 7-point chain
        assert replaced[p] == 1 and best_count[p] == count_pp[p] >= true
        assert (inl[lo:lo + n] | ~s["true"]).all() and int(inl[lo:lo + n].sum()) == best_count[p]
        assert worst <= float(dc.THR)
        assert overlap[p] / before[p] >= 0.8
        assert pool[p] == int((s["label"] != dc.LABEL_PLANE).sum())        # the polished plane is the scene's
        lo += n


def test_scene_b_nothing_is_replaced_and_the_verification_keeps_its_bits():
    """`verified` changes its FORM (one model per pair, best = 0, as polish_f_by_pair leaves it); its content - best_count, the mask,
    the moments and the winning model - keeps every bit."""
    sc = dc.scenes("B")
    batch, cap, out = handed_over(sc)
    dn, dthr = front(batch, cap, out, sc, H7=dc.H7_B)                       # the budget at which the 7-point chain finds the scene
    was = state(out)
    assert np.array_equal(was["best_count"], [int(s["true"].sum()) for s in sc])
    res = batch.degensac_by_pair(out, cap, dc.H_PP, dthr, seed=dc.SEED_PP, norm=dn, on="all")
    assert len(res) == 5
    replaced, overlap, pool, before, count_pp = (t.cpu().numpy() for t in res)
    print("scene B: count_before %s, count_pp %s, pool %s, overlap %s" % (before.tolist(), count_pp.tolist(), pool.tolist(), overlap.tolist()))
    assert not replaced.any() and (count_pp <= before).all() and np.array_equal(before, was["best_count"])
    now = state(out)
    assert all(now[k].tobytes() == was[k].tobytes() for k in was)
    assert tuple(out["verified"][0].shape) == (3, 1) and tuple(out["verified_models"].shape) == (3, 1, 3, 3)


def test_a_mixed_pack_in_a_permuted_order_and_a_second_call_give_the_same_bits():
    sc = dc.scenes("A")
    results = []
    for caller_of in (None, [2, 0, 1], None):                              # slot s holds the caller's pair caller_of[s]
        batch, cap, out = handed_over(sc, caller_of)
        dn, dthr = front(batch, cap, out, sc)
        res = batch.degensac_by_pair(out, cap, dc.H_PP, dthr, seed=dc.SEED_PP, norm=dn, on="all", samples=True)
        F = batch.fundamental_by_pair(out, cap, norm=dn)[0]
        results.append([t.cpu().numpy() for t in res + (F,)])
    for other in results[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0], other))
    assert results[0][0].all()


def test_without_a_plane_the_stage_keeps_the_standing_verification():
    sc = dc.scenes("A")
    batch, cap, out = handed_over(sc)
    dn, dthr = front(batch, cap, out, sc, plane=False)
    batch.verify_h_by_pair(out, cap, torch.zeros((3, 2, 3, 3), device="cuda"), dthr, norm=dn, on="all")
    assert int(out["verified_h"][2].max()) < 4                             # the zero model has no inliers: no plane
    was = state(out)
    replaced, overlap, pool, before, count_pp = (t.cpu().numpy() for t in batch.degensac_by_pair(out, cap, 16, dthr, norm=dn, on="all"))
    assert not replaced.any() and not overlap.any() and not count_pp.any()
    assert all(state(out)[k].tobytes() == was[k].tobytes() for k in was)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_the_ops_refuse_what_their_siblings_refuse(ops):
    ml = torch.zeros((20, 2), device="cuda")
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.tensor([0, 10, 20], device="cuda")
    mh, bh, thr = torch.zeros((2, 1, 3, 3), device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    ok = ops.plane_parallax_hypotheses_by_pair(ml, ml, 4, seed, mh, bh, thr, pair_off=off)
    assert len(ok) == 2 and not ok[0].any() and ok[1].tolist() == [10, 10]       # no plane: no model; a2^2 == 0: every match
    for kw, word in (({"H": 0}, "H = 0"), ({"H": ops.epipolar_max_h() + 1}, "H ="), ({"norm": torch.zeros((3, 8), device="cuda")}, "norm"),
                     ({"parallax": 0.5}, "parallax"), ({"parallax": float("nan")}, "parallax"), ({"models_h": mh[:1]}, "models_h"),
                     ({"models_h": mh.double()}, "models_h"), ({"best_h": bh.long()}, "best_h"), ({"thr": thr[:1]}, "thr"),
                     ({"models_h": mh.cpu()}, "models_h"), ({"matches_l": ml.t().contiguous().t()}, "contiguous"),
                     ({"out": (ok[0],)}, "out must be"), ({"stride": 4}, "either pair_off")):
        args = dict(matches_l=ml, H=4, models_h=mh, best_h=bh, thr=thr, pair_off=off)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            ops.plane_parallax_hypotheses_by_pair(args.pop("matches_l"), ml, args.pop("H"), seed, args.pop("models_h"), args.pop("best_h"),
                                                  args.pop("thr"), **args)
    side = (torch.zeros((2, 1, 3, 3), device="cuda"), bh, torch.zeros(2, dtype=torch.int64, device="cuda"),
            torch.zeros(20, dtype=torch.uint8, device="cuda"))
    assert len(ops.plane_parallax_select_by_pair(ml, ml, thr, mh, bh, side, side, pair_off=off)) == 5
    for bad, word in ((side[:3], "standing must be"), ((side[0], bh, side[2], side[3][:5]), "inlier"),
                      ((side[0].cpu(),) + side[1:], "models"), ((side[0], bh, side[2].int(), side[3]), "best_count")):
        with pytest.raises(RuntimeError, match=word):
            ops.plane_parallax_select_by_pair(ml, ml, thr, mh, bh, bad, side, pair_off=off)
