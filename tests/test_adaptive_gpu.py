"""GPU: the per-pair adaptive verification - ops.{epipolar,homography}_score_adaptive_by_pair and
batch.verify_{,h_}adaptive_by_pair - against its definition (include/pats_amd.h, "Per-pair adaptive verification").  Every
comparison is exact:
    counts         equal to the fixed-budget op's below used[p], exactly 0 from used[p] on
    used           the plain-Python rule (tests/adaptive_cases.py) applied to the fixed-budget counts - and, on planted inputs whose
                   stop round is known in advance, the literal value
    participating  the numpy count of the verification's finite / min_conf rule, 0 for a bad thr
    best, best_count, inlier, moments
                   byte for byte the fixed-budget op run with models[p, used[p]:] zeroed; the mask's population is best_count
Inputs are planted (adaptive_cases.plant_pair): a chosen share of a pair's matches satisfies a model that sits at a chosen index of
the caller's models, the rest is random."""
import numpy as np
import pytest
import torch

import adaptive_cases as ac
import epipolar_cases as ec

pytestmark = pytest.mark.gpu

THR = np.float32(2e-3)
CONF = ac.CONFIDENCE
SAMPLE = {"epi": 8, "hom": 4}
NORM = np.array([0.02, -0.01, 1.25, 1.2, -0.03, 0.015, 1.1, 1.3], np.float32)


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fns(ops, kind):
    name = "epipolar" if kind == "epi" else "homography"
    return getattr(ops, name + "_score_by_pair"), getattr(ops, name + "_score_adaptive_by_pair")


def norm_for(pairs):
    shift = np.linspace(0, 0.01, pairs, dtype=np.float32)[:, None] * np.array([1, -1, 0, 0, -1, 1, 0, 0], np.float32)
    return np.ascontiguousarray(np.repeat(NORM[None], pairs, 0) + shift)


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def check(ops, kind, ml, mr, segs, seg_kw, models, thr, s, g, B, norm=None, conf=None, min_conf=None, moments=True, fixed=None):
    """One adaptive call against the fixed budget; segs = [(lo, n)] per pair on the host.  -> (used, participating, adaptive, fixed)."""
    fixed_op, adaptive_op = fns(ops, kind)
    dl, dr, dm, dt = cu(ml), cu(mr), cu(models), cu(thr)
    kw = dict(seg_kw, norm=None if norm is None else cu(norm), moments=moments)
    if min_conf is not None:
        kw.update(conf=cu(conf), min_conf=min_conf)
    if fixed is None:
        fixed = fixed_op(dl, dr, dm, dt, **kw)
    got = adaptive_op(dl, dr, dm, dt, CONF, s, models_per_sample=g, round_models=B, **kw)
    assert len(got) == len(fixed) + 2 and got[-2].dtype == torch.int32 and got[-1].dtype == torch.int32
    pairs, H = models.shape[:2]
    used, part = got[-2].cpu().numpy(), got[-1].cpu().numpy()
    cf, ca = fixed[0].cpu().numpy(), got[0].cpu().numpy()
    flat_l, flat_r = np.asarray(ml).reshape(-1, 2), np.asarray(mr).reshape(-1, 2)
    for p, (lo, n) in enumerate(segs):
        xl, xr = ec.points32(flat_l[lo:lo + n], flat_r[lo:lo + n], None if norm is None else norm[p])
        want = int(ec.participates(xl, xr, None if conf is None else conf[lo:lo + n], min_conf).sum()) if thr[p] >= 0 else 0
        assert part[p] == want, (p, part[p], want)
        assert used[p] == ac.used_from_counts(cf[p], want, H, B, g, s, CONF), (p, used[p])
        assert np.array_equal(ca[p, :used[p]], cf[p, :used[p]]) and not ca[p, used[p]:].any(), p
    zeroed = dm.clone()
    for p in range(pairs):
        zeroed[p, int(used[p]):] = 0
    ref = fixed_op(dl, dr, zeroed, dt, **kw)
    assert same(got[0], ref[0])
    for name, a, b in zip(("best", "best_count", "inlier", "moments"), got[1:-2], ref[1:]):
        assert same(a, b), name
    inl, bc = got[3].cpu().numpy(), got[2].cpu().numpy()
    for p, (lo, n) in enumerate(segs):
        assert int(inl[lo:lo + n].sum()) == bc[p], p
    assert int(inl.sum()) == int(bc.sum())
    return used, part, got, fixed


def ragged(off):
    return [(int(a), int(b - a)) for a, b in zip(off[:-1], off[1:])], {"pair_off": cu(off)}


# ---- 1. planted stop rounds, the match tile's edges, every kind of pair in one batch ------------------------------------------
@pytest.mark.parametrize("kind", ["epi", "hom"])
def test_planted_pairs_stop_in_the_round_known_in_advance(ops, kind):
    """s = 4, B = 64, H = 448 (seven rounds).  By hand, from k >= ln(1e-5) / ln(1 - w^4):
    w = 0.9 -> 11 samples: round 0;  w = 0.5 -> 179: T_2 = 192;  w = 0.45 -> 275: T_4 = 320, so the better model at index 330 (w =
    0.55) is never tested;  w = 1 -> round 0.  The margins (129 .. 192, 257 .. 320) hold a few accidental inliers."""
    H, B, s = 448, 64, 4
    pairs = [(2049, [(0.9, 5)]), (2048, [(0.5, 70)]), (2047, []), (600, [(0.9, 3)]), (2049, [(0.45, 10), (0.55, 330)]), (0, []),
             (7, [(1.0, 0)]), (8, [(0.5, 3)])]
    ml, mr, off, models = ac.plant_batch(4100, kind, H, pairs)
    thr = np.full(len(pairs), THR, np.float32)
    thr[3] = np.nan
    segs, seg_kw = ragged(off)
    used, part, got, fixed = check(ops, kind, ml, mr, segs, seg_kw, models, thr, s, 1, B)
    print(kind, "used", used.tolist(), "participating", part.tolist(), "best", got[1].tolist(), "best_count", got[2].tolist())
    assert used[:7].tolist() == [64, 192, H, H, 320, H, 64]
    assert part.tolist() == [2049, 2048, 2047, 0, 2049, 0, 7, 8]
    best, counts, cf = got[1].cpu().numpy(), got[0].cpu().numpy(), fixed[0].cpu().numpy()
    assert best[:2].tolist() == [5, 70] and best[4] == 10 and best[6] == 0
    assert counts[4, 330] == 0 and cf[4, 330] > cf[4, 10] > 0              # the better model sits one round late: not found
    assert fixed[1][4] == 330 and not counts[3].any() and not counts[5].any()


# ---- 2. model counts around the chunk and the round ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 65, 256, 257, 320, 1024])
@pytest.mark.parametrize("kind", ["epi", "hom"])
def test_model_counts_and_round_sizes_with_a_ragged_last_round(ops, kind, H):
    s = SAMPLE[kind]
    pairs = [(300, [(0.9, H - 1)]), (2049, [(0.6, min(H - 1, 64))]), (100, []), (700, [(0.95, 0)])]
    ml, mr, off, models = ac.plant_batch(5200 + H, kind, H, pairs)
    thr = np.full(len(pairs), THR, np.float32)
    segs, seg_kw = ragged(off)
    fixed, seen = None, set()
    for B in (64, 128, 256, 320):                       # B > H, B == H and a ragged last round are all among these
        used, _, _, fixed = check(ops, kind, ml, mr, segs, seg_kw, models, thr, s, 1, B, fixed=fixed)
        assert all(u == H or u % B == 0 for u in used.tolist())
        assert used[0] == H and used[2] == H and used[3] == min(H, B)     # the last model; nothing; w = 0.95 in round 0
        seen.update(used.tolist())
    assert len(seen) > 1 or H <= 64


# ---- 3. the forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("kind", ["epi", "hom"])
def test_segment_forms_norm_confidence_gate_and_moments(ops, kind, with_norm, strided):
    """with_norm also gates a third of the matches by min_conf; the strided form runs without moments."""
    H, B, s = 257, 64, SAMPLE[kind]
    lengths = [2049, 0, 500, 64]
    pairs = [(n, [(0.85, 200)] if p == 0 else [(0.8, 66)] if p == 2 else []) for p, n in enumerate(lengths)]
    norm = norm_for(len(pairs)) if with_norm else None
    ml, mr, off, models = ac.plant_batch(6300, kind, H, pairs, norm)
    thr = np.full(len(pairs), THR, np.float32)
    rng = np.random.default_rng(9)
    conf, min_conf = None, None
    if with_norm:
        conf, min_conf = rng.uniform(0, 1, ml.shape[0]).astype(np.float32), 1.0 / 3.0
        conf[5] = np.nan
    if strided:                                         # the top-K layout: rows of `stride`, a count past it is clamped
        stride = 2100
        sl, sr = np.full((len(pairs), stride, 2), 7.5, np.float32), np.full((len(pairs), stride, 2), -3.25, np.float32)
        sc = np.zeros((len(pairs), stride), np.float32)
        for p, n in enumerate(lengths):
            sl[p, :n], sr[p, :n] = ml[off[p]:off[p + 1]], mr[off[p]:off[p + 1]]
            if conf is not None:
                sc[p, :n] = conf[off[p]:off[p + 1]]
        counts = np.array(lengths, np.int64)
        counts[3] = stride + 50                         # clamped to the stride: the row's slack takes part (finite values)
        segs = [(p * stride, min(int(c), stride)) for p, c in enumerate(counts)]
        ml, mr, conf = sl, sr, None if conf is None else sc.reshape(-1)
        seg_kw = {"stride": stride, "counts": cu(counts)}
    else:
        segs, seg_kw = ragged(off)
    used, part, _, _ = check(ops, kind, ml, mr, segs, seg_kw, models, thr, s, 1, B, norm=norm, conf=conf, min_conf=min_conf,
                             moments=not strided)
    print(kind, with_norm, strided, "used", used.tolist(), "participating", part.tolist())
    if with_norm:
        assert 0.6 * 2049 < part[0] < 0.72 * 2049                          # a third is gated: participating < n
    else:
        assert part[0] == 2049 and part[2] == 500
    assert used[0] == 256 and used[1] == H and used[2] == 128             # indices 200 and 66: rounds 3 and 1; at most 63 samples needed


def test_ten_models_per_sample_on_a_padded_tensor(ops):
    """[pairs, 10 H', 3, 3] as the 5-point solver leaves it: a sample's solutions first, zero models behind.  s = 5, g = 10, B = 320:
    w = 0.8 needs 29 samples -> T_0 = 320 (k = 32);  w = 0.7 needs 63 -> T_1 = 640 (k = 64) = H;  a model in round 1 -> 640."""
    samples, H = 64, 640
    pairs = [(900, [(0.8, 50)]), (900, [(0.7, 10)]), (900, [(0.8, 330)])]
    ml, mr, off, models = ac.plant_batch(7400, "epi", H, pairs)
    keep = np.random.default_rng(3).integers(1, 5, samples)                # 1 .. 4 solutions per sample
    for j in range(samples):
        models[:, 10 * j + keep[j]:10 * (j + 1)] = 0
    assert models[0, 50].any() and models[1, 10].any() and models[2, 330].any() and not models[:, 9].any()
    segs, seg_kw = ragged(off)
    used, _, got, _ = check(ops, "epi", ml, mr, segs, seg_kw, models, np.full(3, THR, np.float32), 5, 10, 320)
    assert used.tolist() == [320, 640, 640] and got[1].tolist() == [50, 10, 330]


def test_no_matches_at_all_defines_every_output(ops):
    for kind in ("epi", "hom"):
        _, adaptive_op = fns(ops, kind)
        empty = torch.zeros((0, 2), device="cuda")
        got = adaptive_op(empty, empty, torch.ones((2, 100, 3, 3), device="cuda"), cu(np.full(2, THR)), CONF, 8, round_models=64,
                          pair_off=cu(np.zeros(3, np.int64)), moments=True)
        assert got[-2].tolist() == [100, 100] and got[-1].tolist() == [0, 0] and not got[0].any() and not got[1].any()
        assert not got[2].any() and got[3].numel() == 0 and not got[4].any()


# ---- 4. the batch layer ---------------------------------------------------------------------------------------------------------
def _handed_over(ml, mr, lengths, caller_of):
    """A result dict as forward_pairs_mixed leaves it after group_by_pair, from plain lists in SLOT order."""
    from pats_amd import batch
    pairs = len(lengths)
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([[0], np.cumsum(lengths), [sum(lengths), 0, 0]]).astype(np.int64)          # offsets, M, P, status
    dl, dr, ds = cu(ml), cu(mr), cu(summary)
    return batch, cap, {"matches_l": dl, "matches_r": dr, "by_pair": (dl, dr, ds[:pairs + 1]), "summary": ds, "caller_of": list(caller_of)}


@pytest.mark.parametrize("kind", ["epi", "hom"])
def test_mixed_pack_slots_and_the_stages_downstream(ops, kind):
    H, s = 320, SAMPLE[kind]
    caller_of = [2, 0, 1]                               # slot s_ holds the caller's pair caller_of[s_]
    plan = [(700, [(0.9, 7)]), (1500, [(0.85, 100)]), (400, [])]          # the caller's order
    norm = norm_for(3)
    planted = [ac.plant_pair(8500 + 7 * i, kind, n, H, pl, norm[i]) for i, (n, pl) in enumerate(plan)]
    ml = np.concatenate([planted[i][0] for i in caller_of])
    mr = np.concatenate([planted[i][1] for i in caller_of])
    batch, cap, out = _handed_over(ml, mr, [plan[i][0] for i in caller_of], caller_of)
    models, thr, dn = cu(np.stack([p[2] for p in planted])), cu(np.full(3, THR, np.float32)), cu(norm)
    verify, verify_fixed, key = ((batch.verify_adaptive_by_pair, batch.verify_by_pair, "verified") if kind == "epi" else
                                 (batch.verify_h_adaptive_by_pair, batch.verify_h_by_pair, "verified_h"))
    res = verify(out, cap, models, thr, CONF, s, norm=dn, moments=True)
    assert len(res) == 7 and all(a is b for a, b in zip(out[key] + out[key + "_used"], res)) and len(out[key]) == 5 and out[key + "_on"] == "all"
    used = res[5].cpu().numpy()
    _, adaptive_op = fns(ops, kind)
    for i in range(3):                                  # a pair's result does not depend on its slot
        s_ = caller_of.index(i)
        alone = adaptive_op(cu(planted[i][0]), cu(planted[i][1]), models[i:i + 1], thr[i:i + 1], CONF, s, norm=dn[i:i + 1],
                            pair_off=cu(np.array([0, plan[i][0]], np.int64)), moments=True)
        assert int(alone[5]) == used[s_] and int(alone[1]) == int(res[1][s_]) and int(alone[2]) == int(res[2][s_])
        assert same(alone[4][0], res[4][s_])
    assert [int(used[caller_of.index(i)]) for i in range(3)] == [256, 256, H]          # round_models = None: 256
    zeroed = models.clone()
    for i in range(3):
        zeroed[i, int(used[caller_of.index(i)]):] = 0
    _, _, ref = _handed_over(ml, mr, [plan[i][0] for i in caller_of], caller_of)
    verify_fixed(ref, cap, zeroed, thr, norm=dn, moments=True)
    assert all(same(a, b) for a, b in zip(out[key], ref[key]))
    if kind == "epi":
        a, b = batch.pose_by_pair(out, cap, norm=dn), batch.pose_by_pair(ref, cap, norm=dn)
    else:
        a, b = batch.homography_by_pair(out, cap, norm=dn), batch.homography_by_pair(ref, cap, norm=dn)
    assert len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    for bad in (0, 1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="confidence"):
            verify(out, cap, models, thr, bad, s)
    if kind == "epi":                                   # the split works on the adaptive result as it stands: the caller's order
        assert [t[0].shape[0] for t in batch.split_verified_by_pair(out, cap)] == [700, 1500, 400]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(ops):
    from pats_amd import _lib
    from test_adaptive_cases_host import check_refusals
    lib = _lib.lib()
    live = torch.full((1 << 16,), -777.25, dtype=torch.float32, device="cuda")              # a real allocation behind every pointer
    base = live.data_ptr()
    assert base % 16 == 0
    for branch in ("epipolar", "homography"):
        assert check_refusals(lib, branch, base) > 35
    torch.cuda.synchronize()
    assert bool((live == -777.25).all())                                                # nothing ran: the sentinel stands
    ml, off = torch.zeros((20, 2), device="cuda"), torch.tensor([0, 10, 20], device="cuda")
    models, thr = torch.zeros((2, 128, 3, 3), device="cuda"), torch.zeros(2, device="cuda")
    outs = (torch.full((2, 128), -5, dtype=torch.int32, device="cuda"), torch.full((2,), -5, dtype=torch.int32, device="cuda"),
            torch.full((2,), -5, dtype=torch.int64, device="cuda"), torch.full((20,), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((2,), -5, dtype=torch.int32, device="cuda"), torch.full((2,), -5, dtype=torch.int32, device="cuda"))
    for kind in ("epi", "hom"):
        _, adaptive_op = fns(ops, kind)
        for kw, word in (({"confidence": 1.0}, "confidence"), ({"confidence": float("nan")}, "confidence"), ({"s": 17}, "sample_size"),
                         ({"g": 0}, "models_per_sample"), ({"B": 96}, "multiple of 64"), ({"out": outs[:5]}, "out must be")):
            with pytest.raises(RuntimeError, match=word):
                adaptive_op(ml, ml, models, thr, kw.get("confidence", CONF), kw.get("s", 8), models_per_sample=kw.get("g", 1),
                            round_models=kw.get("B", 64), pair_off=off, out=kw.get("out", outs))
    torch.cuda.synchronize()
    assert all(bool((t == (0xA5 if t.dtype == torch.uint8 else -5)).all()) for t in outs)
