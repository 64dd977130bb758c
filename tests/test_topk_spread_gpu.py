"""GPU: ops.topk_spread_by_pair / batch.topk_spread_by_pair against the definition of include/pats_amd.h ("Per-pair spread top-K"),
computed with numpy inside the test:
    key     = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000), b = the bits of the confidence; eligible: key >= key(min_conf)
    q_a     = u_a > 0 ? int(min(u_a, 2^24)) : 0;  c_a = min(q_a // cell, grid_a - 1);  cellid = c_0 * grid1 + c_1
    winner  = per cell the eligible match with the largest key, the lowest index among equals
    ranking = the winners by key descending, index ascending; occupied = their number; the first K are the selection
Every comparison is exact: top_idx / top_count / occupied as integers, top_conf / top_l / top_r as bits.  The definition is total
(rows past the count are -1 / 0.0), so whole output buffers are compared.

Synthetic points: the integer part of a coordinate chooses the cell, the fractions (row % 1024, row // 1024, in 1024ths, shifted
per side) identify the row - a copy from a wrong row cannot pass.  The arrays are longer than pair_off[pairs] and the rows behind
it hold conf = 2.0 (never to be selected); the six outputs are views into larger canary-filled buffers whose surroundings must
come back untouched.

One case of the issue's list cannot exist: "a cell whose best match is ineligible but whose second is eligible".  Eligibility is
key >= key(min_conf) and the best match is the one with the largest key, so an ineligible best leaves nothing eligible behind it.
test_thresholds holds what the definition allows instead: cells with eligible and ineligible matches mixed (the winner is the best
ELIGIBLE one, whatever the index order), a cell with none eligible, and a threshold equal to a present value."""
import numpy as np
import pytest
import torch

from test_topk_gpu import CANARY_F, CANARY_I, PAD, TAIL, bits, key_of, rand_conf

pytestmark = pytest.mark.gpu

NAMES = ("top_l", "top_r", "top_conf", "top_idx", "top_count", "occupied")


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cell_ids(pts, cell, grid):
    """cellid of every row of pts [n,2] float32."""
    c = []
    for a in (0, 1):
        u = pts[:, a]
        with np.errstate(invalid="ignore"):
            q = np.where(u > 0, np.minimum(u, np.float32(16777216.0)), np.float32(0)).astype(np.int64)
        c.append(np.minimum(q // cell, grid[a] - 1))
    return c[0] * grid[1] + c[1]


def reference(ml, mr, conf, off, K, cell, grid, side="left", min_conf=None):
    """The definition, on host arrays: the six outputs in full."""
    pairs = len(off) - 1
    tl, tr = np.zeros((pairs, K, 2), np.float32), np.zeros((pairs, K, 2), np.float32)
    tc, ti = np.zeros((pairs, K), np.float32), np.full((pairs, K), -1, np.int32)
    tn, occ = np.zeros((pairs,), np.int64), np.zeros((pairs,), np.int64)
    for p in range(pairs):
        lo, hi = int(off[p]), int(off[p + 1])
        n = max(hi - lo, 0)
        key = key_of(conf[lo:lo + n])
        ids = cell_ids((ml if side == "left" else mr)[lo:lo + n], cell, grid)
        i = np.arange(n)
        if min_conf is not None:
            i = i[key >= key_of(np.float32(min_conf).reshape(1))[0]]
        i = i[np.lexsort((i, ~key[i], ids[i]))]                              # by cell, inside a cell by key descending, index ascending
        winners = i[np.concatenate([[True], ids[i][1:] != ids[i][:-1]])] if len(i) else i
        order = winners[np.lexsort((winners, ~key[winners]))]
        occ[p] = len(order)
        order = order[:K]
        c = len(order)
        tn[p] = c
        ti[p, :c] = order
        tl[p, :c], tr[p, :c], tc[p, :c] = ml[lo + order], mr[lo + order], conf[lo + order]
    return tl, tr, tc, ti, tn, occ


def points(pos, shift):
    """pos [total,2] integers below 4096 -> float32 points: pos + the row's fractions (exact in float32)."""
    g = np.arange(pos.shape[0])
    frac = np.stack([g % 1024, g // 1024 % 1024], 1) / 1024.0 + shift / 4096.0
    out = (pos.astype(np.float64) + frac).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), pos + frac) and pos.max(initial=0) < 4096
    return out


def make_inputs(lengths, conf, pos_l, pos_r):
    """conf, pos_l, pos_r: of all pairs, concatenated (sum(lengths) rows); the tail rows lie at the origin."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(off[-1]) + TAIL
    assert total < (1 << 20)                                    # the fractions are unique per row
    tail = np.zeros((TAIL, 2), np.int64)
    ml, mr = points(np.concatenate([pos_l, tail]), 1), points(np.concatenate([pos_r, tail]), 2)
    cf = np.concatenate([np.asarray(conf, np.float32), np.full(TAIL, 2.0, np.float32)])
    assert cf.shape == (total,) and ml.shape == mr.shape == (total, 2)
    return ml, mr, cf, off


def canary_outputs(pairs, K):
    """Six output views inside larger canary-filled buffers -> (views, whole buffers)."""
    shapes = ((pairs, K, 2), (pairs, K, 2), (pairs, K), (pairs, K), (pairs,), (pairs,))
    dts = (torch.float32, torch.float32, torch.float32, torch.int32, torch.int64, torch.int64)
    views, whole = [], []
    for shape, dt in zip(shapes, dts):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), CANARY_F if dt == torch.float32 else CANARY_I, dtype=dt, device="cuda")
        whole.append(buf)
        views.append(buf[PAD:PAD + n].view(shape))
    return tuple(views), whole


def run(ops, ml, mr, cf, off, K, cell, grid, side="left", min_conf=None, pair_off=None, pairs=None):
    """One call on fresh canary buffers; checks the canaries, returns the six outputs as numpy arrays."""
    d = [torch.from_numpy(x).cuda() for x in (ml, mr, cf)]
    po = torch.from_numpy(off).cuda() if pair_off is None else pair_off
    views, whole = canary_outputs(len(off) - 1, K)
    got = ops.topk_spread_by_pair(d[0], d[1], d[2], po, K, cell, grid, side=side, min_conf=min_conf, out=views, pairs=pairs)
    torch.cuda.synchronize()
    assert len(got) == 6 and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    for buf in whole:
        edge = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
        assert bool((edge == (CANARY_F if buf.dtype == torch.float32 else CANARY_I)).all()), "bytes around an output view changed"
    return [v.cpu().numpy() for v in views]


def compare(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(bits(g), bits(w)), "%s differs (%s)" % (name, what)


def check(ops, inputs, K, cell, grid, side="left", min_conf=None, **kw):
    ml, mr, cf, off = inputs
    got = run(ops, ml, mr, cf, off, K, cell, grid, side, min_conf, **kw)
    compare(got, reference(ml, mr, cf, off, K, cell, grid, side, min_conf), "K = %d, cell = %d, grid %s, %s" % (K, cell, grid, side))
    return got


def scatter(rng, n, cell, grid):
    """n integer positions, uniform over the grid's pixels."""
    return np.stack([rng.integers(0, grid[0] * cell, n), rng.integers(0, grid[1] * cell, n)], 1)


def random_inputs(rng, lengths, cell, grid):
    n = sum(lengths)
    return make_inputs(lengths, rand_conf(rng, n), scatter(rng, n, cell, grid), scatter(rng, n, cell, grid))


# ---- segments -----------------------------------------------------------------------------------------------------------------
def test_segment_lengths_around_the_wave_and_the_workgroup(ops):
    lengths = [7, 0, 1, 63, 64, 65, 1023, 1024, 1025, 5000]
    rng = np.random.default_rng(300)
    inputs = random_inputs(rng, lengths, 8, (9, 13))
    got = check(ops, inputs, 40, 8, (9, 13))
    assert got[5].tolist()[1:3] == [0, 1] and got[5][-1] == 117              # 5000 matches fill the 9 x 13 cells
    check(ops, inputs, 40, 8, (9, 13), side="right")


def test_corrupt_offsets_stay_inside_the_arrays(ops):
    """An end beyond cap, a negative start and a pair with hi < lo: clamped to [0, cap], hi <= lo is an empty pair."""
    rng = np.random.default_rng(301)
    ml, mr, cf, off = random_inputs(rng, [400, 400, 400], 8, (6, 6))
    cap = cf.shape[0]
    bad = np.array([-50, 700, 300, cap + 100000], np.int64)
    got = run(ops, ml, mr, cf, off, 20, 8, (6, 6), pair_off=torch.from_numpy(bad).cuda())
    compare(got, reference(ml, mr, cf, np.clip(bad, 0, cap), 20, 8, (6, 6)), "corrupt offsets")
    assert got[4].tolist() == [20, 0, 20] and got[5].tolist() == [36, 0, 36]


def test_summary_buffer_as_pair_off(ops):
    """pairs= given: pair_off may be the longer summary buffer (offsets, then M, P, status)."""
    rng = np.random.default_rng(302)
    inputs = random_inputs(rng, [500, 0, 3000], 8, (10, 10))
    summary = torch.from_numpy(np.concatenate([inputs[3], [inputs[3][-1], 12345, 0]]).astype(np.int64)).cuda()
    check(ops, inputs, 64, 8, (10, 10), pair_off=summary, pairs=3)


def test_empty_arrays_define_every_output(ops):
    """cap == 0: every pair empty, the outputs still defined."""
    z2, z1 = torch.empty((0, 2), device="cuda"), torch.empty((0,), device="cuda")
    views, _ = canary_outputs(3, 5)
    ops.topk_spread_by_pair(z2, z2, z1, torch.zeros(4, dtype=torch.int64, device="cuda"), 5, 16, (3, 4), out=views)
    assert not views[0].any() and not views[1].any() and not views[2].any() and bool((views[3] == -1).all())
    assert not views[4].any() and not views[5].any()


# ---- grids --------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (1, 7), (7, 1), (100, 75), (127, 129), (128, 128)]


def _grid_lengths(grid, density):
    cells = grid[0] * grid[1]
    if density == "sparse":                                     # fewer matches than cells
        return [cells // 3, cells // 2, max(cells - 1, 0)] if cells < 10000 else [cells // 3, 1]
    return [40 * cells + 3, cells + 1, 300] if cells < 10 else [20000, cells + 1]


@pytest.mark.parametrize("density", ["sparse", "dense"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_grids_with_fewer_and_more_matches_than_cells(ops, grid, density):
    lengths = _grid_lengths(grid, density)
    rng = np.random.default_rng(310 + grid[0] * 1000 + grid[1])
    inputs = random_inputs(rng, lengths, 8, grid)
    got = check(ops, inputs, 256, 8, grid)
    cells = grid[0] * grid[1]
    assert all(o <= min(n, cells) for o, n in zip(got[5], lengths))
    if density == "dense":
        assert got[5][0] > 0.6 * cells                          # the table really fills
        if cells < 10:
            assert got[5][0] == cells


# ---- K ------------------------------------------------------------------------------------------------------------------------
def test_K_around_occupied(ops):
    rng = np.random.default_rng(320)
    inputs = random_inputs(rng, [300, 30], 8, (12, 11))
    occ = int(reference(*inputs, 1, 8, (12, 11))[5][0])
    assert 100 < occ < 132
    for K in (1, occ - 1, occ, occ + 1):
        got = check(ops, inputs, K, 8, (12, 11))
        assert got[4][0] == min(K, occ) and got[5][0] == occ


def test_max_k_on_the_largest_grid_and_two_runs_agree(ops):
    max_k, grid = ops.topk_max_k(), (128, 128)
    assert grid[0] * grid[1] == ops.topk_spread_max_cells() and max_k == 8192
    rng = np.random.default_rng(321)
    inputs = random_inputs(rng, [20000, 6000], 8, grid)
    first = check(ops, inputs, max_k, 8, grid)
    assert first[5][0] > max_k and first[4][0] == max_k and first[5][1] < max_k and first[4][1] == first[5][1]
    second = run(ops, *inputs, max_k, 8, grid)                  # fresh output buffers
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, second))


# ---- one cell, one match per cell ---------------------------------------------------------------------------------------------
def test_all_matches_in_one_cell(ops):
    rng = np.random.default_rng(330)
    lengths = [1500, 900, 1]
    conf = rand_conf(rng, sum(lengths))
    conf[1500:2400] = np.float32(0.625)                         # a pair whose confidences are all equal: index 0 wins
    n = sum(lengths)
    inside = np.stack([2 * 8 + rng.integers(0, 8, n), 3 * 8 + rng.integers(0, 8, n)], 1)       # cell (2, 3) of 5 x 5
    inputs = make_inputs(lengths, conf, inside, scatter(rng, n, 8, (5, 5)))
    for K in (1, 4):
        got = check(ops, inputs, K, 8, (5, 5))
        assert got[4].tolist() == [1, 1, 1] and got[5].tolist() == [1, 1, 1]
        best = conf[:1500].max()
        assert (conf[:1500] == best).sum() >= 1 and got[3][0, 0] == np.flatnonzero(conf[:1500] == best)[0]
        assert got[3][1, 0] == 0 and got[3][2, 0] == 0
    got = check(ops, inputs, 8, 8, (1, 1), side="right")        # 1 x 1: the single best of each pair, whatever the points
    assert got[4].tolist() == [1, 1, 1] and got[3][1, 0] == 0


@pytest.mark.parametrize("grid,n", [((9, 13), 117), ((9, 13), 60), ((100, 75), 7000)])
def test_one_match_per_cell_is_the_plain_top_k(ops, grid, n):
    rng = np.random.default_rng(331 + n)
    cells = grid[0] * grid[1]
    lengths = [n, n // 2]
    where = np.concatenate([rng.permutation(cells)[:m] for m in lengths])
    pos = np.stack([where // grid[1] * 8 + rng.integers(0, 8, len(where)), where % grid[1] * 8 + rng.integers(0, 8, len(where))], 1)
    ml, mr, cf, off = make_inputs(lengths, rand_conf(rng, sum(lengths)), pos, scatter(rng, sum(lengths), 8, grid))
    d = [torch.from_numpy(x).cuda() for x in (ml, mr, cf, off)]
    for K in (16, min(n + 5, ops.topk_max_k())):
        for min_conf in (None, 0.75):
            got = check(ops, (ml, mr, cf, off), K, 8, grid, min_conf=min_conf)
            plain = [t.cpu().numpy() for t in ops.topk_by_pair(*d, K, min_conf=min_conf)]
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:5], plain))
            eligible = [int((cf[off[p]:off[p + 1]] >= (min_conf or 0.0)).sum()) for p in range(2)]
            assert got[5].tolist() == eligible


# ---- coordinates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 3, 8, 65536])
def test_coordinate_edges(ops, cell):
    grid = (5, 4)
    rng = np.random.default_rng(340 + cell)

    def edge_values(g):
        return [-3.5, np.nan, np.inf, -np.inf, 16777216.0, g * cell - 0.5, g * cell, g * cell + 1000, 0.0, cell - 0.5, cell,
                (g - 1) * cell - 0.5, (g - 1) * cell]

    a, b = np.meshgrid(np.array(edge_values(grid[0]), np.float32), np.array(edge_values(grid[1]), np.float32), indexing="ij")
    odd = np.stack([a.ravel(), b.ravel()], 1)                   # every combination: 169 rows
    n = odd.shape[0]
    lengths = [n, n]
    ml, mr, cf, off = make_inputs(lengths, rand_conf(rng, 2 * n), np.zeros((2 * n, 2), np.int64), scatter(rng, 2 * n, 8, grid))
    ml[:n] = odd
    ml[n:2 * n] = odd[rng.permutation(n)]
    ids = cell_ids(odd, cell, grid)
    assert ids.min() == 0 and ids.max() == grid[0] * grid[1] - 1
    nan_row = np.array([[np.nan, 2.5 * cell]], np.float32)
    assert cell_ids(nan_row, cell, grid)[0] == 2 and cell_ids(np.array([[np.inf, -np.inf]], np.float32), cell, grid)[0] == 4 * grid[1]
    got = check(ops, (ml, mr, cf, off), 32, cell, grid)
    assert got[5][0] == len(np.unique(ids))
    mr[:2 * n] = ml[:2 * n]                                     # the same through the other side
    check(ops, (np.ascontiguousarray(mr[::-1]), mr, cf, off), 32, cell, grid, side="right")


# ---- side ---------------------------------------------------------------------------------------------------------------------
def test_side_chooses_the_points(ops):
    rng = np.random.default_rng(350)
    lengths, grid = [700, 300], (8, 8)
    n = sum(lengths)
    lump, spread = np.stack([rng.integers(8, 16, n), rng.integers(40, 48, n)], 1), scatter(rng, n, 8, grid)
    conf = rand_conf(rng, n)
    for pos_l, pos_r, many in ((lump, spread, "right"), (spread, lump, "left")):
        inputs = make_inputs(lengths, conf, pos_l, pos_r)
        for side in ("left", "right"):
            got = check(ops, inputs, 100, 8, grid, side=side)
            assert got[5].min() > 50 if side == many else got[5].tolist() == [1, 1]      # the wrong side fails on the count alone


# ---- threshold ----------------------------------------------------------------------------------------------------------------
def test_thresholds(ops):
    """Three cells in a row.  Cell 0 holds eligible and ineligible matches mixed, the ineligible ones first in the list and the best
    eligible one last; cell 1 none eligible; cell 2 one match exactly at the threshold (inclusive)."""
    conf = np.array([0.30, 0.49, 0.70, 0.20, 0.90, 0.10, 0.45, 0.50], np.float32)
    x = np.array([0, 1, 2, 3, 4, 8, 9, 16])                     # cells 0 0 0 0 0 1 1 2 at cell = 8
    pos = np.stack([x, np.zeros_like(x)], 1)
    inputs = make_inputs([8], conf, pos, pos[::-1].copy())
    got = check(ops, inputs, 4, 8, (3, 1), min_conf=0.5)
    assert got[5].tolist() == [2] and got[3][0].tolist() == [4, 7, -1, -1]
    got = check(ops, inputs, 4, 8, (3, 1))
    assert got[5].tolist() == [3] and got[3][0].tolist() == [4, 7, 6, -1]
    got = check(ops, inputs, 4, 8, (3, 1), min_conf=float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert got[5].tolist() == [1] and got[3][0].tolist() == [4, -1, -1, -1]
    got = check(ops, inputs, 4, 8, (3, 1), min_conf=1.5)         # above every match, below the tail rows' 2.0
    assert got[5].tolist() == [0] and got[4].tolist() == [0] and (got[3] == -1).all() and not got[0].any() and not got[2].any()
    rng = np.random.default_rng(360)
    inputs = random_inputs(rng, [3000, 0, 700], 8, (12, 12))
    uniq = np.unique(inputs[2][:3700])
    for thr in (0.75, float(uniq[len(uniq) // 2]), float(uniq[-1])):           # 0.75: the value a fifth of the matches share
        check(ops, inputs, 64, 8, (12, 12), min_conf=thr)
        check(ops, inputs, 64, 8, (12, 12), min_conf=thr, side="right")


def test_bad_arguments_are_refused(ops):
    rng = np.random.default_rng(370)
    ml, mr, cf, off = [torch.from_numpy(x).cuda() for x in random_inputs(rng, [10], 8, (2, 2))]
    most = ops.topk_spread_max_cells()
    for kw in ({"side": "both"}, {"side": 0}, {"grid": (2,)}, {"grid": (2, 0)}, {"grid": (2.5, 2)}, {"grid": 4}, {"grid": (most + 1, 1)},
               {"grid": (1, most + 1)}, {"cell": 0}, {"cell": 65537}, {"cell": 2.5}, {"min_conf": float("nan")}, {"min_conf": -0.5},
               {"K": 0}, {"K": ops.topk_max_k() + 1}):
        a = dict(K=4, cell=8, grid=(2, 2), side="left", min_conf=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match="topk_spread_by_pair"):
            ops.topk_spread_by_pair(ml, mr, cf, off, a["K"], a["cell"], a["grid"], side=a["side"], min_conf=a["min_conf"])
    with pytest.raises(RuntimeError):
        ops.topk_spread_by_pair(ml.double(), mr, cf, off, 4, 8, (2, 2))
    with pytest.raises(RuntimeError):
        ops.topk_spread_by_pair(ml, mr, cf, off.int(), 4, 8, (2, 2))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.topk_spread_by_pair(ml, mr, torch.stack([cf, cf], 1)[:, 0], off, 4, 8, (2, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.topk_spread_by_pair(ml, mr, cf, off, 4, 8, (2, 2), out=ops.topk_by_pair(ml, mr, cf, off, 4))


# ---- batch level --------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("mixed", [False, True])
def test_batch_level(ops, mixed):
    from pats_amd import batch
    from test_confidence_gpu import _small_batch
    _, cap, out, _ = _small_batch(mixed)
    _, _, own, _ = _small_batch(mixed)                       # a second, identical run: regrouped by the caller below
    lists = batch.split_by_pair(own, cap)                    # caller's order for the mixed pack; `own` now holds by_pair
    K, cell = 50, 16
    hw = cap.shapes if mixed else [(cap.h, cap.w)]
    grid = (2 * max(h for h, _ in hw), 2 * max(w for _, w in hw))               # ceil(32 h / 16), ceil(32 w / 16)
    for side in ("left", "right"):
        top = batch.topk_spread_by_pair(out, cap, K, cell, side=side)
        assert top is out["topk"] and len(top) == 5 and top[0].shape == (cap.pairs, K, 2) and top[3].dtype == torch.int32
        occ, c_, g_, s_ = out["topk_spread"]
        assert (c_, g_, s_) == (cell, grid, side) and occ.shape == (cap.pairs,) and occ.dtype == torch.int64
        # the one-copy arrangement: summary, then top_count, in one buffer; occupied a tensor of its own
        assert out["topk_summary"].shape == (2 * cap.pairs + 4,) and torch.equal(out["topk_summary"][:cap.pairs + 4], out["summary"])
        assert top[4].data_ptr() == out["topk_summary"][cap.pairs + 4:].data_ptr() and torch.equal(out["summary"], own["summary"])
        assert torch.equal(top[4], torch.clamp(occ, max=K)) and int(occ.min()) > 8
        # equals ops.topk_spread_by_pair on the regrouped lists
        ml, mr, _, mc = out["by_pair"]
        hand = ops.topk_spread_by_pair(ml, mr, mc, out["summary"], K, cell, grid, side=side, pairs=cap.pairs)
        assert all(_same(a, b) for a, b in zip(list(top) + [occ], hand))
        # split_topk_by_pair: the caller's order, against the definition on the caller's lists
        got = batch.split_topk_by_pair(out, cap)
        for p, (l, r, c) in enumerate(lists):
            hl, hr, hc = (t.cpu().numpy() for t in (l, r, c))
            want = reference(hl, hr, hc, np.array([0, len(hc)]), K, cell, grid, side)
            cnt = int(want[4][0])
            gl, gr, gc, gi = (t.cpu().numpy() for t in got[p])
            assert gi.dtype == np.int32 and np.array_equal(gi, want[3][0, :cnt]), (p, side)
            assert np.array_equal(bits(gl), bits(want[0][0, :cnt])) and np.array_equal(bits(gr), bits(want[1][0, :cnt]))
            assert np.array_equal(bits(gc), bits(want[2][0, :cnt]))
        # after a regroup of the caller's own: the same bits, top_count a tensor of its own
        again = batch.topk_spread_by_pair(own, cap, K, cell, side=side)
        assert "topk_summary" not in own and all(_same(a, b) for a, b in zip(again, top)) and _same(own["topk_spread"][0], occ)
    if mixed:
        assert out["caller_of"] != list(range(cap.pairs))    # the slots are not the caller's order: the comparison above saw it
    # the on="topk" stages run on it unchanged
    norm = torch.from_numpy(np.tile(np.array([160, 120, 1 / 200.0, 1 / 200.0, 160, 120, 1 / 200.0, 1 / 200.0], np.float32),
                                    (cap.pairs, 1))).cuda()
    models = batch.hypothesize_by_pair(out, cap, 16, seed=7, norm=norm, on="topk")
    ver = batch.verify_by_pair(out, cap, models, torch.full((cap.pairs,), 0.05, device="cuda"), norm=norm, on="topk")
    assert tuple(models.shape) == (cap.pairs, 16, 3, 3) and int(ver[2].min()) >= 8 and int(ver[2].max()) <= K
    # a plain top-K afterwards is a plain top-K again
    batch.topk_by_pair(out, cap, K)
    assert "topk_spread" not in out and "topk" in out
