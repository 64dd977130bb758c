"""Host side (-m "not gpu", oracle only): the generators of tests/expand_cases.py are held to what
tests/test_expand_edges_gpu.py relies on - blob_plan reaches the no-match, no-core, border and wrap branches and leaves the
tie classifier next to nothing to excuse; flat_plan's ties are real, its rectangles varied and its strip sums exact in any
summation order.  The oracle's tie-row count per grid is printed (pytest -rA shows it) and asserted against the cap."""
import numpy as np
import pytest

import expand_cases as ec

SWEEP = [(1, 2), (2, 1), (1, 7), (2, 2), (3, 5), (5, 3), (12, 12), (15, 16), (16, 15), (16, 16), (16, 17), (17, 16), (15, 20),
         (20, 15), (19, 20), (20, 20), (24, 32), (38, 50)]


def _rows_for(h, w):
    return max(1, min(40, 600 // (h * w)))


def test_blob_plan_leaves_the_tie_classifier_nothing_to_hide(oracle):
    """Every grid of the sweep, both (iter_num, lower_bound) pairs of the pipeline: tie rows within 0.1 % in total, at most 2
    per call."""
    rows = ties = elem = 0
    for h, w in SWEEP:
        t = e = r = 0
        for it, lb in ((8, 1e-3), (15, 1e-5), (1, 1e-3)):
            rng = np.random.default_rng(1000 * h + w + it)
            P, Z, sx, sy = ec.blob_plan(rng, h, w, _rows_for(h, w))
            assert P.dtype == np.float32 and (P > 0).all() and np.isfinite(Z).all()
            np.testing.assert_allclose(P.sum(-1), 1.0, atol=1e-5)
            s = ec.oracle_stats(oracle.iterative_expand(P, sx, sy, w, h, w, lb, it, with_margin=True), h, w)
            assert s["tie_rows"] <= ec.MAX_TIE_ROWS_PER_CALL, (h, w, it, s)
            t, e, r = t + s["tie_rows"], e + s["elem_tie_rows"], r + s["rows"]
        print("blob_plan %2dx%-2d: %5d rows, %d tie rows, %d element-tie rows" % (h, w, r, t, e))
        rows, ties, elem = rows + r, ties + t, elem + e
    print("blob_plan total: %d rows, %d tie rows, %d element-tie rows" % (rows, ties, elem))
    assert ties <= ec.MAX_TIE_SHARE * rows, "tie rows %d of %d" % (ties, rows)
    assert elem <= 10 * ec.MAX_TIE_SHARE * rows


@pytest.mark.parametrize("h,w", [(12, 12), (15, 20), (20, 15), (24, 32)])
def test_blob_plan_reaches_every_branch(oracle, h, w):
    rng = np.random.default_rng(h * 100 + w)
    P, Z, sx, sy = ec.blob_plan(rng, h, w, max(1, 600 // (h * w)))
    s = ec.oracle_stats(oracle.iterative_expand(P, sx, sy, w, h, w, 1e-3, 8, with_margin=True), h, w)
    print("blob_plan %dx%d it=8 lb=1e-3: %s" % (h, w, s))
    assert s["nomatch"] >= 20 and s["no_core"] >= 20
    assert min(s["on_up"], s["on_down"], s["on_left"], s["on_right"]) >= 1
    assert s["wrap_left"] >= 1 and s["wrap_right"] >= 1
    assert s["mean_area"] >= 5.0                                  # rectangles really grow
    # the dominant dustbin is the row maximum: with M == N that is the `if_nomatching` branch
    assert s["nomatch"] == int((P[:, :-1].argmax(-1) == h * w).sum())
    # independent scales
    assert not np.array_equal(sx, sy)


@pytest.mark.parametrize("h,w", [(12, 12), (16, 16), (15, 20), (20, 15), (24, 32)])
def test_flat_plan_ties_are_real_and_exact(oracle, h, w):
    rng = np.random.default_rng(7)
    M = h * w + 1
    P, sx, sy, start = ec.flat_plan(rng, h, w, 2, M)
    value = np.float32(2.0 ** -8)
    assert set(np.unique(P).tolist()) == {float(value), float(2 * value)}
    # the start cell is the first maximum over the real columns; equal-maxima and dustbin-equal rows are there
    assert np.array_equal(P[:, :, :-1].argmax(-1), start)
    assert ((P[:, :, :-1] == 2 * value).sum(-1) == 2).any() and (P[:, :, -1] == 2 * value).any()
    assert not (P[:, :-1].argmax(-1) == h * w).any()              # the all-column argmax stays on the real column
    out = oracle.iterative_expand(P, sx, sy, w, h, w, 1e-3, 8, with_margin=True)
    s = ec.oracle_stats(out, h, w)
    share = float((out[6][..., 0] == 0).mean())
    print("flat_plan %dx%d it=8: %d distinct rectangles over %d rows, decision margin exactly 0 on %.0f %%"
          % (h, w, s["distinct"], s["rows"], 100 * share))
    assert share >= 0.5 and s["distinct"] >= 30
    # exactness: the cells of every strip next to a few final rectangles sum to the same float32 in any order
    for r in range(0, M - 1, max(1, (M - 1) // 12)):
        for d in range(4):
            cells = ec.strip_cells(P[1, r], out[5][1, r], h, w, d)
            if not (cells > 1e-10).any():
                # sentinels only - the strip lies off the grid.  Its sum does depend on the order, but in every order it stays
                # under 1e-12: it can neither pass lower_bound (1e-5 at least) nor beat a strip with one real cell (2**-8),
                # and among strips that do not pass lower_bound the choice changes nothing
                assert max(ec.f32_sums(cells)) < 1e-12, (r, d, cells)
                continue
            fw, bw, pw = ec.f32_sums(cells)
            assert fw.tobytes() == bw.tobytes() == pw.tobytes(), (r, d, cells)
            assert fw == np.float32(np.sum(cells[cells > 1e-10].astype(np.float64)))     # the sentinels are absorbed


def test_strip_cells_agrees_with_the_oracle_growth_step(oracle):
    """strip_cells is a transcription of the gather: growing by one step from iteration k's rectangle takes the strip whose
    (double) sum is the strict first maximum - checked against the oracle's k + 1 rectangles on blob rows."""
    h, w = 15, 20
    rng = np.random.default_rng(3)
    P, Z, sx, sy = ec.blob_plan(rng, h, w, 1, dust=0.0)
    b1 = oracle.iterative_expand(P, sx, sy, w, h, w, 1e-5, 3)[5][0]
    b2 = oracle.iterative_expand(P, sx, sy, w, h, w, 1e-5, 4)[5][0]
    checked = 0
    for r in range(0, h * w, 7):
        up, down, left, right = b1[r]
        sums = [float(ec.strip_cells(P[0, r], b1[r], h, w, d).astype(np.float64).sum()) for d in range(4)]
        zero = [up == 0, down == h - 1, left == 0, right == w - 1]
        sums = [float(ec.ZERO_F) if z else s for s, z in zip(sums, zero)]
        arg = int(np.argmax(sums))
        want = np.array(b1[r])
        if sums[arg] > 1e-5:
            want[arg] += (-1, 1, -1, 1)[arg]
        assert np.array_equal(want, b2[r]), (r, b1[r], b2[r], sums)
        checked += 1
    assert checked >= 40


def test_tie_threshold_is_the_derived_one():
    assert ec.tie_threshold(12, 12) == 12 * 2.0 ** -23 and ec.tie_threshold(20, 15) == 20 * 2.0 ** -23
    assert ec.tie_threshold(38, 50) == 50 * 2.0 ** -23
    assert ec.GATES["whole_cost"] == dict(atol=3e-6, rtol=5e-5) and ec.GATES["core_cost"] == dict(atol=3e-6, rtol=5e-4)
    assert ec.GATES["average_point"] == dict(atol=2e-4, rtol=2e-5)
    assert ec.GATES["x_scale"] == ec.GATES["y_scale"] == dict(atol=1e-5, rtol=5e-5)
