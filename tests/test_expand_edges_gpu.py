"""-m gpu: the patch-area expansion kernel (csrc/expand.hip: Iterative_expand_matrix + Compute_scaling) at its grid, batch and
count edges, against the CPU oracle (oracle/pats_oracle.c, double-precision strip sums).  Every case goes through ONE
comparison, expand_cases.check_expand: same input on both sides, all six outputs and row_nomatch, `bound` equal on every row
whose oracle decision margin exceeds max(h, w) * 2**-23 (derived in expand_cases.py), float outputs under the gates the
project already uses.  Each test asserts how many rows that margin could have excused (at most 2 per call, 0.1 % per test).

The shapes are chosen by the kernel's code paths: SMALL (h, w <= 16) against the looped strips; 16 rows per workgroup
against 4 (N > 381); the staged-once dustbin row against the per-group copy (m < 8); idle groups in the last workgroup; a
workgroup straddling problems; the counted launch; log input; lim3 != w; the refusals."""
import numpy as np
import pytest
import torch

import expand_cases as ec
from expand_cases import cu

pytestmark = pytest.mark.gpu

SWEEP = [(1, 2), (2, 1), (1, 7), (2, 2), (3, 5), (5, 3), (12, 12), (15, 16), (16, 15), (16, 16), (16, 17), (17, 16), (15, 20),
         (20, 15), (19, 20), (20, 20), (24, 32), (38, 50)]
ZERO = float(ec.ZERO_F)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


def rows_per_wg(N):
    return 16 if 2 * 16 * (N + 3) * 4 <= 48 * 1024 else 4


class Tally:
    """Rows compared and rows the tie classifier could have excused, over one test."""

    def __init__(self):
        self.rows = self.ties = self.excused = self.calls = 0

    def add(self, res):
        self.rows += res["rows"]
        self.ties += res["tie_rows"]
        self.excused += res["excused"]
        self.calls += 1
        return res

    def close(self, what):
        print("%s: %d calls, %d rows, %d tie rows, %d rows excused" % (what, self.calls, self.rows, self.ties, self.excused))
        assert self.ties <= ec.MAX_TIE_SHARE * self.rows, "%s: %d tie rows of %d" % (what, self.ties, self.rows)


def both_domains(ops, oracle, tally, P, Z, sx, sy, h, w, lim3, lb, it, M, **kw):
    lin = tally.add(ec.check_expand(ops, oracle, P, sx, sy, h, w, lim3, lb, it, is_log=False, M=M, **kw))
    log = tally.add(ec.check_expand(ops, oracle, Z, sx, sy, h, w, lim3, lb, it, is_log=True, M=M, **kw))
    return lin, log


# ---- 1. grid sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SWEEP)
def test_grid_sweep(ops, oracle, h, w):
    """Every grid with iter_num in {1, 8, 15} x lower_bound in {1e-5, 1e-3}, linear and log input, with a batch whose row count
    is a multiple of the rows per workgroup and one whose row count is not (M = N, then M = N - 1 or one problem fewer)."""
    n = h * w
    N = n + 1
    R = rows_per_wg(N)
    tally = Tally()
    b_min = max(1, -(-40 // n))                    # at least 40 rows on the tiny grids
    full = next(b for b in range(b_min, b_min + 2 * R + 1) if (b * n) % R == 0)
    ragged = next((b for b in range(b_min, b_min + 2 * R + 1) if (b * n) % R != 0), None)
    # n a multiple of the rows per workgroup: every batch fills whole workgroups, so drop one source row instead
    batches = [(full, N), (ragged, N) if ragged is not None else (1, N - 1)]
    assert (batches[0][0] * n) % R == 0 and (batches[1][0] * (batches[1][1] - 1)) % R != 0
    for b, M in batches:
        for it in (1, 8, 15):
            for lb in (1e-5, 1e-3):
                rng = np.random.default_rng([h, w, it, int(lb * 1e6), b])
                P, Z, sx, sy = ec.blob_plan(rng, h, w, b, M=M)
                both_domains(ops, oracle, tally, P, Z, sx, sy, h, w, w, lb, it, M)
    tally.close("grid %dx%d" % (h, w))


@pytest.mark.parametrize("h,w", [(2, 2), (1, 7), (3, 5), (12, 12)])
def test_border_rule_with_a_threshold_below_a_strip_of_fill_ins(ops, oracle, h, w):
    """lower_bound = 1.5e-14, between the 1e-14 a border strip's sum is replaced by and the sum of an off-grid strip of fill-ins
    (max(h, w) x 1e-14): every real strip passes, the rectangle reaches all four borders, and from then on only the border rule
    (up == 0, down == height - 1, left == 0, right == width - 1) keeps it on the grid.  With any larger threshold the rule at
    the bottom border cannot be observed (the strip below the grid holds fill-ins only).  Landscape and square grids only: on a
    portrait grid the start cells lie off the derived grid and two off-grid strips of fill-ins compete - real ties."""
    tally = Tally()
    width, height = max(h, w), h * w // max(h, w)
    for it in (15, 40):
        rng = np.random.default_rng([h, w, it, 15])
        P, Z, sx, sy = ec.blob_plan(rng, h, w, 3)
        for res in both_domains(ops, oracle, tally, P, Z, sx, sy, h, w, w, 1.5e-14, it, h * w + 1):
            bound = res["got"][5]
            assert bound.min() >= 0 and (bound[..., 1] <= height - 1).all() and (bound[..., 3] <= width - 1).all()
            if it == 40 or h * w <= 15:
                assert (bound == np.array([0, height - 1, 0, width - 1])).all()
    tally.close("fill-in threshold on %dx%d" % (h, w))


# ---- 2. row count != column count ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(12, 12), (15, 20)])
def test_row_count_differs_from_column_count(ops, oracle, h, w):
    """m = M - 1 source rows in {1, 3, 7, 8, 9, 17, 37, n - 1, n + 1, n + 56} against n = h * w real columns: the per-group
    dustbin copy (m < 8), workgroups over three and more problems, and `if_nomatching` compared with the ROW count: a row
    whose maximum over all columns lies in column m < n - a REAL column - is flagged and zeroed, a row whose maximum lies
    in the dustbin column n != m is NOT (while row_nomatch is set for it)."""
    n = h * w
    tally = Tally()
    for m in (1, 3, 7, 8, 9, 17, 37, n - 1, n + 1, n + 56):
        M = m + 1
        b = 11 if m < 40 else 2                                   # 11 * m: never a multiple of 16 for these m
        rng = np.random.default_rng([h, w, m])
        P, Z, sx, sy = ec.blob_plan(rng, h, w, b, M=M, dust=0.3)
        quirk_rows, dust_rows = list(range(0, m, 3)), list(range(1, m, 3))
        ec.force_argmax_column(P, dust_rows, n, rng)              # the maximum in the dustbin column
        if m < n:
            ec.force_argmax_column(P, quirk_rows, m, rng)         # the maximum in real column m
        P /= P.sum(-1, keepdims=True)
        Z = np.log(P.astype(np.float64)).astype(np.float32)
        it, lb = (8, 1e-3) if h == 12 else (15, 1e-5)
        for res, src in zip(both_domains(ops, oracle, tally, P, Z, sx, sy, h, w, w, lb, it, M), (P, Z)):
            whole, core, flag = res["got"][0], res["got"][1], res["flag"]
            amax = src[:, :m, :].argmax(-1)
            assert np.array_equal(whole == ZERO, amax == m), "m=%d: whole_cost is zeroed exactly where the argmax is column m" % m
            assert (core[amax == m] == ZERO).all()
            assert np.array_equal(flag.astype(bool), amax == n)
            if m < n:
                assert (amax[:, quirk_rows] == m).all() and (whole[:, quirk_rows] == ZERO).all()
            dusty = amax == n                                     # n != m for every m of this test
            assert dusty[:, dust_rows].all() and (whole[dusty] != ZERO).all() and flag[dusty].all()
    tally.close("M != N on %dx%d" % (h, w))


# ---- 3. lim3 != w --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(12, 12), (15, 20), (20, 15)])
def test_start_cell_stride_differs_from_the_grid_width(ops, oracle, h, w):
    """limitation[3] in {w - 1, w + 1, max(h, w)} through the list and through a device tensor (the .item() route): the start
    cell max0 // lim3, max0 % lim3 may then lie off the grid, and a rectangle that no cell belongs to must still give the
    reference's centroid and scale (sums of the 1e-14 fill-ins)."""
    tally = Tally()
    for lim3 in (w - 1, w + 1, max(h, w)):
        for as_tensor in (False, True):
            it, lb = (8, 1e-3) if h == 12 else (15, 1e-5)
            rng = np.random.default_rng([h, w, lim3])
            P, Z, sx, sy = ec.blob_plan(rng, h, w, 3)
            both_domains(ops, oracle, tally, P, Z, sx, sy, h, w, lim3, lb, it, h * w + 1, lim_as_tensor=as_tensor)
    tally.close("lim3 != w on %dx%d" % (h, w))


# ---- 4. exact ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(12, 12), (16, 16), (15, 20), (20, 15), (24, 32)])
def test_exact_ties_follow_the_reference_tie_rules(ops, oracle, h, w):
    """flat_plan: every strip sum is exact in fp32 in any order and every growth step is an exact tie, so the result is fixed by
    the tie rules alone (first of up, down, left, right under strict >; first index in the argmax).  No tie exclusion: every
    row, bit-equal bounds - the margin classifier would excuse all of these rows."""
    for it in (8, 15):
        for M in (h * w + 1, 38):
            rng = np.random.default_rng([h, w, it, M])
            P, sx, sy, start = ec.flat_plan(rng, h, w, 3, M)
            res = ec.check_expand(ops, oracle, P, sx, sy, h, w, w, 1e-3, it, is_log=False, M=M, exact=True)
            assert res["excused"] == 0 and res["tie_rows"] == 0
            assert float((res["want"][6][..., 0] == 0).mean()) >= 0.5
            assert not res["flag"].any()
            # power-of-two logs exponentiate exactly: the log input meets the same ties
            Z = np.log2(P).astype(np.float32) * np.float32(np.log(2.0))
            lin = ops.exp(cu(Z)).cpu().numpy()
            if np.array_equal(lin, P):
                res = ec.check_expand(ops, oracle, Z, sx, sy, h, w, w, 1e-3, it, is_log=True, M=M, exact=True)
                assert res["excused"] == 0


# ---- 5. log input is the linear input ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(12, 12), (15, 20)])
def test_log_input_equals_linear_input_bit_for_bit(ops, h, w):
    rng = np.random.default_rng([5, h, w])
    P, Z, sx, sy = ec.blob_plan(rng, h, w, 5, M=h * w - 2)
    dZ, dsx, dsy = cu(Z), cu(sx), cu(sy)
    it, lb = (8, 1e-3) if h == 12 else (15, 1e-5)
    a, fa = ec.gpu_expand(ops, dZ, dsx, dsy, h, w, w, lb, it, is_log=True)
    b, fb = ec.gpu_expand(ops, ops.exp(dZ), dsx, dsy, h, w, w, lb, it, is_log=False)
    for x, y, name in zip(a, b, ec.NAMES):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), name
    assert torch.equal(fa, fb)              # blob rows: no two logs of a row exponentiate to one float at the maximum


def test_row_nomatch_follows_the_logs(ops):
    """Two logs one ulp apart that exponentiate to the same float: the flag is the argmax of the values handed in (the logs),
    the rectangle comes from the exponentiated row (first index on the tie)."""
    h = w = 12
    n = h * w
    base = np.float32(-0.3)
    cand = base + np.arange(0, 4096, dtype=np.float32) * np.float32(2.0 ** -25)
    cand = np.unique(cand)
    e = ops.exp(cu(cand)).cpu().numpy()
    pair = np.nonzero((e[1:] == e[:-1]) & (cand[1:] > cand[:-1]))[0]
    assert len(pair), "no two neighbouring logs with one exponential near -0.3"
    lo, hi = cand[pair[0]], cand[pair[0] + 1]
    Z = np.full((1, 3, n + 1), -12.0, np.float32)        # 12 cells of exp(-12) stay under lower_bound: no growth
    Z[0, 0, 17], Z[0, 0, n] = lo, hi        # the dustbin log is larger: flag set
    Z[0, 1, 17], Z[0, 1, n] = hi, lo        # the real column's log is larger: flag clear
    sx = np.ones((1, n), np.float32)
    got, flag = ec.gpu_expand(ops, cu(Z), cu(sx), cu(sx), h, w, w, 1e-3, 8, is_log=True)
    assert flag.cpu().numpy().tolist() == [[1, 0]]
    lin, flag_lin = ec.gpu_expand(ops, ops.exp(cu(Z)), cu(sx), cu(sx), h, w, w, 1e-3, 8, is_log=False)
    assert flag_lin.cpu().numpy().tolist() == [[0, 0]]            # equal floats: the first index, a real column
    for x, y in zip(got, lin):
        assert torch.equal(x, y)
    assert got[5][0, :, 0].tolist() == [1, 1] and got[5][0, :, 2].tolist() == [5, 5]       # both start at cell 17 = (1, 5)


# ---- 6. counted launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,cap,M", [(12, 12, 64, 145), (12, 12, 64, 41), (12, 12, 64, 6), (24, 32, 5, 769), (24, 32, 5, 770)])
def test_counted_launch(ops, oracle, h, w, cap, M):
    """Capacity `cap`, counts {0, 1, one that ends inside a workgroup (where m allows one), cap - 1, cap, cap + 3}: the first
    min(count, cap) problems equal the plain launch bit for bit, every byte past them keeps its sentinel; the padding
    problems hold NaN / inf plans and scales."""
    n, m = h * w, M - 1
    R = rows_per_wg(n + 1)
    rng = np.random.default_rng([6, h, w, M])
    P, Z, sx, sy = ec.blob_plan(rng, h, w, cap, M=M)
    tally = Tally()
    tally.add(ec.check_expand(ops, oracle, P[:4], sx[:4], sy[:4], h, w, w, 1e-3, 8, is_log=False, M=M))
    tally.close("counted %dx%d M=%d" % (h, w, M))
    inside = [c for c in range(2, cap - 1) if (c * m) % R != 0]
    counts = [0, 1] + inside[:1] + [cap - 1, cap, cap + 3]
    if m % R != 0:
        assert inside, "a count that ends inside a workgroup exists for this m"
    for is_log in (False, True):
        src = cu(Z if is_log else P)
        dsx, dsy = cu(sx), cu(sy)
        plain = ec.sentinel_outputs(cap, m)
        ec.raw_expand(ops, src, dsx, dsy, h, w, w, 1e-3, 8, plain, is_log=is_log)
        assert not any(bool(torch.isnan(o).any()) for o in plain[:5]) and bool((plain[6] < 2).all())
        for count in counts:
            k = min(count, cap)
            hostile = src.clone()
            hsx, hsy = dsx.clone(), dsy.clone()
            if k < cap:
                pad = hostile[k:]
                vals = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30], device="cuda")
                pad.copy_(vals[torch.arange(pad.numel(), device="cuda") % 4].view(pad.shape))
                hsx[k:], hsy[k:] = float("nan"), float("inf")
            outs = ec.sentinel_outputs(cap, m)
            ec.raw_expand(ops, hostile, hsx, hsy, h, w, w, 1e-3, 8, outs, is_log=is_log,
                          count=torch.tensor([count], dtype=torch.int64, device="cuda"))
            torch.cuda.synchronize()
            for o, p, name in zip(outs, plain, ec.NAMES + ("row_nomatch",)):
                assert torch.equal(o[:k], p[:k]), "count %d: %s of the live problems differs from the plain launch" % (count, name)
            assert ec.untouched(outs, k), "count %d: an output past problem %d was written" % (count, k)


# ---- 7. independence of neighbours ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,M", [(12, 12, 6), (12, 12, 25), (12, 12, 145), (15, 20, 10), (15, 20, 27), (24, 32, 4), (24, 32, 7)])
def test_a_problem_does_not_depend_on_its_neighbours(ops, h, w, M):
    """Nine different problems in one launch against the same nine launched one by one: bit-equal (the staged dustbin row must
    be the right problem's - for the second problem of a straddling workgroup, for a workgroup over three and more problems,
    and in the last, partly idle workgroup)."""
    rng = np.random.default_rng([7, h, w, M])
    P, Z, sx, sy = ec.blob_plan(rng, h, w, 9, M=M)
    for is_log in (False, True):
        src, dsx, dsy = cu(Z if is_log else P), cu(sx), cu(sy)
        it, lb = (8, 1e-3) if h == 12 else (15, 1e-5)
        got, flag = ec.gpu_expand(ops, src, dsx, dsy, h, w, w, lb, it, is_log=is_log)
        for i in range(9):
            one, f1 = ec.gpu_expand(ops, src[i:i + 1].contiguous(), dsx[i:i + 1].contiguous(), dsy[i:i + 1].contiguous(), h, w, w,
                                    lb, it, is_log=is_log)
            for x, y, name in zip(got, one, ec.NAMES):
                assert torch.equal(x[i:i + 1], y), "problem %d: %s depends on the batch it is launched in" % (i, name)
            assert torch.equal(flag[i:i + 1], f1)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    rng = np.random.default_rng(8)
    P, Z, sx, sy = ec.blob_plan(rng, 12, 12, 2)
    dP, dsx, dsy = cu(P), cu(sx), cu(sy)
    outs = ec.sentinel_outputs(2, 144)
    with pytest.raises(RuntimeError):                             # the grid does not match the columns
        ec.raw_expand(ops, dP, dsx, dsy, 12, 11, 12, 1e-3, 8, outs)
    with pytest.raises(RuntimeError):
        ec.raw_expand(ops, dP, dsx, dsy, 12, 12, 12, 1e-3, 0, outs)                       # iter_num == 0
    with pytest.raises(RuntimeError):
        ec.raw_expand(ops, dP, dsx, dsy, 12, 12, 0, 1e-3, 8, outs)                        # lim3 == 0
    positions, ranges = ops.Compute_positions_and_ranges(12, 12, "cuda")
    for bad_x, bad_y in ((dsx[:, :-1].contiguous(), dsy), (dsx, dsy[:, :-1].contiguous())):       # scale tensors of the wrong length
        with pytest.raises(RuntimeError):
            ops.Iterative_expand_matrix(dP, bad_x, bad_y, [0, 12, 0, 12], ranges, positions, lower_bound=1e-3, iter_num=8)
    p11, r11 = ops.Compute_positions_and_ranges(12, 11, "cuda")
    with pytest.raises(RuntimeError):
        ops.Iterative_expand_matrix(dP, dsx, dsy, [0, 12, 0, 11], r11, p11, lower_bound=1e-3, iter_num=8)
    with pytest.raises(RuntimeError):
        ops.Iterative_expand_matrix(dP, dsx, dsy, [0, 12, 0, 12], ranges, positions, lower_bound=1e-3, iter_num=0)
    # 46 x 46: N + 3 = 2120 > 2048 floats per staged row
    n = 46 * 46
    big = torch.full((1, 3, n + 1), 1.0 / (n + 1), device="cuda")
    bsx = torch.ones((1, n), device="cuda")
    bouts = ec.sentinel_outputs(1, 2)
    with pytest.raises(RuntimeError):
        ec.raw_expand(ops, big, bsx, bsx, 46, 46, 46, 1e-3, 8, bouts)
    p46, r46 = ops.Compute_positions_and_ranges(46, 46, "cuda")
    with pytest.raises(RuntimeError):
        ops.Iterative_expand_matrix(big, bsx, bsx, [0, 46, 0, 46], r46, p46, lower_bound=1e-3, iter_num=8)
    torch.cuda.synchronize()
    assert ec.untouched(outs) and ec.untouched(bouts)
    # and the largest grid that is accepted (45 x 45, N + 3 = 2029) runs
    n = 45 * 45
    ok = torch.full((1, 3, n + 1), 1.0 / (n + 1), device="cuda")
    osx = torch.ones((1, n), device="cuda")
    oouts = ec.sentinel_outputs(1, 2)
    ec.raw_expand(ops, ok, osx, osx, 45, 45, 45, 1e-3, 8, oouts)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(oouts[0]).any()) and bool((oouts[5] >= 0).all())


# ---- 9. bench-sized launch -----------------------------------------------------------------------------------------------
def test_bench_sized_launch(ops, oracle):
    """20 736 problems of 12 x 12 (the step's size): 64 distinct problems, checked against the oracle, tiled 324 times with a
    random permutation of the source rows per copy - every copy's rows equal its source rows bit for bit.  The launch where
    blockIdx.x * rows-per-workgroup and b * M * N are largest."""
    h = w = 12
    n, B, base_b = 144, 20736, 64
    rng = np.random.default_rng(9)
    P, Z, sx, sy = ec.blob_plan(rng, h, w, base_b)
    tally = Tally()
    for lo in range(0, base_b, 16):
        both_domains(ops, oracle, tally, P[lo:lo + 16], Z[lo:lo + 16], sx[lo:lo + 16], sy[lo:lo + 16], h, w, w, 1e-3, 8, n + 1)
    tally.close("bench-sized base")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    perm = torch.argsort(torch.rand((B, n), device="cuda", generator=gen), dim=1)                    # [B, 144]
    rows = torch.cat([perm, torch.full((B, 1), n, dtype=torch.int64, device="cuda")], 1)             # the dustbin row stays last
    src = torch.arange(B, device="cuda") % base_b
    for is_log in (False, True):
        basep = cu(Z if is_log else P)
        dsx, dsy = cu(sx), cu(sy)
        want, wflag = ec.gpu_expand(ops, basep, dsx, dsy, h, w, w, 1e-3, 8, is_log=is_log)
        big = basep[src[:, None], rows].contiguous()                                                 # [B, 145, 145]
        assert big.shape == (B, n + 1, n + 1)
        got, gflag = ec.gpu_expand(ops, big, dsx[src].contiguous(), dsy[src].contiguous(), h, w, w, 1e-3, 8, is_log=is_log)
        del big
        for x, y, name in zip(got, want, ec.NAMES):
            assert torch.equal(x, y[src[:, None], perm]), "%s of a copy differs from its source rows" % name
        assert torch.equal(gflag, wflag[src[:, None], perm])
