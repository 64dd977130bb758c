"""GPU: the order-preserving compactions of csrc/merge.hip at the tile and round edges of their scan, and the regroup by pair past
one pass of its grid - bit for bit against plain numpy (tests/compaction_cases.py) and the CPU oracle.  Everything here is integer
selection or fp32 arithmetic the oracle mirrors operation by operation: every comparison is array_equal / torch.equal.

    (a) ops.third_inputs / ops.refine_scatter     n = 144 B flags, B on either side of every path change of run_scan
    (b) ops.get_result, level-1 scan              n = 2304 rows1
    (c) ops.get_result, level-0 scan              any n = batch h w, a dozen survivors at the group / wave / tile / round edges
    (d) ops.get_result with more rows than surviving cells (validate=False): what is written and what *count holds
    (e) ops.get_result_chunks (uniform, ragged; with and without conf16) with a level-1 scan of two rounds
    (f) ops.matches_by_pair on a synthetic row table against the stable argsort, up to three passes of the regroup grid
    (g) ops.merge_patches_new / _old with 18 432 and 16 272 coarse cells (the flag scan of the merge on both of its paths)
Every test prints the flag count, tile count and rounds it reached (pytest -rA / -s shows them)."""
import ctypes

import numpy as np
import pytest
import torch

import compaction_cases as cc

pytestmark = pytest.mark.gpu

PAD = 64
SENT_F, SENT_I = -777.25, -123456
SMALL_KINDS = [("none",), ("all",), ("random", 0.02), ("random", 0.5), ("random", 0.98), ("tile_last",), ("tile_first",), ("tiles",),
               ("bytes",), ("single",)]
LARGE_KINDS = [("random", 0.5), ("random", 0.02), ("tile_last",), ("tiles",), ("single",)]
kind_id = cc.spec_id


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def specs_of(kind, n, large=False):
    """The patterns of one kind at n flags (single: every edge position of the path n takes; the last flag only when large)."""
    specs = cc.large_patterns(n) if large else cc.small_patterns(n)
    return [s for s in specs if s[0] == kind[0] and (kind[0] != "random" or s[1] == kind[1])]


def test_the_constants_are_the_kernels():
    k = cc.source_constants()
    assert (cc.T, cc.SMALL, cc.ROUND, cc.PAIR_ROUND, cc.GRID) == (k["SCAN_TILE"], k["SCAN_SMALL"], k["TILE_ROUND"], k["PAIR_ROUND"],
                                                                 k["REGROUP_GRID"]) == (2048, 16384, 1024, 1024, 2048 * 256)


# ---- (a) the 144-flag consumers -------------------------------------------------------------------------------------------------------
def case144(B, spec, seed=0):
    n = B * cc.CELLS2
    f = cc.flags(spec, n, seed).reshape(B, cc.CELLS2)
    rng = np.random.default_rng([seed, B, 7])
    pts = (rng.random((B, cc.CELLS2, 2), dtype=np.float32) * np.float32(12.0))
    pts[0, :4] = np.array([[0.125, 0.375], [0.625, 1.125], [2.875, 3.375], [5.5, 5.5]], np.float32)       # round-half-even cases
    return f, pts, rng


def check_third_inputs(ops, oracle, B, spec, capacity=None):
    f, pts, _ = case144(B, spec)
    w0, w1, wb = oracle.third_inputs(f, pts)
    idx, P = cc.compact_ref(f)
    assert P == cc.survivors(spec, f.size) == wb.shape[0] and np.array_equal(wb, idx // cc.CELLS2)
    if capacity is None:
        m0, m1, bi = ops.third_inputs(cu(f), cu(pts))
        assert m0.shape == (P, 2) and m1.shape == (P, 2) and bi.shape == (P,)
        c = P
    else:
        m0, m1, bi, cnt = ops.third_inputs(cu(f), cu(pts), capacity=capacity, sync=False)
        assert int(cnt.item()) == P
        c = min(P, capacity)
    assert np.array_equal(bi[:c].cpu().numpy(), wb[:c])
    assert np.array_equal(m0[:c].cpu().numpy(), w0[:c]) and np.array_equal(m1[:c].cpu().numpy(), w1[:c])
    return P


@pytest.mark.parametrize("kind", SMALL_KINDS, ids=kind_id)
@pytest.mark.parametrize("B", cc.B_SMALL)
def test_third_inputs_at_the_single_workgroup_and_two_level_edges(ops, oracle, B, kind):
    print(cc.describe("third_inputs B = %d" % B, B * cc.CELLS2))
    specs = specs_of(kind, B * cc.CELLS2)
    assert specs
    for spec in specs:
        check_third_inputs(ops, oracle, B, spec)


@pytest.mark.parametrize("kind", LARGE_KINDS, ids=kind_id)
@pytest.mark.parametrize("B", cc.B_LARGE)
def test_third_inputs_across_the_rounds_of_the_tile_scan(ops, oracle, B, kind):
    """The count is the carry the last round leaves; the rows past the first round's tiles need every earlier round's carry in their
    tile base.  capacity keeps the outputs small: the whole list where it is short, the first 2^17 rows of the dense patterns (whose
    later rows ops.refine_scatter checks below)."""
    n = B * cc.CELLS2
    print(cc.describe("third_inputs B = %d" % B, n))
    (spec,) = specs_of(kind, n, large=True)
    P = check_third_inputs(ops, oracle, B, spec, capacity=min(cc.survivors(spec, n) + 5, 1 << 17))
    if kind[0] != "random" or kind[1] < 0.1:
        assert P + 5 <= 1 << 17                                    # these lists are checked whole


def third_inputs_raw(ops, f, pts, cap):
    """pats_third_inputs_f32 on caller-owned, sentinel-filled buffers PAD rows longer than `cap` -> (mk0, mk1, b_ids, count)."""
    B = f.shape[0]
    m0 = torch.full((cap + PAD, 2), SENT_F, dtype=torch.float32, device="cuda")
    m1 = torch.full((cap + PAD, 2), SENT_F, dtype=torch.float32, device="cuda")
    bi = torch.full((cap + PAD,), SENT_I, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda")
    nws = ops._L().pats_compact_workspace_bytes(B * cc.CELLS2)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device="cuda")
    rc = ops._L().pats_third_inputs_f32(ops._ptr(f), ops._ptr(pts), B, ops._ptr(m0), ops._ptr(m1), ops._ptr(bi), cap, ops._ptr(cnt),
                                        ops._ptr(ws), nws, ops._stream())
    assert rc == 0, ops._L().pats_last_error().decode()
    torch.cuda.synchronize()
    return m0, m1, bi, cnt


@pytest.mark.parametrize("which", ["0", "P-1", "P", "P+5"])
@pytest.mark.parametrize("B,spec", [(cc.B144["small_last"], ("random", 0.5)), (cc.B144["two_level_first"], ("random", 0.5)),
                                    (cc.B144["two_rounds"], ("tiles", cc.edge_tiles(cc.B144["two_rounds"] * cc.CELLS2)))],
                         ids=lambda v: cc.spec_id(v) if isinstance(v, tuple) else str(v))
def test_third_inputs_capacity_bounds_the_rows_not_the_count(ops, oracle, B, spec, which):
    n = B * cc.CELLS2
    print(cc.describe("third_inputs capacity %s, B = %d" % (which, B), n))
    P = cc.survivors(spec, n)
    c = {"0": 0, "P-1": P - 1, "P": P, "P+5": P + 5}[which]
    assert check_third_inputs(ops, oracle, B, spec, capacity=c) == P             # ops.third_inputs(capacity=c, sync=False)
    f, pts, _ = case144(B, spec)
    w0, w1, wb = oracle.third_inputs(f, pts)
    m0, m1, bi, cnt = third_inputs_raw(ops, cu(f), cu(pts), c)
    k = min(P, c)
    assert int(cnt.item()) == P
    assert np.array_equal(m0[:k].cpu().numpy(), w0[:k]) and np.array_equal(m1[:k].cpu().numpy(), w1[:k])
    assert np.array_equal(bi[:k].cpu().numpy(), wb[:k])
    assert bool((m0[k:] == SENT_F).all()) and bool((m1[k:] == SENT_F).all()) and bool((bi[k:] == SENT_I).all())     # nothing past c


def check_refine_scatter(ops, oracle, B, spec, forms):
    """ops.refine_scatter in the given forms - "2d" / "1d": the label as [P*16,2] (column 0 read; column 1 says the opposite) or
    [P*16]; "+conf": with the confidence - against oracle.refine_scatter and conf16_ref.  Compared on the device."""
    f, pts, rng = case144(B, spec)
    P = cc.survivors(spec, f.size)
    mk = rng.random((P, 16, 2), dtype=np.float32) * np.float32(96.0)
    drop = rng.random(P * 16, dtype=np.float32) < 0.2
    label0 = np.where(drop, np.float32(-10.0), np.float32(1e8))
    wf, wp = oracle.refine_scatter(f, pts, mk, label0)
    idx, _ = cc.compact_ref(f)
    assert wf.all() if P == 0 else int((~wf).sum()) == int((~drop).sum())
    fd, pd, mkd, wfd, wpd = cu(f), cu(pts), cu(mk), cu(wf), cu(wp)
    del wp
    labels = {"1d": cu(label0), "2d": cu(np.stack([label0, np.where(drop, np.float32(1e8), np.float32(-10.0))], 1))}
    for form in forms:
        lb = labels[form[:2]]
        if form.endswith("+conf"):
            conf = rng.random((P, 16), dtype=np.float32) + np.float32(0.25)
            f16, p16, c16 = ops.refine_scatter(fd, pd, mkd, lb, conf=cu(conf))
            want = cc.conf16_ref(f, conf, wf)
            assert torch.equal(c16, cu(want)), form
            assert bool(((c16 == 0) == wfd).all())                  # 0 exactly where if_nomatching16 is set (conf > 0 elsewhere)
            del c16
        else:
            f16, p16 = ops.refine_scatter(fd, pd, mkd, lb)
        assert f16.dtype == torch.bool and torch.equal(f16, wfd), form
        assert torch.equal(p16, wpd), form
        del f16, p16
    return P


@pytest.mark.parametrize("kind", SMALL_KINDS, ids=kind_id)
@pytest.mark.parametrize("B", cc.B_SMALL)
def test_refine_scatter_at_the_single_workgroup_and_two_level_edges(ops, oracle, B, kind):
    print(cc.describe("refine_scatter B = %d" % B, B * cc.CELLS2))
    for spec in specs_of(kind, B * cc.CELLS2):
        P = check_refine_scatter(ops, oracle, B, spec, ("2d", "1d", "2d+conf", "1d+conf"))
        assert P > 0 or kind[0] in ("none", "tile_last")           # P = 0: every cell flagged (tile_last keeps nothing of 144 flags)


@pytest.mark.parametrize("kind", LARGE_KINDS, ids=kind_id)
@pytest.mark.parametrize("B", cc.B_LARGE)
def test_refine_scatter_across_the_rounds_of_the_tile_scan(ops, oracle, B, kind):
    n = B * cc.CELLS2
    print(cc.describe("refine_scatter B = %d" % B, n))
    (spec,) = specs_of(kind, n, large=True)
    check_refine_scatter(ops, oracle, B, spec, ("2d", "1d+conf"))
    torch.cuda.empty_cache()


# ---- (b), (c), (d) get_result ---------------------------------------------------------------------------------------------------------
class ResultCase:
    """Inputs of the two-level get_result: f0 [bs, h w] level-0 flags, f1 [rows1, 2304] level-1 flags, random points and scales,
    left_choice mixed at both levels; sc1 = one scale per sub-cell, sc1_row = one per row."""

    def __init__(self, grid, f0, f1, seed):
        self.bs, self.h, self.w = grid
        rng = np.random.default_rng([seed, f0.size, f1.size])
        n0 = self.h * self.w
        self.f0, self.f1 = f0.reshape(self.bs, n0), f1.reshape(-1, cc.SUB)
        self.rows1 = self.f1.shape[0]
        self.ap0 = rng.random((self.bs, n0, 2), dtype=np.float32) * np.float32(max(self.h, self.w))
        self.sc0 = np.exp(rng.random((self.bs, n0, 2), dtype=np.float32) * np.float32(2.4) - np.float32(1.2))
        self.ap1 = rng.random((self.rows1, cc.SUB, 2), dtype=np.float32) * np.float32(48.0)
        self.sc1 = np.exp(rng.random((self.rows1, cc.SUB, 2), dtype=np.float32) * np.float32(2.4) - np.float32(1.2))
        self.sc1_row = np.ascontiguousarray(self.sc1[:, 0, :])
        self.c0 = rng.random(self.bs) < 0.5
        self.c1 = rng.random(self.rows1) < 0.5
        if self.bs > 1:
            self.c0[:2] = [True, False]
        if self.rows1 > 1:
            self.c1[:2] = [False, True]
        self.sizes = [[32, self.h, self.w], [2, 48, 48]]

    def want(self, oracle, per_row):
        sc1 = np.repeat(self.sc1_row[:, None, :], cc.SUB, 1) if per_row else self.sc1
        return oracle.get_result(self.bs, [self.f0, self.f1], [self.ap0, self.ap1], [self.sc0, sc1], self.sizes, [self.c0, self.c1])

    def device(self):
        if not hasattr(self, "_dev"):
            self._dev = {k: cu(getattr(self, k)) for k in ("f0", "f1", "ap0", "ap1", "sc0", "c0", "c1")}
        return self._dev

    def got(self, ops, per_row, validate=True):
        d = self.device()
        return ops.get_result(self.bs, [d["f0"], d["f1"]], [d["ap0"], d["ap1"]], [d["sc0"], cu(self.sc1_row if per_row else self.sc1)],
                              self.sizes, [d["c0"], d["c1"]], validate=validate)


def level1_case(rows1, spec, seed=0):
    """rows1 surviving cells at random places of a (2, h, 7) level-0 batch; the pattern over the 2304 rows1 sub-cell flags."""
    h = (rows1 * 5 // 4) // 14 + 1
    rng = np.random.default_rng([seed, rows1, 3])
    f0 = np.ones(2 * h * 7, np.uint8)
    f0[rng.choice(f0.size, rows1, replace=False)] = 0
    return ResultCase((2, h, 7), f0, cc.flags(spec, rows1 * cc.SUB, seed), seed)


def check_get_result(ops, oracle, case, M_claim=None):
    for per_row in (False, True):                                   # scale[1] as [K,n1,2] and as [K,2]
        wl, wr = case.want(oracle, per_row)
        ml, mr = case.got(ops, per_row)
        assert ml.shape == wl.shape and (M_claim is None or wl.shape[0] == M_claim)
        assert np.array_equal(ml.cpu().numpy(), wl) and np.array_equal(mr.cpu().numpy(), wr), "per_row = %s" % per_row
    return wl.shape[0]


@pytest.mark.parametrize("kind", SMALL_KINDS, ids=kind_id)
@pytest.mark.parametrize("rows1", cc.R_SMALL)
def test_get_result_level1_at_the_single_workgroup_and_two_level_edges(ops, oracle, rows1, kind):
    n = rows1 * cc.SUB
    print(cc.describe("get_result rows1 = %d" % rows1, n))
    for spec in specs_of(kind, n):
        check_get_result(ops, oracle, level1_case(rows1, spec), cc.survivors(spec, n))


@pytest.mark.parametrize("kind", LARGE_KINDS, ids=kind_id)
@pytest.mark.parametrize("rows1", cc.R_LARGE)
def test_get_result_level1_across_the_rounds_of_the_tile_scan(ops, oracle, rows1, kind):
    n = rows1 * cc.SUB
    print(cc.describe("get_result rows1 = %d" % rows1, n))
    (spec,) = specs_of(kind, n, large=True)
    check_get_result(ops, oracle, level1_case(rows1, spec), cc.survivors(spec, n))


@pytest.mark.parametrize("cells", cc.CELLS0)
def test_get_result_level0_survivors_at_every_edge_of_its_scan(ops, oracle, cells):
    """The level-0 scan takes any n = batch h w: about a dozen surviving cells at the first and last cell and on either side of
    every thread-group, wave, tile and round boundary that fits - each must find its own level-1 row."""
    print(cc.describe("get_result level 0, %d x %d x %d" % cc.grid_of(cells), cells))
    pos = cc.boundary_cells(cells)
    f0 = np.ones(cells, np.uint8)
    f0[pos] = 0
    rows1 = len(pos)
    assert 1 <= rows1 <= 16
    case = ResultCase(cc.grid_of(cells), f0, cc.flags(("random", 0.5), rows1 * cc.SUB, cells), seed=cells)
    assert check_get_result(ops, oracle, case) == round(0.5 * rows1 * cc.SUB)


def get_result_raw(ops, case, per_row, cap):
    """pats_get_result_f32 on caller-owned, sentinel-filled match buffers PAD rows longer than `cap` -> (ml, mr, count)."""
    d = case.device()
    s1 = cu(case.sc1_row if per_row else case.sc1)
    ml = torch.full((cap + PAD, 2), SENT_F, dtype=torch.float32, device="cuda")
    mr = torch.full((cap + PAD, 2), SENT_F, dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda")
    n0 = case.h * case.w
    nws = ops._L().pats_get_result_workspace_bytes(case.bs * n0, case.rows1, cc.SUB)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    ps0, ps1 = (ctypes.c_int * 3)(*case.sizes[0]), (ctypes.c_int * 3)(*case.sizes[1])
    rc = ops._L().pats_get_result_f32(case.bs, ops._ptr(d["f0"]), ops._ptr(d["f1"]), case.rows1, ops._ptr(d["ap0"]), ops._ptr(d["ap1"]),
                                      ops._ptr(d["sc0"]), ops._ptr(s1), 0 if per_row else 2, ps0, ps1, ops._ptr(d["c0"].view(torch.uint8)),
                                      ops._ptr(d["c1"].view(torch.uint8)), ops._ptr(ml), ops._ptr(mr), cap, ops._ptr(cnt), ops._ptr(ws), nws,
                                      ops._stream())
    assert rc == 0, ops._L().pats_last_error().decode()
    torch.cuda.synchronize()
    return ml, mr, cnt


@pytest.mark.parametrize("extra", ["flagged", "unflagged"])
@pytest.mark.parametrize("cells", [60, cc.SMALL + 1])
def test_get_result_rows_past_the_surviving_cells(ops, oracle, cells, extra):
    """More level-1 rows than surviving level-0 cells (validate=False; the batch path's capacity-sized tensors).  The rows past
    the survivors emit nothing in either case.  Fully flagged - what the batch path guarantees through merge / refine_scatter -
    *count is the match count.  Left unflagged, *count ALSO counts their unflagged sub-cells (it is the total of the level-1
    scan): the first M_true rows of the outputs are the matches, nothing is written behind them, and *count - M_true slots beyond
    stay unwritten.  include/pats_amd.h (pats_get_result_f32) and INTEGRATION.md state this contract."""
    print(cc.describe("get_result rows past the survivors, level 0", cells))
    pos = cc.boundary_cells(cells) if cells > 100 else np.arange(3, 60, 5)
    K, rows1 = len(pos), len(pos) + 3
    f0 = np.ones(cells, np.uint8)
    f0[pos] = 0
    f1 = cc.flags(("random", 0.5), rows1 * cc.SUB, cells).reshape(rows1, cc.SUB)
    ignored = int((f1[K:] == 0).sum())
    assert ignored > 1000
    if extra == "flagged":
        f1[K:] = 1
    grid = cc.grid_of(cells) if cells > 100 else (2, 5, 6)
    case = ResultCase(grid, f0, f1, seed=cells)
    M_true = int((f1[:K] == 0).sum())
    for per_row in (False, True):
        wl, wr = case.want(oracle, per_row)                          # the oracle walks the surviving cells: K rows
        assert wl.shape[0] == M_true
        ml, mr, cnt = get_result_raw(ops, case, per_row, rows1 * cc.SUB)
        assert int(cnt.item()) == (M_true if extra == "flagged" else M_true + ignored)
        assert np.array_equal(ml[:M_true].cpu().numpy(), wl) and np.array_equal(mr[:M_true].cpu().numpy(), wr)
        assert bool((ml[M_true:] == SENT_F).all()) and bool((mr[M_true:] == SENT_F).all())
    if extra == "flagged":                                           # the wrapper's slices are then the matches
        ml, mr = case.got(ops, True, validate=False)
        assert np.array_equal(ml.cpu().numpy(), wl) and np.array_equal(mr.cpu().numpy(), wr)
    with pytest.raises(IndexError):
        case.got(ops, True, validate=True)


# ---- (e) get_result_chunks --------------------------------------------------------------------------------------------------------------
def chunk_inputs(rng, R, total, cells):
    f16 = (rng.random((R, cc.SUB), dtype=np.float32) < 0.7)
    flat = f16.reshape(-1)
    for i in (0, cc.T - 1, cc.T, cc.ROUND * cc.T - 1, cc.ROUND * cc.T, total * cc.SUB - 1):         # survivors at the tile and round edges
        flat[i] = False
    f16[total:] = True
    pts16 = rng.random((R, cc.SUB, 2), dtype=np.float32) * np.float32(96.0)
    conf16 = rng.random((R, cc.SUB), dtype=np.float32) + np.float32(0.25)
    avn = rng.random((cells, 2), dtype=np.float32) * np.float32(600.0)
    xsn = rng.random((cells, 2), dtype=np.float32) + np.float32(0.2)
    return f16, pts16, conf16, avn, xsn


def check_chunk_outputs(res, res_conf, f16, conf16, total):
    """What holds for every table: the count and match_row are the kept sub-cells of the first `total` rows in order, match_conf is
    conf16 gathered there, and the confidence form returns the plain form's matches."""
    idx, M = cc.compact_ref(f16[:total])
    assert idx[-1] >= cc.ROUND * cc.T, "no match past the first round of the tile scan"
    ml, mr, mrow, cnt = res
    mlc, mrc, mrowc, cntc, mc = res_conf
    assert int(cnt.item()) == M == int(cntc.item())
    assert np.array_equal(mrow[:M].cpu().numpy(), (idx // cc.SUB).astype(np.int32)) and torch.equal(mrowc[:M], mrow[:M])
    assert torch.equal(mlc[:M], ml[:M]) and torch.equal(mrc[:M], mr[:M])
    assert np.array_equal(mc[:M].cpu().numpy(), conf16.reshape(-1)[idx])
    return idx, M


def test_get_result_chunks_uniform_with_a_two_round_level1_scan(ops):
    """ops.get_result_chunks over a table of rows_cap >= 911 rows against ops.get_result on the expanded (chunk, pair) batch (held
    to the oracle above), as test_batched_merge_and_result_against_the_single_chunk_ops does on a one-round table."""
    rng = np.random.default_rng(2024)
    pairs, h, w, once = 4, 15, 20, 80
    N = h * w
    ifn1 = rng.random((pairs, N)) >= 0.93
    rows = ops.chunk_rows(cu(ifn1), h, w, once)
    total, R, C = int(rows.chunk_base[-1].item()), rows.rows_cap, rows.Cmax
    assert int(rows.status.item()) == 0 and R >= total > cc.ROWS1["two_rounds"]
    print(cc.describe("get_result_chunks uniform, %d rows of %d" % (total, R), R * cc.SUB))
    assert cc.scan_path(R * cc.SUB)[1] >= 2
    f16, pts16, conf16, avn, xsn = chunk_inputs(rng, R, total, pairs * N)
    avn, xsn = avn.reshape(pairs, N, 2), xsn.reshape(pairs, N, 2)
    res = ops.get_result_chunks(rows, cu(f16), cu(avn), cu(pts16), cu(xsn))
    res_conf = ops.get_result_chunks(rows, cu(f16), cu(avn), cu(pts16), cu(xsn), conf16=cu(conf16))
    idx, M = check_chunk_outputs(res, res_conf, f16, conf16, total)
    masks = rows.masks.reshape(C * pairs, N)
    av_c, xs_c = cu(np.tile(avn, (C, 1, 1))), cu(np.tile(xsn, (C, 1, 1)))
    sc_rows = xs_c.reshape(-1, 2)[torch.nonzero(~masks.reshape(-1)).flatten()]
    ones = lambda k: torch.ones(k, dtype=torch.bool, device="cuda")       # noqa: E731
    wl, wr = ops.get_result(C * pairs, [masks, cu(f16[:total])], [av_c.flip(dims=[2]) / 32.0, cu(pts16[:total]).flip(dims=[2]) / 2.0],
                            [xs_c, sc_rows], [[32, h, w], [2, 48, 48]], [ones(C * pairs), ones(total)])
    assert wl.shape[0] == M and torch.equal(res[0][:M], wl) and torch.equal(res[1][:M], wr)


def test_get_result_chunks_ragged_with_a_two_round_level1_scan(ops):
    """The ragged entry over four pairs of three grids against each pair's own uniform table (ops.chunk_rows with the pair's chunk
    cap 2 w): the batch's matches of pair p, in order, are that pair's matches alone."""
    rng = np.random.default_rng(2025)
    shapes = [(15, 20), (12, 16), (15, 20), (10, 24)]
    table = ops.PairTable(shapes, torch.device("cuda"))
    ifn1 = rng.random(table.cells) >= 0.95
    rows = ops.chunk_rows_ragged(cu(ifn1), table)
    total, R = int(rows.chunk_base[-1].item()), rows.rows_cap
    assert int(rows.status.item()) == 0 and R >= total > cc.ROWS1["two_rounds"]
    print(cc.describe("get_result_chunks ragged, %d rows of %d" % (total, R), R * cc.SUB))
    assert cc.scan_path(R * cc.SUB)[1] >= 2
    f16, pts16, conf16, avn, xsn = chunk_inputs(rng, R, total, table.cells)
    res = ops.get_result_chunks(rows, cu(f16), cu(avn), cu(pts16), cu(xsn))
    res_conf = ops.get_result_chunks(rows, cu(f16), cu(avn), cu(pts16), cu(xsn), conf16=cu(conf16))
    idx, M = check_chunk_outputs(res, res_conf, f16, conf16, total)
    row_pair = rows.row_pair.cpu().numpy()[:total]
    match_pair = row_pair[idx // cc.SUB]
    ml, mr = res[0][:M].cpu().numpy(), res[1][:M].cpu().numpy()
    base = table.cell_base_host
    for p, (h, w) in enumerate(shapes):
        sel = np.flatnonzero(row_pair == p)
        own = ops.chunk_rows(cu(ifn1[base[p]:base[p + 1]][None]), h, w, 2 * w)
        assert int(own.chunk_base[-1].item()) == len(sel) and int(own.status.item()) == 0
        pad = own.rows_cap - len(sel)
        grow = lambda a, fill: np.concatenate([a[sel], np.full((pad,) + a.shape[1:], fill, a.dtype)])      # noqa: E731
        wl, wr, wrow, wM = ops.get_result_chunks(own, cu(grow(f16, True)), cu(avn[base[p]:base[p + 1]][None]), cu(grow(pts16, 0)),
                                                 cu(xsn[base[p]:base[p + 1]][None]))
        m = int(wM.item())
        assert m == int((match_pair == p).sum()) > 0
        assert np.array_equal(ml[match_pair == p], wl[:m].cpu().numpy()) and np.array_equal(mr[match_pair == p], wr[:m].cpu().numpy())
        assert np.array_equal(sel[wrow[:m].cpu().numpy()], (idx // cc.SUB)[match_pair == p])


# ---- (f) the regroup by pair ------------------------------------------------------------------------------------------------------------
G = cc.GRID
REGROUP = [(0, 3, 3, None), (1, 1, 1, None), (1, 3, 3, None), (G - 1, 3, 3, None), (G, cc.PAIR_ROUND, 1, None),
           (G + 1, cc.PAIR_ROUND + 1, 3, G), (G + 1, 1, 3, G), (1100000, 2 * cc.PAIR_ROUND + 1, 3, G), (1100000, 3, 1, None),
           (1100000, cc.PAIR_ROUND, 3, 2 * G)]


@pytest.mark.parametrize("M,pairs,Cmax,boundary", REGROUP)
def test_matches_by_pair_against_the_stable_argsort(ops, M, pairs, Cmax, boundary):
    """ops.matches_by_pair on the synthetic row table: pairs without a match at the first, a middle and the last position, a pair
    empty in one chunk and present in the next, a run that starts exactly where a pass of the regroup grid ends; with and without
    the summary tail (P) and the confidences, into caller-owned buffers that carry sentinels around what the call may write."""
    print("matches_by_pair: M = %d matches = %d pass(es) of the %d-thread grid, %d pairs = %d round(s) of %d, Cmax = %d"
          % (M, -(-M // G), G, pairs, -(-pairs // cc.PAIR_ROUND), cc.PAIR_ROUND, Cmax))
    host = cc.RowTable(pairs, Cmax, status=2)
    rows = host.on_device(cu)
    lengths = cc.run_lengths(M, pairs, Cmax, seed=17, boundary_at=boundary)
    mrow = cc.match_rows(lengths)
    order, off = cc.regroup_ref(host.pair_of_rows(mrow), pairs)
    if boundary is not None:                                         # a run starts exactly at that match
        assert 0 < boundary < M and (mrow[boundary] // cc.ROWS_PER_RUN) != (mrow[boundary - 1] // cc.ROWS_PER_RUN)
    if pairs > 3 and M > 100:
        assert off[1] == 0 and off[pairs // 2] == off[pairs // 2 + 1] and off[pairs - 1] == off[pairs]
    if pairs > 1 and Cmax > 1 and M > 100:
        assert lengths[0, 1] == 0 and lengths[1, 1] > 0
    cap = M + PAD
    rng = np.random.default_rng(M + pairs)
    ml, mr = rng.random((cap, 2), dtype=np.float32), rng.random((cap, 2), dtype=np.float32)
    conf = rng.random(cap, dtype=np.float32)
    mrow_d = cu(np.concatenate([mrow, np.full(PAD, -1, np.int32)]))          # rows past M are never looked at
    ml_d, mr_d, conf_d = cu(ml), cu(mr), cu(conf)
    M_d = torch.tensor([M], dtype=torch.int64, device="cuda")
    P_d = torch.tensor([4242], dtype=torch.int64, device="cuda")
    for with_P in (False, True):
        for with_conf in (False, True):
            n_off = pairs + 1 + (3 if with_P else 0)
            ol = torch.full((cap, 2), SENT_F, dtype=torch.float32, device="cuda")
            orr = torch.full((cap, 2), SENT_F, dtype=torch.float32, device="cuda")
            oc = torch.full((cap,), SENT_F, dtype=torch.float32, device="cuda")
            off_buf = torch.full((n_off + 2 * PAD,), SENT_I, dtype=torch.int64, device="cuda")
            out = (ol, orr, off_buf[PAD:PAD + n_off]) + ((oc,) if with_conf else ())
            got = ops.matches_by_pair(rows, ml_d, mr_d, mrow_d, M_d, out=out, P=P_d if with_P else None,
                                      match_conf=conf_d if with_conf else None)
            torch.cuda.synchronize()
            what = "P = %s, conf = %s" % (with_P, with_conf)
            assert np.array_equal(got[2].cpu().numpy(), off), what
            if with_P:
                assert got[3].cpu().tolist() == off.tolist() + [M, 4242, 2], what
            assert bool((off_buf[:PAD] == SENT_I).all()) and bool((off_buf[PAD + n_off:] == SENT_I).all()), what
            assert np.array_equal(ol[:M].cpu().numpy(), ml[:M][order]) and np.array_equal(orr[:M].cpu().numpy(), mr[:M][order]), what
            assert bool((ol[M:] == SENT_F).all()) and bool((orr[M:] == SENT_F).all()), what
            if with_conf:
                assert got[-1] is oc and np.array_equal(oc[:M].cpu().numpy(), conf[:M][order]) and bool((oc[M:] == SENT_F).all()), what
            else:
                assert bool((oc == SENT_F).all())


# ---- (g) the flag scan of the merge -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("new", [True, False], ids=["new", "old"])
@pytest.mark.parametrize("bt,h,w", [(24, 24, 32), (113, 12, 12)])
def test_merge_patches_with_a_two_level_and_a_single_workgroup_flag_scan(ops, oracle, bt, h, w, new):
    """merge_patches_new / _old through the single-chunk API with 24 x 24 x 32 = 18 432 coarse cells (the two-level scan of the level-1
    flags) and 113 x 12 x 12 = 16 272 (the last single-workgroup size), against oracle.merge_patches as
    test_merge_patches_large_and_batched does on 768 cells.  The rows sit at the scan's edges: few patches survive."""
    NP = bt * h * w
    assert NP in (cc.CELLS2 * cc.B144["full_tiles"], cc.CELLS2 * cc.B144["small_last"])
    print(cc.describe("merge_patches_%s %d x %d x %d" % ("new" if new else "old", bt, h, w), NP))
    rng = np.random.default_rng(NP + int(new))
    l1 = np.ones(NP, bool)
    l1[cc.single_positions(NP)] = False
    l1[rng.choice(NP, 160, replace=False)] = False
    l1[(NP // 2) + np.arange(3 * w)] = False                        # neighbours: windows that reach into each other
    l1 = l1.reshape(bt, h * w)
    B = int((~l1).sum())
    trust = rng.lognormal(-1.0, 0.9, (B, 144)).astype(np.float32)
    trust[::3] = np.round(trust[::3] * 4) / 4
    f2 = rng.random((B, 144)) < 0.3
    sb0 = np.where(rng.random((bt, h * w, 16, 9)) < 0.5, 0.0, np.round(rng.normal(0, 1, (bt, h * w, 16, 9)), 1) - 5000.0)
    want, wt, wf2, wsb = oracle.merge_patches(new, trust, (h * 32, w * 32), l1, f2, sb0)
    tr, ff, sb = cu(trust), cu(f2), cu(sb0)
    fn = ops.merge_patches_new if new else ops.merge_patches_old
    out, _ = fn(B, tr, (h * 32, w * 32), cu(l1), ff, sb)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(tr.cpu().numpy(), wt) and np.array_equal(ff.cpu().numpy(), wf2)
    assert np.array_equal(sb.cpu().numpy(), wsb)
    assert 0 < (~want).sum()
