"""Host side (-m "not gpu"): tests/compaction_cases.py is held to what tests/test_compaction_edges_gpu.py relies on - the constants
parsed out of csrc/merge.hip are the expected ones, the derived sizes straddle every threshold of the scan and of the regroup,
every flag pattern has the survivor count it claims, the synthetic match rows honour the regroup's precondition, and the numpy
compaction agrees with the CPU oracle before either judges the GPU."""
import numpy as np
import pytest

import compaction_cases as cc


def test_the_parsed_constants_are_the_expected_ones():
    k = cc.source_constants()
    assert (k["SCAN_TILE"], k["SCAN_SMALL"], k["TILE_ROUND"], k["PAIR_ROUND"]) == (2048, 16384, 1024, 1024)
    assert (k["REGROUP_BLOCKS"], k["REGROUP_THREADS"], k["REGROUP_GRID"]) == (2048, 256, 524288)
    assert (k["SMALL_GROUP"], k["FLAGS_GROUP"]) == (16, 8)
    # a constant that moves is read, not remembered
    moved = open(cc.MERGE_HIP).read().replace("constexpr int SCAN_TILE = 2048;", "constexpr int SCAN_TILE = 4096;")
    assert cc.source_constants(moved)["SCAN_TILE"] == 4096
    with pytest.raises(AssertionError):
        cc.source_constants(moved.replace("b0 += 1024", "b0 += 512"))         # the round no longer is the launch's workgroup


def test_the_derived_sizes_straddle_every_threshold():
    assert cc.B144 == {"one": 1, "small_last": 113, "two_level_first": 114, "full_tiles": 128, "one_round": 14563, "two_rounds": 14564,
                       "three_rounds": 29128}
    assert cc.ROWS1 == {"one": 1, "small_last": 7, "two_level_first": 8, "one_round": 910, "two_rounds": 911, "three_rounds": 1821}
    for per, rows in ((cc.CELLS2, cc.B144), (cc.SUB, cc.ROWS1)):
        n = {k: per * v for k, v in rows.items()}
        assert n["small_last"] <= cc.SMALL < n["two_level_first"]
        assert cc.scan_path(n["small_last"])[1] == 0 and cc.scan_path(n["two_level_first"]) == (9, 1)
        assert cc.scan_path(n["one_round"]) == (1024, 1) and n["one_round"] % cc.T != 0          # ragged last tile
        assert cc.scan_path(n["two_rounds"]) == (1025, 2)
        assert cc.scan_path(n["three_rounds"]) == (2049, 3)
    assert (cc.CELLS2 * cc.B144["small_last"], cc.CELLS2 * cc.B144["two_level_first"]) == (16272, 16416)
    assert cc.CELLS2 * cc.B144["full_tiles"] == 9 * cc.T == 18432
    assert cc.SUB * cc.ROWS1["small_last"] == 16128 and cc.SUB * cc.ROWS1["two_level_first"] == 18432
    assert cc.CELLS0 == (1, 15, 17, 2047, 2049, 16383, 16384, 16385, 2162688)
    assert cc.scan_path(cc.CELLS0[-1]) == (1056, 2)
    assert [cc.grid_of(n) for n in cc.CELLS0[5:]] == [(3, 43, 127), (4, 64, 64), (5, 29, 113), (33, 256, 256)]
    for n in cc.CELLS0:
        b, h, w = cc.grid_of(n)
        assert b * h * w == n
        pos = cc.boundary_cells(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and len(pos) <= 16 and len(set(pos.tolist())) == len(pos)
    big = cc.boundary_cells(cc.CELLS0[-1]).tolist()
    assert all(p in big for p in (7, 8, 511, 512, 2047, 2048, cc.ROUND * cc.T - 1, cc.ROUND * cc.T))
    assert all(p in cc.boundary_cells(16384).tolist() for p in (15, 16, 1023, 1024, 2047, 2048))
    # the regroup: grid passes and pair rounds
    assert (cc.GRID, cc.PAIR_ROUND) == (524288, 1024)
    assert cc.single_positions(16272) == [0, 15, 16, 1023, 1024, 2047, 2048, 16271]
    assert cc.single_positions(16416) == [0, 7, 8, 15, 16, 511, 512, 1023, 1024, 2047, 2048, 16415]
    assert cc.edge_tiles(cc.CELLS2 * 29128) == (0, 1022, 1023, 1024, 1025, 2048)
    assert cc.edge_tiles(cc.CELLS2 * 14563) == (0, 1022, 1023)


@pytest.mark.parametrize("n", [1, 144, 2047, 2048, 2049, 16272, 16416, 18432, 144 * 14564])
def test_every_pattern_has_the_survivor_count_it_claims(n):
    specs = cc.small_patterns(n) if n < 10 ** 5 else cc.large_patterns(n) + [("tile_first",), ("bytes",), ("none",), ("all",)]
    for spec in specs:
        f = cc.flags(spec, n, seed=3)
        assert f.dtype == np.uint8 and f.shape == (n,)
        idx, count = cc.compact_ref(f)
        assert count == cc.survivors(spec, n) == int((f == 0).sum()), spec
        assert np.array_equal(cc.flags(spec, n, seed=3), f)                                       # seeded
        if spec[0] == "single":
            assert idx.tolist() == [spec[1]]
        if spec[0] == "tile_last":
            assert np.array_equal(idx, np.arange(cc.T - 1, n, cc.T))
        if spec[0] == "tile_first":
            assert np.array_equal(idx, np.arange(0, n, cc.T))
        if spec[0] == "tiles":
            assert sorted(set((idx // cc.T).tolist())) == list(spec[1])
        if spec[0] == "bytes" and n >= 2048:
            assert set(np.unique(f).tolist()) == {0, 1, 2, 128, 255}
        if spec[0] != "bytes":
            assert set(np.unique(f).tolist()) <= {0, 1}
    idx, count = cc.compact_ref(cc.flags(("random", 0.5), n, 1), capacity=5)
    assert count == round(0.5 * n) and len(idx) == min(5, count)


@pytest.mark.parametrize("M,pairs,Cmax,boundary", [(0, 3, 3, None), (1, 1, 1, None), (1000, 3, 1, None), (5000, 1025, 3, 2500),
                                                   (cc.GRID + 1, 2049, 3, cc.GRID), (9, 5, 2, 4)])
def test_the_synthetic_match_rows_honour_the_regroup_precondition(M, pairs, Cmax, boundary):
    tab = cc.RowTable(pairs, Cmax)
    m = cc.run_lengths(M, pairs, Cmax, seed=5, boundary_at=boundary)
    assert m.shape == (Cmax, pairs) and m.sum() == M and (m >= 0).all()
    if pairs > 3:
        assert not m[:, [0, pairs // 2, pairs - 1]].any()
    if pairs > 1 and Cmax > 1 and M > 100:
        assert m[0, 1] == 0 and m[1, 1] > 0                      # empty in chunk 0, present in chunk 1
    rows = cc.match_rows(m)
    assert rows.dtype == np.int32 and rows.shape == (M,)
    if M:
        assert (np.diff(rows) >= 0).all() and rows.max() < tab.rows_cap
        chunk = np.searchsorted(tab.chunk_base, rows, side="right") - 1
        key = chunk * pairs + tab.pair_of_rows(rows)
        assert (np.diff(key) >= 0).all()                         # (chunk, pair) order, every run contiguous
        assert np.array_equal(np.bincount(key, minlength=Cmax * pairs), m.reshape(-1))
    if boundary is not None:
        assert key[boundary] != key[boundary - 1]
    order, off = cc.regroup_ref(tab.pair_of_rows(rows), pairs)
    assert off[0] == 0 and off[-1] == M and np.array_equal(np.diff(off), m.sum(0))
    assert np.array_equal(np.sort(order), np.arange(M))


@pytest.mark.parametrize("seed,B", [(11, 9), (12, 131)])
def test_the_numpy_compaction_agrees_with_the_oracle(oracle, seed, B):
    """The two checkers against each other: oracle.third_inputs' rows are the kept flags of compact_ref, oracle.get_result emits
    one match per kept sub-cell of the rows that have a surviving level-0 cell, and conf16_ref is the permutation
    oracle.refine_scatter applies to the points."""
    rng = np.random.default_rng(seed)
    f = cc.flags(("bytes",), B * cc.CELLS2, seed).reshape(B, cc.CELLS2)
    pts = rng.uniform(0.0, 12.0, (B, cc.CELLS2, 2)).astype(np.float32)
    mk0, mk1, b_ids = oracle.third_inputs(f, pts)
    idx, P = cc.compact_ref(f)
    assert mk0.shape == (P, 2) and np.array_equal(b_ids, idx // cc.CELLS2)
    cell = idx % cc.CELLS2
    assert np.array_equal(mk0, np.stack([(cell % 12 * 4 + 2) * 2.0, (cell // 12 * 4 + 2) * 2.0], 1).astype(np.float32))
    assert np.array_equal(mk1, (np.rint(pts.reshape(-1, 2)[idx][:, ::-1] * np.float32(4.0)) * np.float32(2.0)))
    conf = rng.random((P, 16)).astype(np.float32) + np.float32(0.5)
    label0 = np.where(rng.random(P * 16) < 0.2, -10.0, 1e8).astype(np.float32)
    f16, p16 = oracle.refine_scatter(f, pts, np.repeat(conf.reshape(P, 16, 1), 2, 2), label0)
    want = np.where(f16, np.float32(0.0), p16[:, :, 0])
    assert np.array_equal(cc.conf16_ref(f, conf, f16), want) and (want > 0).sum() == (~f16).sum() > 0
    # get_result: bs * h * w level-0 cells with exactly B survivors, the level-1 flags of above
    bs, h, w = 2, 5, (B + 6) // 7
    f0 = np.ones(bs * h * w, np.uint8)
    f0[rng.choice(f0.size, B, replace=False)] = 0
    f1 = cc.flags(("random", 0.5), B * cc.SUB, seed + 1).reshape(B, cc.SUB)
    ap0, sc0 = rng.random((bs, h * w, 2)).astype(np.float32), rng.random((bs, h * w, 2)).astype(np.float32)
    ap1, sc1 = rng.random((B, cc.SUB, 2)).astype(np.float32), rng.random((B, cc.SUB, 2)).astype(np.float32)
    ml, mr = oracle.get_result(bs, [f0.reshape(bs, -1), f1], [ap0, ap1], [sc0, sc1], [[32, h, w], [2, 48, 48]],
                               [np.array([1, 0], np.uint8), (rng.random(B) < 0.5).astype(np.uint8)])
    sub, M = cc.compact_ref(f1)
    assert ml.shape == (M, 2) and mr.shape == (M, 2)
    # with left_choice set at both levels the left point of a match depends on its sub-cell and its row's cell alone
    ml1, _ = oracle.get_result(bs, [f0.reshape(bs, -1), f1], [ap0, ap1], [sc0, np.ones_like(sc1)], [[32, h, w], [2, 48, 48]],
                               [np.ones(2, np.uint8), np.ones(B, np.uint8)])
    cell0, _ = cc.compact_ref(f0)
    e, j = cell0[sub // cc.SUB], sub % cc.SUB
    i = e % (h * w)
    want_y = (i // w * 32 + 16.0 - 1.5 * sc0.reshape(-1, 2)[e, 1].astype(np.float64) * 32) + (j // 48 * 2 + 1.0)
    np.testing.assert_allclose(ml1[:, 0], want_y, rtol=1e-5, atol=1e-3)
