"""The order-preserving compactions of pats_amd/csrc/merge.hip restated in numpy, with the sizes and flag patterns that reach every
path of their exclusive scan and of the regroup by pair.  Shared by tests/test_compaction_cases_host.py (CPU) and
tests/test_compaction_edges_gpu.py; imports without a GPU (numpy only).

The scan (run_scan) takes one of three paths by the flag count n:
    n <= SCAN_SMALL                      scan_small_kernel alone: one workgroup, SMALL_GROUP flags a thread, tile bases zeroed
    up to TILE_ROUND tiles of SCAN_TILE  scan_flags_kernel (FLAGS_GROUP flags a thread), then ONE round of scan_tiles_kernel
    more tiles                           scan_tiles_kernel walks rounds of TILE_ROUND tiles and hands a carry through LDS
and the regroup (bypair_runs / _offsets / _copy) walks its matches with a grid of REGROUP_GRID threads and its pairs in rounds of
PAIR_ROUND.  Every constant is parsed out of the source (source_constants) and every size below is derived from the parsed values:
a changed constant moves the cases with it.

A flag byte means "dropped" when it is non-zero: keep == (flag == 0), whatever the non-zero value."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_HIP = os.path.join(REPO, "pats_amd", "csrc", "merge.hip")
CELLS2, SUB = 144, 2304         # flags per level-2 row (12 x 12 cells) and per level-1 row of get_result (48 x 48 sub-cells)
WAVE = 64


def source_constants(text=None):
    """-> dict of the constants the cases hang on, read from merge.hip (every pattern must match exactly once or agree)."""
    src = open(MERGE_HIP).read() if text is None else text

    def one(pattern):
        found = re.findall(pattern, src)
        assert len(set(found)) == 1, "merge.hip: %r matched %r" % (pattern, found)
        return found[0]
    tile = int(one(r"constexpr int SCAN_TILE = (\d+);"))
    small = int(one(r"constexpr int SCAN_SMALL = (\d+);"))
    tile_round = int(one(r"for \(int b0 = 0; b0 < tiles; b0 \+= (\d+)\)"))
    assert int(one(r"hipLaunchKernelGGL\(scan_tiles_kernel, dim3\(1\), dim3\((\d+)\)")) == tile_round
    small_threads = int(one(r"hipLaunchKernelGGL\(scan_small_kernel, dim3\(1\), dim3\((\d+)\)"))
    flags_threads = int(one(r"hipLaunchKernelGGL\(scan_flags_kernel, dim3\(\(unsigned\)tiles\), dim3\((\d+)\)"))
    pair_round = int(one(r"for \(int64_t p0 = 0; p0 < P; p0 \+= (\d+)\)"))
    grid = one(r"hipLaunchKernelGGL\(bypair_(?:runs|copy|copy_conf)_kernel, dim3\((\d+)\), dim3\((\d+)\)")
    return {"SCAN_TILE": tile, "SCAN_SMALL": small, "TILE_ROUND": tile_round, "PAIR_ROUND": pair_round,
            "REGROUP_BLOCKS": int(grid[0]), "REGROUP_THREADS": int(grid[1]), "REGROUP_GRID": int(grid[0]) * int(grid[1]),
            "SMALL_GROUP": small // small_threads, "FLAGS_GROUP": tile // flags_threads}


K = source_constants()
T, SMALL, ROUND = K["SCAN_TILE"], K["SCAN_SMALL"], K["TILE_ROUND"]
GRID, PAIR_ROUND = K["REGROUP_GRID"], K["PAIR_ROUND"]
SMALL_GROUP, FLAGS_GROUP = K["SMALL_GROUP"], K["FLAGS_GROUP"]


def tiles_of(n):
    return (n + T - 1) // T


def scan_path(n):
    """-> (tiles, rounds of scan_tiles_kernel): 0 rounds = the single-workgroup path."""
    return tiles_of(n), (0 if n <= SMALL else (tiles_of(n) + ROUND - 1) // ROUND)


def describe(what, n):
    tiles, rounds = scan_path(n)
    return "%s: n = %d flags, %d tiles, %s" % (what, n, tiles, "single workgroup" if rounds == 0 else "%d round(s)" % rounds)


def _rows_for(per_row):
    """Row counts whose per_row * rows flags sit on either side of every path change: 1, the last single-workgroup count, the
    first two-level one, TILE_ROUND tiles (one round, ragged last tile), TILE_ROUND + 1 tiles, 2 TILE_ROUND + 1 tiles."""
    last_small = SMALL // per_row
    one_round = ROUND * T // per_row
    return {"one": 1, "small_last": last_small, "two_level_first": last_small + 1, "one_round": one_round,
            "two_rounds": one_round + 1, "three_rounds": 2 * ROUND * T // per_row + 1}


def _full_tiles_rows(per_row, above):
    """The smallest row count above `above` whose flags fill whole tiles."""
    step = T // np.gcd(per_row, T)
    return int((above // step + 1) * step)


B144 = _rows_for(CELLS2)                                   # 1, 113, 114, 14 563, 14 564, 29 128
B144["full_tiles"] = _full_tiles_rows(CELLS2, B144["two_level_first"])          # 128: exactly 9 full tiles
B_SMALL = (B144["one"], B144["small_last"], B144["two_level_first"], B144["full_tiles"])
B_LARGE = (B144["one_round"], B144["two_rounds"], B144["three_rounds"])
ROWS1 = _rows_for(SUB)                                     # 1, 7, 8, 910, 911, 1 821
R_SMALL = (ROWS1["one"], ROWS1["small_last"], ROWS1["two_level_first"])
R_LARGE = (ROWS1["one_round"], ROWS1["two_rounds"], ROWS1["three_rounds"])

# level-0 cell counts (batch * h * w, any n): around the thread group, the tile, the single-workgroup limit, and past one round
CELLS0 = (1, SMALL_GROUP - 1, SMALL_GROUP + 1, T - 1, T + 1, SMALL - 1, SMALL, SMALL + 1, (ROUND + 32) * T)
_PREFERRED = ((3, 43, 127), (4, 64, 64), (5, 29, 113), (33, 256, 256))


def grid_of(n):
    """(batch, h, w) with batch * h * w == n: a listed grid when one fits, else the smallest batch whose h, w stay <= 256,
    else one row of n cells."""
    for g in _PREFERRED:
        if g[0] * g[1] * g[2] == n:
            return g
    for b in range(1, 65):
        if n % b:
            continue
        m = n // b
        for h in range(int(np.sqrt(m)), 0, -1):
            if m % h == 0 and m // h <= 256:
                return (b, h, m // h)
    return (1, 1, n)


def boundary_cells(n):
    """About a dozen positions in [0, n): the first and last flag and both sides of every thread-group, wave, tile and round
    boundary of the path n takes, as far as they fit."""
    group = SMALL_GROUP if n <= SMALL else FLAGS_GROUP
    edges = [group, WAVE * group, T]
    if n > SMALL:
        edges += [2 * T, ROUND * T]
    pos = {0, n - 1}
    for e in edges:
        pos.update(p for p in (e - 1, e) if 0 <= p < n)
    return np.array(sorted(pos), np.int64)


# ---- flag patterns: spec = (name, *args); flags(spec, n, seed) -> uint8 [n], survivors(spec, n) -> the count it claims ----------
def single_positions(n):
    """single(i) positions for a 144-flag consumer of n flags: thread-group and wave edges of scan_small_kernel, plus those of
    scan_flags_kernel on the two-level path."""
    pos = [0, SMALL_GROUP - 1, SMALL_GROUP, WAVE * SMALL_GROUP - 1, WAVE * SMALL_GROUP, T - 1, T, n - 1]
    if n > SMALL:
        pos += [FLAGS_GROUP - 1, FLAGS_GROUP, WAVE * FLAGS_GROUP - 1, WAVE * FLAGS_GROUP]
    return sorted({p for p in pos if 0 <= p < n})


def edge_tiles(n):
    """tiles({0, ROUND - 2, ROUND - 1, ROUND, ROUND + 1, last}) clipped to the tiles n has."""
    last = tiles_of(n) - 1
    return tuple(sorted({t for t in (0, ROUND - 2, ROUND - 1, ROUND, ROUND + 1, last) if 0 <= t <= last}))


def small_patterns(n):
    specs = [("none",), ("all",), ("random", 0.02), ("random", 0.5), ("random", 0.98), ("tile_last",), ("tile_first",),
             ("tiles", tuple(sorted({0, tiles_of(n) - 1}))), ("bytes",)]
    return specs + [("single", i) for i in single_positions(n)]


def large_patterns(n):
    return [("random", 0.5), ("random", 0.02), ("tile_last",), ("tiles", edge_tiles(n)), ("single", n - 1)]


def spec_id(spec):
    return "-".join(str(x) if not isinstance(x, tuple) else "x".join(map(str, x)) for x in spec)


def _keep(spec, n, rng):
    name = spec[0]
    keep = np.zeros(n, bool)
    if name == "none":
        pass
    elif name == "all":
        keep[:] = True
    elif name in ("random", "bytes"):                         # exactly round(p n) survivors at random places
        p = spec[1] if name == "random" else 0.5
        keep[rng.choice(n, int(round(p * n)), replace=False)] = True
    elif name == "single":
        keep[spec[1]] = True
    elif name == "tile_last":
        keep[T - 1::T] = True
    elif name == "tile_first":
        keep[::T] = True
    elif name == "tiles":
        for t in spec[1]:
            keep[t * T:(t + 1) * T] = True
    else:
        raise ValueError(spec)
    return keep


def flags(spec, n, seed=0):
    """uint8 [n]: 0 = kept; a dropped flag is 1, or one of 1, 2, 128, 255 at random for the `bytes` pattern."""
    rng = np.random.default_rng([seed, n])
    keep = _keep(spec, n, rng)
    f = np.ones(n, np.uint8)
    if spec[0] == "bytes":
        f = np.array([1, 2, 128, 255], np.uint8)[rng.integers(0, 4, n)]
    f[keep] = 0
    return f


def survivors(spec, n):
    name = spec[0]
    if name in ("random", "bytes"):
        return int(round((spec[1] if name == "random" else 0.5) * n))
    if name == "tiles":
        return sum(min(T, n - t * T) for t in spec[1])
    return {"none": 0, "all": n, "single": 1, "tile_last": n // T, "tile_first": tiles_of(n)}[name]


# ---- plain numpy references ---------------------------------------------------------------------------------------------------------
def compact_ref(f, capacity=None):
    """-> (indices of the kept flags in order, cut to `capacity`; their count before the cut)."""
    idx = np.flatnonzero(np.asarray(f).reshape(-1) == 0)
    return (idx if capacity is None else idx[:capacity]), int(idx.size)


def regroup_ref(pair, pairs):
    """-> (stable order of the matches by pair, offsets [pairs + 1])."""
    pair = np.asarray(pair, np.int64)
    order = np.argsort(pair, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(pair, minlength=pairs))]).astype(np.int64)
    return order, off


_SUB_OFF = np.array([(s // 4) * 48 + s % 4 for s in range(16)], np.int64)


def conf16_ref(f, conf, f16):
    """refine_scatter's conf16 [B,2304]: conf [P,16] of the kept cells by the permutation pts16 gets, 0 where f16 is set."""
    f = np.asarray(f).reshape(-1, CELLS2)
    idx, _ = compact_ref(f)
    b, cell = idx // CELLS2, idx % CELLS2
    base = b * SUB + (cell // 12) * 4 * 48 + (cell % 12) * 4
    out = np.zeros(f.shape[0] * SUB, np.float32)
    out[(base[:, None] + _SUB_OFF[None, :]).reshape(-1)] = np.asarray(conf, np.float32).reshape(-1)
    out[np.asarray(f16).reshape(-1) != 0] = 0.0
    return out.reshape(-1, SUB)


# ---- a synthetic row table for ops.matches_by_pair ----------------------------------------------------------------------------------
ROWS_PER_RUN = 2


class RowTable:
    """What ops.matches_by_pair reads of an ops.ChunkRows: pairs, h, w, Cmax, table = None, row_cell, chunk_base, status (numpy here;
    on_device(to) replaces the arrays by what `to` makes of them).  Every (chunk, pair) owns ROWS_PER_RUN rows, in (chunk, pair,
    cell) order like the planner's: row (c * pairs + p) * ROWS_PER_RUN + j holds cell j of pair p."""

    def __init__(self, pairs, Cmax, status=0):
        self.pairs, self.Cmax, self.h, self.w, self.table = int(pairs), int(Cmax), 1, ROWS_PER_RUN, None
        N = self.h * self.w
        run = np.arange(self.Cmax * self.pairs, dtype=np.int64)
        self.row_cell = ((run % self.pairs)[:, None] * N + np.arange(ROWS_PER_RUN)[None, :]).reshape(-1).astype(np.int32)
        self.chunk_base = (np.arange(self.Cmax + 1, dtype=np.int64) * self.pairs * ROWS_PER_RUN)
        self.status = np.array([status], np.int32)
        self.rows_cap = int(self.row_cell.size)

    def on_device(self, to):
        import copy
        r = copy.copy(self)
        r.row_cell, r.chunk_base, r.status = to(self.row_cell), to(self.chunk_base), to(self.status)
        return r

    def pair_of_rows(self, match_row):
        return self.row_cell[np.asarray(match_row, np.int64)].astype(np.int64) // (self.h * self.w)


def run_lengths(M, pairs, Cmax, seed, boundary_at=None):
    """Match counts [Cmax, pairs] summing to M.  Pairs 0, pairs // 2 and pairs - 1 match nothing (when there are more than three
    pairs); pair 1 is empty in chunk 0 and present in chunk 1 (when both exist and M allows); about a third of the other runs are
    empty.  boundary_at (0 < boundary_at < M): a run starts exactly at that match index."""
    rng = np.random.default_rng([seed, M, pairs, Cmax])
    dense = rng.random((Cmax, pairs)) + 0.01
    w = dense * (rng.random((Cmax, pairs)) < 0.67)
    for a in (dense, w):
        if pairs > 3:
            a[:, [0, pairs // 2, pairs - 1]] = 0.0
        if pairs > 1 and Cmax > 1:
            a[0, 1], a[1, 1] = 0.0, 1.0
    if np.count_nonzero(w) < 2:                                # too few runs left to thin out
        w = dense
    w = w.reshape(-1)
    live = np.flatnonzero(w)

    def deal(total, sel):
        out = np.zeros(w.size, np.int64)
        if total:
            out[sel] = rng.multinomial(total, w[sel] / w[sel].sum())
        return out
    if boundary_at is None or not 0 < boundary_at < M or live.size < 2:
        m = deal(M, live)
    else:
        s = live[live.size // 2]                               # the run that starts at boundary_at
        m = deal(boundary_at, live[live < s]) + deal(M - boundary_at - 1, live[live >= s])
        m[s] += 1
    assert m.sum() == M
    return m.reshape(Cmax, pairs)


def match_rows(lengths):
    """match_row [M] int32 into a RowTable's rows, honouring the precondition of the regroup: matches in (chunk, pair, row) order,
    every (chunk, pair) one contiguous run - the first half of a run on the run's first row, the rest on its second."""
    m = np.asarray(lengths, np.int64).reshape(-1)
    run = np.repeat(np.arange(m.size, dtype=np.int64), m)
    start = np.concatenate([[0], np.cumsum(m)])[:-1]
    within = np.arange(run.size, dtype=np.int64) - start[run]
    return (run * ROWS_PER_RUN + (2 * within >= m[run])).astype(np.int32)
