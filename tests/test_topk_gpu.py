"""GPU: ops.topk_by_pair / batch.topk_by_pair against the definition of include/pats_amd.h, computed with numpy inside the test:
    key   = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000), b = the bits of the confidence
    order = np.lexsort((np.arange(n), ~key)) restricted to the eligible matches (key >= key(min_conf)), then the first K
Every comparison is exact: top_idx / top_count as integers, top_conf / top_l / top_r as bits.  The definition is total (rows past
the count are -1 / 0.0), so whole output buffers are compared.

Synthetic cases: matches_l[g] = (g, -g), matches_r[g] = (g + 0.5, 2g) for global row g (a copy from a wrong row cannot pass); the
arrays are longer than pair_off[pairs] and the rows behind it hold conf = 2.0 (never to be selected); the five outputs are views
into larger canary-filled buffers whose surroundings must come back untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY_F = -777.25
CANARY_I = -123456
PAD = 64            # canary elements on each side of an output view (even: the float2 outputs stay 8-byte aligned)
TAIL = 37           # input rows behind pair_off[pairs]


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.fixture(scope="module")
def max_k(ops):
    return ops.topk_max_k()


def key_of(conf):
    b = np.ascontiguousarray(conf, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def reference(ml, mr, conf, off, K, min_conf=None):
    """The definition, on host arrays: the five outputs in full."""
    pairs = len(off) - 1
    tl, tr = np.zeros((pairs, K, 2), np.float32), np.zeros((pairs, K, 2), np.float32)
    tc, ti, tn = np.zeros((pairs, K), np.float32), np.full((pairs, K), -1, np.int32), np.zeros((pairs,), np.int64)
    for p in range(pairs):
        lo, hi = int(off[p]), int(off[p + 1])
        n = max(hi - lo, 0)
        key = key_of(conf[lo:lo + n])
        order = np.lexsort((np.arange(n), ~key))
        if min_conf is not None:
            order = order[key[order] >= key_of(np.float32(min_conf).reshape(1))[0]]
        order = order[:K]
        c = len(order)
        tn[p] = c
        ti[p, :c] = order
        tl[p, :c], tr[p, :c], tc[p, :c] = ml[lo + order], mr[lo + order], conf[lo + order]
    return tl, tr, tc, ti, tn


def make_inputs(lengths, conf):
    """conf: the confidences of all pairs, concatenated (sum(lengths) float32)."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(off[-1]) + TAIL
    g = np.arange(total, dtype=np.float32)
    ml, mr = np.stack([g, -g], 1), np.stack([g + 0.5, 2 * g], 1)
    cf = np.concatenate([np.asarray(conf, np.float32), np.full(TAIL, 2.0, np.float32)])
    assert cf.shape == (total,) and total < (1 << 24)           # the row numbers are exact floats
    return ml, mr, cf, off


def canary_outputs(pairs, K):
    """Five output views inside larger canary-filled buffers -> (views, whole buffers)."""
    dev = "cuda"
    shapes = ((pairs, K, 2), (pairs, K, 2), (pairs, K), (pairs, K), (pairs,))
    dts = (torch.float32, torch.float32, torch.float32, torch.int32, torch.int64)
    views, whole = [], []
    for shape, dt in zip(shapes, dts):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), CANARY_F if dt == torch.float32 else CANARY_I, dtype=dt, device=dev)
        whole.append(buf)
        views.append(buf[PAD:PAD + n].view(shape))
    return tuple(views), whole


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def run(ops, ml, mr, cf, off, K, min_conf=None, pair_off=None, pairs=None):
    """One call on fresh canary buffers; checks the canaries, returns the five outputs as numpy arrays."""
    d = [torch.from_numpy(x).cuda() for x in (ml, mr, cf)]
    po = torch.from_numpy(off).cuda() if pair_off is None else pair_off
    npairs = len(off) - 1
    views, whole = canary_outputs(npairs, K)
    got = ops.topk_by_pair(d[0], d[1], d[2], po, K, min_conf=min_conf, out=views, pairs=pairs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, views))
    for buf in whole:
        edge = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
        assert bool((edge == (CANARY_F if buf.dtype == torch.float32 else CANARY_I)).all()), "bytes around an output view changed"
    return [v.cpu().numpy() for v in views]


def check(ops, lengths, conf, K, min_conf=None, **kw):
    ml, mr, cf, off = make_inputs(lengths, conf)
    got = run(ops, ml, mr, cf, off, K, min_conf, **kw)
    want = reference(ml, mr, cf, off, K, min_conf)
    for name, g, w in zip(("top_l", "top_r", "top_conf", "top_idx", "top_count"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(bits(g), bits(w)), "%s differs (K = %d, lengths %s)" % (name, K, list(lengths))
    return got


def rand_conf(rng, n):
    """Confidences as the third level makes them: float32 in (0, 1], clustered near the top, with repeated values."""
    c = 1.0 - rng.random(n, dtype=np.float32) ** 3
    c[rng.random(n) < 0.2] = np.float32(0.75)
    return c.astype(np.float32)


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def _K(k, max_k):
    return max_k if k == "max" else k


@pytest.mark.parametrize("k", [1, 2, 64, 1000, "max"])
def test_segment_lengths_against_K_and_the_workgroup(ops, max_k, k):
    K = _K(k, max_k)
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, K - 1, K, K + 1, 3 * K + 7]
    rng = np.random.default_rng(100 + K)
    check(ops, lengths, rand_conf(rng, sum(lengths)), K)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_empty_pair_first_middle_and_last(ops, max_k, where):
    lengths = {"first": [0, 300, 5000], "middle": [300, 0, 5000], "last": [5000, 300, 0]}[where]
    rng = np.random.default_rng(7)
    check(ops, lengths, rand_conf(rng, sum(lengths)), 100)


@pytest.mark.parametrize("n", [0, 1, 700, 9000])
def test_one_pair(ops, n):
    rng = np.random.default_rng(8 + n)
    check(ops, [n], rand_conf(rng, n), 64)


@pytest.mark.parametrize("k", [1000, "max"])
def test_segments_longer_than_lds_holds_and_two_runs_agree(ops, max_k, k):
    K = _K(k, max_k)
    lengths = [max(40000, 9 * max_k + 3136), max(20000, 4 * max_k + 3616)]
    assert min(lengths) > max_k
    rng = np.random.default_rng(11)
    conf = rand_conf(rng, sum(lengths))
    first = check(ops, lengths, conf, K)
    ml, mr, cf, off = make_inputs(lengths, conf)
    second = run(ops, ml, mr, cf, off, K)                    # fresh output buffers
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, second))


def test_summary_buffer_as_pair_off(ops):
    """pairs= given: pair_off may be the longer summary buffer (offsets, then M, P, status)."""
    lengths = [500, 0, 6000]
    rng = np.random.default_rng(12)
    conf = rand_conf(rng, sum(lengths))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    summary = torch.from_numpy(np.concatenate([off, [off[-1], 12345, 0]]).astype(np.int64)).cuda()
    check(ops, lengths, conf, 300, pair_off=summary, pairs=3)


def test_corrupt_offsets_stay_inside_the_arrays(ops):
    """Offsets past cap, negative and descending: clamped to [0, cap], hi <= lo is an empty pair (the definition on the clamped
    offsets); nothing outside the arrays is read, nothing outside the outputs written."""
    lengths = [400, 400, 400]
    rng = np.random.default_rng(13)
    ml, mr, cf, off = make_inputs(lengths, rand_conf(rng, 1200))
    cap = cf.shape[0]
    bad = np.array([-50, 700, 300, cap + 100000], np.int64)
    got = run(ops, ml, mr, cf, off, 50, pair_off=torch.from_numpy(bad).cuda())
    want = reference(ml, mr, cf, np.clip(bad, 0, cap), 50)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
    assert got[4].tolist() == [50, 0, 50]


# ---- ranking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [900, 7000])                  # the whole-segment sort and the radix select
def test_all_equal_gives_the_first_K_indices(ops, n):
    got = check(ops, [n, n + 1], np.full(2 * n + 1, 0.625, np.float32), 200)
    assert np.array_equal(got[3][0], np.arange(200)) and np.array_equal(got[3][1], np.arange(200))


@pytest.mark.parametrize("n", [900, 7000])
def test_four_values_with_the_kth_rank_inside_a_run_of_equals(ops, n):
    rng = np.random.default_rng(21 + n)
    vals = np.array([0.2, 0.4, 0.6, 0.8], np.float32)
    conf = vals[rng.integers(0, 4, 2 * n)]
    K = 3 * n // 8                                          # a quarter of the keys hold each value
    for p in range(2):                                      # the K-th rank falls inside the second-highest value's run
        c = conf[p * n:(p + 1) * n]
        assert (c == vals[3]).sum() < K < (c >= vals[2]).sum()
    check(ops, [n, n], conf, K)


@pytest.mark.parametrize("n", [900, 7000])
@pytest.mark.parametrize("above", ["K", "K-1"])
def test_exactly_K_and_K_minus_1_above_a_plateau(ops, n, above):
    K = 128
    m = K if above == "K" else K - 1
    rng = np.random.default_rng(31 + n)
    conf = np.full(n, 0.5, np.float32)
    where = rng.choice(n, m, replace=False)
    conf[where] = (0.5 + 0.4 * rng.random(m)).astype(np.float32) + np.float32(0.01)
    assert (conf > 0.5).sum() == m
    got = check(ops, [n], conf, K)
    if above == "K-1":
        assert got[3][0, K - 1] == np.flatnonzero(conf == 0.5)[0]            # the plateau's first index takes the last rank


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_every_radix_digit_decides(ops, d):
    """All keys agree except in byte d of the float's bits: a select that drops or mis-orders that pass fails this input alone."""
    n, K = 6000, 100                                        # longer than the sort buffer: the select runs
    rng = np.random.default_rng(40 + d)
    base = np.uint32(0x3F2A5C7E)                            # 0.6654...: a confidence-like value
    digit = rng.integers(0, 256, 2 * n).astype(np.uint32)
    if d == 3:
        digit = digit & np.uint32(0x7F)                     # non-negative floats: the sign bit stays clear
        digit = np.where(digit == 0x7F, np.uint32(0x3E), digit).astype(np.uint32)    # and no NaN / inf exponents with random mantissas
    b = (base & ~np.uint32(0xFF << (8 * d))) | (digit << np.uint32(8 * d))
    check(ops, [n, n], b.astype(np.uint32).view(np.float32), K)
    check(ops, [n, n], b.astype(np.uint32).view(np.float32), K, min_conf=float(np.uint32(base).reshape(1).view(np.float32)[0]))


@pytest.mark.parametrize("n", [64, 5000])
def test_value_edges_follow_the_key_order(ops, n):
    edges = np.array([0.0, np.float32(1e-45), 1.0, np.nextafter(np.float32(1), np.float32(0)), np.inf], np.float32)
    nan = np.array([0x7FC00001], np.uint32).view(np.float32)                 # a positive NaN
    rng = np.random.default_rng(50 + n)
    conf = np.clip(rand_conf(rng, n), np.float32(0.01), np.float32(0.99))     # the edge values appear once each
    spots = rng.choice(n, 6, replace=False)
    conf[spots] = np.concatenate([edges, nan])
    got = check(ops, [n], conf, 16)
    assert got[3][0, :4].tolist() == [spots[5], spots[4], spots[2], spots[3]]          # NaN, +inf, 1.0, nextafter(1, 0)
    got = check(ops, [n], conf, n if n <= 4096 else 4096)
    if n == 64:
        assert got[3][0, -2:].tolist() == [spots[1], spots[0]]                         # the denormal above 0.0, at the very end


# ---- threshold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [800, 7000])
def test_thresholds(ops, n):
    rng = np.random.default_rng(60 + n)
    lengths = [n, 0, n // 2]
    conf = rand_conf(rng, sum(lengths))
    uniq = np.unique(conf)
    at, nxt = uniq[len(uniq) // 2], uniq[len(uniq) // 2 + 1]
    between = np.float32((np.float64(at) + np.float64(nxt)) / 2)
    assert at < between < nxt or between in (at, nxt)
    for K in (100, 4096):
        check(ops, lengths, conf, K, min_conf=None)
        got = check(ops, lengths, conf, K, min_conf=float(at))                 # inclusive: the element itself is kept
        if K == 4096 and n == 800:
            assert got[4][0] == (conf[:n] >= at).sum() and at in got[2][0]
        check(ops, lengths, conf, K, min_conf=float(between))
        check(ops, lengths, conf, K, min_conf=0.75)                            # the value a fifth of the matches share
        got = check(ops, lengths, conf, K, min_conf=float(conf.max()) + 0.5)   # above the maximum (below the tail rows' 2.0)
        assert got[4].tolist() == [0, 0, 0] and (got[3] == -1).all() and not got[0].any() and not got[1].any() and not got[2].any()


def test_nan_threshold_is_refused(ops):
    ml, mr, cf, off = make_inputs([10], np.full(10, 0.5, np.float32))
    with pytest.raises(RuntimeError, match="min_conf"):
        run(ops, ml, mr, cf, off, 4, min_conf=float("nan"))
    with pytest.raises(RuntimeError, match="min_conf"):
        run(ops, ml, mr, cf, off, 4, min_conf=-0.5)


def test_empty_arrays_define_every_output(ops):
    """cap == 0: every pair empty, the outputs still defined."""
    z2, z1 = torch.empty((0, 2), device="cuda"), torch.empty((0,), device="cuda")
    views, whole = canary_outputs(3, 5)
    ops.topk_by_pair(z2, z2, z1, torch.zeros(4, dtype=torch.int64, device="cuda"), 5, out=views)
    assert not views[0].any() and not views[1].any() and not views[2].any() and bool((views[3] == -1).all()) and not views[4].any()


def test_wrong_dtypes_and_non_contiguous_tensors_are_refused(ops):
    ml, mr, cf, off = [torch.from_numpy(x).cuda() for x in make_inputs([10], np.full(10, 0.5, np.float32))]
    with pytest.raises(RuntimeError):
        ops.topk_by_pair(ml.double(), mr, cf, off, 4)
    with pytest.raises(RuntimeError):
        ops.topk_by_pair(ml, mr, cf, off.int(), 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.topk_by_pair(ml, mr, torch.stack([cf, cf], 1)[:, 0], off, 4)
    with pytest.raises(RuntimeError):
        ops.topk_by_pair(ml, mr, cf, off, ops.topk_max_k() + 1)


# ---- pipeline -----------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.cpu().numpy()


def ops_max_k():
    from pats_amd import ops
    return ops.topk_max_k()


@pytest.mark.parametrize("mixed", [False, True])
def test_end_to_end_and_nothing_else_moved(mixed):
    from pats_amd import batch
    from test_confidence_gpu import _small_batch
    _, cap, out, _ = _small_batch(mixed)
    _, _, ref_out, _ = _small_batch(mixed)                   # a second, identical run: the full lists
    lists = batch.split_by_pair(ref_out, cap)                # caller's order for the mixed pack
    assert all(len(x) == 3 and x[0].shape[0] > 100 for x in lists)
    biggest = max(x[0].shape[0] for x in lists)
    assert biggest + 9 <= ops_max_k()
    before = {k: out[k].clone() for k in ("matches_l", "matches_r", "match_conf")}
    for n_call, K in enumerate((50, biggest + 9)):
        top = batch.topk_by_pair(out, cap, K)
        assert top is out["topk"] and top[0].shape == (cap.pairs, K, 2) and top[3].dtype == torch.int32
        if n_call == 0:                                      # topk_by_pair did the regroup: one buffer, summary then counts
            assert out["topk_summary"].shape == (2 * cap.pairs + 4,)
            assert torch.equal(out["topk_summary"][:cap.pairs + 4], out["summary"]) and torch.equal(out["summary"], ref_out["summary"])
            assert top[4].data_ptr() == out["topk_summary"][cap.pairs + 4:].data_ptr()
            by_pair = [t.clone() for t in out["by_pair"]]
        assert torch.equal(out["topk_summary"][cap.pairs + 4:], top[4])
        got = batch.split_topk_by_pair(out, cap)
        for p, (l, r, c) in enumerate(lists):
            n = l.shape[0]
            order = np.lexsort((np.arange(n), ~key_of(_host(c))))[:K]
            gl, gr, gc, gi = got[p]
            assert gi.dtype == torch.int32 and np.array_equal(_host(gi), order), (p, K)
            assert np.array_equal(bits(_host(gl)), bits(_host(l)[order])) and np.array_equal(bits(_host(gr)), bits(_host(r)[order]))
            assert np.array_equal(bits(_host(gc)), bits(_host(c)[order]))
            assert len(order) == min(K, n) and (K == 50 or len(order) == n)
        # nothing else moved
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(by_pair[:2] + by_pair[3:], out["by_pair"][:2] + out["by_pair"][3:]))
        assert torch.equal(by_pair[2], out["by_pair"][2])
        assert all(torch.equal(before[k].view(torch.int32), out[k].view(torch.int32)) for k in before)
    if mixed:
        assert out["caller_of"] != list(range(cap.pairs))    # the slots are not the caller's order: the comparison above saw it
    # after a regroup of the caller's own: top_count is a tensor of its own, two copies at the hand-over
    own = {k: v for k, v in ref_out.items() if k != "topk"}
    assert "by_pair" in own and "topk_summary" not in own
    top = batch.topk_by_pair(own, cap, 50, min_conf=0.5)
    assert "topk_summary" not in own and top[4].shape == (cap.pairs,)
    for p, (l, r, c) in enumerate(lists):
        ch = _host(c)
        order = np.lexsort((np.arange(len(ch)), ~key_of(ch)))
        order = order[ch[order] >= 0.5][:50]
        assert np.array_equal(_host(batch.split_topk_by_pair(own, cap)[p][3]), order)
