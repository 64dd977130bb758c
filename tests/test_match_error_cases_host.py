"""CPU-only: the match-error stage's float64 restatement (tests/match_error_cases.py) against what the definition implies, and what the
C entry refuses before any launch.
    statuses     every status value 0 .. 6 occurs in the cases, and the builder's margins hold
    offsets      a scored match whose right point is the exact projection plus a known offset has err within 1e-3 px of the offset's
                 length: 4 float32 ulps of a 2048 px coordinate - the rounding of the stored right point and of the lifted X
    epipolar     the distance of the right point from the ground truth's epipolar line (the reference's get_pose_error `result`) is
                 <= err + 1e-3 px: the projection lies on that line, so the stage is at least as strict as the existing yardstick
    frames       swapped = 1 equals swapped = 0 with a ground truth conjugated beforehand, bit for bit
    consistency  an edge at 0 reproduces tally[:, 1] and correct; every row of confusion sums to tally[:, 1]
    refusals     pats_match_error_by_pair_f64 through ctypes with made-up addresses (tests/test_host_refusals.py's way): every item of
                 the header's "refused before any launch" is turned away, with the message that names it"""
import ctypes

import numpy as np
import pytest

import match_error_cases as mc

LENGTHS = (0, 1, 511, 512, 513, 1300)


@pytest.fixture(scope="module")
def batch():
    return mc.make_batch(LENGTHS, 900)


@pytest.fixture(scope="module")
def full(batch):
    return mc.reference_of(batch, min_conf=mc.MIN_CONF, edges=mc.EDGES, mask=batch["mask"])


def test_every_status_occurs_and_the_margins_hold(batch, full):
    mc.assert_margins(full, batch["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    assert set(np.unique(full["status"])) == set(range(7)), np.bincount(full["status"])
    assert (full["tally"][:, 7] == 0).all() and (full["tally"].sum(1) == np.array(LENGTHS)).all()
    print("rows per status:", full["tally"].sum(0)[:7])
    # the same without the options that can only take matches away: still decided, and more are scored
    bare = mc.reference_of(batch, depths_r=None, size_r=None)
    mc.assert_margins(bare, batch["conf"])
    assert set(np.unique(bare["status"])) == {0, 1, 2, 3} and bare["tally"][:, 1].sum() > full["tally"][:, 1].sum()
    nomap = mc.reference_of(batch, depths_r=[None] * len(LENGTHS), size_r=None)
    assert np.array_equal(nomap["status"], bare["status"])


def test_known_offsets(batch, full):
    sc = full["status"] == 1
    gap = np.abs(full["err"][sc] - batch["delta"][sc])
    print("scored %d, largest | err - |delta| | = %.3g px" % (sc.sum(), gap.max()))
    assert sc.sum() > 500 and gap.max() <= 1e-3
    assert (batch["delta"][sc] == 0).sum() > 20                                   # exact matches among them: err is the rounding alone


def test_epipolar_bound(batch, full):
    worst = -np.inf
    for (lo, n), c in zip(batch["segs"], batch["pairs"]):
        sl = slice(lo, lo + n)
        sc = full["status"][sl] == 1
        d = mc.epipolar_distance(batch["ml"][sl][sc], batch["mr"][sl][sc], c["norm"], c["R"], c["t"])
        over = d - full["err"][sl][sc]
        worst = max(worst, over.max(initial=-np.inf))
        assert (over <= 1e-3).all()
    print("largest epipolar distance - err = %.3g px" % worst)


def test_frame_equivalence(batch):
    a = mc.reference_of(batch)                                                    # swapped = 1, the extrinsics' frame
    T1 = np.tile(np.eye(4), (len(LENGTHS), 1, 1))
    for k, c in enumerate(batch["pairs"]):
        R, t = mc.pc.ground_truth64(c["T1"], c["T0"])
        T1[k, :3, :3], T1[k, :3, 3] = mc.conjugate(R, t)
    b = mc.reference_of(batch, T1=T1, T0=None, swapped=False)
    for key in ("status", "tally", "correct"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["err"], b["err"], equal_nan=True) and np.array_equal(a["err_sum"], b["err_sum"])


def test_internal_consistency(batch):
    r = mc.reference_of(batch, edges=(0.0,), mask=batch["mask"])
    assert np.array_equal(r["sweep"][:, 0, 0], r["tally"][:, 1]) and np.array_equal(r["sweep"][:, 0, 1:], r["correct"])
    assert np.array_equal(r["confusion"].sum(1), r["tally"][:, 1])
    assert np.array_equal(r["confusion"][:, 0] + r["confusion"][:, 2], r["correct"][:, 0])
    s = mc.reference_of(batch, edges=mc.EDGES)["sweep"]
    assert (np.diff(s, axis=1) <= 0).all() and (np.diff(s[:, :, 1:], axis=2) >= 0).all() and (s[:, :, 1:] <= s[:, :, :1]).all()


# ---- what the C entry refuses ------------------------------------------------------------------------------------------------------
NAMES = ("points", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "norm", "T1", "T0", "swapped", "depth_r_table",
         "occl_rel", "size_r", "use_min_conf", "min_conf", "thr", "n_thr", "edges", "B", "mask", "err", "status", "tally", "correct", "err_sum",
         "sweep", "confusion", "stream")
PAIRS, CAP = 2, 20
WHO = "match_error_by_pair"


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


def arguments(**kw):
    """A well-formed ragged call with every option on (thr and edges are real host arrays: the entry reads them), kw on top."""
    a = {n: address(k) for k, n in enumerate(NAMES)}
    a.update(stride=0, counts_in=None, pairs=PAIRS, cap=CAP, swapped=1, occl_rel=0.2, use_min_conf=1, min_conf=0.1, stream=None,
             thr=(ctypes.c_double * 3)(1.0, 3.0, 5.0), n_thr=3, edges=(ctypes.c_float * 2)(0.0, 0.5), B=2)
    for n, v in kw.items():
        assert n in a, n
        a[n] = v
    return [a[n] for n in NAMES]


def refused(lib, message, **kw):
    rc = lib.pats_match_error_by_pair_f64(*arguments(**kw))
    assert rc == 1, "%s was not refused: %d" % (kw, rc)
    assert lib.pats_last_error().decode() == "%s: %s" % (WHO, message)


REQUIRED = {"points": 4, "matches_r": 8, "T1": 8, "err": 8, "status": 1, "tally": 8, "correct": 8, "err_sum": 8}
OPTIONAL = {"conf": 4, "norm": 4, "pair_off": 8, "T0": 8, "depth_r_table": 8, "size_r": 4, "sweep": 8, "confusion": 8}


def test_null_and_alignment_rules(lib):
    for name, align in REQUIRED.items():
        refused(lib, "null %s" % name, **{name: None})
        if align > 1:
            refused(lib, "%s must be %d-byte aligned" % (name, align), **{name: address(50) + align // 2})
    refused(lib, "null thr", thr=None)
    for name, align in OPTIONAL.items():
        refused(lib, "%s must be %d-byte aligned" % (name, align), **{name: address(50) + align // 2})
    refused(lib, "counts_in must be 8-byte aligned", pair_off=None, counts_in=address(50) + 4, stride=10)


def test_segment_rules(lib):
    one = "exactly one of pair_off (ragged segments) and counts_in (strided segments) must be given"
    refused(lib, one, pair_off=None)
    refused(lib, one, counts_in=address(40))
    refused(lib, "pairs = 0 (1 .. 2^31 - 1)", pairs=0)
    refused(lib, "cap = -1 (0 .. 2^31 - 2)", cap=-1)
    refused(lib, "cap = 2147483647 (0 .. 2^31 - 2)", cap=2**31 - 1)
    refused(lib, "stride = 0 must be at least 1", pair_off=None, counts_in=address(40), stride=0)
    refused(lib, "pairs * stride = 2 * 11 exceeds cap = 20", pair_off=None, counts_in=address(40), stride=11)


def test_the_stage_s_own_rules(lib):
    nan, inf = float("nan"), float("inf")
    refused(lib, "min_conf needs conf", conf=None, edges=None, sweep=None)
    refused(lib, "min_conf = -0.5 must be a non-negative number", min_conf=-0.5)
    refused(lib, "min_conf = nan must be a non-negative number", min_conf=nan)
    for v in (2, -1):
        refused(lib, "swapped = %d must be 0 or 1" % v, swapped=v)
    for v, text in ((0.0, "0"), (-0.2, "-0.2"), (nan, "nan"), (inf, "inf")):
        refused(lib, "occl_rel = %s must be finite and positive" % text, occl_rel=v)
    for v in (0, 9, -1):
        refused(lib, "n_thr = %d (1 .. 8)" % v, n_thr=v)
    for vals, k, text in (((0.0, 3.0, 5.0), 0, "0"), ((1.0, nan, 5.0), 1, "nan"), ((1.0, 3.0, inf), 2, "inf"), ((-1.0, 3.0, 5.0), 0, "-1")):
        refused(lib, "thr[%d] = %s must be finite and positive" % (k, text), thr=(ctypes.c_double * 3)(*vals))
    refused(lib, "thr[1] = 1 does not ascend strictly", thr=(ctypes.c_double * 3)(1.0, 1.0, 5.0))
    refused(lib, "thr[2] = 2 does not ascend strictly", thr=(ctypes.c_double * 3)(1.0, 3.0, 2.0))
    refused(lib, "edges and sweep go together", edges=None)
    refused(lib, "edges and sweep go together", sweep=None)
    refused(lib, "mask and confusion go together", mask=None)
    refused(lib, "mask and confusion go together", confusion=None)
    refused(lib, "edges need conf", conf=None, use_min_conf=0)
    for v in (0, 65):
        refused(lib, "B = %d (1 .. 64)" % v, B=v)
    for vals, k, text in (((nan, 0.5), 0, "nan"), ((0.0, inf), 1, "inf"), ((-inf, 0.5), 0, "-inf")):
        refused(lib, "edges[%d] = %s must be finite" % (k, text), edges=(ctypes.c_float * 2)(*vals))
    refused(lib, "edges[1] = 0.5 does not ascend strictly", edges=(ctypes.c_float * 2)(0.5, 0.5))


def test_occl_rel_is_not_looked_at_without_a_table_and_the_ops_layer_exists(lib):
    """Without depth_r_table occl_rel is not checked: the next rule (here a bad n_thr) is what refuses the call.  The ops layer carries
    the stage and refuses CPU tensors like every other stage."""
    refused(lib, "n_thr = 0 (1 .. 8)", depth_r_table=None, occl_rel=float("nan"), n_thr=0)
    import torch
    from pats_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.match_error_by_pair(torch.zeros(4, 3), torch.zeros(4, 2), torch.eye(4, dtype=torch.float64)[None],
                                pair_off=torch.tensor([0, 4]))
    with pytest.raises(RuntimeError, match="match_error_by_pair: T1 must be float64"):
        ops.match_error_by_pair(torch.zeros(4, 3), torch.zeros(4, 2), torch.eye(4)[None], pair_off=torch.tensor([0, 4]))
