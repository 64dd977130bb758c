"""GPU: ops.match_error_by_pair / batch.match_error_by_pair / batch.split_match_error_by_pair against the definition of
include/pats_amd.h ("Per-pair match error against ground truth") restated in numpy float64 (tests/match_error_cases.py), on identical
float32 inputs:
    status, tally, correct, sweep, confusion    equal
    err          the same NaN pattern, exact zeros outside the segments, within 1e-9 px where scored: fewer than 64 rounded float64
                 operations on coordinates below 4096 px, 64 * 2^-52 * 4096 = 6e-11, rounded up
    err_sum      within n_scored * (1e-9 + 2^-52 * err_sum): every term's own error plus one rounding per addition
The builder's margins (match_error_cases.assert_margins) hold for every case, so no match is left out of any comparison.  Every output
lies inside a larger sentinel-filled buffer and every input list in a larger NaN-filled one: a call defines every byte of its views,
none around them, and reads no row beyond cap."""
import ctypes

import numpy as np
import pytest
import torch

import match_error_cases as mc

pytestmark = pytest.mark.gpu

PAD = 64
SENT = {torch.float64: -777.25, torch.int64: -123456, torch.uint8: 0xAB}
F32 = np.float32
NAN = float("nan")
LENGTHS = (1, 511, 0, 512, 513, 1300)                   # the empty pair in the middle; 512 = two full trips of the 256-thread walk
SMALL = (300, 0, 70)


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(a, fill=NAN):
    """A list as the view of a longer buffer whose rows beyond cap are NaN (0xFF for bytes)."""
    t = cu(a)
    buf = torch.full((a.shape[0] + PAD,) + tuple(a.shape[1:]), fill if t.dtype.is_floating_point else 0xFF, dtype=t.dtype, device="cuda")
    buf[:a.shape[0]] = t
    return buf[:a.shape[0]]


class Sentinel:
    """Output views inside sentinel-filled buffers; check() asserts that nothing around them changed."""

    def __init__(self):
        self.bufs = []

    def view(self, shape, dtype):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENT[dtype], dtype=dtype, device="cuda")
        self.bufs.append((buf, SENT[dtype], n))
        return buf[PAD:PAD + n].view(*shape)

    def check(self, untouched=False):
        torch.cuda.synchronize()
        for buf, sent, n in self.bufs:
            around = torch.cat([buf[:PAD], buf[PAD + n:]]) if not untouched else buf
            assert bool((around == sent).all()), "bytes around an output view changed" if not untouched else "a refused call wrote an output"


def destinations(s, cap, pairs, n_thr, B=None, mask=False):
    dest = [s.view((cap,), torch.float64), s.view((cap,), torch.uint8), s.view((pairs, 8), torch.int64), s.view((pairs, n_thr), torch.int64),
            s.view((pairs,), torch.float64)]
    if B is not None:
        dest.append(s.view((pairs, B, 1 + n_thr), torch.int64))
    if mask:
        dest.append(s.view((pairs, 4), torch.int64))
    return tuple(dest)


KEYS = ("err", "status", "tally", "correct", "err_sum", "sweep", "confusion")


def device_maps(depths, view=False):
    """The right depth maps on the device; view: each as a strided view of a wider NaN-filled buffer."""
    out = []
    for d in depths:
        if d is None:
            out.append(None)
        elif view:
            store = torch.full((d.shape[0], d.shape[1] + 11), NAN, dtype=torch.float32, device="cuda")
            store[:, :d.shape[1]] = cu(d)
            out.append(store[:, :d.shape[1]])
            assert not out[-1].is_contiguous()
        else:
            out.append(cu(d))
    return out


def run(ops, b, view=False, **kw):
    """ops.match_error_by_pair on a make_batch result with the options of match_error_cases.reference_of -> dict of numpy outputs."""
    args = dict(T0=b["T0"], thr=mc.THR, norm=b["norm"], swapped=True, depths_r=b["depths_r"], occl_rel=mc.OCCL, size_r=b["size_r"],
                conf=b["conf"], min_conf=None, edges=None, mask=None)
    args.update(kw)
    T1 = args.pop("T1", b["T1"])
    pairs, cap = len(b["segs"]), b["cap"]
    s = Sentinel()
    dest = destinations(s, cap, pairs, len(args["thr"]), None if args["edges"] is None else len(args["edges"]), args["mask"] is not None)
    seg = {"pair_off": cu(b["pair_off"])} if b["stride"] is None else {"stride": b["stride"], "counts": cu(b["counts"])}
    dev = {k: (None if args[k] is None else cu(args[k])) for k in ("T0", "norm", "size_r")}
    maps = None if args["depths_r"] is None else device_maps(args["depths_r"], view)
    got = ops.match_error_by_pair(guarded(b["points"]), guarded(b["mr"]), cu(T1), thr=args["thr"], swapped=args["swapped"], depths_r=maps,
                                  occl_rel=args["occl_rel"], conf=None if args["conf"] is None else guarded(args["conf"]),
                                  min_conf=args["min_conf"], edges=args["edges"], mask=None if args["mask"] is None else guarded(args["mask"]),
                                  out=dest, **dev, **seg)
    s.check()
    assert len(got) == 7 and [g is None for g in got] == [False] * 5 + [args["edges"] is None, args["mask"] is None]
    assert all(a.data_ptr() == d.data_ptr() for a, d in zip([g for g in got if g is not None], dest))
    return {k: (None if g is None else g.cpu().numpy()) for k, g in zip(KEYS, got)}


def compare(got, ref, segs, what):
    """The agreement the module's docstring states; prints the figures before it asserts."""
    for k in ("status", "tally", "correct", "sweep", "confusion"):
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), "%s: %s differs" % (what, k)
    inside = np.zeros(ref["err"].shape[0], bool)
    for lo, n in segs:
        inside[lo:lo + n] = True
    assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"])), "%s: the NaN pattern of err differs" % what
    assert not got["err"][~inside].view(np.int64).any() and not got["status"][~inside].any(), "%s: a row outside the segments is not zero" % what
    sc = ref["status"] == 1
    gap = np.abs(got["err"][sc] - ref["err"][sc]).max(initial=0.0)
    n_scored = ref["tally"][:, 1]
    sum_gap = np.abs(got["err_sum"] - ref["err_sum"])
    sum_tol = n_scored * (1e-9 + 2.0 ** -52 * ref["err_sum"])
    print("%s: statuses %s, scored %d, max |err - ref| = %.3g px (1e-9), max |err_sum - ref| / tolerance = %.3g" %
          (what, ref["tally"].sum(0)[:7].tolist(), sc.sum(), gap, (sum_gap / np.maximum(sum_tol, 1e-300)).max(initial=0.0)))
    assert gap <= 1e-9
    assert (sum_gap <= sum_tol).all()


@pytest.fixture(scope="module")
def big():
    """The ragged batch of all lengths and its full-option reference: computed once, shared, never changed."""
    b = mc.make_batch(LENGTHS, 4100)
    ref = mc.reference_of(b, min_conf=mc.MIN_CONF, edges=mc.EDGES, mask=b["mask"])
    mc.assert_margins(ref, b["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    assert set(np.unique(ref["status"])) == set(range(7))
    return b, ref


FULL = dict(min_conf=mc.MIN_CONF, edges=mc.EDGES)


# ---- 1. shapes --------------------------------------------------------------------------------------------------------------------
def test_ragged_lengths_with_every_option_and_two_calls_with_the_same_bits(ops, big):
    b, ref = big
    got = run(ops, b, mask=b["mask"], **FULL)
    compare(got, ref, b["segs"], "ragged")
    again = run(ops, b, mask=b["mask"], **FULL)
    for k in KEYS:                                                                # determinism: all seven outputs, bit for bit
        assert got[k].tobytes() == again[k].tobytes(), k


def test_strided_form_with_counts_below_the_stride(ops):
    b = mc.make_batch(LENGTHS, 4200, stride=1304, slack_rows=5)
    ref = mc.reference_of(b, mask=b["mask"], **FULL)
    mc.assert_margins(ref, b["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    compare(run(ops, b, mask=b["mask"], **FULL), ref, b["segs"], "strided")


@pytest.mark.parametrize("slack", [0, 7])
def test_one_empty_pair(ops, slack):
    b = mc.make_batch((0,), 4300, slack_rows=slack)                               # slack = 0: cap == 0, a valid call
    ref = mc.reference_of(b, mask=b["mask"], **FULL)
    got = run(ops, b, mask=b["mask"], **FULL)
    compare(got, ref, b["segs"], "one empty pair, cap = %d" % slack)
    assert not got["tally"].any() and not got["sweep"].any() and not got["confusion"].any() and got["err_sum"].tobytes() == bytes(8)


def test_slack_rows_behind_the_last_segment(ops):
    b = mc.make_batch(SMALL, 4400, slack_rows=23)
    ref = mc.reference_of(b, mask=b["mask"], **FULL)
    mc.assert_margins(ref, b["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    compare(run(ops, b, mask=b["mask"], **FULL), ref, b["segs"], "slack rows")


# ---- 2. the options, one at a time ---------------------------------------------------------------------------------------------
def conjugate4(T):
    P = np.eye(4)[[1, 0, 2, 3]]
    return P @ T @ P


THR8 = (0.25, 0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 50.0)
EDGES64 = tuple(np.linspace(0.0, 0.945, 64).astype(F32).tolist())

OPTIONS = {
    "without T0": lambda b: dict(T1=np.stack([np.block([[c["R"], c["t"][:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]) for c in b["pairs"]]),
                                 T0=None),
    "swapped 0": lambda b: dict(T1=np.stack([conjugate4(T) for T in b["T1"]]), T0=np.stack([conjugate4(T) for T in b["T0"]]), swapped=False),
    "swapped 1": lambda b: dict(),
    "without right maps": lambda b: dict(depths_r=None),
    "one null map": lambda b: dict(depths_r=[None] + b["depths_r"][1:]),
    "without size_r": lambda b: dict(size_r=None),
    "min_conf": lambda b: dict(min_conf=0.5),
    "n_thr 1": lambda b: dict(thr=(2.0,), edges=mc.EDGES, mask=b["mask"]),
    "n_thr 8": lambda b: dict(thr=THR8, edges=mc.EDGES, mask=b["mask"]),
    "B 1": lambda b: dict(edges=(0.0,)),
    "B 64": lambda b: dict(edges=EDGES64),
    "with mask": lambda b: dict(mask=b["mask"]),
    "without conf": lambda b: dict(conf=None),
    "occl_rel 0.0005": lambda b: dict(occl_rel=0.0005),                           # below the maps' depth step per pixel: fewer are covisible
    "occl_rel 2": lambda b: dict(occl_rel=2.0),                                   # the occluder no longer hides anything
}


@pytest.fixture(scope="module")
def small():
    return mc.make_batch(SMALL, 4500)


@pytest.mark.parametrize("option", sorted(OPTIONS))
def test_option(ops, small, option):
    kw = OPTIONS[option](small)
    ref = mc.reference_of(small, **kw)
    mc.assert_margins(ref, small["conf"], kw.get("thr", mc.THR), kw.get("edges"), kw.get("min_conf"))
    compare(run(ops, small, **kw), ref, small["segs"], option)
    if option == "B 1":                                                           # an edge at 0 holds every scored match
        assert np.array_equal(ref["sweep"][:, 0, 0], ref["tally"][:, 1]) and np.array_equal(ref["sweep"][:, 0, 1:], ref["correct"])
    if option.startswith("occl_rel"):
        assert ref["tally"][:, 6].sum() != mc.reference_of(small)["tally"][:, 6].sum()
    if option == "without T0":                                                    # the same ground truth: the same verdicts
        assert np.array_equal(ref["status"], mc.reference_of(small)["status"])


def test_without_norm(ops, small):
    """norm = None: q = u.  The right points are given normalised, the thresholds in normalised units; no maps, no size."""
    b = dict(small)
    mr = small["mr"].copy()
    for (lo, n), c in zip(small["segs"], small["pairs"]):
        mr[lo:lo + n] = (mr[lo:lo + n] - c["norm"][4:6]) * c["norm"][6:8]
    b["mr"] = mr.astype(F32)
    kw = dict(norm=None, depths_r=None, size_r=None, thr=tuple(v / mc.FOCAL for v in mc.THR))
    ref = mc.reference_of(b, **kw)
    assert ref["tally"][:, 1].sum() > 100 and ref["correct"].sum() > 100
    compare(run(ops, b, **kw), ref, b["segs"], "without norm")


def test_maps_of_different_sizes_as_strided_views(ops):
    b = mc.make_batch(SMALL, 4600, shapes=[(96, 128), (64, 80), (120, 160)])
    ref = mc.reference_of(b, **FULL)
    mc.assert_margins(ref, b["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    assert (ref["status"] == 5).any() and (ref["status"] == 6).any()
    compare(run(ops, b, view=True, **FULL), ref, b["segs"], "maps of three sizes, strided views")


def test_table_made_earlier_and_allocated_outputs(ops, small):
    """table_r= a lift_table made once; out=None allocates; both give the bits of the call with depths_r and destinations."""
    ref = run(ops, small, **FULL)
    tab = ops.lift_table(device_maps(small["depths_r"]))
    got = ops.match_error_by_pair(cu(small["points"]), cu(small["mr"]), cu(small["T1"]), T0=cu(small["T0"]), norm=cu(small["norm"]), swapped=True,
                                  table_r=tab, size_r=cu(small["size_r"]), conf=cu(small["conf"]), pair_off=cu(small["pair_off"]), **FULL)
    for k, g in zip(KEYS, got):
        assert (g is None and ref[k] is None) or g.cpu().numpy().tobytes() == ref[k].tobytes(), k


# ---- 3. through batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ["all", "topk"])
def test_through_batch_in_the_caller_s_order(ops, on):
    from pats_amd import batch
    n, shapes = 160, [(96, 128), (64, 80), (120, 160)]
    b = mc.make_batch((n, n, n), 4700, shapes=shapes)                             # the CALLER's order
    pairs = 3
    mixed = on == "all"
    caller_of = [2, 0, 1] if mixed else [0, 1, 2]                                 # slot s holds the caller's pair caller_of[s]
    rows = np.concatenate([np.arange(i * n, (i + 1) * n) for i in caller_of])     # slot order
    cap = batch.Capacities(pairs, 5, 6)
    summary = np.concatenate([np.arange(pairs + 1) * n, [pairs * n, 0, 0]]).astype(np.int64)
    dl, dr, dc, ds = cu(b["ml"][rows]), cu(b["mr"][rows]), cu(b["conf"][rows]), cu(summary)
    out = {"matches_l": dl, "matches_r": dr, "match_conf": dc, "by_pair": (dl, dr, ds[:pairs + 1], dc), "summary": ds}
    if mixed:
        out["caller_of"] = caller_of
    else:                                                                         # the same rows as a top-K result
        out["topk"] = (dl.view(pairs, n, 2), dr.view(pairs, n, 2), dc.view(pairs, n),
                       torch.arange(n, dtype=torch.int32, device="cuda").repeat(pairs, 1), cu(np.full(pairs, n, np.int64)))
    norm, T1, T0, size_r = cu(b["norm"]), cu(b["T1"]), cu(b["T0"]), cu(b["size_r"])
    depths_l = [cu(c["depth_l"]) for c in b["pairs"]]
    depths_r = device_maps(b["depths_r"], view=True)

    with pytest.raises(ValueError, match="match_error_by_pair.*lift_by_pair"):
        batch.match_error_by_pair(out, cap, T1, T0=T0, norm=norm, swapped=True)
    lifted = batch.lift_by_pair(out, cap, depths_l, norm, on=on)
    assert np.array_equal(lifted[0].cpu().numpy(), b["points"][rows], equal_nan=True)      # the lift of the cases
    # a mask: the verification of the ground-truth pose itself (M = 1), on the lifted lists
    models = np.stack([np.concatenate(mc.conjugate(c["R"], c["t"])[:1] + (mc.conjugate(c["R"], c["t"])[1][:, None],), 1) for c in b["pairs"]])
    batch.verify_abs_by_pair(out, cap, cu(models.astype(F32)[:, None]), cu(np.full(pairs, 2.0 / mc.FOCAL, F32)), norm=norm)
    mask_slot = out["verified_abs"][3].cpu().numpy()
    before = dict(out)

    res = batch.match_error_by_pair(out, cap, T1, T0=T0, thr=mc.THR, norm=norm, swapped=True, depths_r=depths_r, occl_rel=mc.OCCL, size_r=size_r,
                                    min_conf=mc.MIN_CONF, edges=mc.EDGES, mask="verified_abs")
    split = batch.split_match_error_by_pair(out, cap)
    torch.cuda.synchronize()
    assert out["match_error"] is res and set(out) == set(before) | {"match_error"}
    assert all(out[k] is v for k, v in before.items())                            # no other entry was replaced
    mask = np.empty(pairs * n, np.uint8)
    mask[rows] = mask_slot                                                        # the mask in the caller's row order
    ref = mc.reference_of(b, mask=mask, **FULL)
    mc.assert_margins(ref, b["conf"], mc.THR, mc.EDGES, mc.MIN_CONF)
    got = {k: (None if g is None else g.cpu().numpy()) for k, g in zip(KEYS, res)}
    slot_view = dict(ref, err=ref["err"][rows], status=ref["status"][rows])       # per-match outputs: slot order; per-pair: the caller's
    compare(got, slot_view, [(s_ * n, n) for s_ in range(pairs)], "batch on=%s" % on)
    assert ref["confusion"][:, 0].sum() > 50 and ref["confusion"][:, 3].sum() > 50
    for i in range(pairs):
        e, st, tally, correct, err_sum = split[i]
        assert np.array_equal(st.cpu().numpy(), ref["status"][i * n:(i + 1) * n])
        assert np.array_equal(np.isnan(e.cpu().numpy()), np.isnan(ref["err"][i * n:(i + 1) * n]))
        assert torch.equal(tally, res[2][i]) and torch.equal(correct, res[3][i]) and torch.equal(err_sum, res[4][i])

    # a mask that was computed on other lists is refused, and so is one that was not computed at all
    out["verified_abs_on"] = "topk" if mixed else "all"
    with pytest.raises(ValueError, match="match_error_by_pair.*verified_abs.*not aligned"):
        batch.match_error_by_pair(out, cap, T1, T0=T0, norm=norm, swapped=True, mask="verified_abs")
    with pytest.raises(ValueError, match="match_error_by_pair.*verified_h"):
        batch.match_error_by_pair(out, cap, T1, T0=T0, norm=norm, swapped=True, mask="verified_h")
    with pytest.raises(ValueError, match="match_error_by_pair.*mask must be one of"):
        batch.match_error_by_pair(out, cap, T1, T0=T0, norm=norm, swapped=True, mask="inlier")


# ---- 4. refusals: an error, and nothing launched ------------------------------------------------------------------------------------
NAMES = ("points", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "norm", "T1", "T0", "swapped", "depth_r_table",
         "occl_rel", "size_r", "use_min_conf", "min_conf", "thr", "n_thr", "edges", "B", "mask", "err", "status", "tally", "correct", "err_sum",
         "sweep", "confusion", "stream")
D3, F2 = ctypes.c_double * 3, ctypes.c_float * 2
REFUSALS = {
    "null points": dict(points=None), "null T1": dict(T1=None), "null thr": dict(thr=None), "null err": dict(err=None),
    "null tally": dict(tally=None), "points off 4 bytes": dict(points=+2), "matches_r off 8 bytes": dict(matches_r=+4),
    "T0 off 8 bytes": dict(T0=+4), "err off 8 bytes": dict(err=+4), "both segment forms": dict(counts_in="pair_off"),
    "neither segment form": dict(pair_off=None), "pairs 0": dict(pairs=0), "cap negative": dict(cap=-1),
    "stride 0": dict(pair_off=None, counts_in="pair_off", stride=0), "pairs * stride above cap": dict(pair_off=None, counts_in="pair_off", stride=10 ** 6),
    "n_thr 0": dict(n_thr=0), "n_thr 9": dict(n_thr=9), "B 0": dict(B=0), "B 65": dict(B=65),
    "threshold 0": dict(thr=D3(0.0, 3.0, 5.0)), "threshold NaN": dict(thr=D3(1.0, NAN, 5.0)), "threshold inf": dict(thr=D3(1.0, 3.0, float("inf"))),
    "thresholds descend": dict(thr=D3(1.0, 5.0, 3.0)), "thresholds equal": dict(thr=D3(1.0, 1.0, 3.0)),
    "edge NaN": dict(edges=F2(NAN, 0.5)), "edge inf": dict(edges=F2(0.0, float("inf"))), "edges equal": dict(edges=F2(0.5, 0.5)),
    "edges without conf": dict(conf=None, use_min_conf=0), "min_conf without conf": dict(conf=None, edges=None, sweep=None),
    "edges without sweep": dict(sweep=None), "mask without confusion": dict(confusion=None),
    "occl_rel 0": dict(occl_rel=0.0), "occl_rel NaN": dict(occl_rel=NAN), "occl_rel inf": dict(occl_rel=float("inf")),
    "swapped 2": dict(swapped=2), "swapped -1": dict(swapped=-1), "min_conf negative": dict(min_conf=-0.5),
}


EXPECT = {"stride 0": "stride = 0 must be at least 1", "pairs * stride above cap": "exceeds cap", "both segment forms": "exactly one of",
          "neither segment form": "exactly one of"}


@pytest.fixture(scope="module")
def call(ops, small):
    """A well-formed call of the C entry on real device memory, every option on: (arguments by name, the sentinel of its outputs,
    what keeps the memory alive)."""
    from pats_amd import _lib
    b = small
    pairs, cap = len(b["segs"]), b["cap"]
    s = Sentinel()
    dest = destinations(s, cap, pairs, 3, 2, True)
    tab = ops.lift_table(device_maps(b["depths_r"]))
    t = {"points": cu(b["points"]), "matches_r": cu(b["mr"]), "conf": cu(b["conf"]), "pair_off": cu(b["pair_off"]), "norm": cu(b["norm"]),
         "T1": cu(b["T1"]), "T0": cu(b["T0"]), "depth_r_table": tab.dev, "size_r": cu(b["size_r"]), "mask": cu(b["mask"])}
    t.update(zip(("err", "status", "tally", "correct", "err_sum", "sweep", "confusion"), dest))
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update(stride=0, counts_in=None, pairs=pairs, cap=cap, swapped=1, occl_rel=mc.OCCL, use_min_conf=1, min_conf=0.1, thr=D3(1.0, 3.0, 5.0),
             n_thr=3, edges=F2(0.0, 0.5), B=2, stream=None)
    return _lib.lib(), a, s, (t, tab)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_launch(call, case):
    lib, a, s, _ = call
    good, a = a, dict(a)
    for k, v in REFUSALS[case].items():                                           # an int on a pointer: that many bytes off; a name: that pointer
        assert k in a
        a[k] = good[k] + v if isinstance(v, int) and k in ("points", "matches_r", "T0", "err") else (good[v] if isinstance(v, str) else v)
    rc = lib.pats_match_error_by_pair_f64(*[a[n] for n in NAMES])
    print("%s: rc = %d, %s" % (case, rc, lib.pats_last_error().decode()))
    assert rc == 1 and lib.pats_last_error().decode().startswith("match_error_by_pair: ")
    if case in EXPECT:
        assert EXPECT[case] in lib.pats_last_error().decode()
    s.check(untouched=True)


def test_the_well_formed_call_of_the_refusal_cases_is_accepted(call, small):
    """Last in the file: the call the refusal cases start from does run (so each of them was refused for its one change)."""
    lib, a, s, _ = call
    assert lib.pats_match_error_by_pair_f64(*[a[n] for n in NAMES]) == 0, lib.pats_last_error().decode()
    s.check()
    ref = mc.reference_of(small, min_conf=0.1, edges=(0.0, 0.5), mask=small["mask"])
    assert np.array_equal(s.bufs[2][0][PAD:-PAD].cpu().numpy().reshape(-1, 8), ref["tally"])
