"""-m gpu: the fine level's 145 x 145 Sinkhorn solve (csrc/sinkhorn.hip launch_fine145: sinkhorn_blk145w2_kernel, or
sinkhorn_blk145_kernel under PATS_FINE_W2=0, then sinkhorn_rc_kernel<145, MODE> on the problems they flagged - stabilised linear
sweeps that re-base a drifting scaling into its stabiliser, and log-sum-exp sweeps behind a re-solve that still fails its guard)
against a float64 reference of the reference's log-domain iteration, on the case table of tests/fine_cases.py
(tests/test_fine_cases_host.py holds the table, the fp32 model that classifies it and the CPU oracle to the same gates).

Every test runs in both solver modes: "kernel" (the above) and "log" (sinkhorn_rc_kernel's log-sum-exp sweeps for everything).

What the model predicts and the library counts must agree exactly, in kernel mode: sinkhorn_fallbacks() = the problems the plain
solve flags, sinkhorn_tail_solves() = those of them whose stabilised re-solve fails too.  The second count is what makes a broken
re-base visible at all: the log-sum-exp tail repairs the plan of whatever the stabilised sweeps got wrong.

Shown to bite on a scratch build of csrc/sinkhorn.hip with `stab -= lg` turned into `stab += lg`: see the note at the end of
test_regimes_against_float64's docstring.  The other mutant of the re-base, `frd = fwr` (the drift flags read from the half being
written), was judged from the code and not run: the waves can then disagree on a branch that holds five barriers (it can
hang), and where they agree every re-base comes one sweep late, which the model shows to change no verdict of any case
(docs/parity.md, "Fine-level solver edges")."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):                       # (the PATS_FINE_W2=0 child runs this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fine_cases as fc  # noqa: E402
from fine_cases import cu  # noqa: E402

pytestmark = pytest.mark.gpu

FULL = 100
BIAS = 2.0                                    # outdoor (second_layer.py:107-112)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    return o


@pytest.fixture(params=["kernel", "log"])
def mode(request, ops):
    prev = ops.set_sinkhorn_mode(request.param)
    yield request.param
    ops.set_sinkhorn_mode(prev)


def bits(t):
    return t.contiguous().view(torch.int32)


def inputs(names):
    """Device inputs of the batch `names` (one entry point): (Z, ns [b, 1, 144]) or (Z, log_mu, log_nu)."""
    entry = fc.ROW[names[0]][1]
    assert all(fc.ROW[n][1] == entry for n in names)
    if entry == "o":
        return entry, (cu(fc.stacked(names, "Z")), cu(fc.stacked(names, "ns")[:, None, :]))
    return entry, (cu(fc.stacked(names, "Z")), cu(fc.stacked(names, "log_mu")), cu(fc.stacked(names, "log_nu")))


def launch(ops, entry, dev, sweeps, bias=0.0):
    if entry == "o":
        return ops.log_optimal_transport2(dev[0], 1.0, dev[1], sweeps, bias_k=bias)
    return ops.log_sinkhorn_iterations(dev[0], dev[1], dev[2], sweeps)


def counted(ops, fn):
    """fn() between two resets of the library's counters -> (result, guard trips, tail solves)."""
    ops.sinkhorn_fallbacks(reset=True)
    ops.sinkhorn_tail_solves(reset=True)
    out = fn()
    return out, ops.sinkhorn_fallbacks(reset=True), ops.sinkhorn_tail_solves(reset=True)


def expected_counts(mode, names, sweeps, desc=False):
    if mode != "kernel":
        return 0, 0
    return sum(fc.flagged(n, sweeps, desc) for n in names), sum(fc.tail(n, sweeps, desc) for n in names)


def check_batch(got, names, sweeps, bias, what, desc=False):
    """Every problem of a batch against float64 under its gates; every figure is printed before the first failure is raised."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    worst, failures = {}, []
    for k, n in enumerate(names):
        rec = {}
        try:
            fc.check_case(got[k], n, sweeps, bias, what, desc, record=rec)
        except AssertionError as e:
            failures.append(str(e))
        regime = fc.ROW[n][2]
        fc.fold(worst, regime, {(g if fc.flagged(n, sweeps, desc) or regime != "c" else g + " (kept by the block kernel)"): s
                                for g, s in rec.items()})
    print(fc.report(worst, what))
    assert not failures, "%d of %d problems miss a gate:\n%s" % (len(failures), len(names), "\n".join(failures))


# ---- 1. the regimes against float64 -------------------------------------------------------------------------------------------
RUNS = [("o", it, b) for it in fc.SWEEPS_ALL for b in fc.BIASES] + [("s", it, 0.0) for it in fc.SWEEPS_ALL]


@pytest.mark.parametrize("entry,sweeps,bias", RUNS, ids=["%s-it%d-bias%g" % r for r in RUNS])
def test_regimes_against_float64(ops, mode, entry, sweeps, bias):
    """Every case of the table that runs at this sweep count, in one launch: log_optimal_transport2 at bias 0, 2 and 3 (MODE 2 of
    sinkhorn_rc_kernel) or log_sinkhorn_iterations with given marginals (MODE 0).  The largest error per regime is printed as a
    share of each gate (pytest -rA); the guard trips and the tail solves are the model's, exactly.

    Mutant `stab += lg` (the absorption's sign, scratch build, never committed): every re-base then throws the iterate 2 ln a
    off, the scalings drift again at once, the final guard fails and the log-sum-exp tail repairs the plan - no gate moves.  It
    fails here in regimes (b), (c), (d) and (e) through sinkhorn_tail_solves(), which counts every flagged problem where the model
    expects the non-finite ones and the one- and two-sweep runs of regime (d) only; regime (a) never enters the re-solve and passes.
    Measured on an MI355X: 7 of the 16 kernel-mode runs fail (12 tail solves for the model's 3 at `o`, 100 sweeps; 7 for 1 at
    `s`; 1 for 0 at `o`, 3 sweeps), every plan stays within its gates, all 16 log-mode runs pass."""
    names = fc.cases_at(entry, sweeps)
    assert len(names) <= 130
    _, dev = inputs(names)
    got, trips, tails = counted(ops, lambda: launch(ops, entry, dev, sweeps, bias))
    check_batch(got, names, sweeps, bias, "%s %s it=%d bias=%g:" % (mode, entry, sweeps, bias))
    want = expected_counts(mode, names, sweeps)
    print("%s %s it=%d: %d problems, guard trips %d (model %d), tail solves %d (model %d)" % ((mode, entry, sweeps, len(names), trips, want[0], tails, want[1])))
    assert (trips, tails) == want


# ---- 2. flag isolation and batch edges ----------------------------------------------------------------------------------------
_ALONE = {}


def alone(ops, mode):
    """{case: its log-plan on the device} with the tame cases solved in a batch of their own and every flagged case in a launch
    of its own (100 sweeps, bias 2).  test_regimes_against_float64 holds the same cases at the same bias to float64; here the
    counts and the non-finite pattern are checked, so that nothing later is bit-equal to a problem nobody solved."""
    if mode not in _ALONE:
        base = {}
        _, dev = inputs(fc.TAME_O)
        got, trips, _ = counted(ops, lambda: launch(ops, "o", dev, FULL, BIAS))
        assert trips == 0 and bool(torch.isfinite(got).all())
        base.update(zip(fc.TAME_O, got))
        for n in fc.FLAGGED_O:
            _, dev = inputs([n])
            got, trips, tails = counted(ops, lambda: launch(ops, "o", dev, FULL, BIAS))
            assert (trips, tails) == expected_counts(mode, [n], FULL), (n, trips, tails)
            assert fc.same_nonfinite(got[0].cpu().numpy(), fc.reference(n)[FULL]), n
            base[n] = got[0]
        pool = list(fc.TAME_O) + list(fc.FLAGGED_O)
        _, dev = inputs(pool)
        _ALONE[mode] = (pool, dev, torch.stack([base[n] for n in pool]))
    return _ALONE[mode]


def run_layout(ops, mode, names, what):
    """One launch of `names` gathered on the device from the pool: every row has the bits its case has alone, whatever its
    position and neighbours, and the trips are the flagged problems, exactly."""
    pool, dev, base = alone(ops, mode)
    idx = torch.tensor([pool.index(n) for n in names], device="cuda")
    sel = tuple(torch.index_select(t, 0, idx) for t in dev)
    got, trips, tails = counted(ops, lambda: launch(ops, "o", sel, FULL, BIAS))
    diff = (bits(got) != bits(base[idx])).flatten(1).any(1).nonzero().flatten().tolist()
    assert not diff, "%s: %d of %d problems differ from their solve alone: %s" % (
        what, len(diff), len(names), ", ".join("%d (%s)" % (k, names[k]) for k in diff[:8]))
    assert (trips, tails) == expected_counts(mode, names, FULL), (what, trips, tails)
    return trips


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_flag_isolation_at_the_batch_edges(ops, mode, B):
    """Flagged problems at index 0, 63, 64 and last of a batch of tame ones; the flag workspace is rounded up to 64 problems and
    257 problems exceed the 256 CUs."""
    names = [fc.TAME_O[k % len(fc.TAME_O)] for k in range(B)]
    spots = sorted({p for p in (0, 63, 64, B - 1) if p < B})
    for k, p in enumerate(spots):
        names[p] = fc.FLAGGED_O[k % len(fc.FLAGGED_O)]
    trips = run_layout(ops, mode, names, "%s batch of %d, flagged at %s" % (mode, B, spots))
    assert trips == (len(spots) if mode == "kernel" else 0)


def test_all_flagged_and_none_flagged_batches(ops, mode):
    B = 65
    every = [fc.FLAGGED_O[k % len(fc.FLAGGED_O)] for k in range(B)]
    assert run_layout(ops, mode, every, "%s all flagged" % mode) == (B if mode == "kernel" else 0)
    none = [fc.TAME_O[k % len(fc.TAME_O)] for k in range(B)]
    assert run_layout(ops, mode, none, "%s none flagged" % mode) == 0
    # neighbours of different kinds in a row: every flagged case next to every other
    mixed = [n for a in fc.FLAGGED_O for b in fc.FLAGGED_O for n in (a, b, fc.TAME_O[0])][:130]
    run_layout(ops, mode, mixed, "%s flagged pairs" % mode)


# ---- 3. non-finite problems ---------------------------------------------------------------------------------------------------
NONFINITE_BATCHES = [
    ("o", FULL, ("tame_iid_half_o", "nan_score_o", "tame_iid_4_o", "posinf_score_o", "neginf_row_o", "tame_peak_1_o")),
    ("o", 1, ("tame_iid_half_o", "posinf_score_o", "tame_iid_4_o")),
    ("s", FULL, ("tame_iid_half_s", "posinf_score_s", "tame_iid_4_s")),
]


@pytest.mark.parametrize("entry,sweeps,names", NONFINITE_BATCHES, ids=["%s-it%d" % b[:2] for b in NONFINITE_BATCHES])
def test_nonfinite_problems_end_in_the_tail_and_touch_nobody(ops, mode, entry, sweeps, names):
    """One NaN score, one +inf score, one row of -inf only: the NaN / -inf / +inf pattern of the plan is the float64 reference's,
    finite entries within NEGINF_ATOL, one guard trip and one tail solve each, and the tame neighbours of the same launch have
    the bits they have in a launch without them."""
    wild = [k for k, n in enumerate(names) if fc.ROW[n][2] == "f"]
    tame = [k for k in range(len(names)) if k not in wild]
    bias = BIAS if entry == "o" else 0.0
    _, dev = inputs(names)
    got, trips, tails = counted(ops, lambda: launch(ops, entry, dev, sweeps, bias))
    check_batch(got, names, sweeps, bias, "%s %s it=%d non-finite:" % (mode, entry, sweeps))
    assert (trips, tails) == ((len(wild), len(wild)) if mode == "kernel" else (0, 0))
    _, dev_t = inputs([names[k] for k in tame])
    quiet, t2, _ = counted(ops, lambda: launch(ops, entry, dev_t, sweeps, bias))
    assert t2 == 0 and torch.equal(bits(got[tame]), bits(quiet)), "a non-finite problem changed a neighbour"


# ---- 4. the counted launch ----------------------------------------------------------------------------------------------------
def desc_inputs():
    d0, d1 = fc.descriptors(fc.DESC_O)
    return cu(d0), cu(d1), cu(fc.stacked(fc.DESC_O, "ns")[:, None, :])


def own_flags(Z):
    return Z[:, -1, :-1] > Z[:, :-1, :-1].max(1).values          # second_layer.py:243,248


def test_counted_launch_solves_the_live_rows_only(ops, mode):
    """cost_ot(variant 2, return_flags=True, count=...) over a capacity of 12 descriptor problems with flagged ones on both sides
    of the count: rows before the count have the bits (plan and column flags) of the uncounted call, the trips are the flagged
    LIVE rows, and what the padding rows hold - NaN, inf, negative ns - changes nothing."""
    cap = len(fc.DESC_O)
    d0, d1, ns = desc_inputs()
    (Zu, fu), trips, tails = counted(ops, lambda: ops.cost_ot(d0, d1, 2, 1.0, ns, FULL, bias_k=BIAS, return_flags=True))
    assert (trips, tails) == expected_counts(mode, fc.DESC_O, FULL, desc=True)
    assert torch.equal(fu, own_flags(Zu)) and bool(torch.isfinite(Zu).all())
    for count in (0, 5, cap):
        live, pad = fc.DESC_O[:count], fc.DESC_O[count:]
        if 0 < count < cap:
            assert any(fc.flagged(n, FULL, True) for n in live) and any(fc.flagged(n, FULL, True) for n in pad)
        for poison in (False, True):
            e0, e1, es = d0.clone(), d1.clone(), ns.clone()
            if poison:
                e0[count:], e1[count:], es[count:] = float("nan"), float("inf"), -1.0
            cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
            (Z, f), trips, tails = counted(ops, lambda: ops.cost_ot(e0, e1, 2, 1.0, es, FULL, bias_k=BIAS, return_flags=True, count=cnt))
            what = "%s count %d of %d%s" % (mode, count, cap, ", poisoned padding" if poison else "")
            assert (trips, tails) == expected_counts(mode, live, FULL, desc=True), (what, trips, tails)
            assert torch.equal(bits(Z[:count]), bits(Zu[:count])), what + ": a live row differs from the uncounted call"
            assert torch.equal(f[:count], fu[:count]), what + ": a live row's column flags differ from the uncounted call"


# ---- 5. the three ways in -----------------------------------------------------------------------------------------------------
def three_ways(ops):
    """The mixed batches through every way in that this process has: log_optimal_transport2 on scores (regimes a, b, c, e),
    cost_ot on descriptors by the two-kernel path and by the fused kernel, whose redo runs in place (regimes a, b, c, g).
    -> {way: (plans as numpy, guard trips, tail solves)}."""
    out = {}
    _, dev = inputs(fc.MIXED_O)
    got, trips, tails = counted(ops, lambda: launch(ops, "o", dev, FULL, BIAS))
    out["scores"] = (got.cpu().numpy(), trips, tails)
    d0, d1, ns = desc_inputs()
    prev = ops.set_fine_fused(False)
    try:
        for way, fused in (("two_kernel", False), ("fused", True)):
            ops.set_fine_fused(fused)
            got, trips, tails = counted(ops, lambda: ops.cost_ot(d0, d1, 2, 1.0, ns, FULL, bias_k=BIAS))
            out[way] = (got.cpu().numpy(), trips, tails)
    finally:
        ops.set_fine_fused(prev)
    return out


def check_three_ways(res, mode, head):
    for way, (got, trips, tails) in res.items():
        names, desc = (fc.MIXED_O, False) if way == "scores" else (fc.DESC_O, True)
        check_batch(got, names, FULL, BIAS, "%s %s %s:" % (mode, head, way), desc)
        assert (int(trips), int(tails)) == expected_counts(mode, names, FULL, desc), (head, way, trips, tails)


def test_three_ways_in_against_float64(ops, mode, tmp_path):
    """The default path, the fused cost -> OT kernel (the redo re-solves in place, Zin == out) and - kernel mode, one child
    process - the four-wave block kernel under PATS_FINE_W2=0 (read once per process): each against the float64 reference of the
    float64 cost, under the same gates."""
    check_three_ways(three_ways(ops), mode, "two-wave")
    if mode != "kernel":
        return                                  # the forced log domain runs neither block kernel: nothing for the child to add
    path = str(tmp_path / "w2_0.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, PATS_FINE_W2="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "PATS_FINE_W2=0 child: exit %s\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    with np.load(path) as z:
        assert str(z["w2"]) == "0"
        res = {way: (z[way], z[way + "_counts"][0], z[way + "_counts"][1]) for way in ("scores", "two_kernel", "fused")}
    check_three_ways(res, mode, "four-wave")


# ---- 6. repeatability -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(ops, mode):
    first, again = three_ways(ops), three_ways(ops)
    for way in first:
        assert np.array_equal(first[way][0].view(np.int32), again[way][0].view(np.int32)) and first[way][1:] == again[way][1:], way
    names = fc.cases_at("s", FULL)
    _, dev = inputs(names)
    assert torch.equal(bits(launch(ops, "s", dev, FULL)), bits(launch(ops, "s", dev, FULL)))


def child_main(path):
    from pats_amd import ops as o
    o.set_sinkhorn_mode("kernel")
    res = three_ways(o)
    np.savez(path, w2=os.environ.get("PATS_FINE_W2", ""), **{way: r[0] for way, r in res.items()},
             **{way + "_counts": np.array(r[1:], np.int64) for way, r in res.items()})


if __name__ == "__main__":
    child_main(sys.argv[1])
