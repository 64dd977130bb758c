"""-m gpu: the walk by which the third level's two follow-up kernels find the problems the guarded linear solve flagged
(third_fused3_stab_kernel, third_fused_kernel in scan mode), at the sizes production runs: more problems than the 6144
workgroups of the walk, so that lanes other than 0 claim a problem, one workgroup re-solves several problems in a row, the
outer loop takes a second trip, and a counted launch (pats_third_level_counted_f32) has flagged problems on both sides of
the device-side count.

A launch of P problems is assembled ON THE DEVICE from a base set of 96 problems (32 of them wild) by an index vector; problems
are independent and results are bit-identical by contract (tests/test_determinism_gpu.py), so row p of any launch must equal,
bit for bit, the row of base problem idx[p] in the plain 96-problem launch - which is checked against the CPU oracle under the
gates of tests/test_gpu_parity.py.  Wild problems sit at positions chosen from the walk: with W = min(P, 6144) workgroups,
problem p is looked at by workgroup p % W, lane (p % (64 W)) / W, on trip p / (64 W) of the outer loop (walk_slot).  Every
launch writes into buffers the test owns, pre-filled with NaN and - if_matching1 - with the sentinel the walk looks for, so
a problem nobody re-solved, and a row past the count that somebody did, both show.

The same cases run in a child process under PATS_THIRD_STAB=0 (this file run as a script), where the scan kernel's walk sees
every flagged problem instead of what the stabilised kernel leaves.

Shown to bite on three one-line mutants of both walks, none of which the older third-level tests notice: the re-solved index taken
one lane low (first + (k > 0 ? k - 1 : 0) W: nine tests here fail, from P = 6145 on), `cand < g.P` for `cand < live` (the counted
tests fail: rows past the count written), the outer loop ended after one trip (the full-size and the counted full-size test fail)."""
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from pats_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

W = 6144                        # workgroups of the two walks (launch_third_fused / launch_third_fused3)
TRIP = 64 * W                   # problems one trip of the outer loop covers
FULL = 414720                   # the headline batch (tests/test_determinism_gpu.py launches the same size)
K, NWILD = 96, 32               # base set: problems 0..31 wild, 32..95 tame
AMPS = np.tile(np.array([3.0, 5.0, 9.0, 14.0], np.float32), NWILD // 4)    # test_stabilised_third_level_resolve_...'s amplitudes
MIN_TRIPS = 8                   # of the 32 wild base problems, launched alone
REDO = 0xEE                     # THIRD_REDO (csrc/third_device.hpp)
NAN_BITS = 0x7FC00000
CLEAR_REL = 1e-3                # the `clear` mask of test_third_level_guard_trips_are_resolved_by_the_scan_kernel
CLEAR_CAP = 0.02                # share of (wild problem, centre row) entries the mask may leave out
M1_TOL = 3e-4 * 8               # tests/test_gpu_parity.py's gate on mkpts1_f, px
NAMES = ("mkpts0_f", "mkpts1_f", "label", "if_matching1")


def walk_slot(p, P):
    """(workgroup, lane, trip) of the walk that looks at problem p in a launch over P problems (or a capacity of P)."""
    w = min(P, W)
    return p % w, (p % (64 * w)) // w, p // (64 * w)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def per_problem(outs, P):
    """The four outputs as [P, ...] (label comes as [P * 16, 2])."""
    m0, m1, label, ifm = outs
    return m0, m1, label.view(P, 16, 2), ifm


def prefilled(P):
    """Output buffers of a launch: floats NaN, if_matching1 the sentinel of the walk."""
    nan = lambda *s: torch.full(s, NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)     # noqa: E731
    return nan(P, 16, 2), nan(P, 16, 2), nan(P * 16, 2), torch.full((P, 16), REDO, dtype=torch.uint8, device="cuda")


def gathered(base, sel):
    """The inputs of the launch that idx vector `sel` (on the device) describes."""
    return tuple(torch.index_select(t, 0, sel) for t in base.dev)


def run_third(ops, inputs, count=None):
    """One launch over `inputs` (d0, d1, scale, p_s, p_t) into pre-filled buffers.  Returns (outputs, guard trips counted)."""
    d0, d1, scale, ps, pt = inputs
    out = prefilled(d0.shape[0])
    ops.sinkhorn_fallbacks(reset=True)
    got = ops.third_level(d0, d1, scale, ps, pt, outdoor=True, out=out,
                          count=None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda"))
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    return out, ops.sinkhorn_fallbacks(reset=True)


def make_base(ops, oracle):
    """The base set, its oracle reference, each wild problem's trip count alone, and the 96-problem launch everything else is
    compared with - checked here against the oracle, so that nothing later passes on a base that is wrong or never trips."""
    inp = synth.third_inputs(seed=synth.SEED + 64, P=K)
    d0, d1 = inp["d0"].copy(), inp["d1"].copy()
    d0[:NWILD] *= AMPS[:, None, None]
    d1[:NWILD] *= AMPS[:, None, None]
    Zr = oracle.log_optimal_transport2(oracle.cost(d0, d1), 1.0, inp["scale"], 100)
    sq = np.sqrt(inp["scale"] + np.float32(1e-8)).astype(np.float32)
    r0, r1, _, rlabel, rifm = oracle.compute_result(np.exp(Zr), sq, sq, inp["p_s"], inp["p_t"], True)
    assert np.isfinite(Zr).all() and np.isfinite(r1).all(), "the oracle's own result is not finite"
    S = np.exp(Zr)[:NWILD, :-1, :].reshape(NWILD, 8, 8, 65)[:, 2:6, 2:6, :].reshape(NWILD, 16, 65)
    top = np.sort(S, axis=2)[:, :, -2:]
    clear = (top[:, :, 1] - top[:, :, 0]) > CLEAR_REL * top[:, :, 1]
    unclear = 1.0 - clear.mean()
    assert unclear <= CLEAR_CAP, "the near-tie mask leaves out %.2f %% of the wild centre rows (cap %.0f %%)" % (100 * unclear, 100 * CLEAR_CAP)

    base = SimpleNamespace(dev=(cu(d0), cu(d1), cu(inp["scale"]), cu(inp["p_s"]), cu(inp["p_t"])), unclear=unclear)
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    base.trips = np.array([run_third(ops, gathered(base, one + i))[1] for i in range(NWILD)], dtype=np.int64)
    assert set(base.trips.tolist()) <= {0, 1}, "a single problem counted %s guard trips" % sorted(set(base.trips.tolist()))
    assert base.trips.sum() >= MIN_TRIPS, ("only %d of the %d wild base problems trip the guard (need %d): trips by amplitude %s"
                                           % (base.trips.sum(), NWILD, MIN_TRIPS, trips_by_amp(base.trips)))
    base.trips_dev = cu(np.concatenate([base.trips, np.zeros(K - NWILD, np.int64)]))
    # tripping problems in an order whose neighbours differ in amplitude wherever more than one amplitude trips
    by_amp = [[i for i in range(NWILD) if base.trips[i] and AMPS[i] == a] for a in (3.0, 5.0, 9.0, 14.0)]
    base.tripping = [g[j] for j in range(NWILD) for g in by_amp if j < len(g)]

    outs, n = run_third(ops, base.dev)
    base.out = per_problem(outs, K)
    assert n == base.trips.sum(), "the 96-problem launch counted %d guard trips, its problems alone %d" % (n, base.trips.sum())
    m0, m1, label, ifm = (t.cpu().numpy() for t in base.out)
    assert set(np.unique(ifm)) <= {0, 1}, "if_matching1 of the base launch holds %s" % np.unique(ifm)
    assert np.array_equal(m0, r0), "mkpts0_f of the base launch differs from the oracle"
    tame = slice(NWILD, K)
    assert np.array_equal(label[tame], rlabel.reshape(K, 16, 2)[tame]), "label of a tame base problem differs from the oracle"
    assert np.array_equal(ifm.astype(bool)[tame], rifm.astype(bool)[tame]), "if_matching1 of a tame base problem differs from the oracle"
    d = np.abs(m1[tame] - r1[tame]).max()
    assert d <= M1_TOL, "mkpts1_f of a tame base problem is %g px off the oracle" % d
    assert np.array_equal(ifm.astype(bool)[:NWILD][clear], rifm.astype(bool)[:NWILD][clear]), \
        "if_matching1 of a wild base problem differs from the oracle away from near-ties"
    assert np.isfinite(m1).all() and np.isfinite(label).all(), "a base result is not finite"
    return base


def trips_by_amp(trips):
    return {float(a): int(trips[AMPS == a].sum()) for a in (3.0, 5.0, 9.0, 14.0)}


def mixed_group(base, j, n=4):
    """n different tripping base problems for one workgroup, neighbours of different amplitude where the tripping set allows."""
    rot = (j * n) % len(base.tripping)
    pool, group = base.tripping[rot:] + base.tripping[:rot], []
    for _ in range(n):
        rest = [b for b in pool if b not in group]
        other = [b for b in rest if group and AMPS[b] != AMPS[group[-1]]]
        group.append((other or rest)[0])
    return group


class Layout:
    """idx[P] into the base set: tame problems cycling by default, wild ones where put() places them."""

    def __init__(self, base, P):
        self.base, self.P, self.n = base, P, 0
        self.idx = NWILD + np.arange(P, dtype=np.int64) % (K - NWILD)
        self.wild = {}

    def put(self, p, cycle_all=False, b=None):
        """A wild problem at p: base problem b, else the next one that trips alone, or (cycle_all) the next of all 32."""
        if 0 <= p < self.P and p not in self.wild:
            pool = list(range(NWILD)) if cycle_all else self.base.tripping
            self.idx[p] = self.wild[p] = pool[self.n % len(pool)] if b is None else b
            self.n += 1
        return self

    def expected_trips(self, live):
        return int(sum(self.base.trips[b] for p, b in self.wild.items() if p < live))

    def describe(self, p):
        return "problem %d (workgroup %d, lane %d, trip %d; base problem %d%s)" % (
            (p,) + walk_slot(p, self.P) + (int(self.idx[p]), ", wild x%g" % AMPS[self.idx[p]] if self.idx[p] < NWILD else ", tame"))


def check_rows(lay, outs, want, rows, what):
    """outs[:rows] == want, bit for bit in all four outputs; names the first rows that differ and where the walk had them."""
    bad = torch.zeros(rows, dtype=torch.bool, device="cuda")
    which = []
    for name, g, w in zip(NAMES, per_problem(outs, lay.P), want):
        diff = (bits(g[:rows]) != bits(w)).flatten(1).any(1)
        if bool(diff.any()):
            which.append(name)
            bad |= diff
    if which:
        rows_bad = bad.nonzero().flatten()
        first = [int(p) for p in rows_bad[:6]]
        left = int((outs[3][:rows, 0] == REDO).sum())
        raise AssertionError("%s: %d of %d live problems differ from the base launch in %s (%d still carry the sentinel): %s"
                             % (what, rows_bad.numel(), rows, ", ".join(which), left, "; ".join(lay.describe(p) for p in first)))
    assert rows == 0 or int(outs[3][:rows].max()) <= 1, "%s: if_matching1 holds values other than 0 and 1" % what


def check_untouched(lay, outs, rows, what):
    """Every byte of the rows at or past `rows` is still the pre-fill."""
    for name, g in zip(NAMES, per_problem(outs, lay.P)):
        tail = bits(g[rows:])
        hit = (tail != (REDO if name == "if_matching1" else NAN_BITS)).flatten(1).any(1).nonzero().flatten()
        if hit.numel():
            first = [rows + int(p) for p in hit[:6]]
            raise AssertionError("%s: %d rows at or past the count %d were written (%s): %s"
                                 % (what, hit.numel(), rows, name, "; ".join(lay.describe(p) for p in first)))


def check_launch(ops, lay, what, count=None):
    """One launch of the layout, plain or counted: live rows against the base launch, the fallback counter against the wild
    problems that are live, and for a counted launch the rows past the count and the plain launch over exactly `count` rows."""
    base = lay.base
    live = lay.P if count is None else max(0, min(count, lay.P))
    sel = cu(lay.idx)
    inputs = gathered(base, sel)
    outs, trips = run_third(ops, inputs, count=count)
    check_rows(lay, outs, [w[sel[:live]] for w in base.out], live, what)
    assert trips == lay.expected_trips(live), "%s: %d guard trips counted, %d wild live problems trip alone" % (what, trips, lay.expected_trips(live))
    assert trips == int(base.trips_dev[sel[:live]].sum())
    if count is not None:
        check_untouched(lay, outs, live, what)
        if live:
            # sqrt(scale + 1e-8) formed in the kernel (counted) against the caller's (plain): the same bits
            plain, ptrips = run_third(ops, tuple(t[:live] for t in inputs))
            for name, g, w in zip(NAMES, per_problem(outs, lay.P), per_problem(plain, live)):
                assert torch.equal(bits(g[:live]), bits(w)), "%s: %s differs from the plain launch over %d rows" % (what, name, live)
            assert ptrips == trips
    return trips


# ---- the cases (also run by the PATS_THIRD_STAB=0 child: anything added here is added there) ------------------------------
def case_grid_edge(ops, base, P):
    """Wild problems on either side of the grid's edge; P = 6145 is the launch in which exactly one workgroup has a second lane."""
    lay = Layout(base, P)
    for p in (0, 1, W - 1, W, P - 1, 2 * W - 1, 2 * W):
        lay.put(p)
    assert check_launch(ops, lay, "grid edge, P = %d" % P) >= 3


def case_same_workgroup(ops, base):
    """Workgroup q re-solves four different wild problems (lanes 0, 1, 3, 7) with a tame one (lane 2) between them: whatever the
    previous problem left in LDS or registers would change the bits of the next."""
    lay = Layout(base, 8 * W)
    amps = len({AMPS[b] for b in base.tripping})
    for j, q in enumerate((0, 17, W - 1)):
        group = mixed_group(base, j)
        assert len(set(group)) == 4 and len({AMPS[b] for b in group}) >= min(2, amps)
        for lane, b in zip((0, 1, 3, 7), group):
            lay.put(q + lane * W, b=b)
            assert walk_slot(q + lane * W, lay.P) == (q, lane, 0)
        assert lay.idx[q + 2 * W] >= NWILD
    assert check_launch(ops, lay, "four problems per workgroup, P = 8 x 6144") == 12


def case_run(ops, base):
    """What one wild fine row produces: 200 consecutive wild problems, across the grid's edge, cycling through all 32."""
    lay = Layout(base, 3 * W)
    for p in range(W - 100, W + 100):
        lay.put(p, cycle_all=True)
    check_launch(ops, lay, "run of 200 across 6144, P = 3 x 6144")


FULL_PICKS = (0, W - 1, W, 2 * W - 1, TRIP - 1, TRIP, TRIP + W, FULL - 1)
FULL_SLOTS = ((0, 0, 0), (6143, 0, 0), (0, 1, 0), (6143, 1, 0), (6143, 63, 0), (0, 0, 1), (0, 1, 1), (3071, 3, 1))


def full_layout(base):
    lay = Layout(base, FULL)
    for p in FULL_PICKS + (5, 5 + W, 5 + TRIP):           # the second group: one workgroup, two lanes and both trips
        lay.put(p)
    for p in range(TRIP - 50, TRIP + 50):                 # a run across the end of the first trip
        lay.put(p, cycle_all=True)
    for p in range(1009, FULL, 1009):                     # a prime stride: every lane index, both trips
        lay.put(p, cycle_all=True)
    return lay


def case_full_size(ops, base):
    assert tuple(walk_slot(p, FULL) for p in FULL_PICKS) == FULL_SLOTS
    assert [walk_slot(p, FULL) for p in (5, 5 + W, 5 + TRIP)] == [(5, 0, 0), (5, 1, 0), (5, 0, 1)]
    lay = full_layout(base)
    tripping = [p for p, b in lay.wild.items() if base.trips[b]]
    assert {walk_slot(p, FULL)[1] for p in lay.wild} == set(range(64)), "a lane index has no wild problem"
    assert {1, 3, 63} <= {walk_slot(p, FULL)[1] for p in tripping} and {walk_slot(p, FULL)[2] for p in tripping} == {0, 1}
    print("P = %d: lanes with a problem that trips: %d of 64" % (FULL, len({walk_slot(p, FULL)[1] for p in tripping})))
    for p in FULL_PICKS:
        print("P = %d: %s" % (FULL, lay.describe(p)))
    trips = check_launch(ops, lay, "full size, P = %d, D = 128" % FULL)
    print("P = %d: %d wild problems, %d guard trips" % (FULL, len(lay.wild), trips))


def counts(cap):
    return 0, 1, 70, W, W + 1, cap - 1, cap, cap + 10 ** 6


def counted_layout(base, cap, count):
    """Wild problems below the count (count - 1 and the grid-edge positions) and at or past it (count, count + 1,
    count + 6144, cap - 1): those must stay exactly as the pre-fill left them, sentinel included."""
    lay = Layout(base, cap)
    for p in (count - 1, count, count + 1, count + W, cap - 1, 0, 1, W - 1, W, 2 * W - 1, 2 * W, TRIP - 1, TRIP, TRIP + W):
        lay.put(p)
    return lay


def case_counted(ops, base, cap, count):
    lay = counted_layout(base, cap, count)
    live = min(count, cap)
    assert live == 0 or any(p < live for p in lay.wild)
    assert live == cap or any(p >= live for p in lay.wild)
    check_launch(ops, lay, "counted launch, capacity %d, count %d" % (cap, count), count=count)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from pats_amd import ops as o
    prev = o.set_sinkhorn_mode("kernel")                  # the guarded linear solver: the log mode has no guard and no walk
    yield o
    o.set_sinkhorn_mode(prev)
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def base(ops, oracle):
    return make_base(ops, oracle)


def test_walk_slot_is_the_kernels_loop():
    """walk_slot against the loop of third_fused_kernel / third_fused3_stab_kernel, modelled directly."""
    for P in (1, 70, 600, W, W + 1, 2 * W + 5, FULL):
        w = min(P, W)
        seen = np.full((P, 3), -1, np.int64)
        for trip, start in enumerate(range(0, P, 64 * w)):
            first = start + np.arange(w)[:, None]                        # first = blockIdx.x + trip * 64 W
            cand = first + np.arange(64)[None, :] * w                    # cand = first + lane * W
            wg, lane = np.broadcast_arrays(np.arange(w)[:, None], np.arange(64)[None, :])
            ok = (first < P) & (cand < P)
            seen[cand[ok]] = np.stack([wg[ok], lane[ok], np.full(ok.sum(), trip)], 1)
        assert (seen >= 0).all()
        probe = np.unique(np.clip(np.array([0, 1, w - 1, w, 2 * w - 1, 64 * w - 1, 64 * w, 64 * w + w, P - 1, P // 2]), 0, P - 1))
        for p in probe:
            assert walk_slot(int(p), P) == tuple(seen[p]), (p, P)
    assert {walk_slot(p, 600)[1:] for p in range(600)} == {(0, 0)}       # what the suite covered before this file


def test_base_set_trips_and_agrees_with_the_oracle(base):
    """The fixture's checks (make_base), reported: how many wild base problems trip alone, by amplitude."""
    print("guard trips alone: %d of %d, by amplitude %s; near-tie mask leaves out %.2f %% of the wild centre rows"
          % (base.trips.sum(), NWILD, trips_by_amp(base.trips), 100 * base.unclear))
    assert base.trips.sum() >= MIN_TRIPS and len(base.tripping) == base.trips.sum()


@pytest.mark.parametrize("P", [W, W + 1, W + 70, 2 * W + 5])
def test_wild_problems_at_the_grid_edge(ops, base, P):
    case_grid_edge(ops, base, P)


def test_one_workgroup_resolves_four_problems(ops, base):
    case_same_workgroup(ops, base)


def test_a_run_of_wild_problems_across_the_grid_edge(ops, base):
    case_run(ops, base)


def test_full_size_launch_takes_every_lane_and_a_second_trip(ops, base):
    """414 720 problems at D = 128 (two 13.8 GB descriptor tensors, gathered on the device)."""
    try:
        case_full_size(ops, base)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("cap", [2 * W + 5, FULL])
def test_counted_launches_leave_rows_past_the_count_alone(ops, base, cap):
    """pats_third_level_counted_f32 over a capacity, the count on the device: flagged problems on both sides of the count."""
    try:
        for count in counts(cap):
            case_counted(ops, base, cap, count)
    finally:
        torch.cuda.empty_cache()


CHILD_CASES = (["grid_edge:%d" % P for P in (W, W + 1, W + 70, 2 * W + 5)] + ["same_workgroup", "run"]
               + ["counted:%d:%d" % (2 * W + 5, c) for c in (W + 1, 2 * W + 4)]
               + ["full_size", "counted:%d:%d" % (FULL, FULL - 1)])      # the scan kernel's own second trip


def test_scan_kernel_walk_alone_under_PATS_THIRD_STAB_0(tmp_path):
    """PATS_THIRD_STAB is read once per process: a child with it at 0 sends every flagged problem to the scan kernel's walk.  The
    child builds its own base launch (checked against the oracle there too) and compares with that, bit for bit."""
    report = str(tmp_path / "child.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), report] + CHILD_CASES, env=dict(os.environ, PATS_THIRD_STAB="0"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:] + "\n" + r.stderr[-3000:])
    with open(report) as f:
        done = json.load(f)
    assert done["stab"] == "0" and done["cases"] == CHILD_CASES and done["trips"] >= MIN_TRIPS


def child_main(report, cases):
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import pats_oracle
    pats_oracle.lib()
    from pats_amd import ops as o
    o.set_sinkhorn_mode("kernel")
    b = make_base(o, pats_oracle)
    for case in cases:
        name, *args = case.split(":")
        {"grid_edge": case_grid_edge, "same_workgroup": case_same_workgroup, "run": case_run, "counted": case_counted,
         "full_size": case_full_size}[name](o, b, *map(int, args))
        print("ok", case, flush=True)
    with open(report, "w") as f:
        json.dump({"stab": os.environ.get("PATS_THIRD_STAB"), "cases": cases, "trips": int(b.trips.sum())}, f)


if __name__ == "__main__":
    t0 = time.time()
    child_main(sys.argv[1], sys.argv[2:])
    print("%.1f s" % (time.time() - t0))
