"""CPU-only: the numpy restatement of the per-pair MSAC scoring (tests/msac_cases.py) on its committed cases, and the C-ABI surface of
the feature.
  1  gain64 against a plain scalar loop of the MSAC cost: participating - cost == gain to 1e-9 relative
  2  a float32 emulation of the definition WITHOUT fused multiply-adds stays within the per-cell bound b on every committed case -
     the evidence that eps = 8 * 2^-24 is not too tight for plain float32 (the device's FMAs round less often).  The test prints
     the worst share of a bound that was used; docs/parity.md ("MSAC scoring") records it
  3  the cap that keeps the GPU test's sandwich from hiding a failure: S[h] = sum of b <= 4 for every model of every committed case
  4  every disagreement seed meets its two conditions: the count decidedly picks the perturbed model, the gain decidedly the true one
  5  the refusals through the C ABI: everything the count entries refuse, in their wording and order, then gains / best_gain
  6  the three new symbols are exported with the header's prototypes (tests/test_host_abi.py holds header == ctypes table)"""
import ctypes
import os
import re

import numpy as np
import pytest

import epipolar_cases as ec
import homography_cases as hm
import msac_cases as mc
from conftest import REPO

BASE = 0x7f0000001000


@pytest.fixture(scope="module")
def cases():
    """Every committed case with its points, gains and bounds, computed once."""
    out = []
    for fam, label, c in mc.committed_cases():
        xl, xr = ec.points32(c["ml"], c["mr"])
        part = ec.participates(xl, xr)
        out.append({"family": fam, "label": label, "xl": xl, "xr": xr, "part": part, "models": c["models"], "thr": c["thr"],
                    "g64": mc.gain64(fam, xl, xr, part, c["models"], c["thr"]), "b": mc.slack(fam, xl, xr, part, c["models"], c["thr"])})
    return out


def test_the_committed_cases_cover_both_families_three_thresholds_and_the_disagreements():
    labels = [(fam, label) for fam, label, _ in mc.committed_cases()]
    for fam in mc.FAMILIES:
        assert sum(1 for f, l in labels if f == fam and l.startswith("host")) == 6 * len(mc.THRS)
        assert len(mc.DISAGREEMENTS[fam]) >= 3
    assert mc.THRS == (5e-4, 2e-3, 1e-2) and mc.ONE == 1 << 20


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_gain_is_participating_minus_the_plain_loop_cost(family):
    seed, n, H = (103, 500, 64)
    for thr in mc.THRS + (0.0,):
        c = mc.make_case(family, seed, n, H, thr)
        xl, xr = ec.points32(c["ml"], c["mr"])
        xl[7, 0] = np.nan                                                         # a match that does not participate
        part = ec.participates(xl, xr)
        models = c["models"][:12].copy()
        models[0] = c["models"][c["true"]]
        models[5] = 0                                                             # a zero model: no inliers, cost = participating
        cost, m = mc.cost64_loop(family, xl, xr, part, models, thr)
        gain = mc.gain64(family, xl, xr, part, models, thr).sum(1)
        assert m == n - 1 and gain[5] == 0 and cost[5] == m
        assert np.all(np.abs((m - cost) - gain) <= 1e-9 * np.maximum(1.0, gain)), (thr, (m - cost) - gain)
        if thr > 0:
            assert gain.argmax() == 0 and gain[0] > 10                            # the true model
    for bad in (np.nan, -1.0):
        assert not mc.gain64(family, xl, xr, part, models, bad).any() and not mc.slack(family, xl, xr, part, models, bad).any()


def test_float32_without_fma_stays_within_the_bound_cell_by_cell(cases):
    worst, where = 0.0, None
    for c in cases:
        g32 = mc.gain32(c["family"], c["xl"], c["xr"], c["part"], c["models"], c["thr"]) / mc.ONE
        err = np.abs(g32 - c["g64"])
        assert np.all(err <= c["b"]), (c["label"], float((err - c["b"]).max()))
        used = float(np.max(np.where(c["b"] > 0, err / np.where(c["b"] > 0, c["b"], 1.0), 0.0)))
        if used > worst:
            worst, where = used, (c["family"], c["label"])
    print("float32 without FMA: the worst cell used %.3f of its bound (%s)" % (worst, where))
    assert worst > 0.05, "the bound is so loose that the emulation says nothing about it"


def test_the_summed_bound_is_at_most_four_gain_units(cases):
    worst = max((float(c["b"].sum(1).max()), c["family"], c["label"]) for c in cases)
    print("largest S[h] over the committed cases: %.3f (%s, %s)" % worst)
    for c in cases:
        assert np.all(c["b"].sum(1) <= 4.0), (c["label"], float(c["b"].sum(1).max()))


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_every_disagreement_seed_meets_its_two_conditions(family):
    for seed, n in mc.DISAGREEMENTS[family]:
        kept, r = mc.disagrees(family, mc.disagreement_case(family, seed, n))
        print("%s seed %d n %d: strict %s loose %s G64 %s S %s" % (family, seed, n, r["strict"], r["loose"], np.round(r["G64"], 2), np.round(r["S"], 3)))
        assert kept, (family, seed, n)
        assert r["strict"][0] > r["loose"][1] and r["G64"][1] - r["S"][1] > r["G64"][0] + r["S"][0] + 1
        assert r["G64"][3] == 0 and r["S"][3] == 0                                # the zero model


def test_rules_that_do_not_depend_on_rounding():
    c = mc.make_case("epipolar", 7, 200, 4, 2e-3)
    xl, xr = ec.points32(c["ml"], c["mr"])
    conf = np.linspace(0, 1, 200).astype(np.float32)
    part = ec.participates(xl, xr, conf, 0.5)
    for fam in mc.FAMILIES:
        g, b = mc.gain64(fam, xl, xr, part, c["models"], 2e-3), mc.slack(fam, xl, xr, part, c["models"], 2e-3)
        assert not g[:, ~part].any() and not b[:, ~part].any()
        assert (g >= 0).all() and (g <= 1).all() and (b >= 0).all() and (b <= 1).all()
        g32 = mc.gain32(fam, xl, xr, part, c["models"], 2e-3)
        assert g32.min() >= 0 and g32.max() <= mc.ONE and not g32[:, ~part].any()


# ---- the C-ABI surface ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_library_exports_the_three_symbols_with_the_headers_prototypes(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert "Per-pair MSAC scoring (ABI 8, symbols added)" in header
    for name, nargs in (("pats_msac_gain_one", 0), ("pats_epipolar_score_msac_by_pair_f32", 24), ("pats_homography_score_msac_by_pair_f32", 24)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs and name in _lib.SIGNATURES and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
        if nargs:                                                                 # the count entry's list through stream, then the two
            count = re.search(r"\b%s\(([^;]*)\);" % name.replace("_msac", ""), header).group(1)
            assert [p.split()[-1] for p in params[:22]] == [p.strip().split()[-1] for p in count.replace("\n", " ").split(",")]
            assert [p.replace(" ", "") for p in params[22:]] == ["int64_t*gains", "int64_t*best_gain"]
    assert lib.pats_msac_gain_one() == mc.ONE
    assert lib.pats_abi_version() == 8


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_what_the_count_entry_refuses_is_refused_in_its_wording_and_order(lib, family):
    """Fake device addresses: validation refuses them before anything touches them."""
    cases = hm.refusals(lib, "score", BASE)
    assert len(cases) > 40
    for kw, words in cases:
        assert mc.c_call(lib, family, BASE, count=True, **kw) != 0
        want = lib.pats_last_error()
        # a null gains on top: the count entry's refusal still comes first
        assert mc.c_call(lib, family, BASE, gains=0, **kw) != 0, kw
        got = lib.pats_last_error()
        assert mc.ENTRY[family]["tag"] in got and all(w in got for w in words), (kw, got)
        assert got == want.replace(mc.COUNT_TAG[family], mc.ENTRY[family]["tag"]), (kw, got, want)


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_a_null_or_misaligned_gain_output_is_refused_by_name(lib, family):
    for name in ("gains", "best_gain"):
        assert mc.c_call(lib, family, BASE, **{name: 0}) != 0
        msg = lib.pats_last_error()
        assert mc.ENTRY[family]["tag"] in msg and b"null" in msg and name.encode() in msg, msg
        for off in (1, 2, 4):
            assert mc.c_call(lib, family, BASE, **{name: BASE + off}) != 0
            msg = lib.pats_last_error()
            assert mc.ENTRY[family]["tag"] in msg and b"8-byte aligned" in msg and name.encode() in msg, msg
    # gains comes before best_gain; "best_gain" is not mistaken for "gains" in the first message
    assert mc.c_call(lib, family, BASE, gains=0, best_gain=0) != 0
    assert b"null gains" in lib.pats_last_error()


def test_ops_and_batch_signatures_and_refusals_without_a_gpu():
    import inspect
    from pats_amd import batch, ops
    for name in ("epipolar_score", "homography_score"):
        count, msac = getattr(ops, name + "_by_pair"), getattr(ops, name + "_msac_by_pair")
        assert list(inspect.signature(count).parameters) == list(inspect.signature(msac).parameters)
    for count, msac in ((batch.verify_by_pair, batch.verify_msac_by_pair), (batch.verify_h_by_pair, batch.verify_h_msac_by_pair)):
        assert str(inspect.signature(count)) == str(inspect.signature(msac))
        cap = batch.Capacities(2, 5, 6)
        plain = {"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}
        with pytest.raises(ValueError, match="on must be"):                      # the shared checks, before any device work
            msac(dict(plain), cap, None, None, on="best")
        with pytest.raises(ValueError, match="confidence=True"):
            msac(dict(plain), cap, None, None, min_conf=0.5)
