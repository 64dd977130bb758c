"""CPU-only: the numpy restatement of the per-pair local optimisation (tests/polish_cases.py) on its committed seeds - LO from a noisy
minimal-sample model gains support, and a walk that loses support in a later round keeps its best - and the new entry points: declared
and exported with the header's argument counts, every bad argument refused before any launch with a message that names it, the Python
layers refusing what they must.  No kernel runs here (tests/test_polish_gpu.py runs them)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import epipolar_cases as ec
import polish_cases as pz
from conftest import REPO

POLISH = {"pats_epipolar_polish_workspace_bytes": (ctypes.c_size_t, 3), "pats_epipolar_polish_by_pair_f32": (ctypes.c_int, 25),
          "pats_homography_polish_workspace_bytes": (ctypes.c_size_t, 3), "pats_homography_polish_by_pair_f32": (ctypes.c_int, 25)}
A16 = 0x7f0000001000        # a fake device address: validation refuses before anything touches it


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.fixture(autouse=True)
def entry_points(lib):
    """The cases describe entry points of the built library: without them nothing here has a subject."""
    for name in POLISH:
        getattr(lib, name)


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib, build
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in POLISH.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "polish.hip" in build.SOURCES
    assert lib.pats_epipolar_polish_workspace_bytes(48, 1, 2 ** 31 - 2) == 0 == lib.pats_homography_polish_workspace_bytes(48, 1, 100)
    src = open(os.path.join(REPO, "pats_amd", "csrc", "polish.hip")).read()
    assert int(re.search(r"constexpr int POLISH_MAX_ROUNDS = (\d+);", src).group(1)) == pz.MAX_ROUNDS
    # the shared device code is used, not copied
    csrc = os.path.join(REPO, "pats_amd", "csrc")
    for fn, home in (("void test2(", "verify.hpp"), ("double verify_moments_sum(", "verify.hpp"), ("bool pose_decompose(", "refit.hpp"),
                     ("int refit_eigvec(", "refit.hpp"), ("void hom_write(", "refit.hpp"), ("void jacobi9_sweeps(", "jacobi9.hpp"),
                     ("void epi_load(", "epipolar.hpp")):
        holders = sorted(f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f)) and fn in open(os.path.join(csrc, f)).read())
        assert holders == [home], (fn, holders)


@pytest.mark.parametrize("family,seed,n", pz.HELPS)
def test_lo_from_a_noisy_minimal_sample_gains_support(family, seed, n):
    c = pz.make_pair(family, seed, n)
    w = pz.walk64(family, c["ml"], c["mr"], c["model"], c["thr"], pz.HELPS_ROUNDS)
    print(family, seed, w["counts"].tolist())
    assert w["best_count"] - w["counts"][0] >= pz.GAIN * n
    assert w["best_count"] == w["counts"].max() and w["counts"][w["best_round"]] == w["best_count"]
    assert int(w["masks"][w["best_round"]].sum()) == w["best_count"]


@pytest.mark.parametrize("family,seed,n,outliers,noise,rounds", pz.KEEPS)
def test_a_walk_that_loses_support_keeps_its_best_round(family, seed, n, outliers, noise, rounds):
    c = pz.make_pair(family, seed, n, outliers=outliers, noise=noise)
    w = pz.walk64(family, c["ml"], c["mr"], c["model"], c["thr"], rounds)
    print(family, seed, w["counts"].tolist())
    b = w["best_round"]
    assert 0 < b < rounds and w["best_count"] == w["counts"].max() >= w["counts"][0]
    assert w["best_count"] - w["counts"][rounds] >= pz.KEEPS_MARGIN         # the last round is NOT the best
    assert not (w["counts"][:b] == w["best_count"]).any()                   # the lowest round among equals


@pytest.mark.parametrize("family", ["epipolar", "homography"])
def test_walk_ends_of_the_restatement(family):
    c = pz.make_pair(family, 3, 200)
    zero = pz.walk64(family, c["ml"], c["mr"], np.zeros((3, 3), np.float32), c["thr"], 3)
    assert not zero["counts"].any() and zero["best_round"] == 0 and not zero["models"].any()
    for thr in (np.float32("nan"), np.float32(-1.0)):
        w = pz.walk64(family, c["ml"], c["mr"], c["model"], thr, 3)
        assert not w["counts"].any() and w["best_round"] == 0 and np.array_equal(w["models"][0], c["model"]) and not w["models"][1:].any()
    few = pz.MIN_INLIERS[family] - 1                                        # c_0 < min_F: no refit, every later round zero
    w = pz.walk64(family, c["ml"][:few], c["mr"][:few], c["model"], np.float32(10.0), 3)
    assert w["counts"].tolist() == [few, 0, 0, 0] and w["best_round"] == 0
    same = np.tile(c["ml"][:1], (50, 1))                                    # one point fifty times: no model through it
    w = pz.walk64(family, same, same, c["model"], np.float32(10.0), 2)
    assert w["best_round"] == 0 and np.isfinite(w["models"]).all()
    part = ec.participates(c["ml"], c["mr"])
    assert part.all()


@pytest.mark.parametrize("family", ["epipolar", "homography"])
def test_every_bad_argument_is_refused_by_name(lib, family):
    assert pz.check_refusals(lib, family, A16) > 70


def test_ops_refuse_cpu_tensors_bad_layouts_and_bad_types():
    import torch
    from pats_amd import ops
    ml, mr, off = torch.zeros(20, 2), torch.zeros(20, 2), torch.tensor([0, 10, 20])
    models, thr, best = torch.zeros(2, 4, 3, 3), torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    for fn in (ops.epipolar_polish_by_pair, ops.homography_polish_by_pair):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(ml, mr, models, thr, best=best, pair_off=off)
        with pytest.raises(RuntimeError, match="matches_l must be contiguous"):
            fn(torch.zeros(20, 4)[:, ::2], mr, models, thr, best=best, pair_off=off)
        with pytest.raises(RuntimeError, match="models must be contiguous"):
            fn(ml, mr, models.transpose(2, 3), thr, best=best, pair_off=off)
        with pytest.raises(RuntimeError, match="matches_r must be float32"):
            fn(ml, mr.double(), models, thr, best=best, pair_off=off)
        with pytest.raises(RuntimeError, match="best must be int32"):
            fn(ml, mr, models, thr, best=best.long(), pair_off=off)
        with pytest.raises(RuntimeError, match="thr must be float32"):
            fn(ml, mr, models, thr.double(), best=best, pair_off=off)
        with pytest.raises(RuntimeError, match="pair_off must be int64"):
            fn(ml, mr, models, thr, best=best, pair_off=off.int())
        with pytest.raises(RuntimeError, match="min_conf needs conf"):
            fn(ml, mr, models, thr, best=best, pair_off=off, min_conf=0.5)
        for bad in (0, 17, -2):
            with pytest.raises(RuntimeError, match="rounds"):
                fn(ml, mr, models, thr, best=best, rounds=bad, pair_off=off)
        for kw in ({}, {"pair_off": off, "stride": 10, "counts": torch.tensor([3, 3])}, {"stride": 10}):
            with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
                fn(ml, mr, models, thr, best=best, **kw)
        assert str(inspect.signature(fn)) == ("(matches_l, matches_r, models, thr, best=None, rounds=4, pair_off=None, stride=None, "
                                              "counts=None, conf=None, min_conf=None, norm=None, out=None, pairs=None)")


def test_batch_polish_needs_a_verification():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}
    with pytest.raises(ValueError, match="verify_by_pair"):
        batch.polish_by_pair(dict(plain), cap, None)
    with pytest.raises(ValueError, match="verify_h_by_pair"):
        batch.polish_h_by_pair(dict(plain), cap, None)
    assert str(inspect.signature(batch.polish_by_pair)) == "(out, cap, thr, rounds=4, norm=None, min_conf=None)"
    assert str(inspect.signature(batch.polish_h_by_pair)) == "(out, cap, thr, rounds=4, norm=None, min_conf=None)"
