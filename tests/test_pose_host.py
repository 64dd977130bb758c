"""CPU-only: the per-pair pose entry points (ABI 8, symbols added) are declared and exported with the argument counts of the
header, refuse every bad argument before any launch with a message that names it, and the Python layers refuse what they must.
No kernel runs here: every C call below fails validation.  (tests/test_pose_gpu.py repeats the refusals on a machine with a GPU,
where a launch would be possible.)"""
import ctypes
import inspect
import os
import re

import pytest

from conftest import REPO

POSE = {"pats_epipolar_pose_workspace_bytes": (ctypes.c_size_t, 2), "pats_epipolar_pose_by_pair_f64": (ctypes.c_int, 26)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in POSE.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "pose.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES
    # the stages share one way of forming a match's point
    csrc = os.path.join(REPO, "pats_amd", "csrc")
    assert "void epi_load(" in open(os.path.join(csrc, "epipolar.hpp")).read()
    assert "void epi_load(" not in open(os.path.join(csrc, "epipolar.hip")).read()


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
REQUIRED = ("matches_l", "matches_r", "inlier", "best_count", "E", "R", "t", "front_counts", "choice", "front_count")
OPTIONAL = ("pair_off", "counts_in", "moments", "models", "best", "norm", "front", "e_refit")
ALIGN = {"matches_l": 8, "matches_r": 8, "moments": 8, "E": 8, "R": 8, "t": 8, "e_refit": 8, "pair_off": 8, "counts_in": 8,
         "best_count": 8, "front_count": 8, "models": 4, "best": 4, "norm": 4, "front_counts": 4, "choice": 4}
ORDER = ("matches_l", "matches_r", "inlier", "pair_off", "stride", "counts_in", "pairs", "cap", "best_count", "moments", "models", "H",
         "best", "norm", "swapped", "E", "R", "t", "front_counts", "choice", "front_count", "front", "e_refit")


def call(lib, pairs=2, cap=100, H=8, stride=0, swapped=0, ws=A16, ws_bytes=1 << 20, **ptrs):
    a = {n: A16 for n in REQUIRED + OPTIONAL}
    a["counts_in"] = 0                                   # the ragged form unless a test says otherwise
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    p.update(pairs=pairs, cap=cap, H=H, stride=stride, swapped=swapped)
    return lib.pats_epipolar_pose_by_pair_f64(*[p[n] for n in ORDER], ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def refusals(lib, base=A16):
    """Every refusal of the header's list -> [(keyword arguments of call(), the words the message must hold)]; `base`: the address
    the misaligned pointers are derived from."""
    max_h = lib.pats_epipolar_max_h()
    strided = {"pair_off": 0, "counts_in": base}
    out = [({name: 0}, (b"null", name.encode())) for name in REQUIRED]
    for name in sorted(ALIGN):
        form = dict(strided, stride=10) if name == "counts_in" else {}
        out += [(dict(form, **{name: base + off}), (b"%d-byte aligned" % ALIGN[name], name.encode()))
                for off in ((1, 2, 3) if ALIGN[name] == 4 else (1, 2, 4))]
    out += [(dict(strided, pair_off=base, stride=10), (b"pair_off", b"counts_in")), ({"pair_off": 0}, (b"pair_off", b"counts_in"))]
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"cap": -1}, b"cap"),
                                           ({"cap": 2 ** 31 - 1}, b"cap"), ({"cap": 2 ** 40}, b"cap"), ({"swapped": 2}, b"swapped"),
                                           ({"swapped": -1}, b"swapped"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="),
                                           ({"H": max_h + 1}, b"max_h"), ({"moments": 0, "H": 0}, b"H ="))]
    out += [(kw, (b"moments", b"models", b"best")) for kw in ({"moments": 0, "models": 0}, {"moments": 0, "best": 0},
                                                               {"moments": 0, "models": 0, "best": 0})]
    out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                            {"stride": 1, "cap": 0})]
    need = lib.pats_epipolar_pose_workspace_bytes(2, 100)
    if need > 0:                                         # 0 today: then no size can be too small
        out.append(({"ws_bytes": need - 1}, (b"workspace",)))
    return out


def refused(lib, kw, words):
    assert call(lib, **kw) != 0, kw
    msg = lib.pats_last_error()
    assert b"epipolar_pose_by_pair" in msg and all(w in msg for w in words), (kw, msg)


def test_every_bad_argument_is_refused_by_name(lib):
    cases = refusals(lib)
    assert len(cases) > 70
    for kw, words in cases:
        refused(lib, kw, words)
    assert lib.pats_epipolar_pose_workspace_bytes(48, 2 ** 31 - 2) < (1 << 32)


def test_ops_refuses_cpu_tensors_bad_layouts_and_bad_types():
    import torch
    from pats_amd import ops
    ml, mr, off = torch.zeros(20, 2), torch.zeros(20, 2), torch.tensor([0, 10, 20])
    inl, bc, mom = torch.zeros(20, dtype=torch.uint8), torch.tensor([10, 10]), torch.zeros(2, 9, 9, dtype=torch.float64)
    models, best = torch.zeros(2, 4, 3, 3), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="matches_l must be contiguous"):
        ops.epipolar_pose_by_pair(torch.zeros(20, 4)[:, ::2], mr, inl, bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="moments must be contiguous"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom.transpose(1, 2), pair_off=off)
    with pytest.raises(RuntimeError, match="norm must be contiguous"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom, pair_off=off, norm=torch.zeros(8, 2).t())
    with pytest.raises(RuntimeError, match="matches_r must be float32"):
        ops.epipolar_pose_by_pair(ml, mr.double(), inl, bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="inlier must be uint8"):
        ops.epipolar_pose_by_pair(ml, mr, inl.bool(), bc, moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="best_count must be int64"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc.int(), moments=mom, pair_off=off)
    with pytest.raises(RuntimeError, match="moments must be float64"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom.float(), pair_off=off)
    with pytest.raises(RuntimeError, match="best must be int32"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, models=models, best=best.long(), pair_off=off)
    with pytest.raises(RuntimeError, match="models must be float32"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, models=models.double(), best=best, pair_off=off)
    with pytest.raises(RuntimeError, match="pair_off must be int64"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom, pair_off=off.int())
    with pytest.raises(RuntimeError, match="counts must be int64"):
        ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom, stride=10, counts=torch.tensor([3, 3], dtype=torch.int32))
    for kw in ({}, {"pair_off": off, "stride": 10, "counts": torch.tensor([3, 3])}, {"stride": 10}, {"counts": torch.tensor([3, 3])}):
        with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
            ops.epipolar_pose_by_pair(ml, mr, inl, bc, moments=mom, **kw)
    for kw in ({}, {"models": models}, {"best": best}):
        with pytest.raises(RuntimeError, match="give moments, or models and best"):
            ops.epipolar_pose_by_pair(ml, mr, inl, bc, pair_off=off, **kw)
    assert str(inspect.signature(ops.epipolar_pose_by_pair)) == (
        "(matches_l, matches_r, inlier, best_count, moments=None, models=None, best=None, pair_off=None, stride=None, counts=None, "
        "norm=None, swapped=False, return_front=False, return_refit=False, out=None, pairs=None)")


def test_batch_pose_by_pair_needs_a_verification():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}
    with pytest.raises(ValueError, match="verify_by_pair"):
        batch.pose_by_pair(dict(plain), cap)
    with pytest.raises(ValueError, match="pose_by_pair"):
        batch.split_pose_by_pair(dict(plain), cap)
    assert str(inspect.signature(batch.pose_by_pair)) == "(out, cap, norm=None, swapped=False, front=False)"
    assert str(inspect.signature(batch.split_pose_by_pair)) == "(out, cap)"
    assert str(inspect.signature(batch.verify_by_pair)) == "(out, cap, models, thr, norm=None, min_conf=None, on='all', moments=False)"
