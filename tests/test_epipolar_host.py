"""CPU-only: the per-pair model verification entry points (ABI 8, symbols added) are declared and exported with the argument counts
of the header, refuse every bad argument before any launch with a message that names it, and the Python layers refuse what they
must; the functions this change leaves alone keep their signatures.  No kernel runs here: every C call below fails validation."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import REPO

EPI = {"pats_epipolar_max_h": (ctypes.c_int64, 0), "pats_epipolar_workspace_bytes": (ctypes.c_size_t, 3),
       "pats_epipolar_score_by_pair_f32": (ctypes.c_int, 22)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in EPI.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name


def test_max_h_is_at_least_4096(lib):
    from pats_amd import ops
    assert lib.pats_epipolar_max_h() >= 4096 and ops.epipolar_max_h() == lib.pats_epipolar_max_h()


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
REQUIRED = ("matches_l", "matches_r", "models", "thr", "counts", "best", "best_count", "inlier")
OPTIONAL = ("conf", "pair_off", "counts_in", "norm", "moments")
ALIGN = {"matches_l": 8, "matches_r": 8, "models": 4, "thr": 4, "norm": 4, "conf": 4, "counts": 4, "best": 4, "pair_off": 8,
         "counts_in": 8, "best_count": 8, "moments": 8}


def _call(lib, pairs=2, cap=100, H=8, stride=0, use_min_conf=0, min_conf=0.0, ws=A16, ws_bytes=1 << 20, **ptrs):
    a = {n: A16 for n in REQUIRED + OPTIONAL}
    a["counts_in"] = 0                                   # the ragged form unless a test says otherwise
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    return lib.pats_epipolar_score_by_pair_f32(p["matches_l"], p["matches_r"], p["conf"], p["pair_off"], stride, p["counts_in"], pairs,
                                               cap, p["models"], H, p["thr"], p["norm"], use_min_conf, min_conf, p["counts"], p["best"],
                                               p["best_count"], p["inlier"], p["moments"], ctypes.c_void_p(ws) if ws else None,
                                               ws_bytes, None)


def _refused(lib, *words, **kw):
    assert _call(lib, **kw) != 0, kw
    msg = lib.pats_last_error()
    assert b"epipolar_score_by_pair" in msg and all(w in msg for w in words), (kw, msg)


@pytest.mark.parametrize("name", REQUIRED)
def test_null_required_pointers_are_refused_by_name(lib, name):
    _refused(lib, b"null", name.encode(), **{name: 0})


@pytest.mark.parametrize("name", sorted(ALIGN))
def test_misaligned_pointers_are_refused_by_name(lib, name):
    strided = {"pair_off": 0, "stride": 10} if name == "counts_in" else {}
    for off in ((1, 2, 3) if ALIGN[name] == 4 else (1, 2, 4)):
        _refused(lib, b"%d-byte aligned" % ALIGN[name], name.encode(), **dict(strided, **{name: A16 + off}))


def test_exactly_one_segment_form(lib):
    _refused(lib, b"pair_off", b"counts_in", counts_in=A16, stride=10)                      # both
    _refused(lib, b"pair_off", b"counts_in", pair_off=0)                                   # neither


def test_sizes_are_refused_by_name(lib):
    max_h = lib.pats_epipolar_max_h()
    for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="), ({"H": max_h + 1}, b"max_h"),
                     ({"cap": -1}, b"cap"), ({"cap": 2 ** 31 - 1}, b"cap"), ({"cap": 2 ** 40}, b"cap")):
        _refused(lib, word, **kw)
    strided = {"pair_off": 0, "counts_in": A16}
    for kw, word in (({"stride": 0}, b"stride"), ({"stride": -4}, b"stride"), ({"stride": 51}, b"stride"), ({"stride": 10, "pairs": 11}, b"stride"),
                     ({"stride": 1, "cap": 0}, b"stride")):
        _refused(lib, word, **dict(strided, **kw))
    _refused(lib, b"pairs", pairs=2 ** 31 - 1, cap=2 ** 31 - 2, H=max_h)                     # a grid of 2^31 workgroups or more


def test_threshold_must_be_a_non_negative_number_and_needs_conf(lib):
    for bad in (math.nan, -0.25, -math.inf):
        _refused(lib, b"min_conf", use_min_conf=1, min_conf=bad)
    _refused(lib, b"min_conf", b"conf", use_min_conf=1, min_conf=0.5, conf=0)


def test_workspace_too_small_is_refused(lib):
    """The kernels may need no workspace (0 bytes: then no size can be too small); whatever they ask for, one byte less is refused."""
    need = lib.pats_epipolar_workspace_bytes(2, 8, 100)
    assert need >= 0 and lib.pats_epipolar_workspace_bytes(48, lib.pats_epipolar_max_h(), 2 ** 31 - 2) < (1 << 32)
    if need > 0:
        _refused(lib, b"workspace", ws_bytes=need - 1)


def _cpu_inputs():
    import torch
    return (torch.zeros(6, 2), torch.zeros(6, 2), torch.zeros(2, 3, 3, 3), torch.full((2,), 0.01), torch.tensor([0, 3, 6]))


def test_ops_refuses_cpu_tensors_bad_layouts_and_bad_types():
    import torch
    from pats_amd import ops
    ml, mr, models, thr, off = _cpu_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epipolar_score_by_pair(ml, mr, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="matches_l must be contiguous"):
        ops.epipolar_score_by_pair(torch.zeros(6, 4)[:, ::2], mr, models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="models must be contiguous"):
        ops.epipolar_score_by_pair(ml, mr, models.transpose(2, 3), thr, pair_off=off)
    with pytest.raises(RuntimeError, match="conf must be contiguous"):
        ops.epipolar_score_by_pair(ml, mr, models, thr, pair_off=off, conf=torch.zeros(6, 2)[:, 0], min_conf=0.5)
    with pytest.raises(RuntimeError, match="matches_r must be float32"):
        ops.epipolar_score_by_pair(ml, mr.double(), models, thr, pair_off=off)
    with pytest.raises(RuntimeError, match="models must be float32"):
        ops.epipolar_score_by_pair(ml, mr, models.half(), thr, pair_off=off)
    with pytest.raises(RuntimeError, match="pair_off must be int64"):
        ops.epipolar_score_by_pair(ml, mr, models, thr, pair_off=off.int())
    with pytest.raises(RuntimeError, match="counts must be int64"):
        ops.epipolar_score_by_pair(ml, mr, models, thr, stride=3, counts=torch.tensor([3, 3], dtype=torch.int32))
    # the segment forms and the gate
    for kw in ({}, {"pair_off": off, "stride": 3, "counts": torch.tensor([3, 3])}, {"stride": 3}, {"counts": torch.tensor([3, 3])}):
        with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
            ops.epipolar_score_by_pair(ml, mr, models, thr, **kw)
    with pytest.raises(RuntimeError, match="min_conf needs conf"):
        ops.epipolar_score_by_pair(ml, mr, models, thr, pair_off=off, min_conf=0.5)
    assert str(inspect.signature(ops.epipolar_score_by_pair)) == (
        "(matches_l, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None, norm=None, "
        "moments=False, out=None, pairs=None)")


def test_batch_verify_by_pair_refuses_what_it_cannot_score():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}
    with pytest.raises(ValueError, match="topk_by_pair"):
        batch.verify_by_pair(dict(plain), cap, None, None, on="topk")
    with pytest.raises(ValueError, match="on must be"):
        batch.verify_by_pair(dict(plain), cap, None, None, on="best")
    with pytest.raises(ValueError, match="confidence=True"):
        batch.verify_by_pair(dict(plain), cap, None, None, min_conf=0.5)
    with pytest.raises(ValueError, match="verify_by_pair first"):
        batch.split_verified_by_pair(dict(plain), cap)
    assert str(inspect.signature(batch.verify_by_pair)) == "(out, cap, models, thr, norm=None, min_conf=None, on='all', moments=False)"
    assert str(inspect.signature(batch.split_verified_by_pair)) == "(out, cap)"


def test_untouched_functions_keep_their_signatures():
    from pats_amd import batch, ops
    want = {
        batch.forward_pairs: "(lefts, rights, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None, "
                             "confidence=False)",
        batch.forward_pairs_mixed: "(pack, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None, "
                                   "confidence=False)",
        batch.group_by_pair: "(out, cap, buffers=None, confidence=False)",
        batch.split_by_pair: "(out, cap)",
        batch.topk_by_pair: "(out, cap, K, min_conf=None)",
        batch.split_topk_by_pair: "(out, cap)",
        ops.topk_by_pair: "(matches_l, matches_r, conf, pair_off, K, min_conf=None, out=None, pairs=None)",
        ops.matches_by_pair: "(rows, matches_l, matches_r, match_row, M, out=None, P=None, match_conf=None)",
    }
    for fn, sig in want.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__
