"""CPU-only: the per-pair top-K entry points (ABI 8, symbols added) are declared and exported with the argument counts of the
header, refuse every bad argument before any launch with a message that names it, and the Python layers refuse what they must;
the functions this change leaves alone keep their signatures.  No kernel runs here: every C call below fails validation."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import REPO

TOPK = {"pats_topk_by_pair_max_k": (ctypes.c_int64, 0), "pats_topk_by_pair_workspace_bytes": (ctypes.c_size_t, 2),
        "pats_topk_by_pair_f32": (ctypes.c_int, 17)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in TOPK.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name


def test_max_k_is_at_least_4096(lib):
    assert lib.pats_topk_by_pair_max_k() >= 4096


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
POINTERS = ("matches_l", "matches_r", "conf", "pair_off", "top_l", "top_r", "top_conf", "top_idx", "top_count")
ALIGN = {"matches_l": 8, "matches_r": 8, "top_l": 8, "top_r": 8, "conf": 4, "top_conf": 4, "top_idx": 4, "pair_off": 8, "top_count": 8}


def _call(lib, pairs=2, cap=100, K=8, use_min_conf=0, min_conf=0.0, ws=A16, ws_bytes=1 << 20, **ptrs):
    a = {n: A16 for n in POINTERS}
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    return lib.pats_topk_by_pair_f32(p["matches_l"], p["matches_r"], p["conf"], p["pair_off"], pairs, cap, K, use_min_conf, min_conf,
                                     p["top_l"], p["top_r"], p["top_conf"], p["top_idx"], p["top_count"],
                                     ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


@pytest.mark.parametrize("name", POINTERS)
def test_null_and_misaligned_pointers_are_refused_by_name(lib, name):
    assert _call(lib, **{name: 0}) != 0
    msg = lib.pats_last_error()
    assert b"topk_by_pair" in msg and b"null" in msg and name.encode() in msg, msg
    offsets = (1, 2, 3) if ALIGN[name] == 4 else (1, 2, 4)
    for off in offsets:
        assert _call(lib, **{name: A16 + off}) != 0, (name, off)
        msg = lib.pats_last_error()
        assert b"%d-byte aligned" % ALIGN[name] in msg and name.encode() in msg, msg


def test_sizes_are_refused_by_name(lib):
    max_k = lib.pats_topk_by_pair_max_k()
    for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"cap": -1}, b"cap"), ({"K": 0}, b"K ="), ({"K": -1}, b"K ="),
                     ({"K": max_k + 1}, b"max_k")):
        assert _call(lib, **kw) != 0, kw
        msg = lib.pats_last_error()
        assert b"topk_by_pair" in msg and word in msg, (kw, msg)


def test_threshold_must_be_a_non_negative_number(lib):
    for bad in (math.nan, -0.25, -math.inf):
        assert _call(lib, use_min_conf=1, min_conf=bad) != 0, bad
        assert b"min_conf" in lib.pats_last_error()


def test_workspace_too_small_is_refused(lib):
    """The kernel may need no workspace (0 bytes: then no size can be too small); whatever it asks for, one byte less is refused."""
    need = lib.pats_topk_by_pair_workspace_bytes(2, 8)
    assert need >= 0 and lib.pats_topk_by_pair_workspace_bytes(48, lib.pats_topk_by_pair_max_k()) < (1 << 30)
    if need > 0:
        assert _call(lib, ws_bytes=need - 1) != 0 and b"workspace" in lib.pats_last_error()
        assert _call(lib, ws=0, ws_bytes=need) != 0 and b"workspace" in lib.pats_last_error()


def test_ops_topk_by_pair_refuses_cpu_tensors():
    import torch
    from pats_amd import ops
    ml, mr, cf, off = torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_by_pair(ml, mr, cf, off, 2)
    assert list(inspect.signature(ops.topk_by_pair).parameters)[:7] == ["matches_l", "matches_r", "conf", "pair_off", "K", "min_conf",
                                                                         "out"]
    assert inspect.signature(ops.topk_by_pair).parameters["min_conf"].default is None


def test_batch_topk_by_pair_needs_a_confidence_result():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    with pytest.raises(ValueError, match="confidence=True"):
        batch.topk_by_pair({"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}, cap, 10)
    with pytest.raises(ValueError):
        batch.split_topk_by_pair({"match_conf": None}, cap)
    assert list(inspect.signature(batch.topk_by_pair).parameters) == ["out", "cap", "K", "min_conf"]
    assert list(inspect.signature(batch.split_topk_by_pair).parameters) == ["out", "cap"]


def test_untouched_functions_keep_their_signatures():
    from pats_amd import batch
    want = {
        batch.forward_pairs: "(lefts, rights, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None, "
                             "confidence=False)",
        batch.forward_pairs_mixed: "(pack, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None, "
                                   "confidence=False)",
        batch.group_by_pair: "(out, cap, buffers=None, confidence=False)",
        batch.split_by_pair: "(out, cap)",
    }
    for fn, sig in want.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__
