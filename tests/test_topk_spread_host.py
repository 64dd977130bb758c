"""CPU-only: the per-pair spread top-K entry points (ABI 8, symbols added) are declared and exported with the argument counts of
the header, refuse every bad argument before any launch with a message that names it, and the Python layers refuse what they
must; the top-K functions beside them keep their signatures.  No kernel runs here: every C call below fails validation."""
import ctypes
import inspect
import math
import os
import re

import pytest

from conftest import REPO

SPREAD = {"pats_topk_spread_by_pair_max_cells": (ctypes.c_int64, 0), "pats_topk_spread_by_pair_workspace_bytes": (ctypes.c_size_t, 4),
          "pats_topk_spread_by_pair_f32": (ctypes.c_int, 22)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    assert "Per-pair spread top-K" in header
    for name, (res, nargs) in SPREAD.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name


def test_max_cells_is_at_least_4096(lib):
    from pats_amd import ops
    assert lib.pats_topk_spread_by_pair_max_cells() >= 4096
    assert ops.topk_spread_max_cells() == lib.pats_topk_spread_by_pair_max_cells()


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
POINTERS = ("matches_l", "matches_r", "conf", "pair_off", "top_l", "top_r", "top_conf", "top_idx", "top_count", "occupied")
ALIGN = {"matches_l": 8, "matches_r": 8, "top_l": 8, "top_r": 8, "conf": 4, "top_conf": 4, "top_idx": 4, "pair_off": 8, "top_count": 8,
         "occupied": 8}


def _call(lib, pairs=2, cap=100, K=8, use_min_conf=0, min_conf=0.0, side=0, cell=16, grid0=4, grid1=5, ws=A16, ws_bytes=1 << 20,
          **ptrs):
    a = {n: A16 for n in POINTERS}
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    return lib.pats_topk_spread_by_pair_f32(p["matches_l"], p["matches_r"], p["conf"], p["pair_off"], pairs, cap, K, use_min_conf,
                                            min_conf, side, cell, grid0, grid1, p["top_l"], p["top_r"], p["top_conf"], p["top_idx"],
                                            p["top_count"], p["occupied"], ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def _refused(lib, **kw):
    assert _call(lib, **kw) != 0, kw
    msg = lib.pats_last_error()
    assert msg.startswith(b"topk_spread_by_pair:"), (kw, msg)
    return msg


@pytest.mark.parametrize("name", POINTERS)
def test_null_and_misaligned_pointers_are_refused_by_name(lib, name):
    msg = _refused(lib, **{name: 0})
    assert b"null" in msg and name.encode() in msg, msg
    offsets = (1, 2, 3) if ALIGN[name] == 4 else (1, 2, 4)
    for off in offsets:
        msg = _refused(lib, **{name: A16 + off})
        assert b"%d-byte aligned" % ALIGN[name] in msg and name.encode() in msg, msg


def test_sizes_are_refused_by_name(lib):
    from pats_amd import ops
    max_k = ops.topk_max_k()
    for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"cap": -1}, b"cap"), ({"K": 0}, b"K ="), ({"K": -1}, b"K ="),
                     ({"K": max_k + 1}, b"max_k"), ({"side": 2}, b"side"), ({"side": -1}, b"side"), ({"cell": 0}, b"cell"),
                     ({"cell": -16}, b"cell"), ({"cell": 65537}, b"cell"), ({"grid0": 0}, b"grid0"), ({"grid0": -2}, b"grid0"),
                     ({"grid1": 0}, b"grid1"), ({"grid1": -2}, b"grid1")):
        assert word in _refused(lib, **kw), kw
    assert _call(lib, pairs=0, cell=0) != 0 and b"pairs" in lib.pats_last_error()        # the order: topk_by_pair's refusals first


def test_the_wording_is_topk_by_pairs_apart_from_the_prefix(lib):
    """Everything pats_topk_by_pair_f32 refuses is refused here with the same words."""
    p = [ctypes.c_void_p(A16)] * 4
    o = [ctypes.c_void_p(A16)] * 5
    for kw in ({"pairs": 0}, {"cap": -1}, {"K": 0}, {"use_min_conf": 1, "min_conf": -0.5}):
        a = dict(pairs=2, cap=100, K=8, use_min_conf=0, min_conf=0.0)
        a.update(kw)
        assert lib.pats_topk_by_pair_f32(*p, a["pairs"], a["cap"], a["K"], a["use_min_conf"], a["min_conf"], *o, None, 0, None) != 0
        plain = lib.pats_last_error()
        assert plain.startswith(b"topk_by_pair:")
        assert _refused(lib, **kw) == b"topk_spread_by_pair:" + plain[len(b"topk_by_pair:"):]


def test_the_product_is_refused_with_both_numbers(lib):
    most = lib.pats_topk_spread_by_pair_max_cells()
    for g0, g1 in ((most + 1, 1), (1, most + 1), (most // 2 + 1, 2), (1 << 40, 1 << 40)):
        msg = _refused(lib, grid0=g0, grid1=g1)
        assert b"max_cells" in msg and str(g0).encode() in msg and str(g1).encode() in msg and str(most).encode() in msg, msg


def test_threshold_must_be_a_non_negative_number(lib):
    for bad in (math.nan, -0.25, -math.inf):
        assert b"min_conf" in _refused(lib, use_min_conf=1, min_conf=bad), bad


def test_workspace_too_small_is_refused(lib):
    """The kernel may need no workspace (0 bytes: then no size can be too small); whatever it asks for, one byte less is refused."""
    need = lib.pats_topk_spread_by_pair_workspace_bytes(2, 8, 4, 5)
    assert need >= 0 and lib.pats_topk_spread_by_pair_workspace_bytes(48, 8192, 128, 128) < (1 << 30)
    if need > 0:
        assert b"workspace" in _refused(lib, ws_bytes=need - 1)


def test_ops_topk_spread_by_pair_refuses_cpu_tensors():
    import torch
    from pats_amd import ops
    ml, mr, cf, off = torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(4), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_spread_by_pair(ml, mr, cf, off, 2, 16, (3, 3))
    assert str(inspect.signature(ops.topk_spread_by_pair)) == ("(matches_l, matches_r, conf, pair_off, K, cell, grid, side='left', "
                                                               "min_conf=None, out=None, pairs=None)")


def test_batch_topk_spread_by_pair_needs_a_confidence_result_and_a_grid_that_fits():
    from pats_amd import batch, ops
    cap = batch.Capacities(2, 5, 6)
    with pytest.raises(ValueError, match="confidence=True"):
        batch.topk_spread_by_pair({"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}, cap, 10, 16)
    most = ops.topk_spread_max_cells()
    assert 160 * 192 > most                               # cell = 1 on this grid's 160 x 192 pixels
    with pytest.raises(ValueError, match="max_cells") as e:
        batch.topk_spread_by_pair({"match_conf": None}, cap, 10, 1)
    fits = int(re.search(r"smallest cell that fits is (\d+)", str(e.value)).group(1))
    cells = lambda c: -(-160 // c) * -(-192 // c)
    assert cells(fits) <= most < cells(fits - 1) and all(cells(c) > most for c in range(1, fits))
    mixed = batch.MixedCapacities([(37, 10), (10, 50)])   # the largest h and the largest w: 1184 x 1600 pixels
    with pytest.raises(ValueError, match="max_cells"):
        batch.topk_spread_by_pair({"match_conf": None}, mixed, 10, 8)
    with pytest.raises(ValueError, match="confidence=True"):            # 74 x 100 cells fit
        batch.topk_spread_by_pair({}, mixed, 10, 16)
    for bad in (0, -4, 2.5, 65537):
        with pytest.raises(ValueError, match="cell"):
            batch.topk_spread_by_pair({"match_conf": None}, cap, 10, bad)
    assert str(inspect.signature(batch.topk_spread_by_pair)) == "(out, cap, K, cell, min_conf=None, side='left')"


def test_the_functions_beside_it_keep_their_signatures():
    from pats_amd import batch, ops
    want = {
        batch.topk_by_pair: "(out, cap, K, min_conf=None)",
        batch.split_topk_by_pair: "(out, cap)",
        ops.topk_by_pair: "(matches_l, matches_r, conf, pair_off, K, min_conf=None, out=None, pairs=None)",
    }
    for fn, sig in want.items():
        assert str(inspect.signature(fn)) == sig, fn.__name__
