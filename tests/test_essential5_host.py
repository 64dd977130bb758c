"""CPU-only: the per-pair 5-point hypotheses entry points (ABI 8, symbols added) are declared and exported with the argument counts
of the header, refuse every bad argument before any launch with a message that names it, and the Python layers refuse what they
must.  No kernel runs here: every C call below fails validation.  (tests/test_essential5_gpu.py repeats the refusals on a machine
with a GPU, where a launch would be possible.)"""
import ctypes
import inspect
import os
import re

import pytest

from conftest import REPO

HYP5 = {"pats_epipolar_hypotheses5_workspace_bytes": (ctypes.c_size_t, 2), "pats_epipolar_hypotheses5_by_pair_f32": (ctypes.c_int, 17)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exist_with_the_headers_argument_counts(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in HYP5.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "hypotheses5.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES


def test_no_workspace(lib):
    for pairs, H in ((1, 1), (48, 100), (4096, lib.pats_epipolar_max_h() // 10)):
        assert lib.pats_epipolar_hypotheses5_workspace_bytes(pairs, H) == 0


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
REQUIRED = ("matches_l", "matches_r", "pair_seed", "models")
OPTIONAL = ("pair_off", "counts_in", "norm", "sample_idx", "n_models")
ALIGN = {"matches_l": 8, "matches_r": 8, "models": 4, "norm": 4, "sample_idx": 4, "n_models": 4, "pair_off": 8, "counts_in": 8,
         "pair_seed": 8}


def call(lib, pairs=2, cap=100, H=8, stride=0, progressive=0, ws=A16, ws_bytes=1 << 20, **ptrs):
    a = {n: A16 for n in REQUIRED + OPTIONAL}
    a["counts_in"] = 0                                   # the ragged form unless a test says otherwise
    a.update(ptrs)
    p = {n: (ctypes.c_void_p(v) if v else None) for n, v in a.items()}
    return lib.pats_epipolar_hypotheses5_by_pair_f32(p["matches_l"], p["matches_r"], p["pair_off"], stride, p["counts_in"], pairs, cap, H,
                                                     p["pair_seed"], p["norm"], progressive, p["models"], p["sample_idx"], p["n_models"],
                                                     ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


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
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="),
                                           ({"H": max_h + 1}, b"max_h"), ({"H": max_h // 10 + 1}, b"H ="), ({"H": max_h}, b"10 H"),
                                           ({"cap": -1}, b"cap"), ({"cap": 2 ** 31 - 1}, b"cap"),
                                           ({"cap": 2 ** 40}, b"cap"), ({"progressive": 2}, b"progressive"), ({"progressive": -1}, b"progressive"),
                                           ({"pairs": 2 ** 31 - 1, "cap": 2 ** 31 - 2, "H": max_h // 10}, b"pairs"))]
    out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                            {"stride": 1, "cap": 0})]
    need = lib.pats_epipolar_hypotheses5_workspace_bytes(2, 8)
    if need > 0:                                         # 0 today: then no size can be too small
        out.append(({"ws_bytes": need - 1}, (b"workspace",)))
    return out


def refused(lib, kw, words):
    assert call(lib, **kw) != 0, kw
    msg = lib.pats_last_error()
    assert b"epipolar_hypotheses5_by_pair" in msg and all(w in msg for w in words), (kw, msg)


def test_every_bad_argument_is_refused_by_name(lib):
    cases = refusals(lib)
    assert len(cases) > 45
    for kw, words in cases:
        refused(lib, kw, words)


def test_ops_refuses_cpu_tensors_bad_layouts_and_bad_types():
    import torch
    from pats_amd import ops
    ml, mr, off, seed = torch.zeros(20, 2), torch.zeros(20, 2), torch.tensor([0, 10, 20]), torch.tensor([1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed, pair_off=off)
    with pytest.raises(RuntimeError, match="epipolar_hypotheses5_by_pair: matches_l must be contiguous"):
        ops.epipolar_hypotheses5_by_pair(torch.zeros(20, 4)[:, ::2], mr, 4, seed, pair_off=off)
    with pytest.raises(RuntimeError, match="norm must be contiguous"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed, pair_off=off, norm=torch.zeros(8, 2).t())
    with pytest.raises(RuntimeError, match="matches_r must be float32"):
        ops.epipolar_hypotheses5_by_pair(ml, mr.double(), 4, seed, pair_off=off)
    with pytest.raises(RuntimeError, match="seed must be int64"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed.int(), pair_off=off)
    with pytest.raises(RuntimeError, match="seed must be an int64 GPU tensor"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, 7, pair_off=off)
    with pytest.raises(RuntimeError, match="pair_off must be int64"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed, pair_off=off.int())
    with pytest.raises(RuntimeError, match="counts must be int64"):
        ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed, stride=10, counts=torch.tensor([3, 3], dtype=torch.int32))
    for kw in ({}, {"pair_off": off, "stride": 10, "counts": torch.tensor([3, 3])}, {"stride": 10}, {"counts": torch.tensor([3, 3])}):
        with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
            ops.epipolar_hypotheses5_by_pair(ml, mr, 4, seed, **kw)
    assert str(inspect.signature(ops.epipolar_hypotheses5_by_pair)) == (
        "(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False, return_samples=False, "
        "return_counts=False, out=None, pairs=None)")
    # the 8-point generator keeps its signature
    assert str(inspect.signature(ops.epipolar_hypotheses_by_pair)) == (
        "(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False, return_samples=False, "
        "out=None, pairs=None)")


def test_batch_hypothesize5_by_pair_refuses_what_it_cannot_sample():
    from pats_amd import batch
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": None, "matches_r": None, "match_row": None, "M": None, "P": None}
    with pytest.raises(ValueError, match="hypothesize5_by_pair.*topk_by_pair"):
        batch.hypothesize5_by_pair(dict(plain), cap, 16)                  # on="topk" is the default
    with pytest.raises(ValueError, match="hypothesize5_by_pair: on must be"):
        batch.hypothesize5_by_pair(dict(plain), cap, 16, on="best")
    assert str(inspect.signature(batch.hypothesize5_by_pair)) == "(out, cap, H, seed=0, norm=None, on='topk', progressive=None, samples=False)"
    assert str(inspect.signature(batch.hypothesize_by_pair)) == "(out, cap, H, seed=0, norm=None, on='topk', progressive=None, samples=False)"
