"""CPU-only: the output-typed entry points of the descriptor gathers (pats_*_descriptors_typed_out, ABI 8) are declared,
exported and refuse bad arguments before any launch, ops takes out_dtype, and the values tests/test_half_out_gpu.py plants
really tell round-to-nearest-even from truncation and from round-half-up.  No kernel runs here: every C call below fails
validation or is an empty launch."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

TYPED_OUT = ("pats_fine_descriptors_typed_out", "pats_third_descriptors_typed_out")

# What the GPU tests plant where a map value reaches the store unchanged (float32 values; a test keeps those its map type
# holds exactly): signed zeros; fp16's largest value, the tie between it and infinity, a value beyond; fp16 subnormal ties
# (2^-25 lies between 0 and 2^-24: down to the even 0; 3 * 2^-25 between 2^-24 and 2^-23: up to the even 2^-23); fp16 ties
# in the normal range, down (1 + 2^-11) and up (1 + 3 * 2^-11); the same for bf16 (ulp 2^-7 at 1); values just above and just
# below a tie; infinities; a NaN.
SPECIALS = [0.0, -0.0, 65504.0, 65520.0, 1e5, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25),
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8),
            1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 3 * 2.0 ** -8 - 2.0 ** -20,
            float("inf"), float("-inf"), float("nan")]


def specials_for(map_dtype):
    """SPECIALS that `map_dtype` holds exactly (a NaN counts), as a float32 tensor."""
    v = torch.tensor(SPECIALS, dtype=torch.float32)
    back = v.to(map_dtype).float()
    keep = (back.view(torch.int32) == v.view(torch.int32)) | torch.isnan(v)
    return v[keep]


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_and_ctypes_table_agree_on_the_typed_out_gathers(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name in TYPED_OUT:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):           # pointers <-> c_void_p, the enums and int <-> c_int, int64_t <-> c_int64
            want = ctypes.c_void_p if ("*" in p or p.startswith("pats_stream_t")) else \
                ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (name, p)
        assert sum(p.startswith("pats_map_dtype_t") for p in params) == 2, name
        assert "pats_map_dtype_t out_dtype" in m.group(1), name
        assert not re.search(r"float\* (desc|out0|out1)\b", m.group(1)), name      # the outputs are void*
    # the _typed entries' argument lists with void* outputs and the out_dtype behind them
    for name in TYPED_OUT:
        base = _lib.SIGNATURES[name[:-4]][1]
        assert len(_lib.SIGNATURES[name][1]) == len(base) + 1


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000          # 16-byte aligned
A4 = A16 + 4                  # 4-byte but not 16-byte aligned
A2 = A16 + 2                  # 2-byte aligned: an odd half-element offset
A1 = A16 + 1                  # off a half element


def _p(a):
    return ctypes.c_void_p(a) if a else None


def _fine(lib, out_dtype, cl=0, dtype=0, maps=(A16, A16, A16), desc=A16, B=1, title=A16, rubbish=A16):
    return lib.pats_fine_descriptors_typed_out(_p(maps[0]), _p(maps[1]), _p(maps[2]), dtype, cl, _p(title), _p(rubbish), B, None,
                                               _p(desc), out_dtype, None)


def _third(lib, out_dtype, cl=0, dtype=0, maps=(A16, A16), outs=(A16, A16), P=4, B=1, other=A16):
    f = _p(other)
    return lib.pats_third_descriptors_typed_out(_p(maps[0]), _p(maps[1]), dtype, cl, f, f, f, f, f, P, None, B, _p(outs[0]),
                                                _p(outs[1]), out_dtype, None, None, None)


@pytest.mark.parametrize("bad", [3, -1, 7])
def test_typed_out_gathers_refuse_an_unknown_out_dtype(lib, bad):
    assert _fine(lib, bad) == 1 and b"unknown output dtype" in lib.pats_last_error()
    assert _third(lib, bad, cl=1) == 1 and b"unknown output dtype" in lib.pats_last_error()
    # and an unknown map dtype, for every output type
    for ot in (0, 1, 2):
        assert _fine(lib, ot, dtype=bad) == 1 and b"unknown map dtype" in lib.pats_last_error()
        assert _third(lib, ot, dtype=bad) == 1 and b"unknown map dtype" in lib.pats_last_error()


@pytest.mark.parametrize("ot", [0, 1, 2])
@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("cl", [0, 1])
def test_typed_out_gathers_refuse_null_pointers(lib, ot, dtype, cl):
    for maps in ((None, A16, A16), (A16, None, A16), (A16, A16, None)):
        assert _fine(lib, ot, cl, dtype, maps=maps) == 1 and b"null pointer" in lib.pats_last_error()
    for kw in ({"desc": 0}, {"title": 0}, {"rubbish": 0}):
        assert _fine(lib, ot, cl, dtype, **kw) == 1 and b"null pointer" in lib.pats_last_error()
    for maps in ((None, A16), (A16, None)):
        assert _third(lib, ot, cl, dtype, maps=maps) == 1 and b"null pointer" in lib.pats_last_error()
    for outs in ((0, A16), (A16, 0)):
        assert _third(lib, ot, cl, dtype, outs=outs) == 1 and b"null pointer" in lib.pats_last_error()
    assert _third(lib, ot, cl, dtype, other=0) == 1 and b"null pointer" in lib.pats_last_error()


@pytest.mark.parametrize("ot", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_out_gathers_refuse_misaligned_half_outputs(lib, ot, dtype):
    # NCHW: 2-byte and 4-byte-pair stores at 2-byte alignment -> only an address off the element size is refused
    assert _fine(lib, ot, 0, dtype, desc=A1) == 1 and b"2-byte aligned" in lib.pats_last_error()
    for outs in ((A1, A16), (A16, A1)):
        assert _third(lib, ot, 0, dtype, outs=outs) == 1 and b"2-byte aligned" in lib.pats_last_error()
    # channels-last: the linear copy stores 16 bytes at a time
    for bad in (A2, A4):
        assert _fine(lib, ot, 1, dtype, desc=bad) == 1 and b"16-byte aligned" in lib.pats_last_error()
        for outs in ((bad, A16), (A16, bad)):
            assert _third(lib, ot, 1, dtype, outs=outs) == 1 and b"16-byte aligned" in lib.pats_last_error()
    # the maps' rules are those of the _typed entries
    assert _fine(lib, ot, 0, dtype, maps=(A2, A16, A16)) == 1 and b"aligned" in lib.pats_last_error()
    assert _fine(lib, ot, 1, dtype, maps=(A16, A4, A16)) == 1 and b"16-byte aligned" in lib.pats_last_error()
    assert _third(lib, ot, 0, dtype, maps=(A16, A2)) == 1 and b"aligned" in lib.pats_last_error()
    assert _third(lib, ot, 1, dtype, maps=(A2, A16)) == 1 and b"aligned" in lib.pats_last_error()


def test_typed_out_gathers_f32_output_keeps_the_typed_entries_rules(lib):
    assert _fine(lib, 0, 1, 0, desc=A4) == 1 and b"fine_descriptors_typed: " in lib.pats_last_error()
    assert _third(lib, 0, 0, 1, maps=(A2, A16)) == 1 and b"third_descriptors_typed: " in lib.pats_last_error()


@pytest.mark.parametrize("ot", [0, 1, 2])
def test_typed_out_gathers_empty_launches_are_no_ops(lib, ot):
    for cl in (0, 1):
        assert lib.pats_fine_descriptors_typed_out(None, None, None, 1, cl, None, None, 0, None, None, ot, None) == 0
        assert lib.pats_third_descriptors_typed_out(None, None, 2, cl, None, None, None, None, None, 0, None, 1, None, None, ot,
                                                    None, None, None) == 0
    assert _third(lib, ot, B=0) == 1 and b"bad shape" in lib.pats_last_error()


def _fine_args(dt=torch.float32):
    maps = [torch.zeros(s, dtype=dt) for s in ((2, 64, 48, 48), (2, 64, 24, 24), (2, 128, 12, 12))]
    return maps, torch.zeros(1, 8), torch.zeros(1, 264)


def _third_args(dt=torch.float32):
    f = torch.zeros((1, 128, 52, 52), dtype=dt)
    return f, f, torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, dtype=torch.int64), torch.zeros(128, 64), torch.zeros(1, 128, 144)


def test_ops_raise_on_an_out_dtype_conflict_and_on_unsupported_output_dtypes():
    from pats_amd import ops
    for half, other in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float16)):
        with pytest.raises(RuntimeError, match="conflicts"):
            ops.fine_descriptors(*_fine_args(), out=torch.zeros((2, 1, 264, 145), dtype=half), out_dtype=other)
        o = torch.zeros((1, 128, 65), dtype=half)
        with pytest.raises(RuntimeError, match="conflicts"):
            ops.third_descriptors(*_third_args(), out=(o, o), out_dtype=other)
        with pytest.raises(RuntimeError, match="one dtype"):
            ops.third_descriptors(*_third_args(), out=(o, o.to(other)))
    for bad in (torch.float64, torch.int16, torch.uint8):
        name = str(bad).replace("torch.", "")
        with pytest.raises(RuntimeError, match=name):
            ops.fine_descriptors(*_fine_args(), out_dtype=bad)
        with pytest.raises(RuntimeError, match=name):
            ops.third_descriptors(*_third_args(), out_dtype=bad)
        with pytest.raises(RuntimeError, match=name):
            ops.fine_descriptors(*_fine_args(), out=torch.zeros((2, 1, 264, 145), dtype=bad))
        o = torch.zeros((1, 128, 65), dtype=bad)
        with pytest.raises(RuntimeError, match=name):
            ops.third_descriptors(*_third_args(), out=(o, o))
    with pytest.raises(TypeError):
        ops.fine_descriptors(*_fine_args(), out_dtype="bfloat16")


@pytest.mark.parametrize("ot", [torch.float32, torch.float16, torch.bfloat16])
def test_ops_take_the_three_output_dtypes(ot):
    """A supported out_dtype (or out) passes the dtype checks; these CPU tensors are then refused for being on the CPU."""
    from pats_amd import ops
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.fine_descriptors(*_fine_args(dt), out_dtype=ot)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.third_descriptors(*_third_args(dt), out_dtype=ot)
        o = torch.zeros((1, 128, 65), dtype=ot)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.third_descriptors(*_third_args(dt), out=(o, o), out_dtype=ot)


# ---- the planted values: what a wrong conversion would do to them ----------------------------------------------------------------
def _neighbours(v, dt):
    """the two `dt` values around the finite positive float32 v: (towards zero, away from zero), as float32"""
    h = v.to(dt)
    bits = h.view(torch.int16).to(torch.int32)
    below = h.float() <= v
    lo = torch.where(below, bits, bits - 1).to(torch.int16).view(dt).float()
    hi = torch.where(below, bits + 1, bits).to(torch.int16).view(dt).float()
    return lo, hi


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_planted_values_catch_truncation_and_round_half_up(dt):
    v = torch.tensor([x for x in SPECIALS if 0 < x < 1e30], dtype=torch.float32)
    rne = v.to(dt).float()                                  # the yardstick: round to nearest even (to inf above the largest)
    lo, hi = _neighbours(v, dt)
    assert bool(((lo <= v) & (v <= hi)).all())
    trunc = lo
    half_up = torch.where(v.double() - lo.double() >= hi.double() - v.double(), hi, lo)
    exact = lo == v
    assert int((trunc != rne).sum()) >= 3, "a truncating conversion must be caught"
    assert int(((half_up != rne) & ~exact).sum()) >= 1, "a round-half-up conversion must be caught"
    # the ties of this type: one resolved down and one up, both to the even neighbour
    tie = (v.double() - lo.double() == hi.double() - v.double()) & ~exact & torch.isfinite(hi)
    assert bool((rne[tie] == lo[tie]).any()) and bool((rne[tie] == hi[tie]).any())
    even = lambda t: (t.to(dt).view(torch.int16) & 1) == 0      # noqa: E731
    assert bool(even(rne[tie]).all())
    if dt == torch.float16:                                 # overflow: the tie 65520 and everything above go to inf, 65504 stays
        assert torch.tensor([65504.0, 65520.0, 1e5]).to(dt).tolist() == [65504.0, float("inf"), float("inf")]
        assert torch.tensor([2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25]).to(dt).float().tolist() == [2.0 ** -24, 0.0, 2.0 ** -23]
    for m in (torch.float32, torch.float16, torch.bfloat16):  # every map type still carries ties of both output types or a subnormal one
        s = specials_for(m)
        assert bool(torch.isnan(s).any()) and bool(torch.isinf(s).any()) and s.numel() >= 9
        fin = s[torch.isfinite(s)]
        assert bool((fin.to(dt).float() != fin).any()) or m == dt, (m, dt)
