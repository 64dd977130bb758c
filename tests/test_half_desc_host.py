"""CPU-only: the typed entry points of the cost builds (descriptors in float32 / float16 / bfloat16, ABI 8) are declared,
exported and refuse bad arguments before any launch.  No kernel runs here: every call below fails validation or is empty."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TYPED = ("pats_cost_typed", "pats_cost_ot_typed", "pats_third_level_typed")


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_the_typed_cost_entries():
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header)
    for name in TYPED:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        assert "pats_map_dtype_t dtype" in m.group(1), name      # the one dtype numbering of the library


def test_library_exports_the_typed_cost_entries_at_abi_8(lib):
    from pats_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name in TYPED:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000          # 16-byte aligned
A2 = A16 + 2                  # an odd half-element offset: fine for 2-byte elements, misaligned for float32
A1 = A16 + 1                  # an odd byte: misaligned for every element type


def _p(a):
    return ctypes.c_void_p(a) if a else None


def _cost(lib, d0, d1, dtype, out=A16, batch=2):
    return lib.pats_cost_typed(_p(d0), _p(d1), dtype, batch, 264, 145, 145, _p(out), None)


def _cost_ot(lib, d0, d1, dtype, Z=A16, ns=A16, batch=2, variant=2, n=145, flags=A16, cnt=0):
    return lib.pats_cost_ot_typed(_p(d0), _p(d1), dtype, batch, _p(cnt), 264, n, n, variant, _p(A16), _p(ns), 100, 2.0 if variant == 2 else 0.0,
                                  _p(Z), _p(flags), _p(A16), 1 << 40, None)


def _third(lib, d0, d1, dtype, P=4, out=A16, sxy=A16, cnt=0, Z=0):
    f, o = _p(A16), _p(out)
    return lib.pats_third_level_typed(_p(d0), _p(d1), dtype, P, _p(cnt), 128, f, _p(sxy), _p(sxy), f, f, 100, 1, o, o, o, o, _p(Z), None)


@pytest.mark.parametrize("bad", [3, -1, 7])
def test_typed_cost_entries_refuse_an_unknown_dtype(lib, bad):
    for call in (_cost, _cost_ot, _third):
        assert call(lib, A16, A16, bad) == 1
        assert b"unknown descriptor dtype" in lib.pats_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_cost_entries_refuse_null_pointers(lib, dtype):
    for call in (_cost, _cost_ot, _third):
        for d0, d1 in ((0, A16), (A16, 0)):
            assert call(lib, d0, d1, dtype) == 1 and b"null pointer" in lib.pats_last_error()
    assert _cost(lib, A16, A16, dtype, out=0) == 1 and b"null pointer" in lib.pats_last_error()
    assert _cost_ot(lib, A16, A16, dtype, Z=0) == 1 and b"null pointer" in lib.pats_last_error()
    assert _cost_ot(lib, A16, A16, dtype, ns=0) == 1 and b"null pointer" in lib.pats_last_error()
    assert _third(lib, A16, A16, dtype, out=0) == 1 and b"null pointer" in lib.pats_last_error()
    assert _third(lib, A16, A16, dtype, sxy=0) == 1 and b"null pointer" in lib.pats_last_error()      # plain form: scale_x / scale_y required


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_cost_entries_refuse_misaligned_descriptors(lib, dtype):
    bad = A2 if dtype == 0 else A1          # below the element size
    for call in (_cost, _cost_ot, _third):
        for d0, d1 in ((bad, A16), (A16, bad)):
            assert call(lib, d0, d1, dtype) == 1 and b"aligned" in lib.pats_last_error()
    # the 65-wide cost_ot route (variant 2, 65 x 65) validates in the same place
    assert lib.pats_cost_ot_typed(_p(bad), _p(A16), dtype, 3, None, 128, 65, 65, 2, _p(A16), _p(A16), 100, 0.0, _p(A16), None, None, 0,
                                  None) == 1 and b"aligned" in lib.pats_last_error()


def test_typed_cost_ot_and_third_level_refuse_forms_that_do_not_exist(lib):
    # column flags / a device-side count belong to variant 2 (the count: to the fine level, with flags)
    assert _cost_ot(lib, A16, A16, 1, variant=1, n=300) == 1 and b"variant 2" in lib.pats_last_error()
    assert _cost_ot(lib, A16, A16, 1, n=97, cnt=A16) == 1 and b"fine level" in lib.pats_last_error()
    assert _cost_ot(lib, A16, A16, 2, flags=0, cnt=A16) == 1 and b"fine level" in lib.pats_last_error()
    # the plan does not come with a device-side count
    assert _third(lib, A16, A16, 1, cnt=A16, Z=A16) == 1 and b"device-side count" in lib.pats_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_cost_entries_empty_calls_are_no_ops(lib, dtype):
    assert _cost(lib, 0, 0, dtype, out=0, batch=0) == 0
    assert _cost_ot(lib, 0, 0, dtype, Z=0, ns=0, batch=0, flags=0) == 0
    assert _third(lib, 0, 0, dtype, P=0, out=0, sxy=0) == 0


def test_ops_take_half_descriptors_and_refuse_other_dtypes_naming_them():
    import torch
    from pats_amd import ops
    z2 = torch.zeros(2, dtype=torch.int64).reshape(1, 2)
    for dt in (torch.float16, torch.bfloat16):
        d = torch.zeros((1, 32, 40), dtype=dt)
        # half descriptors pass the dtype check; these CPU tensors are then refused for being on the CPU, as float32 ones are
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.cost(d, d)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.cost_ot(d, d, 1, 0.5, torch.ones(1, 1, 40), 10)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.cost_ot(d, d, 2, 1.0, torch.ones(1, 1, 39), 10, bias_k=2.0, return_flags=True)
        f = torch.zeros((1, 128, 65), dtype=dt)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.third_level(f, f, torch.ones(1, 1, 64), z2, z2)
    for dt, name in ((torch.float64, "float64"), (torch.int32, "int32")):
        d = torch.zeros((1, 32, 40), dtype=dt)
        with pytest.raises(RuntimeError, match=name):
            ops.cost(d, torch.zeros((1, 32, 40)))
        with pytest.raises(RuntimeError, match=name):
            ops.cost_ot(torch.zeros((1, 32, 40)), d, 1, 0.5, torch.ones(1, 1, 40), 10)
        f = torch.zeros((1, 128, 65), dtype=dt)
        with pytest.raises(RuntimeError, match=name):
            ops.third_level(f, f, torch.ones(1, 1, 64), z2, z2)
