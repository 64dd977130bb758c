"""CPU-only: the half-precision map entry points of the descriptor gathers (ABI 8) are declared, exported and refuse bad
arguments before any launch.  No kernel runs here: every call below fails validation."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TYPED = ("pats_fine_descriptors_typed", "pats_third_descriptors_typed")


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_the_map_dtype_enum_and_the_typed_gathers():
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header)
    enum = re.search(r"typedef enum \{([^}]*)\} pats_map_dtype_t;", header)
    assert enum, "pats_map_dtype_t not declared"
    values = dict(re.findall(r"(PATS_MAP_\w+)\s*=\s*(\d+)", enum.group(1)))
    assert values == {"PATS_MAP_F32": "0", "PATS_MAP_F16": "1", "PATS_MAP_BF16": "2"}
    for name in TYPED:
        assert re.search(r"\bint %s\(" % name, header), name


def test_library_exports_the_typed_gathers_at_abi_8(lib):
    from pats_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name in TYPED:
        assert name in _lib.SIGNATURES and hasattr(lib, name)


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000          # 16-byte aligned
A4 = A16 + 4                  # 4-byte but not 16-byte aligned
A2 = A16 + 2                  # 2-byte aligned: an odd half-element offset


def _fine(lib, maps, dtype, cl, desc=A16, B=1, title=A16, rubbish=A16):
    p = [ctypes.c_void_p(m) if m else None for m in maps]
    return lib.pats_fine_descriptors_typed(p[0], p[1], p[2], dtype, cl, ctypes.c_void_p(title) if title else None,
                                           ctypes.c_void_p(rubbish) if rubbish else None, B, None,
                                           ctypes.c_void_p(desc) if desc else None, None)


def _third(lib, maps, dtype, cl, P=4, B=1, out=A16):
    p = [ctypes.c_void_p(m) if m else None for m in maps]
    o = ctypes.c_void_p(out) if out else None
    f = ctypes.c_void_p(A16)
    return lib.pats_third_descriptors_typed(p[0], p[1], dtype, cl, f, f, f, f, f, P, None, B, o, o, None, None, None)


@pytest.mark.parametrize("bad", [3, -1, 7])
def test_typed_gathers_refuse_an_unknown_dtype(lib, bad):
    assert _fine(lib, (A16, A16, A16), bad, 0) == 1
    assert b"unknown map dtype" in lib.pats_last_error()
    assert _third(lib, (A16, A16), bad, 1) == 1
    assert b"unknown map dtype" in lib.pats_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("cl", [0, 1])
def test_typed_gathers_refuse_null_pointers(lib, dtype, cl):
    for maps in ((None, A16, A16), (A16, None, A16), (A16, A16, None)):
        assert _fine(lib, maps, dtype, cl) == 1 and b"null pointer" in lib.pats_last_error()
    assert _fine(lib, (A16, A16, A16), dtype, cl, desc=0) == 1 and b"null pointer" in lib.pats_last_error()
    assert _fine(lib, (A16, A16, A16), dtype, cl, title=0) == 1 and b"null pointer" in lib.pats_last_error()
    for maps in ((None, A16), (A16, None)):
        assert _third(lib, maps, dtype, cl) == 1 and b"null pointer" in lib.pats_last_error()
    assert _third(lib, (A16, A16), dtype, cl, out=0) == 1 and b"null pointer" in lib.pats_last_error()


@pytest.mark.parametrize("dtype", [1, 2])
def test_typed_gathers_refuse_misaligned_half_maps(lib, dtype):
    # NCHW: 4-byte pair loads -> a map at an odd half-element offset is refused
    for maps in ((A2, A16, A16), (A16, A2, A16), (A16, A16, A2)):
        assert _fine(lib, maps, dtype, 0) == 1 and b"aligned" in lib.pats_last_error()
    for maps in ((A2, A16), (A16, A2)):
        assert _third(lib, maps, dtype, 0) == 1 and b"aligned" in lib.pats_last_error()
    # channels-last: 16-byte pixel loads -> 4-byte alignment is not enough
    for maps in ((A4, A16, A16), (A16, A4, A16), (A16, A16, A4)):
        assert _fine(lib, maps, dtype, 1) == 1 and b"16-byte aligned" in lib.pats_last_error()
    assert _fine(lib, (A16, A16, A16), dtype, 1, desc=A4) == 1 and b"16-byte aligned" in lib.pats_last_error()
    for maps in ((A4, A16), (A16, A4)):
        assert _third(lib, maps, dtype, 1) == 1 and b"16-byte aligned" in lib.pats_last_error()


def test_typed_gathers_refuse_misaligned_f32_maps(lib):
    assert _fine(lib, (A2, A16, A16), 0, 0) == 1 and b"aligned" in lib.pats_last_error()
    assert _fine(lib, (A4, A16, A16), 0, 1) == 1 and b"16-byte aligned" in lib.pats_last_error()
    assert _third(lib, (A16, A2), 0, 0) == 1 and b"aligned" in lib.pats_last_error()
    assert _third(lib, (A2, A16), 0, 1) == 1 and b"aligned" in lib.pats_last_error()


def test_typed_gathers_empty_launches_are_no_ops(lib):
    assert _fine(lib, (None, None, None), 1, 0, B=0) == 0
    assert _third(lib, (None, None), 2, 1, P=0) == 0
    assert _third(lib, (A16, A16), 1, 0, B=0) == 1 and b"bad shape" in lib.pats_last_error()


def test_ops_take_half_maps_and_refuse_other_dtypes_naming_them():
    import torch
    from pats_amd import ops
    # half maps pass the dtype check; these CPU tensors are then refused for being on the CPU, as float32 ones are
    for dt in (torch.float16, torch.bfloat16):
        maps = [torch.zeros(s, dtype=dt) for s in ((2, 64, 48, 48), (2, 64, 24, 24), (2, 128, 12, 12))]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.fine_descriptors(maps, torch.zeros(1, 8), torch.zeros(1, 264))
        f = torch.zeros((1, 128, 52, 52), dtype=dt)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.third_descriptors(f, f, torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, dtype=torch.int64),
                                  torch.zeros(128, 64), torch.zeros(1, 128, 144))
    maps = [torch.zeros((2, 64, 48, 48), dtype=torch.float64), torch.zeros((2, 64, 24, 24)), torch.zeros((2, 128, 12, 12))]
    with pytest.raises(RuntimeError, match="float64"):
        ops.fine_descriptors(maps, torch.zeros(1, 8), torch.zeros(1, 264))
    f = torch.zeros((1, 128, 52, 52), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="int32"):
        ops.third_descriptors(f, f, torch.zeros(1, 2), torch.zeros(1, 2), torch.zeros(1, dtype=torch.int64),
                              torch.zeros(128, 64), torch.zeros(1, 128, 144))
