"""CPU-only: the typed crop entry points (uint8 / half images, crops in the backbone's format) are declared, exported and
refuse bad arguments before any launch, and ops.CropFormat validates its fields.  No kernel runs here: every call below fails
validation (or is an empty launch)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TYPED = ("pats_left_crops_typed", "pats_tensor_resize_hwc_typed", "pats_tensor_resize_typed")


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_declares_the_image_dtypes_the_format_and_the_typed_crops():
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header)
    enum = re.search(r"typedef enum \{([^}]*)\} pats_img_dtype_t;", header)
    assert enum, "pats_img_dtype_t not declared"
    assert dict(re.findall(r"(PATS_IMG_\w+)\s*=\s*(\d+)", enum.group(1))) == {
        "PATS_IMG_F32": "0", "PATS_IMG_F16": "1", "PATS_IMG_BF16": "2", "PATS_IMG_U8": "3"}
    layout = re.search(r"typedef enum \{([^}]*)\} pats_crop_layout_t;", header)
    assert layout and dict(re.findall(r"(PATS_CROP_\w+)\s*=\s*(\d+)", layout.group(1))) == {"PATS_CROP_HWC": "0", "PATS_CROP_CHW": "1"}
    fmt = re.search(r"typedef struct pats_crop_format \{([^}]*)\} pats_crop_format_t;", header)
    assert fmt, "pats_crop_format_t not declared"
    assert re.findall(r"(\w+)(?:\[3\])?;", fmt.group(1)) == ["dtype", "layout", "normalize", "mean", "std"]
    # the map dtype enum of the descriptor gathers is untouched
    enum = re.search(r"typedef enum \{([^}]*)\} pats_map_dtype_t;", header)
    assert dict(re.findall(r"(PATS_MAP_\w+)\s*=\s*(\d+)", enum.group(1))) == {"PATS_MAP_F32": "0", "PATS_MAP_F16": "1", "PATS_MAP_BF16": "2"}
    for name in TYPED:
        assert re.search(r"\bint %s\(" % name, header), name


def test_library_exports_the_typed_crops_at_abi_8(lib):
    from pats_amd import _lib
    assert _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name in TYPED:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.CropFormat) == 36


A16 = 0x7f0000001000          # fake device addresses, 16-byte aligned
A8, A2, A1 = A16 + 8, A16 + 2, A16 + 1


def _fmt(dtype=0, layout=0, normalize=0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    from pats_amd import _lib
    f = _lib.CropFormat()
    f.dtype, f.layout, f.normalize = dtype, layout, normalize
    for c in range(3):
        f.mean[c], f.std[c] = mean[c], std[c]
    return f


def _p(a):
    return ctypes.c_void_p(a) if a else None


def _left(lib, fmt, dtype=0, img=A16, out=A16, bound=A16, K=4):
    return lib.pats_left_crops_typed(None, _p(img), dtype, 1, 480, 640, 15, 20, _p(bound), K, None,
                                     ctypes.byref(fmt) if fmt is not None else None, _p(out), None)


def _right(lib, fmt, dtype=0, img=A16, out=A16, bound=A16, K=4):
    return lib.pats_tensor_resize_hwc_typed(None, _p(img), dtype, 1, 480, 640, 128, _p(bound), K, None,
                                            ctypes.byref(fmt) if fmt is not None else None, _p(out), None, None)


def _chw(lib, fmt, dtype=0, img=A16, out=A16, bound=A16, K=4, C=3):
    return lib.pats_tensor_resize_typed(_p(img), dtype, 1, C, 200, 240, _p(bound), K, None,
                                        ctypes.byref(fmt) if fmt is not None else None, _p(out), None, None)


def _refused(lib, rc, what):
    assert rc == 1, rc
    assert what.encode() in lib.pats_last_error(), lib.pats_last_error()


@pytest.mark.parametrize("call", [_left, _right, _chw])
def test_typed_crops_refuse_unknown_dtypes_and_layouts(lib, call):
    ok = _fmt(layout=1)
    for bad in (4, -1, 9):
        _refused(lib, call(lib, ok, dtype=bad), "unknown image dtype")
        _refused(lib, call(lib, _fmt(dtype=bad, layout=1)), "unknown crop dtype")
    for bad in (2, -1):
        _refused(lib, call(lib, _fmt(layout=bad)), "unknown crop layout")


def test_typed_crops_refuse_uint8_output_where_it_is_not_an_exact_copy(lib):
    for call in (_right, _chw):
        _refused(lib, call(lib, _fmt(dtype=3, layout=1), dtype=3), "uint8 output is for left crops only")
    for dt in (0, 1, 2):
        _refused(lib, _left(lib, _fmt(dtype=3), dtype=dt), "uint8 output needs uint8 images")
    _refused(lib, _left(lib, _fmt(dtype=3, normalize=1, std=(1.0, 2.0, 3.0)), dtype=3), "cannot be normalised")


@pytest.mark.parametrize("call", [_left, _right, _chw])
@pytest.mark.parametrize("mean, std", [((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)), ((float("nan"), 0.0, 0.0), (1.0, 1.0, 1.0)),
                                       ((0.0, float("inf"), 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, float("inf"))),
                                       ((0.0, 0.0, 0.0), (float("nan"), 1.0, 1.0)), ((0.0, 0.0, 0.0), (-0.0, 1.0, 1.0))])
def test_typed_crops_refuse_bad_normalisation(lib, call, mean, std):
    _refused(lib, call(lib, _fmt(dtype=2, layout=1, normalize=1, mean=mean, std=std)), "finite")
    # without normalisation the mean / std fields are not read
    assert call(lib, _fmt(dtype=2, layout=1, normalize=0, mean=mean, std=std), K=0) == 0


@pytest.mark.parametrize("call", [_left, _right, _chw])
def test_typed_crops_refuse_null_pointers(lib, call):
    f = _fmt(dtype=1, layout=1)
    _refused(lib, call(lib, None), "null pointer")
    _refused(lib, call(lib, f, img=0), "null pointer")
    _refused(lib, call(lib, f, out=0), "null pointer")
    _refused(lib, call(lib, f, bound=0), "null pointer")


@pytest.mark.parametrize("call", [_left, _right, _chw])
def test_typed_crops_refuse_misaligned_pointers(lib, call):
    _refused(lib, call(lib, _fmt(layout=1), dtype=0, img=A2), "4-byte aligned")
    for dt in (1, 2):
        _refused(lib, call(lib, _fmt(layout=1), dtype=dt, img=A1), "2-byte aligned")
    for out in (A8, A2):
        _refused(lib, call(lib, _fmt(dtype=2, layout=1), dtype=3, out=out), "16-byte aligned")
    assert call(lib, _fmt(layout=1), dtype=3, img=A1, K=0) == 0        # uint8 images: any byte; K == 0: nothing launched


def test_typed_tensor_resize_refusals_of_its_own(lib):
    _refused(lib, _chw(lib, _fmt(layout=0)), "layout must be chw")
    _refused(lib, _chw(lib, _fmt(layout=1, normalize=1), C=4), "C == 3")
    assert _chw(lib, _fmt(layout=1, normalize=1), C=3, K=0) == 0


def test_typed_crops_refuse_a_bad_pair_table(lib):
    from pats_amd import _lib
    t = _lib.PairTable(0, None, None, None, None, None)
    rc = lib.pats_left_crops_typed(ctypes.byref(t), _p(A16), 3, 0, 0, 0, 0, 0, _p(A16), 4, None, ctypes.byref(_fmt()), _p(A16), None)
    _refused(lib, rc, "pair table")
    rc = lib.pats_tensor_resize_hwc_typed(ctypes.byref(t), _p(A16), 3, 0, 0, 0, 128, _p(A16), 4, None, ctypes.byref(_fmt()),
                                          _p(A16), None, None)
    _refused(lib, rc, "pair table")


def test_crop_format_validation():
    import torch
    from pats_amd import ops
    d = ops.CropFormat()
    assert d.is_default() and d.shape(5) == (5, 96, 96, 3) and not d.normalize
    b = ops.CropFormat.backbone(torch.bfloat16)
    assert b.layout == "chw" and b.dtype == torch.bfloat16 and b.shape(2) == (2, 3, 96, 96)
    assert b.mean == (0.485, 0.456, 0.406) and b.std == (0.229, 0.224, 0.225)
    c = b._c()
    assert (c.dtype, c.layout, c.normalize) == (2, 1, 1) and abs(c.std[2] - 0.225) < 1e-7
    for bad in ("nhwc", "HWC", None):
        with pytest.raises(ValueError, match="layout"):
            ops.CropFormat(layout=bad)
    for bad in (torch.float64, torch.int32, "bf16", None):
        with pytest.raises(ValueError, match="dtype"):
            ops.CropFormat(dtype=bad)
    with pytest.raises(ValueError, match="3 values"):
        ops.CropFormat(mean=(1.0, 2.0), std=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="3 values"):
        ops.CropFormat(mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="together"):
        ops.CropFormat(mean=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="non-zero"):
        ops.CropFormat(mean=(1.0, 2.0, 3.0), std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="normalised"):
        ops.CropFormat(torch.uint8, mean=(1.0, 2.0, 3.0), std=(1.0, 1.0, 1.0))


def test_ops_tensor_resize_takes_half_and_names_the_dtype_otherwise():
    import torch
    from pats_amd import ops
    b = torch.zeros((1, 5), dtype=torch.int64)
    for dt in (torch.float16, torch.bfloat16):          # half passes the dtype check; a CPU tensor is then refused
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.tensor_resize(torch.zeros((1, 3, 8, 8), dtype=dt), b)
    for dt in (torch.float64, torch.uint8, torch.int32):
        with pytest.raises(RuntimeError, match="float32"):
            ops.tensor_resize(torch.zeros((1, 3, 8, 8), dtype=dt), b)
