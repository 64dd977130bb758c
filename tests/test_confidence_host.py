"""CPU-only: the per-match confidence entry points (ABI 8, symbols added) are declared, exported with the ctypes signatures
_lib.py holds, and refuse a null or misaligned confidence pointer before any launch; the Python layer takes the new keyword
arguments; the production library gains no environment switch.  No kernel runs here: every C call below fails validation."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import REPO

CONF = ("pats_third_level_typed_conf", "pats_compute_result_ws_conf_f32", "pats_refine_scatter_conf_f32",
        "pats_get_result_chunks_conf_f32", "pats_get_result_chunks_ragged_conf_f32", "pats_matches_by_pair_summary_conf_f32",
        "pats_matches_by_row_pair_summary_conf_f32")
# the entry each one is named after, and the pointers it adds
PLAIN = {"pats_third_level_typed_conf": ("pats_third_level_typed", 1),
         "pats_compute_result_ws_conf_f32": ("pats_compute_result_ws_f32", 1),
         "pats_refine_scatter_conf_f32": ("pats_refine_scatter_f32", 2),
         "pats_get_result_chunks_conf_f32": ("pats_get_result_chunks_f32", 2),
         "pats_get_result_chunks_ragged_conf_f32": ("pats_get_result_chunks_ragged_f32", 2),
         "pats_matches_by_pair_summary_conf_f32": ("pats_matches_by_pair_summary_f32", 2),
         "pats_matches_by_row_pair_summary_conf_f32": ("pats_matches_by_row_pair_summary_f32", 2)}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_header_and_ctypes_table_agree_on_the_confidence_entries(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name in CONF:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):           # pointers <-> c_void_p (int[3] and the pair table: the plain entries' types)
            if p.startswith("const pats_pair_table_t*"):
                want = _lib.SIGNATURES["pats_get_result_chunks_ragged_f32"][1][0]
            elif p.startswith("const int*"):
                want = ctypes.POINTER(ctypes.c_int)
            elif p.startswith("size_t"):
                want = ctypes.c_size_t
            elif "*" in p or p.startswith("pats_stream_t"):
                want = ctypes.c_void_p
            else:
                want = ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (name, p)
        plain, extra = PLAIN[name]
        assert len(args) == len(_lib.SIGNATURES[plain][1]) + extra, name
        assert sum("conf" in p for p in params) == extra, name


# fake device addresses: validation must refuse them before anything touches them (nothing is launched on a refusal)
A16 = 0x7f0000001000
A2 = A16 + 2
A1 = A16 + 1


def _p(a):
    return ctypes.c_void_p(a) if a else None


def _third(lib, conf, P_dev=0):
    f = _p(A16)
    sxy = None if P_dev else f
    return lib.pats_third_level_typed_conf(f, f, 0, 4, _p(P_dev), 128, f, sxy, sxy, f, f, 100, 1, f, f, f, f, None, _p(conf), None)


def _cr(lib, conf):
    f = _p(A16)
    return lib.pats_compute_result_ws_conf_f32(f, 0, 4, f, f, f, f, 1, f, f, None, f, f, _p(conf), None, 0, None)


def _scatter(lib, conf, conf16):
    f = _p(A16)
    return lib.pats_refine_scatter_conf_f32(f, f, f, f, 2, _p(conf), 1, 4, f, f, _p(conf16), f, 1 << 20, None)


def _chunks(lib, conf16, mconf):
    f = _p(A16)
    ps = (ctypes.c_int * 3)(32, 5, 6)
    ps1 = (ctypes.c_int * 3)(2, 48, 48)
    return lib.pats_get_result_chunks_conf_f32(1, 1, f, f, 4, f, f, f, _p(conf16), ps, ps1, f, f, f, f, _p(mconf), f, 16, f, f,
                                               1 << 20, None)


def _ragged(lib, conf16, mconf):
    f = _p(A16)
    ps1 = (ctypes.c_int * 3)(2, 48, 48)
    return lib.pats_get_result_chunks_ragged_conf_f32(None, 1, f, f, 4, f, f, f, _p(conf16), ps1, f, f, f, f, _p(mconf), f, 16, f, f,
                                                      1 << 20, None)


def _pair(lib, mconf, oconf):
    f = _p(A16)
    return lib.pats_matches_by_pair_summary_conf_f32(f, f, _p(mconf), f, f, f, f, 1, 2, 30, f, f, _p(oconf), f, f, f, f, 1 << 20, None)


def _row_pair(lib, mconf, oconf):
    f = _p(A16)
    return lib.pats_matches_by_row_pair_summary_conf_f32(f, f, _p(mconf), f, f, f, f, 1, 2, f, f, _p(oconf), f, f, f, f, 1 << 20,
                                                         None)


def test_one_confidence_pointer_entries_refuse_null_and_misaligned(lib):
    for call in (_third, lambda l, c: _third(l, c, P_dev=A16), _cr):
        assert call(lib, 0) == 1 and b"null conf" in lib.pats_last_error()
        for bad in (A1, A2):
            assert call(lib, bad) == 1 and b"conf must be 4-byte aligned" in lib.pats_last_error()


@pytest.mark.parametrize("call,names", [(_scatter, b"conf / conf16"), (_chunks, b"conf16 / match_conf"),
                                        (_ragged, b"conf16 / match_conf"), (_pair, b"match_conf / out_conf"),
                                        (_row_pair, b"match_conf / out_conf")])
def test_two_confidence_pointer_entries_refuse_null_and_misaligned(lib, call, names):
    for a, b in ((0, A16), (A16, 0)):
        assert call(lib, a, b) == 1, names
        msg = lib.pats_last_error()
        assert b"null" in msg and names in msg, msg
    for a, b in ((A1, A16), (A16, A2), (A2, A16), (A16, A1)):
        assert call(lib, a, b) == 1, names
        msg = lib.pats_last_error()
        assert b"4-byte aligned" in msg and names in msg, msg


def test_plain_entries_keep_their_rules(lib):
    """The entries the new ones are named after still refuse what they refused, under their own names."""
    f = _p(A16)
    assert lib.pats_refine_scatter_f32(None, f, f, f, 2, 1, 4, f, f, f, 1 << 20, None) == 1
    assert b"refine_scatter: null pointer" in lib.pats_last_error()
    assert lib.pats_matches_by_pair_summary_f32(f, f, f, f, f, f, 1, 2, 30, f, f, f, f, None, f, 1 << 20, None) == 1
    assert b"matches_by_pair_summary: null status" in lib.pats_last_error()


def test_python_layer_takes_the_confidence_keywords_with_defaults_off():
    from pats_amd import batch, ops
    for fn, kw, default in ((ops.third_level, "return_confidence", False), (ops.Compute_result, "return_confidence", False),
                            (ops.refine_scatter, "conf", None), (ops.get_result_chunks, "conf16", None),
                            (ops.matches_by_pair, "match_conf", None), (batch.forward_pairs, "confidence", False),
                            (batch.forward_pairs_mixed, "confidence", False), (batch.third_stage, "confidence", False),
                            (batch.group_by_pair, "confidence", False)):
        p = inspect.signature(fn).parameters
        assert kw in p and p[kw].default is default, (fn.__name__, kw)


def test_production_library_gains_no_environment_switch(lib):
    """The confidence is chosen by the entry point, never by the environment: every string of the shipped library that is
    exactly an environment-variable name has its row in INTEGRATION.md's table (which this change leaves as it was), and none
    of them speaks of the confidence."""
    from pats_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    in_binary = {m.decode() for m in re.findall(rb"(?<=\x00)(PATS_[A-Z0-9_]+)(?=\x00)", blob)} - {"PATS_REQUIRE"}
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    table = doc[doc.index("## 6. Environment switches"):]
    documented = set(re.findall(r"^\| `(PATS_[A-Z0-9_]+)", table, flags=re.M))
    assert in_binary and in_binary <= documented, sorted(in_binary - documented)
    assert not any("CONF" in n for n in in_binary | documented), sorted(in_binary | documented)
