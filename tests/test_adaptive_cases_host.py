"""CPU-only: the plain-Python restatement of the adaptive verification's stopping rule (tests/adaptive_cases.py) and the C-ABI
surface of the feature.  Literal values are pinned once by hand from the definition so that the restatement cannot drift with the
kernel; the rule is cross-checked against the closed form of the reference's criterion, k >= log(1 - confidence) / log(1 - w^s)
(cv2.findEssentialMat's, utils/metrics.py:42-44), on cases that all lie clear of an integer; the built library exports the four
new symbols with the header's prototypes and the ctypes table's."""
import ctypes
import math
import os
import re

import pytest

import adaptive_cases as ac
from conftest import REPO

SYMBOLS = {"pats_epipolar_score_adaptive_workspace_bytes": (ctypes.c_size_t, 3), "pats_epipolar_score_adaptive_by_pair_f32": (ctypes.c_int, 28),
           "pats_homography_score_adaptive_workspace_bytes": (ctypes.c_size_t, 3), "pats_homography_score_adaptive_by_pair_f32": (ctypes.c_int, 28)}
CTYPE_OF = (("*", ctypes.c_void_p), ("pats_stream_t", ctypes.c_void_p), ("int64_t", ctypes.c_int64), ("size_t", ctypes.c_size_t),
            ("double", ctypes.c_double), ("float", ctypes.c_float), ("int", ctypes.c_int))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_pinned_miss():
    """By hand: 0.5^10 = 2^-10 exactly; 1^k = 1; 0^1 = 0; k = 0 is the empty product."""
    assert ac.miss(0.5, 10) == 0.0009765625
    assert ac.miss(1.0, 65536) == 1.0
    assert ac.miss(0.0, 1) == 0.0
    assert ac.miss(0.37, 0) == 1.0 and ac.miss(0.0, 0) == 1.0


def test_miss_walks_the_bits_from_the_top():
    """k = 5 = 101b: ((1 * q)^2)^2 * q, in that order - not q * q * q * q * q from the left."""
    q = 0.7
    assert ac.miss(q, 5) == ((q * q) * (q * q)) * q
    assert ac.miss(q, 6) == ((q * q) * q) * ((q * q) * q)


@pytest.mark.parametrize("w,s,g,B,H,want", [
    (0.9, 8, 1, 64, 65536 // 4, 0),          # 1 - 0.9^8 = 0.5695: 21 samples suffice, round 0 holds 64
    (0.5, 4, 1, 64, 65536 // 4, 2),          # 1 - 1/16: 179 samples, T_2 = 192
    (0.5, 5, 10, 320, 65536, 11),            # 1 - 1/32: 363 samples of ten models each = 3630 models, T_11 = 3840
    (0.3, 8, 1, 256, 1024, None),            # 1 - 0.3^8: 175 470 samples - never within H = 1024
])
def test_pinned_stop_rounds(w, s, g, B, H, want):
    """Worked out by hand from k >= ln(1e-5) / ln(1 - w^s), ln(1e-5) = -11.5129."""
    assert ac.stop_round(int(round(w * 1000)), 1000, s, g, B, ac.CONFIDENCE, H) == want
    counts = [0] * H
    counts[0] = int(round(w * 1000))
    assert ac.used_from_counts(counts, 1000, H, B, g, s, ac.CONFIDENCE) == (H if want is None else min(H, (want + 1) * B))


def test_used_from_counts_follows_the_running_best():
    counts = [0] * 448
    counts[10], counts[330] = 450, 550       # 0.45 from round 0: (1 - 0.45^4)^k <= 1e-5 from k = 275 on -> T_4 = 320, before 330 is seen
    assert ac.used_from_counts(counts, 1000, 448, 64, 1, 4, ac.CONFIDENCE) == 320
    counts[10] = 0                           # without it nothing is known before round 5; 0.55 then stops at once (k = 384 >= 120)
    assert ac.used_from_counts(counts, 1000, 448, 64, 1, 4, ac.CONFIDENCE) == 384
    assert ac.used_from_counts([0] * 100, 0, 100, 64, 1, 8, ac.CONFIDENCE) == 100             # nobody participates: w = 0, never
    assert ac.used_from_counts([7] * 100, 7, 100, 64, 1, 8, ac.CONFIDENCE) == 64              # w = 1: q = 0, 0^64 = 0
    assert ac.used_from_counts([7] * 5, 7, 5, 64, 10, 8, ac.CONFIDENCE) == 5                  # k = 5 // 10 = 0: miss = 1


def test_the_rule_is_the_references_criterion():
    """The stop round from miss <= eta equals the stop round from the closed form wherever log(eta) / log(1 - w^s) lies further
    than 1e-9 (relative) from an integer - and the cases are chosen so that all of them do."""
    eta = 1.0 - ac.CONFIDENCE
    cases = [(c, 1000, s, g, B, H) for c in range(300, 1000, 15) for s in (4, 5, 8) for g, B in ((1, 64), (1, 256), (10, 320))
             for H in (1024, 16384)]
    cases += [(c, 997, 4, 1, 128, 4096) for c in range(100, 997, 31)] + [(1000, 1000, 8, 1, 64, 64), (0, 1000, 8, 1, 64, 256)]
    unqualified = 0
    for c, part, s, g, B, H in cases:
        w = c / part
        q = 1.0 - w ** s
        if q == 0.0:
            need = 1                                                      # an all-inlier model: one sample
        elif q == 1.0:
            need = math.inf
        else:
            x = math.log(eta) / math.log(q)
            if abs(x - round(x)) <= 1e-9 * x:
                unqualified += 1
                continue
            need = math.ceil(x)
        want = next((r for r in range(-(-H // B)) if min(H, (r + 1) * B) // g >= need), None)
        assert ac.stop_round(c, part, s, g, B, ac.CONFIDENCE, H) == want, (c, part, s, g, B, H)
    assert len(cases) > 800 and unqualified / len(cases) == 0


# ---- the C-ABI surface ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def test_the_library_exports_the_four_symbols_with_the_headers_prototypes(lib):
    from pats_amd import _lib
    header = open(os.path.join(REPO, "include", "pats_amd.h")).read()
    assert re.search(r"#define PATS_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8 and lib.pats_abi_version() == 8
    for name, (res, nargs) in SYMBOLS.items():
        m = re.search(r"\b(?:int|int64_t|size_t)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",") if p.strip() not in ("", "void")]
        assert len(params) == nargs, (name, params)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and len(got_args) == nargs, name
        for p, a in zip(params, got_args):                                # the prototype's types against the ctypes table's
            want = next(ct for word, ct in CTYPE_OF if (word == "*" and "*" in p) or re.search(r"\b%s\b" % re.escape(word), p))
            assert a is want, (name, p, a)
    # the fixed-budget arguments, in their order, come first
    fixed = re.search(r"\bint\s+pats_epipolar_score_by_pair_f32\(([^;]*)\);", header).group(1)
    for branch in ("epipolar", "homography"):
        adaptive = re.search(r"\bint\s+pats_%s_score_adaptive_by_pair_f32\(([^;]*)\);" % branch, header).group(1)
        assert " ".join(adaptive.split()).startswith(" ".join(fixed.split()) + ", double confidence, int sample_size, int models_per_sample, "
                                                     "int64_t round_models, int32_t* used, int32_t* participating")
    assert "adaptive.hip" in __import__("pats_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.pats_epipolar_score_adaptive_workspace_bytes(48, 1024, 100000) == 48 * 4           # a few words per pair: one
    assert lib.pats_homography_score_adaptive_workspace_bytes(48, 4096, 0) == 48 * 4


def c_call(lib, branch, base, **kw):
    """One raw call with `base` behind every pointer (the ragged form), `kw` overriding arguments by name."""
    a = dict(matches_l=base, matches_r=base, conf=base, pair_off=base, stride=0, counts_in=0, pairs=2, cap=100, models=base, H=512,
             thr=base, norm=base, use_min_conf=0, min_conf=0.0, counts=base, best=base, best_count=base, inlier=base, moments=base,
             workspace=base, workspace_bytes=1 << 20, stream=0, confidence=ac.CONFIDENCE, sample_size=8, models_per_sample=1,
             round_models=256, used=base, participating=base)
    assert not set(kw) - set(a)
    a.update(kw)
    ptr = lambda v: ctypes.c_void_p(v) if v else None                     # noqa: E731
    from pats_amd import _lib
    types = _lib.SIGNATURES["pats_%s_score_adaptive_by_pair_f32" % branch][1]
    args = [ptr(v) if t is ctypes.c_void_p else v for v, t in zip(a.values(), types)]
    return getattr(lib, "pats_%s_score_adaptive_by_pair_f32" % branch)(*args)


def new_refusals(base):
    """The refusals this feature adds -> [(keyword arguments of c_call(), the words the message must hold)]."""
    out = [({"confidence": v}, (b"confidence",)) for v in (0.0, 1.0, 1.5, -0.1, float("nan"), float("inf"))]
    out += [({"sample_size": v}, (b"sample_size",)) for v in (0, -1, 17)]
    out += [({"models_per_sample": v}, (b"models_per_sample",)) for v in (0, -1, 17)]
    out += [({"round_models": v}, (b"round_models", b"multiple of 64")) for v in (0, -64, 63, 65, 100, 320 + 32)]
    out += [({"round_models": 64, "H": 64 * 256 + 1}, (b"rounds",)), ({"round_models": 128, "H": 65536}, (b"rounds",))]
    out += [({name: 0}, (b"null", name.encode())) for name in ("used", "participating", "workspace")]
    out += [({name: base + off}, (b"4-byte aligned", name.encode())) for name in ("used", "participating", "workspace") for off in (1, 2, 3)]
    out += [({"workspace_bytes": 7}, (b"workspace too small",)), ({"workspace_bytes": 0}, (b"workspace too small",))]
    # and what the fixed-budget entry refuses is refused here too
    out += [({"matches_l": 0}, (b"null matches_l",)), ({"H": 0}, (b"H =",)), ({"pairs": 0}, (b"pairs",)), ({"counts_in": base}, (b"pair_off", b"counts_in")),
            ({"use_min_conf": 1, "min_conf": -0.5}, (b"min_conf",)), ({"best_count": base + 4}, (b"8-byte aligned", b"best_count"))]
    return out


def check_refusals(lib, branch, base):
    cases = new_refusals(base)
    for kw, words in cases:
        assert c_call(lib, branch, base, **kw) != 0, (branch, kw)
        msg = lib.pats_last_error()
        assert b"%s_score_adaptive_by_pair" % branch.encode() in msg and all(w in msg for w in words), (branch, kw, msg)
    return len(cases)


@pytest.mark.parametrize("branch", ["epipolar", "homography"])
def test_every_new_bad_argument_is_refused_by_name_before_any_launch(lib, branch):
    """Fake device addresses: validation refuses them before anything touches them (tests/test_adaptive_gpu.py repeats this with a
    real allocation behind the pointers, where a launch would be possible)."""
    assert check_refusals(lib, branch, 0x7f0000001000) > 35


def test_ops_and_batch_signatures_and_refusals_without_a_gpu():
    import inspect
    import torch
    from pats_amd import batch, ops
    sig = ("(matches_l, matches_r, models, thr, confidence, sample_size, models_per_sample=1, round_models=256, pair_off=None, stride=None, "
           "counts=None, conf=None, min_conf=None, norm=None, moments=False, out=None, pairs=None)")
    assert str(inspect.signature(ops.epipolar_score_adaptive_by_pair)) == sig == str(inspect.signature(ops.homography_score_adaptive_by_pair))
    sig = ("(out, cap, models, thr, confidence, sample_size, models_per_sample=1, round_models=None, norm=None, min_conf=None, on='all', "
           "moments=False)")
    assert str(inspect.signature(batch.verify_adaptive_by_pair)) == sig == str(inspect.signature(batch.verify_h_adaptive_by_pair))
    ml, off = torch.zeros(20, 2), torch.tensor([0, 10, 20])
    models, thr = torch.zeros(2, 4, 3, 3), torch.zeros(2)
    cap = batch.Capacities(2, 5, 6)
    plain = {"matches_l": ml, "matches_r": ml, "match_row": None, "M": None, "P": None}
    for fn, verify in ((ops.epipolar_score_adaptive_by_pair, batch.verify_adaptive_by_pair),
                       (ops.homography_score_adaptive_by_pair, batch.verify_h_adaptive_by_pair)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(ml, ml, models, thr, ac.CONFIDENCE, 8, pair_off=off)
        for bad in (0, 1, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match="confidence"):
                fn(ml, ml, models, thr, bad, 8, pair_off=off)
            with pytest.raises(ValueError, match="%s: confidence" % verify.__name__):          # tensor-free: before any device work
                verify(dict(plain), cap, models, thr, bad, 8)
        with pytest.raises(RuntimeError, match="sample_size"):
            fn(ml, ml, models, thr, ac.CONFIDENCE, 0, pair_off=off)
        with pytest.raises(RuntimeError, match="multiple of 64"):
            fn(ml, ml, models, thr, ac.CONFIDENCE, 8, round_models=100, pair_off=off)
        with pytest.raises(RuntimeError, match="models must be float32"):
            fn(ml, ml, models.double(), thr, ac.CONFIDENCE, 8, pair_off=off)
        with pytest.raises(RuntimeError, match="either pair_off, or stride and counts"):
            fn(ml, ml, models, thr, ac.CONFIDENCE, 8)
        with pytest.raises(ValueError, match="on must be"):
            verify(dict(plain), cap, models, thr, ac.CONFIDENCE, 8, on="some")
        with pytest.raises(ValueError, match="confidence=True"):
            verify(dict(plain), cap, models, thr, ac.CONFIDENCE, 8, min_conf=0.5)
