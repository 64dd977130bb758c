"""GPU: the refusals the per-pair hand-over wrappers of pats_amd.ops share (topk_by_pair, epipolar_score_by_pair,
epipolar_hypotheses_by_pair, epipolar_pose_by_pair), each under the wrapper's own name and word for word.  They need GPU tensors -
a CPU tensor is turned away before any of them is reached (the *_host.py tests) - but every one is raised in Python before the C
call: nothing is launched here."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS, CAP, H, K = 2, 20, 4, 4
EPIPOLAR = ("epipolar_score_by_pair", "epipolar_hypotheses_by_pair", "epipolar_pose_by_pair")
ALL = ("topk_by_pair",) + EPIPOLAR
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64
# the destinations of a call without optional outputs: (name, dtype, shape)
OUTPUTS = {
    "topk_by_pair": (("top_l", torch.float32, (PAIRS, K, 2)), ("top_r", torch.float32, (PAIRS, K, 2)),
                     ("top_conf", torch.float32, (PAIRS, K)), ("top_idx", I32, (PAIRS, K)), ("top_count", I64, (PAIRS,))),
    "epipolar_score_by_pair": (("counts", I32, (PAIRS, H)), ("best", I32, (PAIRS,)), ("best_count", I64, (PAIRS,)), ("inlier", U8, (CAP,))),
    "epipolar_hypotheses_by_pair": (("models", torch.float32, (PAIRS, H, 3, 3)),),
    "epipolar_pose_by_pair": (("E", F64, (PAIRS, 3, 3)), ("R", F64, (PAIRS, 3, 3)), ("t", F64, (PAIRS, 3)), ("front_count", I64, (PAIRS,)),
                              ("front_counts", I32, (PAIRS, 4)), ("choice", I32, (PAIRS,))),
}


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def call(name, ragged=True, **kw):
    """The wrapper on well-formed zeros - the ragged form (pair_off) or the strided one (stride, counts) - with kw on top."""
    from pats_amd import ops
    a = {"matches_l": z(CAP, 2), "matches_r": z(CAP, 2)}
    a.update({"pair_off": z(PAIRS + 1, dtype=I64)} if ragged else {"stride": CAP // PAIRS, "counts": z(PAIRS, dtype=I64)})
    if name == "topk_by_pair":
        a.update(conf=z(CAP), K=K)
    elif name == "epipolar_score_by_pair":
        a.update(models=z(PAIRS, H, 3, 3), thr=z(PAIRS))
    elif name == "epipolar_hypotheses_by_pair":
        a.update(H=H, seed=z(PAIRS, dtype=I64))
    else:
        a.update(inlier=z(CAP, dtype=U8), best_count=z(PAIRS, dtype=I64), moments=z(PAIRS, 9, 9, dtype=F64))
    a.update(kw)
    return getattr(ops, name)(**{k: v for k, v in a.items() if v is not None})


def refused(name, message, **kw):
    with pytest.raises(RuntimeError, match="^" + re.escape("%s: %s" % (name, message))):
        call(name, **kw)


@pytest.mark.parametrize("name", EPIPOLAR)
def test_exactly_one_segment_form(name):
    message = "give either pair_off, or stride and counts"
    refused(name, message, pair_off=None)
    refused(name, message, stride=10, counts=z(PAIRS, dtype=I64))
    refused(name, message, pair_off=None, stride=10)
    refused(name, message, pair_off=None, counts=z(PAIRS, dtype=I64))


@pytest.mark.parametrize("name", ALL)
def test_ragged_segments(name):
    refused(name, "pair_off must be an int64 vector", pair_off=z(1, PAIRS + 1, dtype=I64))
    refused(name, "pair_off holds 2 entries, 2 pairs need 3", pair_off=z(PAIRS, dtype=I64), pairs=PAIRS)
    refused(name, "pair_off holds 1 entries, 0 pairs need 1", pair_off=z(1, dtype=I64))
    refused(name, "pair_off holds 7 entries, 7 pairs need 8", pair_off=z(PAIRS + 5, dtype=I64), pairs=PAIRS + 5)


@pytest.mark.parametrize("name", EPIPOLAR)
def test_strided_segments(name):
    refused(name, "counts must hold one int64 per pair", ragged=False, counts=z(PAIRS + 1, dtype=I64), pairs=PAIRS)
    refused(name, "counts must hold one int64 per pair", ragged=False, counts=z(0, dtype=I64))
    refused(name, "stride = 11: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=CAP // PAIRS + 1)
    refused(name, "stride = 0: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=0)
    refused(name, "stride = -3: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=-3)


@pytest.mark.parametrize("name", EPIPOLAR)
def test_match_lists_and_norm(name):
    message = "matches_l / matches_r must be [cap,2]"
    refused(name, message, matches_l=z(CAP, 3), matches_r=z(CAP, 3))
    refused(name, message, matches_l=z(2 * CAP))
    refused(name, message, matches_r=z(CAP // 2, 2))
    refused(name, message, matches_l=z(PAIRS, CAP // PAIRS, 2))                # a [pairs,K,2] list against a [cap,2] one
    for norm in (z(PAIRS, 7), z(PAIRS + 1, 8), z(PAIRS * 8), z(8, PAIRS)):
        refused(name, "norm must be [pairs,8]", norm=norm)
        refused(name, "norm must be [pairs,8]", ragged=False, norm=norm)


@pytest.mark.parametrize("name", ALL)
def test_destinations(name):
    want = OUTPUTS[name]
    good = [z(*shape, dtype=dt) for _, dt, shape in want]
    names = "out must be (%s)" % ", ".join(n for n, _, _ in want)
    refused(name, names, out=())
    refused(name, names, out=tuple(good) + (z(1),))
    for i, (n, dt, shape) in enumerate(want):
        message = "%s must be a contiguous GPU %s tensor of shape %s" % (n, dt, list(shape))
        longer = z(*((shape[0] + 1,) + shape[1:]), dtype=dt)
        other = z(*shape, dtype=F64 if dt != F64 else torch.float32)
        strided = z(*((2 * shape[0],) + shape[1:]), dtype=dt)[::2]
        for bad in (longer, other, strided, None):
            refused(name, message, out=tuple(good[:i] + [bad] + good[i + 1:]))
