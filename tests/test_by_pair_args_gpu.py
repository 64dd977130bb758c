"""GPU: the refusals the per-pair hand-over wrappers of pats_amd.ops share (topk_by_pair, the epipolar score / hypotheses / pose /
polish stages, the absolute branch's lift / hypotheses / score / polish), each under the wrapper's own name and word for word.
They need GPU tensors - a CPU tensor is turned away before any of them is reached (the *_host.py tests) - but every one is raised
in Python before the C call: nothing is launched here."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS, CAP, H, K = 2, 20, 4, 4
EPIPOLAR = ("epipolar_score_by_pair", "epipolar_hypotheses_by_pair", "epipolar_pose_by_pair")
ABSOLUTE = ("absolute_hypotheses_by_pair", "absolute_score_by_pair", "absolute_polish_by_pair")
LIFT = ("lift_by_pair",)
ALL = ("topk_by_pair",) + EPIPOLAR
SCORES = ("epipolar_score_by_pair", "homography_score_by_pair", "absolute_score_by_pair")
POLISHES = ("epipolar_polish_by_pair", "homography_polish_by_pair", "fundamental_polish_by_pair", "absolute_polish_by_pair")
GENERATORS = ("epipolar_hypotheses_by_pair", "absolute_hypotheses_by_pair")
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64
ROUNDS = 4                                               # the polishes' default
# the destinations of a call without optional outputs: (name, dtype, shape)
OUTPUTS = {
    "topk_by_pair": (("top_l", torch.float32, (PAIRS, K, 2)), ("top_r", torch.float32, (PAIRS, K, 2)),
                     ("top_conf", torch.float32, (PAIRS, K)), ("top_idx", I32, (PAIRS, K)), ("top_count", I64, (PAIRS,))),
    "epipolar_score_by_pair": (("counts", I32, (PAIRS, H)), ("best", I32, (PAIRS,)), ("best_count", I64, (PAIRS,)), ("inlier", U8, (CAP,))),
    "epipolar_hypotheses_by_pair": (("models", torch.float32, (PAIRS, H, 3, 3)),),
    "epipolar_pose_by_pair": (("E", F64, (PAIRS, 3, 3)), ("R", F64, (PAIRS, 3, 3)), ("t", F64, (PAIRS, 3)), ("front_count", I64, (PAIRS,)),
                              ("front_counts", I32, (PAIRS, 4)), ("choice", I32, (PAIRS,))),
    "epipolar_polish_by_pair": (("model", torch.float32, (PAIRS, 3, 3)), ("best_count", I64, (PAIRS,)), ("inlier", U8, (CAP,)),
                                ("moments", F64, (PAIRS, 9, 9)), ("best_round", I32, (PAIRS,)), ("counts", I32, (PAIRS, ROUNDS + 1))),
    "absolute_hypotheses_by_pair": (("models", torch.float32, (PAIRS, H, 4, 3, 4)),),
    "absolute_score_by_pair": (("counts", I32, (PAIRS, H)), ("best", I32, (PAIRS,)), ("best_count", I64, (PAIRS,)), ("inlier", U8, (CAP,))),
    "absolute_polish_by_pair": (("model", torch.float32, (PAIRS, 3, 4)), ("best_count", I64, (PAIRS,)), ("inlier", U8, (CAP,)),
                                ("best_round", I32, (PAIRS,)), ("counts", I32, (PAIRS, ROUNDS + 1)), ("cost", F64, (PAIRS, ROUNDS + 1))),
    "lift_by_pair": (("points", torch.float32, (CAP, 3)), ("valid", U8, (CAP,)), ("lift_count", I64, (PAIRS,))),
}
OUTPUTS["homography_score_by_pair"] = OUTPUTS["epipolar_score_by_pair"]
OUTPUTS["homography_polish_by_pair"] = OUTPUTS["fundamental_polish_by_pair"] = OUTPUTS["epipolar_polish_by_pair"]


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda")


def absolute(name):
    return name.startswith("absolute")


def model_shape(name):
    """(the model's shape, the letter of the model count in the wrapper's messages)"""
    return ((3, 4), "M") if absolute(name) else ((3, 3), "H")


def call(name, ragged=True, **kw):
    """The wrapper on well-formed zeros - the ragged form (pair_off) or the strided one (stride, counts) - with kw on top."""
    from pats_amd import ops
    a = {"matches_l": z(CAP, 2), "matches_r": z(CAP, 2)}
    if absolute(name):
        a = {"points": z(CAP, 3), "matches_r": z(CAP, 2)}
    elif name == "lift_by_pair":
        a = {"matches": z(CAP, 2), "depths": None, "table": z(PAIRS, 4, dtype=I64)}
    a.update({"pair_off": z(PAIRS + 1, dtype=I64)} if ragged else {"stride": CAP // PAIRS, "counts": z(PAIRS, dtype=I64)})
    if name == "topk_by_pair":
        a.update(conf=z(CAP), K=K)
    elif name in SCORES:
        a.update(models=z(PAIRS, H, *model_shape(name)[0]), thr=z(PAIRS))
    elif name in POLISHES:
        a.update(models=z(PAIRS, H, *model_shape(name)[0]), thr=z(PAIRS), best=z(PAIRS, dtype=I32))
    elif name in GENERATORS:
        a.update(H=H, seed=z(PAIRS, dtype=I64))
    elif name == "epipolar_pose_by_pair":
        a.update(inlier=z(CAP, dtype=U8), best_count=z(PAIRS, dtype=I64), moments=z(PAIRS, 9, 9, dtype=F64))
    a.update(kw)
    return getattr(ops, name)(**{k: v for k, v in a.items() if v is not None or k == "depths"})


def refused(name, message, **kw):
    with pytest.raises(RuntimeError, match="^" + re.escape("%s: %s" % (name, message))):
        call(name, **kw)


@pytest.mark.parametrize("name", EPIPOLAR + ABSOLUTE + LIFT + POLISHES[:3])
def test_exactly_one_segment_form(name):
    message = "give either pair_off, or stride and counts"
    refused(name, message, pair_off=None)
    refused(name, message, stride=10, counts=z(PAIRS, dtype=I64))
    refused(name, message, pair_off=None, stride=10)
    refused(name, message, pair_off=None, counts=z(PAIRS, dtype=I64))


@pytest.mark.parametrize("name", ALL + ABSOLUTE + LIFT + POLISHES[:3])
def test_ragged_segments(name):
    refused(name, "pair_off must be an int64 vector", pair_off=z(1, PAIRS + 1, dtype=I64))
    refused(name, "pair_off holds 2 entries, 2 pairs need 3", pair_off=z(PAIRS, dtype=I64), pairs=PAIRS)
    refused(name, "pair_off holds 1 entries, 0 pairs need 1", pair_off=z(1, dtype=I64))
    refused(name, "pair_off holds 7 entries, 7 pairs need 8", pair_off=z(PAIRS + 5, dtype=I64), pairs=PAIRS + 5)


@pytest.mark.parametrize("name", EPIPOLAR + ABSOLUTE + LIFT + POLISHES[:3])
def test_strided_segments(name):
    refused(name, "counts must hold one int64 per pair", ragged=False, counts=z(PAIRS + 1, dtype=I64), pairs=PAIRS)
    refused(name, "counts must hold one int64 per pair", ragged=False, counts=z(0, dtype=I64))
    refused(name, "stride = 11: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=CAP // PAIRS + 1)
    refused(name, "stride = 0: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=0)
    refused(name, "stride = -3: pairs * stride must lie in 1 .. cap = 20", ragged=False, stride=-3)


@pytest.mark.parametrize("name", EPIPOLAR + POLISHES[:3] + SCORES[1:2])
def test_match_lists_and_norm(name):
    message = "matches_l / matches_r must be [cap,2]"
    refused(name, message, matches_l=z(CAP, 3), matches_r=z(CAP, 3))
    refused(name, message, matches_l=z(2 * CAP))
    refused(name, message, matches_r=z(CAP // 2, 2))
    refused(name, message, matches_l=z(PAIRS, CAP // PAIRS, 2))                # a [pairs,K,2] list against a [cap,2] one
    for norm in (z(PAIRS, 7), z(PAIRS + 1, 8), z(PAIRS * 8), z(8, PAIRS)):
        refused(name, "norm must be [pairs,8]", norm=norm)
        refused(name, "norm must be [pairs,8]", ragged=False, norm=norm)


@pytest.mark.parametrize("name", ABSOLUTE)
def test_lifted_lists_and_norm(name):
    message = "points must be [cap,3] and matches_r [cap,2]"
    refused(name, message, points=z(CAP, 2))
    refused(name, message, points=z(3 * CAP))
    refused(name, message, matches_r=z(CAP, 3))
    refused(name, message, matches_r=z(2 * CAP))
    refused(name, message, matches_r=z(CAP // 2, 2))
    refused(name, message, points=z(CAP + 1, 3))
    for norm in (z(PAIRS, 7), z(PAIRS + 1, 8), z(PAIRS * 8), z(8, PAIRS)):
        refused(name, "norm must be [pairs,8]", norm=norm)
        refused(name, "norm must be [pairs,8]", ragged=False, norm=norm)


def test_lift_list_norm_and_table():
    name = "lift_by_pair"
    refused(name, "matches must be [cap,2]", matches=z(CAP, 3))
    refused(name, "matches must be [cap,2]", matches=z(2 * CAP))
    for norm in (z(PAIRS, 7), z(PAIRS + 1, 8), z(PAIRS * 8), z(8, PAIRS)):
        refused(name, "norm must be [pairs,8]", norm=norm)
    refused(name, "the depth table must be [pairs,4] int64 (2 pairs), got [3, 4]", table=z(PAIRS + 1, 4, dtype=I64))
    refused(name, "depths must hold one map (or None) per pair (2), got None", table=None)
    refused(name, "max_depth must hold one float32 per pair (2), got 3", max_depth=z(PAIRS + 1))
    refused(name, "interp must be \"nearest\" (0) or \"bilinear\" (1), got 'cubic'", interp="cubic")


@pytest.mark.parametrize("name", SCORES + POLISHES)
def test_confidence_gate(name):
    refused(name, "min_conf needs conf", min_conf=0.5)
    refused(name, "min_conf needs conf", ragged=False, min_conf=0.0)
    refused(name, "conf must be [cap]", conf=z(CAP + 1))
    refused(name, "conf must be [cap]", conf=z(CAP - 1), min_conf=0.5)
    refused(name, "conf must be [cap]", ragged=False, conf=z(CAP, 2))


@pytest.mark.parametrize("name", SCORES + POLISHES)
def test_models_and_their_count(name):
    from pats_amd import ops
    shape, letter = model_shape(name)
    want = "[pairs,%s,%d,%d]" % (letter, shape[0], shape[1])
    other = (3, 3) if absolute(name) else (3, 4)
    refused(name, "models must be %s" % want, models=z(PAIRS, H, *other))
    refused(name, "models must be %s" % want, models=z(PAIRS * H, *shape))
    refused(name, "models must be %s" % want, models=z(PAIRS, H, 1, *shape))
    refused(name, "models %s and thr [pairs] must hold 2 pairs" % want, models=z(PAIRS + 1, H, *shape))
    refused(name, "models %s and thr [pairs] must hold 2 pairs" % want, thr=z(PAIRS + 1))
    refused(name, "models %s and thr [pairs] must hold 2 pairs" % want, ragged=False, thr=z(1))
    top = ops.epipolar_max_h()
    refused(name, "%s = 0, must lie in 1 .. %d" % (letter, top), models=z(PAIRS, 0, *shape))
    refused(name, "%s = %d, must lie in 1 .. %d" % (letter, top + 1, top), models=z(PAIRS, top + 1, *shape))


@pytest.mark.parametrize("name", POLISHES)
def test_best_and_the_walk(name):
    shape, letter = model_shape(name)
    refused(name, "best may be left out with %s == 1 only, got %s = %d" % (letter, letter, H), best=None)
    refused(name, "best must hold one int32 per pair (2), got 3", best=z(PAIRS + 1, dtype=I32))
    refused(name, "best must be int32, got torch.int64", best=z(PAIRS, dtype=I64))
    refused(name, "rounds = 0, must lie in 1 .. 16", rounds=0)
    refused(name, "rounds = 17, must lie in 1 .. 16", rounds=17)
    if absolute(name):
        refused(name, "steps = 0, must lie in 1 .. 8", steps=0)
        refused(name, "steps = 9, must lie in 1 .. 8", steps=9)
        refused(name, "rounds = 17, must lie in 1 .. 16", rounds=17, steps=9)
    refused(name, "min_conf needs conf", min_conf=0.5, rounds=0)                # the order: the gate before the walk's length


@pytest.mark.parametrize("name", GENERATORS)
def test_seed_and_samples(name):
    from pats_amd import ops
    slots = 4 if absolute(name) else 1
    top = ops.epipolar_max_h() // slots
    tail = " (4 H models)" if absolute(name) else ""
    refused(name, "seed must be an int64 GPU tensor [pairs]", seed=7)
    refused(name, "seed must be int64, got torch.int32", seed=z(PAIRS, dtype=I32))
    refused(name, "seed must hold one int64 per pair (2), got 3", seed=z(PAIRS + 1, dtype=I64))
    refused(name, "H = 0, must lie in 1 .. %d%s" % (top, tail), H=0)
    refused(name, "H = %d, must lie in 1 .. %d%s" % (top + 1, top, tail), H=top + 1)
    refused(name, "seed must hold one int64 per pair (2), got 3", seed=z(PAIRS + 1, dtype=I64), H=0)


@pytest.mark.parametrize("name", EPIPOLAR[:2] + ABSOLUTE + LIFT + POLISHES[:1])
def test_layout_and_dtype(name):
    first = "points" if absolute(name) else ("matches" if name == "lift_by_pair" else "matches_l")
    width = 3 if absolute(name) else 2
    refused(name, "%s must be contiguous" % first, **{first: z(2 * CAP, width)[::2]})
    refused(name, "%s must be float32, got torch.float64" % first, **{first: z(CAP, width, dtype=F64)})
    refused(name, "pair_off must be int64, got torch.int32", pair_off=z(PAIRS + 1, dtype=I32))
    refused(name, "counts must be int64, got torch.int32", ragged=False, counts=z(PAIRS, dtype=I32))
    refused(name, "norm must be contiguous", norm=z(PAIRS, 16)[:, ::2])
    refused(name, "norm must be float32, got torch.float16", norm=z(PAIRS, 8, dtype=torch.float16))
    if name != "lift_by_pair":
        refused(name, "matches_r must be contiguous", matches_r=z(2 * CAP, 2)[::2])
        refused(name, "matches_r must be float32, got torch.float64", matches_r=z(CAP, 2, dtype=F64))
    # a bad layout is refused before a missing segment form
    refused(name, "%s must be contiguous" % first, **{first: z(2 * CAP, width)[::2], "pair_off": None})


@pytest.mark.parametrize("name", ALL + ABSOLUTE + LIFT + POLISHES[:1])
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
