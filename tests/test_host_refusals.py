"""CPU-only: what the C entries of the per-pair verification, local-optimisation and hypothesis stages refuse, word for word
(pats_last_error), and in which order.  The entries are called through ctypes with made-up integer addresses - aligned, misaligned
or null; they are not memory, so EVERY call here is one the host checks turn away before anything touches a device."""
import pytest

SCORE = ("first", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "models", "H", "thr", "norm", "use_min_conf",
         "min_conf", "counts", "best", "best_count", "inlier", "moments", "workspace", "workspace_bytes", "stream")
POLISH = ("first", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "thr", "norm", "use_min_conf", "min_conf",
          "models", "H", "best", "rounds", "model", "best_count", "inlier", "moments", "best_round", "counts", "workspace",
          "workspace_bytes", "stream")
HYPOTHESES = ("first", "matches_r", "pair_off", "stride", "counts_in", "pairs", "cap", "H", "pair_seed", "norm", "progressive", "models",
              "sample_idx", "workspace", "workspace_bytes", "stream")
ABS_HYPOTHESES = HYPOTHESES[:13] + ("n_models", "stream")
ABS_SCORE = SCORE[:18] + ("stream",)
ABS_POLISH = ("first", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "models", "H", "thr", "norm", "use_min_conf",
              "min_conf", "best", "rounds", "steps", "model", "best_count", "inlier", "best_round", "counts", "cost", "stream")
# entry -> (the name its messages carry, its arguments in order, the name and alignment of its first list, the letter of the
# null-best message)
ENTRIES = {
    "pats_epipolar_score_by_pair_f32": ("epipolar_score_by_pair", SCORE, "matches_l", 8, "H"),
    "pats_homography_score_by_pair_f32": ("homography_score_by_pair", SCORE, "matches_l", 8, "H"),
    "pats_epipolar_polish_by_pair_f32": ("epipolar_polish_by_pair", POLISH, "matches_l", 8, "H"),
    "pats_homography_polish_by_pair_f32": ("homography_polish_by_pair", POLISH, "matches_l", 8, "H"),
    "pats_fundamental_polish_by_pair_f32": ("fundamental_polish_by_pair", POLISH, "matches_l", 8, "H"),
    "pats_epipolar_hypotheses_by_pair_f32": ("epipolar_hypotheses_by_pair", HYPOTHESES, "matches_l", 8, "H"),
    "pats_absolute_hypotheses_by_pair_f32": ("absolute_hypotheses_by_pair", ABS_HYPOTHESES, "points", 4, "M"),
    "pats_absolute_score_by_pair_f32": ("absolute_score_by_pair", ABS_SCORE, "points", 4, "M"),
    "pats_absolute_polish_by_pair_f32": ("absolute_polish_by_pair", ABS_POLISH, "points", 4, "M"),
}
SCORES = [e for e in ENTRIES if "_score_" in e]
POLISHES = [e for e in ENTRIES if "_polish_" in e]
GENERATORS = [e for e in ENTRIES if "_hypotheses_" in e]
GATED = SCORES + POLISHES                               # the entries with conf / min_conf and candidate models
PAIRS, CAP = 2, 20
# the alignment every pointer must have (the first list's is the entry's); inlier is a byte mask, the workspace is not looked at
ALIGN = {"matches_r": 8, "conf": 4, "pair_off": 8, "counts_in": 8, "models": 4, "thr": 4, "norm": 4, "counts": 4, "best": 4, "best_count": 8,
         "moments": 8, "model": 4, "best_round": 4, "cost": 8, "pair_seed": 8, "sample_idx": 4, "n_models": 4}
# the pointers that may be null - two of them in some entries only: a score writes moments on request and always writes best, a local
# optimisation always writes moments and reads best unless there is one model
OPTIONAL = ("conf", "norm", "pair_off", "counts_in", "sample_idx", "n_models")
INTEGERS = {"stride": 0, "pairs": PAIRS, "cap": CAP, "H": 2, "use_min_conf": 0, "min_conf": 0.0, "rounds": 4, "steps": 3, "progressive": 0,
            "workspace_bytes": 0}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


def arguments(entry, **kw):
    """A well-formed ragged call of the entry (every pointer but counts_in, the workspace and the stream set) with kw on top; the
    first list goes by "first" here and by its own name in kw."""
    _, names, first, _, _ = ENTRIES[entry]
    a = {}
    for k, n in enumerate(names):
        a[n] = INTEGERS[n] if n in INTEGERS else (None if n in ("counts_in", "workspace", "stream") else address(k))
    for n, v in kw.items():
        n = "first" if n == first else n
        assert n in a, n
        a[n] = v
    return [a[n] for n in names]


def refused(lib, entry, message, **kw):
    """The call is turned away (PATS_ERR_INVALID = 1) with exactly this message behind the entry's name."""
    rc = getattr(lib, entry)(*arguments(entry, **kw))
    assert rc == 1, "%s(%s) was not refused: %d" % (entry, kw, rc)
    assert lib.pats_last_error().decode() == "%s: %s" % (ENTRIES[entry][0], message)


def strided(**kw):
    """The strided form's arguments: counts_in instead of pair_off."""
    return dict({"pair_off": None, "counts_in": address(40), "stride": CAP // PAIRS}, **kw)


def optional(entry):
    """The names of the pointers the entry takes as null."""
    return OPTIONAL + (("best",) if entry in POLISHES else ("moments",) if entry in SCORES else ())


def pointers(entry):
    """(name, alignment, may be null) of every pointer the entry checks, the first list under its own name."""
    _, names, first, first_align, _ = ENTRIES[entry]
    return [(first, first_align, False)] + [(n, ALIGN[n], n in optional(entry)) for n in names if n in ALIGN] + \
           ([("inlier", 1, False)] if "inlier" in names else [])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_pointer(lib, entry):
    for name, align, may_be_null in pointers(entry):
        if name == "pair_off":                          # null pair_off is the other segment form: below
            refused(lib, entry, "pair_off must be 8-byte aligned", pair_off=address(0) + 4)
            continue
        if name == "counts_in":
            refused(lib, entry, "counts_in must be 8-byte aligned", **strided(counts_in=address(40) + 4))
            continue
        if not may_be_null:
            refused(lib, entry, "null %s" % name, **{name: None})
        if align > 1:
            refused(lib, entry, "%s must be %d-byte aligned" % (name, align), **{name: address(50) + align // 2})


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_segments(lib, entry):
    one = "exactly one of pair_off (ragged segments) and counts_in (strided segments) must be given"
    refused(lib, entry, one, pair_off=None)
    refused(lib, entry, one, counts_in=address(40))
    refused(lib, entry, "pairs = 0 (1 .. 2^31 - 1)", pairs=0)
    refused(lib, entry, "pairs = 0 (1 .. 2^31 - 1)", **strided(pairs=0))
    refused(lib, entry, "cap = -1 (0 .. 2^31 - 2)", cap=-1)
    refused(lib, entry, "stride = 0 must be at least 1", **strided(stride=0))
    refused(lib, entry, "pairs * stride = 2 * 11 exceeds cap = 20", **strided(stride=CAP // PAIRS + 1))
    refused(lib, entry, "pairs * stride = 2 * 21 exceeds cap = 20", **strided(stride=CAP + 1))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_model_count(lib, entry):
    max_h = lib.pats_epipolar_max_h()
    refused(lib, entry, "H = 0 (1 .. max_h = %d)" % max_h, H=0)
    refused(lib, entry, "H = -1 (1 .. max_h = %d)" % max_h, H=-1)
    refused(lib, entry, "H = %d (1 .. max_h = %d)" % (max_h + 1, max_h), H=max_h + 1)
    refused(lib, entry, "H = %d (1 .. max_h = %d)" % (max_h + 1, max_h), **strided(H=max_h + 1))


@pytest.mark.parametrize("entry", GATED)
def test_min_conf(lib, entry):
    refused(lib, entry, "min_conf needs conf", use_min_conf=1, conf=None)
    refused(lib, entry, "min_conf = -1 must be a non-negative number", use_min_conf=1, min_conf=-1.0)
    refused(lib, entry, "min_conf = -0.5 must be a non-negative number", use_min_conf=1, min_conf=-0.5)
    refused(lib, entry, "min_conf = nan must be a non-negative number", use_min_conf=1, min_conf=float("nan"))


@pytest.mark.parametrize("entry", POLISHES)
def test_rounds_steps_and_best(lib, entry):
    letter = ENTRIES[entry][4]
    refused(lib, entry, "rounds = 0 (1 .. 16)", rounds=0)
    refused(lib, entry, "rounds = 17 (1 .. 16)", rounds=17)
    refused(lib, entry, "null best needs %s == 1, got %s = 2" % (letter, letter), best=None, H=2)
    if "steps" in ENTRIES[entry][1]:
        refused(lib, entry, "steps = 0 (1 .. 8)", steps=0)
        refused(lib, entry, "steps = 9 (1 .. 8)", steps=9)
        refused(lib, entry, "rounds = 17 (1 .. 16)", rounds=17, steps=9)               # rounds before steps
        refused(lib, entry, "steps = 9 (1 .. 8)", steps=9, best=None, H=2)              # steps before the null best


@pytest.mark.parametrize("entry", GENERATORS)
def test_generators(lib, entry):
    max_h = lib.pats_epipolar_max_h()
    refused(lib, entry, "progressive = 2 must be 0 or 1", progressive=2)
    refused(lib, entry, "progressive = -1 must be 0 or 1", progressive=-1)
    if entry.startswith("pats_absolute"):               # four models per sample
        H = max_h // 4 + 1
        refused(lib, entry, "H = %d gives 4 H = %d models (<= max_h = %d)" % (H, 4 * H, max_h), H=H)
        refused(lib, entry, "H = %d gives 4 H = %d models (<= max_h = %d)" % (H, 4 * H, max_h), H=H, progressive=2)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_order_of_the_refusals(lib, entry):
    """A call that is wrong twice is refused for the reason that comes first: the required pointers in the entry's order, then the
    optional pointers' alignment, the segments, the model count, the confidence gate, the walk's lengths."""
    name, names, first, first_align, letter = ENTRIES[entry]
    max_h = lib.pats_epipolar_max_h()
    refused(lib, entry, "null %s" % first, **{first: None, "matches_r": None})
    refused(lib, entry, "%s must be %d-byte aligned" % (first, first_align), **{first: address(50) + first_align // 2, "matches_r": None})
    refused(lib, entry, "null matches_r", matches_r=None, models=None)
    refused(lib, entry, "null models", models=None, norm=address(50) + 2)
    refused(lib, entry, "norm must be 4-byte aligned", norm=address(50) + 2, pair_off=address(0) + 4)
    refused(lib, entry, "pair_off must be 8-byte aligned", pair_off=address(0) + 4, pairs=0)
    refused(lib, entry, "pairs = 0 (1 .. 2^31 - 1)", pairs=0, H=0)
    refused(lib, entry, "cap = -1 (0 .. 2^31 - 2)", cap=-1, H=0)
    refused(lib, entry, "pairs * stride = 2 * 11 exceeds cap = 20", **strided(stride=CAP // PAIRS + 1, H=max_h + 1))
    if entry in GATED:
        last = [n for n in names if n in ALIGN and n not in optional(entry)][-1]        # the last required pointer: before every optional one
        refused(lib, entry, "null %s" % last, **{last: None, "conf": address(50) + 2})
        refused(lib, entry, "null thr", thr=None, **{last: None})
        refused(lib, entry, "null inlier", inlier=None, conf=address(50) + 2)
        refused(lib, entry, "conf must be 4-byte aligned", conf=address(50) + 2, norm=address(51) + 2)
        refused(lib, entry, "H = 0 (1 .. max_h = %d)" % max_h, H=0, use_min_conf=1, conf=None)
        refused(lib, entry, "min_conf needs conf", use_min_conf=1, conf=None, min_conf=-1.0)
    if entry in SCORES:                                 # best is an output here: required, in its place between counts and best_count
        refused(lib, entry, "null best", best=None, conf=address(50) + 2)
        refused(lib, entry, "null best", best=None, best_count=None)
        refused(lib, entry, "null counts", counts=None, best=None)
        refused(lib, entry, "best must be 4-byte aligned", best=address(50) + 2, inlier=None)
    if entry in SCORES and "moments" in names:
        refused(lib, entry, "counts_in must be 8-byte aligned", **strided(counts_in=address(40) + 4, moments=address(50) + 4))
        refused(lib, entry, "moments must be 8-byte aligned", moments=address(50) + 4, pairs=0)
    if entry in POLISHES:
        refused(lib, entry, "counts_in must be 8-byte aligned", **strided(counts_in=address(40) + 4, best=address(50) + 2))
        refused(lib, entry, "best must be 4-byte aligned", best=address(50) + 2, pairs=0)
        refused(lib, entry, "min_conf = -1 must be a non-negative number", use_min_conf=1, min_conf=-1.0, rounds=0)
        refused(lib, entry, "rounds = 0 (1 .. 16)", rounds=0, best=None, H=2)
    if entry in GENERATORS:
        refused(lib, entry, "null pair_seed", pair_seed=None, models=None)
        refused(lib, entry, "sample_idx must be 4-byte aligned", sample_idx=address(50) + 2, pair_off=address(0) + 4)
        refused(lib, entry, "H = 0 (1 .. max_h = %d)" % max_h, H=0, progressive=2)
