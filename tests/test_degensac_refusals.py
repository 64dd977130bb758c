"""CPU-only: what the two C entries of the plane-and-parallax stage (csrc/plane_parallax.hip) refuse, word for word
(pats_last_error), and in which order - the method of tests/test_host_refusals_backend.py: the entries are called through ctypes with
made-up integer addresses, aligned, misaligned or null; they are not memory, so EVERY call here is one the host checks turn away
before anything touches a device.
    hypotheses  everything pats_epipolar_hypotheses7_by_pair_f32 refuses arrives first and in its wording (the two entries are called
                with the same wrong arguments and the messages compared); then parallax, Mh, models_h, best_h, thr, pool
    hand-over   its pointers in their order, the segments, Ha / Hb, the moments rule, the plane"""
import ctypes
import itertools

import pytest

PAIRS, CAP = 2, 20
SCALARS = {"stride": 0, "pairs": PAIRS, "cap": CAP, "H": 4, "Mh": 3, "Ha": 2, "Hb": 4, "parallax": 2.0, "progressive": 0,
           "workspace_bytes": 0}
NULLS = ("counts_in", "workspace", "stream")

HYP = ("pats_plane_parallax_hypotheses_by_pair_f32", "plane_parallax_hypotheses_by_pair",
       "matches_l matches_r pair_off stride counts_in pairs cap H pair_seed norm models_h Mh best_h thr parallax models sample_idx pool "
       "workspace workspace_bytes stream")
SEVEN = ("pats_epipolar_hypotheses7_by_pair_f32", "epipolar_hypotheses7_by_pair",
         "matches_l matches_r pair_off stride counts_in pairs cap H pair_seed norm progressive models sample_idx n_models workspace "
         "workspace_bytes stream")
SELECT = ("pats_plane_parallax_select_by_pair", "plane_parallax_select_by_pair",
          "matches_l matches_r pair_off stride counts_in pairs cap norm models_h Mh best_h thr models_a Ha best_a best_count_a inlier_a "
          "moments_a models_b Hb best_b best_count_b inlier_b moments_b model best_count inlier moments replaced overlap stream")

# what the 7-point entry checks, in its order: the pointers (name, alignment, may be null), then the scalars (wrong arguments, message)
SEVEN_POINTERS = [("matches_l", 8, False), ("matches_r", 8, False), ("pair_seed", 8, False), ("models", 4, False), ("norm", 4, True),
                  ("sample_idx", 4, True), ("pair_off", 8, True), ("counts_in", 8, True)]
SEVEN_AFTER = [({"pair_off": None}, "exactly one of pair_off (ragged segments) and counts_in (strided segments) must be given"),
               ({"pairs": 0}, "pairs = 0 (1 .. 2^31 - 1)"), ({"cap": -1}, "cap = -1 (0 .. 2^31 - 2)"),
               ({"pair_off": None, "counts_in": 0x7f0000100000, "stride": 0}, "stride = 0 must be at least 1"),
               ({"pair_off": None, "counts_in": 0x7f0000100000, "stride": 11}, "pairs * stride = 2 * 11 exceeds cap = 20"),
               ({"H": 0}, "H = 0 (1 .. max_h = %(max_h)d)")]
# what the new entry adds behind them, in its order
NEW_AFTER = [({"parallax": 0.5}, "parallax = 0.5 must be a finite number >= 1"), ({"parallax": float("nan")}, "parallax = nan must be a finite number >= 1"),
             ({"parallax": float("inf")}, "parallax = inf must be a finite number >= 1"), ({"Mh": 0}, "Mh = 0 (1 .. max_h = %(max_h)d)"),
             ({"models_h": None}, "null models_h"), ({"best_h": None}, "null best_h"), ({"thr": None}, "null thr"), ({"pool": None}, "null pool")]
ALL_NEW_WRONG = {"parallax": 0.5, "Mh": 0, "models_h": None, "best_h": None, "thr": None, "pool": None}

SELECT_POINTERS = [("matches_l", 8, False), ("matches_r", 8, False), ("models_a", 4, False), ("best_a", 4, False), ("best_count_a", 8, False),
                   ("inlier_a", 1, False), ("models_b", 4, False), ("best_b", 4, False), ("best_count_b", 8, False), ("inlier_b", 1, False),
                   ("model", 4, False), ("best_count", 8, False), ("inlier", 1, False), ("replaced", 1, False), ("overlap", 4, False),
                   ("norm", 4, True), ("pair_off", 8, True), ("counts_in", 8, True), ("moments_a", 8, True), ("moments_b", 8, True),
                   ("moments", 8, True)]
SELECT_AFTER = [({"pairs": 0}, "pairs = 0 (1 .. 2^31 - 1)"), ({"Ha": 0}, "Ha = 0 (1 .. max_h = %(max_h)d)"),
                ({"Hb": 0}, "Hb = 0 (1 .. max_h = %(max_h)d)"), ({"moments_a": None}, "moments needs moments_a and moments_b"),
                ({"Mh": 0}, "Mh = 0 (1 .. max_h = %(max_h)d)"), ({"models_h": None}, "null models_h"), ({"best_h": None}, "null best_h"),
                ({"thr": None}, "null thr")]


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


def call(lib, entry, **kw):
    """A well-formed ragged call of the entry with kw on top -> (rc, pats_last_error)."""
    names = entry[2].split()
    a = {n: SCALARS[n] if n in SCALARS else (None if n in NULLS else address(k)) for k, n in enumerate(names)}
    for n, v in kw.items():
        if n in a:                                      # an argument the entry does not have is not wrong in it
            a[n] = v
    rc = getattr(lib, entry[0])(*[a[n] for n in names])
    return rc, lib.pats_last_error().decode()


def refused(lib, entry, message, **kw):
    rc, said = call(lib, entry, **kw)
    assert rc == 1, "%s(%s) was not refused: %d" % (entry[0], kw, rc)
    assert said == "%s: %s" % (entry[1], message % {"max_h": lib.pats_epipolar_max_h()}), kw


def wrongs(pointer):
    name, align, may_be_null = pointer
    w = [] if may_be_null else [(None, "null %s" % name)]
    if align > 1:
        w.append((address(50) + align // 2, "%s must be %d-byte aligned" % (name, align)))
    return w


def test_the_new_symbols_are_in_the_built_library_and_the_tables_are_its_signatures(lib):
    assert lib.pats_plane_parallax_pool_max() == 8192 and 4 * lib.pats_plane_parallax_pool_max() <= 64 * 1024
    assert lib.pats_plane_parallax_hypotheses_workspace_bytes(3, 64) == 0
    assert lib.pats_abi_version() == 8                  # symbols were added: the version stays
    for entry in (HYP, SELECT):
        names, argtypes = entry[2].split(), getattr(lib, entry[0]).argtypes
        assert len(names) == len(argtypes) and len(set(names)) == len(names)
        for n, t in zip(names, argtypes):
            assert (n in SCALARS) == (t is not ctypes.c_void_p), (entry[0], n)


def test_every_sibling_refusal_arrives_first_and_in_the_siblings_wording(lib):
    """The same wrong argument into the 7-point entry and into the new one - which has every argument of its own wrong as well: the
    two messages differ by the entry's name alone."""
    cases = [({p[0]: v}, None) for p in SEVEN_POINTERS for v, _ in wrongs(p)] + SEVEN_AFTER
    assert len(cases) >= 18
    for kw, _ in cases:
        rc, said = call(lib, SEVEN, **kw)
        assert rc == 1 and said.startswith(SEVEN[1] + ": "), (kw, said)
        refused(lib, HYP, said[len(SEVEN[1]) + 2:].replace("%", "%%"), **dict(ALL_NEW_WRONG, **kw))
    for (pa, pb) in zip(SEVEN_POINTERS, SEVEN_POINTERS[1:]):          # and among themselves the siblings' order
        for (va, message), (vb, _) in itertools.product(wrongs(pa), wrongs(pb)):
            refused(lib, HYP, message, **{pa[0]: va, pb[0]: vb})
    for kw, message in SEVEN_AFTER:
        refused(lib, HYP, message, **kw)


def test_every_new_refusal_names_its_argument_and_keeps_its_place(lib):
    for kw, message in NEW_AFTER:
        refused(lib, HYP, message, **kw)
    for (ka, message), (kb, _) in zip(NEW_AFTER, NEW_AFTER[1:]):
        if not set(ka) & set(kb):
            refused(lib, HYP, message, **dict(ka, **kb))
    for name in ("models_h", "best_h", "thr", "pool"):
        refused(lib, HYP, "%s must be 4-byte aligned" % name, **{name: address(50) + 2})
    rc, said = call(lib, HYP, Mh=lib.pats_epipolar_max_h() + 1)
    assert rc == 1 and "Mh = %d" % (lib.pats_epipolar_max_h() + 1) in said
    rc, said = call(lib, HYP, H=lib.pats_epipolar_max_h() + 1)
    assert rc == 1 and said.startswith(HYP[1] + ": H = ")


def test_the_hand_over_checks_its_pointers_then_its_sizes_then_the_plane(lib):
    for pointer in SELECT_POINTERS:
        for value, message in wrongs(pointer):
            refused(lib, SELECT, message, **{pointer[0]: value})
    order = [p for p in SELECT_POINTERS if wrongs(p)]
    for a, b in zip(order, order[1:]):
        for (va, message), (vb, _) in itertools.product(wrongs(a), wrongs(b)):
            refused(lib, SELECT, message, **{a[0]: va, b[0]: vb})
    for kw, message in SELECT_AFTER:
        refused(lib, SELECT, message, **kw)
    for (ka, message), (kb, _) in zip(SELECT_AFTER, SELECT_AFTER[1:]):
        refused(lib, SELECT, message, **dict(ka, **kb))
    last = order[-1]
    for value, message in wrongs(last):
        for kw, _ in SELECT_AFTER:
            if last[0] not in kw:
                refused(lib, SELECT, message, **dict(kw, **{last[0]: value}))
    rc, said = call(lib, SELECT, moments=None, moments_a=None, moments_b=None, pairs=0)      # no moments at all is a valid form
    assert rc == 1 and said.endswith("pairs = 0 (1 .. 2^31 - 1)")
