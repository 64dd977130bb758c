"""CPU-only: what the C entries of the per-pair back end - the poses, the E-or-H choice, the triangulation, the pose and match
errors, the refits, the lift, the selections, the preparation - refuse, word for word (pats_last_error), and in which order.  The
method of test_host_refusals.py: the entries are called through ctypes with made-up integer addresses - aligned, misaligned or
null; they are not memory, so EVERY call here is one the host checks turn away before anything touches a device."""
import ctypes
import itertools

import pytest

PAIRS, CAP = 2, 20
# what an argument that is not a device pointer gets in a well-formed call; counts_in (the strided form), the workspace and the stream
# are null, a name that is neither here nor there is a pointer and gets a made-up address
SCALARS = {"stride": 0, "pairs": PAIRS, "cap": CAP, "H": 2, "swapped": 0, "workspace_bytes": 0, "min_baseline": 0.0, "min_matches": 0,
           "min_gt_t": 0.0, "n_err": 4, "n_thr": 1, "interp": 0, "use_max_jump": 0, "max_jump": 0.0, "K": 4, "use_min_conf": 0, "min_conf": 0.0,
           "side": 0, "cell": 8, "grid0": 2, "grid1": 2, "occl_rel": 0.5, "B": 0, "n_img": 1, "left_elems": 0, "right_elems": 0, "dtype": 0}
NULLS = ("counts_in", "workspace", "stream", "edges")
HOST_THRESHOLDS = (ctypes.c_double * 2)(1.0, 2.0)       # thr and thresholds are host arrays the entry reads: real memory
HOST = {"thr": HOST_THRESHOLDS, "thresholds": HOST_THRESHOLDS}

SEGMENTS = "pairs = 0 (1 .. 2^31 - 1)"
SWAPPED = "swapped = 2 must be 0 or 1"
SOURCE = "the refit needs moments, or models and best (the winning model)"
MIN_CONF = "min_conf = -1 must be a non-negative number"

# entry -> (the name its messages carry,
#           its arguments in the order of the C signature,
#           its pointers in the order the entry checks them: (name, alignment, may be null),
#           what it checks behind the pointers, in its order: (arguments that are wrong in one way, the message))
ENTRIES = {
    "pats_epipolar_pose_by_pair_f64": (
        "epipolar_pose_by_pair",
        "matches_l matches_r inlier pair_off stride counts_in pairs cap best_count moments models H best norm swapped E R t "
        "front_counts choice front_count front e_refit workspace workspace_bytes stream",
        [("matches_l", 8, False), ("matches_r", 8, False), ("inlier", 1, False), ("best_count", 8, False), ("E", 8, False),
         ("R", 8, False), ("t", 8, False), ("front_counts", 4, False), ("choice", 4, False), ("front_count", 8, False),
         ("moments", 8, True), ("models", 4, True), ("best", 4, True), ("norm", 4, True), ("pair_off", 8, True), ("counts_in", 8, True),
         ("e_refit", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"swapped": 2}, SWAPPED), ({"moments": None, "best": None}, SOURCE)]),
    "pats_homography_pose_by_pair_f64": (
        "homography_pose_by_pair",
        "matches_l matches_r inlier pair_off stride counts_in pairs cap best_count moments models H best norm thr swapped min_baseline "
        "E R t n baseline vis sup choice status front_count cand_R cand_t cand_n front workspace workspace_bytes stream",
        [("matches_l", 8, False), ("matches_r", 8, False), ("inlier", 1, False), ("best_count", 8, False), ("E", 8, False),
         ("R", 8, False), ("t", 8, False), ("n", 8, False), ("baseline", 8, False), ("vis", 4, False), ("sup", 4, False),
         ("choice", 4, False), ("status", 4, False), ("front_count", 8, False), ("moments", 8, True), ("models", 4, True),
         ("best", 4, True), ("norm", 4, True), ("thr", 4, True), ("pair_off", 8, True), ("counts_in", 8, True), ("cand_R", 8, True),
         ("cand_t", 8, True), ("cand_n", 8, True)],
        [({"cand_t": None}, "cand_R, cand_t and cand_n must be given together"), ({"pairs": 0}, SEGMENTS), ({"swapped": 2}, SWAPPED),
         ({"moments": None, "best": None}, SOURCE), ({"min_baseline": -1.0}, "min_baseline = -1 must be a number >= 0")]),
    "pats_pose_select_by_pair": (
        "pose_select_by_pair",
        "pair_off stride counts_in pairs cap R_e t_e E_e front_count_e front_e best_count_e inlier_e R_h t_h E_h front_count_h front_h "
        "status_h best_count_h inlier_h ratio R t E front_count branch inlier_sel front_sel workspace workspace_bytes stream",
        [("R_e", 8, False), ("t_e", 8, False), ("E_e", 8, False), ("front_count_e", 8, False), ("best_count_e", 8, False),
         ("inlier_e", 1, False), ("R_h", 8, False), ("t_h", 8, False), ("E_h", 8, False), ("front_count_h", 8, False),
         ("status_h", 4, False), ("best_count_h", 8, False), ("inlier_h", 1, False), ("ratio", 4, False), ("R", 8, False),
         ("t", 8, False), ("E", 8, False), ("front_count", 8, False), ("branch", 4, False), ("inlier_sel", 1, False),
         ("pair_off", 8, True), ("counts_in", 8, True)],
        [({"front_e": None}, "front_sel needs front_e and front_h"), ({"pairs": 0}, SEGMENTS)]),
    "pats_epipolar_triangulate_by_pair_f64": (
        "epipolar_triangulate_by_pair",
        "matches_l matches_r pair_off stride counts_in pairs cap mask norm R t swapped max_reproj max_cos points depths reproj "
        "cos_parallax valid tri_count reproj_sum workspace workspace_bytes stream",
        [("matches_l", 8, False), ("matches_r", 8, False), ("mask", 1, False), ("R", 8, False), ("t", 8, False), ("points", 4, False),
         ("valid", 1, False), ("tri_count", 8, False), ("reproj_sum", 8, False), ("norm", 4, True), ("max_reproj", 4, True),
         ("max_cos", 4, True), ("depths", 4, True), ("reproj", 4, True), ("cos_parallax", 4, True), ("pair_off", 8, True),
         ("counts_in", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"swapped": 2}, SWAPPED)]),
    "pats_pose_error_by_pair_f64": (
        "pose_error_by_pair",
        "R t T1 T0 counts pairs min_matches min_gt_t err_R err_t err status stream",
        [("R", 8, False), ("t", 8, False), ("T1", 8, False), ("err_R", 8, False), ("err_t", 8, False), ("err", 8, False),
         ("status", 4, False), ("T0", 8, True), ("counts", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"min_matches": -1}, "min_matches = -1 must not be negative"),
         ({"min_gt_t": -1.0}, "min_gt_t = -1 must be a non-negative number")]),
    "pats_pose_auc_f64": (
        "pose_auc",
        "errors n_err thresholds n_thr auc below sorted stream",
        [("errors", 8, False), ("thresholds", 1, False), ("auc", 8, False), ("below", 8, False), ("sorted", 8, True)],
        [({"n_err": -1}, "n = -1 (0 .. max_n = 16384)"), ({"n_thr": 0}, "n_thr = 0 (1 .. 8)"),
         ({"thresholds": (ctypes.c_double * 1)(0.0)}, "thresholds[0] = 0 must be finite and positive")]),
    "pats_homography_refit_by_pair_f64": (
        "homography_refit_by_pair",
        "best_count moments models H best norm pairs swapped H_out H_px eig workspace workspace_bytes stream",
        [("best_count", 8, False), ("H_out", 8, False), ("eig", 8, False), ("moments", 8, True), ("models", 4, True), ("best", 4, True),
         ("norm", 4, True), ("H_px", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"swapped": 2}, SWAPPED), ({"moments": None, "best": None}, SOURCE)]),
    "pats_fundamental_refit_by_pair_f64": (
        "fundamental_refit_by_pair",
        "best_count moments models H best norm pairs swapped F F_px eig sigma f_refit workspace workspace_bytes stream",
        [("best_count", 8, False), ("F", 8, False), ("eig", 8, False), ("sigma", 8, False), ("moments", 8, True), ("models", 4, True),
         ("best", 4, True), ("norm", 4, True), ("F_px", 8, True), ("f_refit", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"swapped": 2}, SWAPPED), ({"moments": None, "best": None}, SOURCE)]),
    "pats_lift_by_pair_f32": (
        "lift_by_pair",
        "matches pair_off stride counts_in pairs cap norm depth_table max_depth interp use_max_jump max_jump points valid lift_count stream",
        [("matches", 8, False), ("depth_table", 8, False), ("points", 4, False), ("valid", 1, False), ("lift_count", 8, False),
         ("norm", 4, True), ("max_depth", 4, True), ("pair_off", 8, True), ("counts_in", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"interp": 2}, "interp = 2 must be 0 (nearest) or 1 (bilinear)"),
         ({"use_max_jump": 2}, "use_max_jump = 2 must be 0 or 1")]),
    "pats_topk_by_pair_f32": (
        "topk_by_pair",
        "matches_l matches_r conf pair_off pairs cap K use_min_conf min_conf top_l top_r top_conf top_idx top_count workspace "
        "workspace_bytes stream",
        [("matches_l", 8, False), ("matches_r", 8, False), ("conf", 4, False), ("pair_off", 8, False), ("top_l", 8, False),
         ("top_r", 8, False), ("top_conf", 4, False), ("top_idx", 4, False), ("top_count", 8, False)],
        [({"pairs": 0}, SEGMENTS), ({"cap": -1}, "cap = -1 (0 .. 2^31 - 2: top_idx is int32)"), ({"K": 0}, "K = 0 (1 .. max_k = %(max_k)d)"),
         ({"use_min_conf": 1, "min_conf": -1.0}, MIN_CONF)]),
    # occupied is the one pointer of the back end that is checked behind scalars: the selections' shared checks come first
    "pats_topk_spread_by_pair_f32": (
        "topk_spread_by_pair",
        "matches_l matches_r conf pair_off pairs cap K use_min_conf min_conf side cell grid0 grid1 top_l top_r top_conf top_idx top_count "
        "occupied workspace workspace_bytes stream",
        [("matches_l", 8, False), ("matches_r", 8, False), ("conf", 4, False), ("pair_off", 8, False), ("top_l", 8, False),
         ("top_r", 8, False), ("top_conf", 4, False), ("top_idx", 4, False), ("top_count", 8, False)],
        [({"pairs": 0}, SEGMENTS), ({"cap": -1}, "cap = -1 (0 .. 2^31 - 2: top_idx is int32)"), ({"K": 0}, "K = 0 (1 .. max_k = %(max_k)d)"),
         ({"use_min_conf": 1, "min_conf": -1.0}, MIN_CONF), ({"occupied": None}, "null occupied"),
         ({"occupied": 0x7f00000f0004}, "occupied must be 8-byte aligned"), ({"side": 2}, "side = 2 (0 = matches_l, 1 = matches_r)"),
         ({"cell": 0}, "cell = 0 (1 .. 65536 pixels)")]),
    "pats_match_error_by_pair_f64": (
        "match_error_by_pair",
        "points matches_r conf pair_off stride counts_in pairs cap norm T1 T0 swapped depth_r_table occl_rel size_r use_min_conf min_conf "
        "thr n_thr edges B mask err status tally correct err_sum sweep confusion stream",
        [("points", 4, False), ("matches_r", 8, False), ("T1", 8, False), ("err", 8, False), ("status", 1, False), ("tally", 8, False),
         ("correct", 8, False), ("err_sum", 8, False), ("thr", 1, False), ("conf", 4, True), ("norm", 4, True), ("pair_off", 8, True),
         ("counts_in", 8, True), ("T0", 8, True), ("depth_r_table", 8, True), ("size_r", 4, True), ("mask", 1, True), ("sweep", 8, True),
         ("confusion", 8, True)],
        [({"pairs": 0}, SEGMENTS), ({"use_min_conf": 1, "conf": None}, "min_conf needs conf"), ({"swapped": 2}, SWAPPED),
         ({"occl_rel": 0.0}, "occl_rel = 0 must be finite and positive"), ({"n_thr": 0}, "n_thr = 0 (1 .. 8)")]),
    "pats_prepare_images_u8": (
        "prepare_images",
        "images_host images n_img left left_elems right right_elems dtype stream",
        [("images_host", 1, False), ("images", 8, False), ("left", 16, False), ("right", 16, False)],
        [({"dtype": 99}, "unknown output dtype 99"), ({"n_img": 0}, "n_img = 0 (1 .. 65535)"), ({"left_elems": -1}, "negative store size")]),
}


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


def arguments(entry, **kw):
    """A well-formed ragged call of the entry with kw on top."""
    names = ENTRIES[entry][1].split()
    a = {}
    for k, n in enumerate(names):
        a[n] = SCALARS[n] if n in SCALARS else (None if n in NULLS else HOST[n] if n in HOST else address(k))
    for n, v in kw.items():
        assert n in a, n
        a[n] = v
    return [ctypes.cast(a[n], ctypes.c_void_p) if isinstance(a[n], ctypes.Array) else a[n] for n in names]


def refused(lib, entry, message, **kw):
    """The call is turned away (PATS_ERR_INVALID = 1) with exactly this message behind the entry's name."""
    rc = getattr(lib, entry)(*arguments(entry, **kw))
    assert rc == 1, "%s(%s) was not refused: %d" % (entry, kw, rc)
    message = message % {"max_k": lib.pats_topk_by_pair_max_k()}
    assert lib.pats_last_error().decode() == "%s: %s" % (ENTRIES[entry][0], message), kw


def wrongs(pointer):
    """The ways this pointer can be wrong, each as (its value, the message): null where it is required, misaligned where that exists."""
    name, align, may_be_null = pointer
    w = []
    if not may_be_null:
        w.append((None, "null %s" % name))
    if align > 1:
        w.append((address(50) + align // 2, "%s must be %d-byte aligned" % (name, align)))
    return w


def test_the_table_names_every_pointer_argument(lib):
    """The signatures above are the library's: as many arguments as its argtypes, and a pointer where the table checks one."""
    for entry, (_, names, pointers, _) in ENTRIES.items():
        names = names.split()
        argtypes = getattr(lib, entry).argtypes
        assert len(names) == len(argtypes), entry
        assert len(set(names)) == len(names), entry
        for name, _, _ in pointers:
            assert argtypes[names.index(name)] is ctypes.c_void_p, (entry, name)
        for n, t in zip(names, argtypes):
            assert (n in SCALARS) == (t is not ctypes.c_void_p), (entry, n)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_pointer(lib, entry):
    for pointer in ENTRIES[entry][2]:
        for value, message in wrongs(pointer):
            refused(lib, entry, message, **{pointer[0]: value})


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_earlier_pointer_wins(lib, entry):
    """Two neighbours of the entry's order wrong at once, in every way each can be: the earlier one's message.  A pointer that
    cannot be wrong (an optional byte mask) is no neighbour."""
    order = [p for p in ENTRIES[entry][2] if wrongs(p)]
    assert len(order) >= 2
    for a, b in zip(order, order[1:]):
        for (va, message), (vb, _) in itertools.product(wrongs(a), wrongs(b)):
            refused(lib, entry, message, **{a[0]: va, b[0]: vb})


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_pointers_come_first(lib, entry):
    """What the entry checks behind its pointers - the segments, the scalars - is refused in its own words and order, and loses
    against the LAST pointer of the order, so against every pointer."""
    _, _, pointers, after = ENTRIES[entry]
    for kw, message in after:
        refused(lib, entry, message, **kw)
    last = [p for p in pointers if wrongs(p)][-1]
    for value, message in wrongs(last):
        for kw, _ in after:
            if last[0] not in kw:
                refused(lib, entry, message, **dict(kw, **{last[0]: value}))
    for (ka, message), (kb, _) in zip(after, after[1:]):
        if not set(ka) & set(kb):
            refused(lib, entry, message, **dict(ka, **kb))
