"""CPU-only: the host side of the hand-over (csrc/merge.hip) - what its workspace queries answer, value for value, and what the
entries whose checks are shared refuse, word for word (pats_last_error) and in which order: the four pats_get_result_chunks*, the
two *_summary_conf_f32 regroup entries, pats_refine_scatter_conf_f32 and the three merges over a row table.  The method of
test_gnn_host.py: the entries are called through ctypes with made-up aligned addresses, which are not memory, so EVERY call here
carries at least one fault that a host check answers (or a zero count that returns at once) before anything touches a device.  The
real memory is the host side of a pats_pair_table_t and the patch_size triples, which the checks read."""
import ctypes

import numpy as np
import pytest

OK, INVALID = 0, 1
BIG = 1 << 30                                   # a workspace size no query here exceeds


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


ODD = address(90) + 2                           # on no 4-byte boundary


def table(shapes=((6, 7), (5, 9))):
    """pats_pair_table_t with real host arrays (the checks read them) and made-up device arrays; largest h = 6."""
    from pats_amd import _lib
    sh = np.ascontiguousarray(np.array(shapes, np.int32))
    cb = np.concatenate([[0], np.cumsum(sh[:, 0].astype(np.int64) * sh[:, 1])]).astype(np.int64)
    t = _lib.PairTable(len(shapes), sh.ctypes.data, cb.ctypes.data, address(200), address(201), address(202))
    t._keep = (sh, cb)
    return t


# ---- the sizes ------------------------------------------------------------------------------------------------------------------
def scan_bytes(n):
    """offsets [n] and tile bases [ceil(n / 2048)], each rounded up to four int32"""
    tiles = (n + 2047) // 2048
    return (((n + 3) & ~3) + ((tiles + 3) & ~3)) * 4


def merge_bytes(B, H, W, bn):
    if B < 0 or H < 32 or W < 32 or bn < 1:
        return 0
    NP, per = bn * (H // 32) * (W // 32), (H // 32) * 4 * (W // 32) * 4 * 9
    return scan_bytes(NP) + (((NP + 3) & ~3) + ((B + 4) & ~3) + bn * per) * 4 + 64


@pytest.mark.parametrize("args", [(0, 32, 32, 1), (37, 192, 224, 1), (113, 480, 640, 2), (5000, 1024, 1344, 3), (-1, 192, 224, 1),
                                  (10, 31, 224, 1), (10, 192, 16, 1), (10, 192, 224, 0)])
def test_merge_workspace_bytes(lib, args):
    assert lib.pats_merge_workspace_bytes(*args) == merge_bytes(*args)
    assert (merge_bytes(*args) == 0) == (args[0] < 0 or args[1] < 32 or args[2] < 32 or args[3] < 1)


@pytest.mark.parametrize("args, size", [((1, 32, 32), 144 * 4 + 64), ((3, 192, 224), 3 * 42 * 144 * 4 + 64), ((6, 480, 640), 6 * 300 * 144 * 4 + 64),
                                        ((0, 192, 224), 0), ((3, 31, 224), 0), ((3, 192, 31), 0)])
def test_merge_batch_workspace_bytes(lib, args, size):
    assert lib.pats_merge_batch_workspace_bytes(*args) == size


@pytest.mark.parametrize("cells, size", [(1, 640), (87, 87 * 576 + 64), (1 << 20, (1 << 20) * 576 + 64), (0, 0), (-5, 0)])
def test_merge_ragged_workspace_bytes(lib, cells, size):
    assert lib.pats_merge_ragged_workspace_bytes(cells) == size


@pytest.mark.parametrize("n", [0, 1, 144, 2048, 2049, 16384, 16385, 144 * 14564, -1])
def test_compact_workspace_bytes(lib, n):
    assert lib.pats_compact_workspace_bytes(n) == (0 if n < 0 else scan_bytes(n) + 64)


@pytest.mark.parametrize("args", [(0, 0, 0), (42, 10, 2304), (6 * 300, 1821, 2304), (1 << 20, 7, 2304), (-1, 10, 2304), (42, -1, 2304),
                                  (42, 10, -1)])
def test_get_result_workspace_bytes(lib, args):
    c0, r1, c1 = args
    want = 0 if min(args) < 0 else scan_bytes(c0) + scan_bytes(r1 * c1) + ((r1 + 4) & ~3) * 4 + 64
    assert lib.pats_get_result_workspace_bytes(*args) == want


@pytest.mark.parametrize("args, size", [((1, 1), 24), ((7, 33), 7 * 33 * 24), ((3, 100000), 7200000), ((0, 5), 0), ((5, 0), 0), ((-1, 5), 0)])
def test_matches_by_pair_workspace_bytes(lib, args, size):
    assert lib.pats_matches_by_pair_workspace_bytes(*args) == size


# ---- the entries: name -> (arguments in the order of the C signature, the scalars among them, the checks in the order they are made) --
# a check: (what is wrong, return code, message or None).  Arguments that are not scalars are made-up addresses; "tab", "patch_size0"
# and "patch_size1" are real host memory.
def chunks_entry(who, ragged, conf):
    names = ("tab Cmax" if ragged else "Cmax pairs") + " masks if_nomatching16 rows_cap pts_new pts16 scales" + (" conf16" if conf else "") + \
        ("" if ragged else " patch_size0") + " patch_size1 left_choice0 left_choice1 matches_l matches_r" + \
        (" match_conf" if conf else "") + " match_row capacity count workspace workspace_bytes stream"
    checks = []
    if conf:
        checks += [({"conf16": None}, INVALID, who + ": null conf16 / match_conf"),
                   ({"match_conf": ODD}, INVALID, who + ": conf16 / match_conf must be 4-byte aligned")]
    if ragged:
        checks += [({"tab": None}, INVALID, who + ": null or empty pair table"), ({"Cmax": 8}, INVALID, who + ": bad shape")]
    else:
        checks += [({"Cmax": 0}, INVALID, who + ": bad shape"), ({"pairs": 1 << 31}, INVALID, who + ": batch too large")]
    checks += [({"rows_cap": -1}, INVALID, "get_result: bad shape"), ({"count": None}, INVALID, "get_result: null count"),
               ({"patch_size1": "empty"}, INVALID, "get_result: bad patch_size"),
               ({"workspace_bytes": 16}, INVALID, "get_result: workspace too small"), ({"masks": None}, INVALID, "get_result: null pointer")]
    return names, {"Cmax": 2, "pairs": 3, "rows_cap": 10, "capacity": 100, "workspace_bytes": BIG, "stream": None}, checks


def regroup_entry(who, by_row_pair):
    rows = "row_pair" if by_row_pair else "row_cell"
    names = "matches_l matches_r match_conf match_row M_dev %s chunk_base Cmax pairs%s out_l out_r out_conf pair_off P_dev status " \
            "workspace workspace_bytes stream" % (rows, "" if by_row_pair else " N")
    checks = [({"match_conf": None}, INVALID, who + ": null match_conf / out_conf"),
              ({"out_conf": ODD}, INVALID, who + ": match_conf / out_conf must be 4-byte aligned"),
              ({rows: None}, INVALID, "%s: null %s" % (who, rows)),
              ({"Cmax": 0}, INVALID, "matches_by_pair: bad shape"), ({"matches_l": None}, INVALID, "matches_by_pair: null pointer"),
              ({"workspace_bytes": 16}, INVALID, "matches_by_pair: workspace too small")]
    return names, {"Cmax": 2, "pairs": 3, "N": 42, "workspace_bytes": BIG, "stream": None}, checks


def merge_entry(who, head, scalars, first_checks, a_pointer):
    names = head + " trust_score if_nomatching1_L2 scores_back zero_scores_back out workspace workspace_bytes stream"
    checks = first_checks + [({a_pointer: None}, INVALID, who + ": null pointer"), ({"workspace_bytes": 16}, INVALID, who + ": workspace too small")]
    # merge_new = 0: the workspace is needed, so its check is reached
    return names, dict({"merge_new": 0, "Cmax": 2, "zero_scores_back": 1, "workspace_bytes": BIG, "stream": None}, **scalars), checks


ENTRIES = {
    "pats_get_result_chunks_f32": chunks_entry("get_result_chunks", False, False),
    "pats_get_result_chunks_ragged_f32": chunks_entry("get_result_chunks_ragged", True, False),
    "pats_get_result_chunks_conf_f32": chunks_entry("get_result_chunks_conf", False, True),
    "pats_get_result_chunks_ragged_conf_f32": chunks_entry("get_result_chunks_ragged_conf", True, True),
    "pats_matches_by_pair_summary_conf_f32": regroup_entry("matches_by_pair_summary_conf", False),
    "pats_matches_by_row_pair_summary_conf_f32": regroup_entry("matches_by_row_pair_summary_conf", True),
    "pats_refine_scatter_conf_f32": (
        "if_nomatching pts mkpts1_f label label_stride conf B P if_nomatching16 pts16 conf16 workspace workspace_bytes stream",
        {"label_stride": 1, "B": 4, "P": 5, "workspace_bytes": BIG, "stream": None},
        [({"B": -1}, INVALID, "refine_scatter_conf: bad shape"), ({"B": 0}, OK, None),
         ({"conf16": None}, INVALID, "refine_scatter_conf: null conf / conf16"),
         ({"conf": ODD}, INVALID, "refine_scatter_conf: conf / conf16 must be 4-byte aligned"),
         ({"if_nomatching": None}, INVALID, "refine_scatter: null pointer"),
         ({"workspace_bytes": 16}, INVALID, "refine_scatter: workspace too small")]),
    "pats_merge_patches_batch": merge_entry(
        "merge_patches_batch", "merge_new Cmax pairs H W rows_cap chunk_base row_cell row_slot row_forced",
        {"pairs": 3, "H": 192, "W": 224, "rows_cap": 50},
        [({"H": 31}, INVALID, "merge_patches_batch: bad shape"), ({"pairs": 0}, OK, None)], "out"),
    "pats_merge_patches_chunks": merge_entry(
        "merge_patches_chunks", "merge_new Cmax c_lo c_hi pairs H W row_origin rows_local chunk_base row_cell row_slot row_forced",
        {"c_lo": 0, "c_hi": 1, "pairs": 3, "H": 192, "W": 224, "row_origin": 0, "rows_local": 20},
        [({"c_hi": 3}, INVALID, "merge_patches_chunks: bad shape"), ({"rows_local": 0}, OK, None)], "row_slot"),
    "pats_merge_patches_ragged": merge_entry(
        "merge_patches_ragged", "tab merge_new Cmax rows_cap chunk_base row_cell row_pair row_slot row_forced", {"rows_cap": 50},
        [({"tab": None}, INVALID, "merge_patches_ragged: null or empty pair table"), ({"Cmax": 8}, INVALID, "merge_patches_ragged: bad shape"),
         ({"rows_cap": 0}, OK, None)], "row_pair"),
}


def answered(lib, entry, rc_want, message, **wrong):
    """The host checks answer the call with `wrong` in it: this return code and - where one is given - exactly this message."""
    assert wrong, "a call without a fault would reach the launches"
    names, scalars, _ = ENTRIES[entry]
    names = names.split()
    a = {n: scalars[n] if n in scalars else address(k) for k, n in enumerate(names)}
    held = [table(), (ctypes.c_int * 3)(32, 6, 7), (ctypes.c_int * 3)(2, 48, 48), (ctypes.c_int * 3)(2, 0, 48)]
    a.update({n: v for n, v in zip(("tab", "patch_size0", "patch_size1"), (ctypes.byref(held[0]), held[1], held[2])) if n in a})
    for n, v in wrong.items():
        assert n in a, n
        a[n] = held[3] if v == "empty" else v
    rc = getattr(lib, entry)(*[a[n] for n in names])
    del held
    assert rc == rc_want, "%s(%s): %d" % (entry, wrong, rc)
    if message is not None:
        assert lib.pats_last_error().decode() == message, (entry, wrong)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals(lib, entry):
    for wrong, rc, message in ENTRIES[entry][2]:
        answered(lib, entry, rc, message, **wrong)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_earlier_check_wins(lib, entry):
    checks = ENTRIES[entry][2]
    for i, (first, rc, message) in enumerate(checks):
        for later, _, _ in checks[i + 1:]:
            if set(first) & set(later):
                continue                                # two faults of one argument
            answered(lib, entry, rc, message, **dict(later, **first))


def test_the_conf_pair_is_checked_as_a_pair(lib):
    """either pointer null, either pointer misaligned - the same two messages; refine_scatter's conf may be null without problems
    (P = 0) and is then not what the call is refused for"""
    for entry, a, b in (("pats_get_result_chunks_conf_f32", "conf16", "match_conf"),
                        ("pats_get_result_chunks_ragged_conf_f32", "conf16", "match_conf"),
                        ("pats_matches_by_pair_summary_conf_f32", "match_conf", "out_conf"),
                        ("pats_matches_by_row_pair_summary_conf_f32", "match_conf", "out_conf"),
                        ("pats_refine_scatter_conf_f32", "conf", "conf16")):
        who = entry[len("pats_"):-len("_f32")]
        for name in (a, b):
            answered(lib, entry, INVALID, "%s: null %s / %s" % (who, a, b), **{name: None})
            answered(lib, entry, INVALID, "%s: %s / %s must be 4-byte aligned" % (who, a, b), **{name: ODD})
        answered(lib, entry, INVALID, "%s: null %s / %s" % (who, a, b), **{a: None, b: ODD})
    answered(lib, "pats_refine_scatter_conf_f32", INVALID, "refine_scatter: null pointer", conf=None, P=0, if_nomatching=None)
    answered(lib, "pats_refine_scatter_conf_f32", INVALID, "refine_scatter_conf: null conf / conf16", conf16=None, P=0)


def test_merge_new_over_a_table_needs_no_workspace(lib):
    """merge_new = 1: the workspace check is not made - a null workspace beside a null pointer is refused for the pointer"""
    for entry, who, ptr in (("pats_merge_patches_batch", "merge_patches_batch", "out"),
                            ("pats_merge_patches_chunks", "merge_patches_chunks", "row_slot"),
                            ("pats_merge_patches_ragged", "merge_patches_ragged", "row_pair")):
        answered(lib, entry, INVALID, who + ": null pointer", merge_new=1, workspace=None, workspace_bytes=0, **{ptr: None})
        answered(lib, entry, INVALID, who + ": workspace too small", merge_new=0, workspace=None)
    answered(lib, "pats_merge_patches_chunks", INVALID, "merge_patches_chunks: bad shape", pairs=65536)
    answered(lib, "pats_merge_patches_chunks", OK, None, c_lo=1, c_hi=1, out=None)
