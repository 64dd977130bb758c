"""CPU-only: the host side of ragged throughput batches - MixedCapacities, the slot order of pack_pairs, and the C-ABI's
refusal of bad pair tables before any launch (no GPU is touched: every call below fails its argument check)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("if_local", [True, False])
@pytest.mark.parametrize("shape", [(15, 20), (24, 32), (5, 6)])
def test_mixed_capacities_of_one_shape_equal_capacities(shape, if_local):
    from pats_amd import batch
    for kw in ({}, {"p_cap_per_pair": 100}, {"rows_cap": 77}):
        a = batch.Capacities(3, shape[0], shape[1], if_local=if_local, **kw)
        b = batch.MixedCapacities([shape] * 3, if_local=if_local, **kw)
        assert vars(a) and all(getattr(b, k) == v for k, v in vars(a).items()), (shape, kw)


def test_mixed_capacities_add_the_pairs_worst_cases():
    from pats_amd import batch, ops
    shapes = [(24, 32), (32, 24), (32, 32), (22, 32), (24, 32)]
    for if_local in (True, False):
        cap = batch.MixedCapacities(shapes, if_local=if_local)
        cm = [ops.max_chunks(h, w, 2 * w if if_local else 512) for h, w in shapes]
        assert cap.pairs == 5 and cap.h is None and cap.w is None
        assert cap.Cmax == max(cm)
        assert cap.rows_cap == sum(h * w + (c - 1) * w for (h, w), c in zip(shapes, cm))
        assert cap.P_cap == sum(int(1.25 * 16 * h * w) for h, w in shapes)
    assert batch.MixedCapacities(shapes, p_cap_per_pair=10).P_cap == 50
    assert batch.MixedCapacities(shapes, rows_cap=123).rows_cap == 123


def test_slot_order_is_stable_and_round_trips():
    from pats_amd import batch
    shapes = [(24, 32), (15, 20), (32, 24), (15, 20), (24, 32), (20, 15), (24, 32)]
    caller_of = batch.slot_order(shapes)
    assert sorted(caller_of) == list(range(len(shapes)))
    slotted = [shapes[i] for i in caller_of]
    assert slotted == sorted(shapes)                                   # every shape group is contiguous
    for sh in set(shapes):                                             # equal shapes keep the caller's order
        members = [i for i in caller_of if shapes[i] == sh]
        assert members == sorted(members)
    slot_of = [0] * len(shapes)
    for s, i in enumerate(caller_of):
        slot_of[i] = s
    assert [caller_of[slot_of[i]] for i in range(len(shapes))] == list(range(len(shapes)))


def _table(shapes, cell_base=None, pairs=None):
    from pats_amd import _lib
    sh = np.ascontiguousarray(np.array(shapes, np.int32).reshape(-1, 2))
    n = sh[:, 0].astype(np.int64) * sh[:, 1]
    cb = np.ascontiguousarray(np.concatenate([[0], np.cumsum(n)]).astype(np.int64) if cell_base is None
                              else np.array(cell_base, np.int64))
    fake = 0x1000                    # device arrays: never dereferenced - the host copies fail the check first
    t = _lib.PairTable(len(shapes) if pairs is None else pairs, sh.ctypes.data, cb.ctypes.data, fake, fake, fake)
    t._keep = (sh, cb)
    return t


def test_ragged_entry_points_reject_bad_tables_without_gpu(lib):
    bad = [None, _table([(5, 6)], pairs=0), _table([(5, 6), (0, 4)]), _table([(5, 6), (3, -1)]),
           _table([(5, 6), (4, 4)], cell_base=[0, 30, 29]), _table([(5, 6), (4, 4)], cell_base=[1, 31, 47]),
           _table([(200, 60)])]
    fake = ctypes.c_void_p(0x1000)
    for t in bad:
        ref = None if t is None else ctypes.byref(t)
        assert lib.pats_chunk_rows_ragged(ref, fake, 1, 2, 100, *([fake] * 14), 1 << 20, None) == 1
        assert b"chunk_rows_ragged" in lib.pats_last_error()
        assert lib.pats_compute_imgs_bounds_ragged_f32(ref, *([fake] * 10), None) == 1
        assert lib.pats_left_crops_ragged_f32(ref, fake, fake, 10, fake, fake, None) == 1
        assert lib.pats_tensor_resize_hwc_ragged_f32(ref, fake, 128, fake, 10, fake, fake, None, None) == 1
        assert lib.pats_merge_patches_ragged(ref, 1, 2, 100, *([fake] * 8), 1, fake, fake, 1 << 20, None) == 1
        ps1 = (ctypes.c_int * 3)(2, 48, 48)
        assert lib.pats_get_result_chunks_ragged_f32(ref, 2, fake, fake, 100, fake, fake, fake, ps1, fake, fake, fake, fake, fake,
                                                     1000, fake, fake, 1 << 20, None) == 1
    # a valid table, Cmax outside [1, max h + 1]
    good = ctypes.byref(_table([(5, 6), (8, 10)]))
    for cmax in (0, 10):
        assert lib.pats_chunk_rows_ragged(good, fake, 1, cmax, 100, *([fake] * 14), 1 << 20, None) == 1
        assert b"Cmax" in lib.pats_last_error()
        assert lib.pats_merge_patches_ragged(good, 1, cmax, 100, *([fake] * 8), 1, fake, fake, 1 << 20, None) == 1
    # the row-pair hand-over needs row_pair (status may be null: offsets only)
    assert lib.pats_matches_by_row_pair_summary_f32(fake, fake, fake, fake, None, fake, 2, 3, fake, fake, fake, None, fake, fake,
                                                    1 << 20, None) == 1
    assert lib.pats_merge_ragged_workspace_bytes(0) == 0 and lib.pats_merge_ragged_workspace_bytes(10) >= 10 * 144 * 4
