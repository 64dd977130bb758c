"""-m gpu: the forms of one throughput stage give the same bits.  ops.third_level, ops.merge_patches_batch and the two
Compute_imgs functions each build ONE argument list and pick the C entry from the form (device count or not, confidence or
not, caller's outputs or fresh ones, uniform or ragged table); the mixed-batch and confidence tests hold whole steps to each
other, these hold the forms of a single call that no step compares."""
import pytest
import torch

from pats_amd import synth
from test_batch_gpu import cu
from test_confidence_gpu import SENTINEL, _small_batch, inputs, run, same_bits  # noqa: F401  (inputs: the 67-problem fixture)
from test_crop_formats_gpu import cell_inputs

pytestmark = pytest.mark.gpu

P_CAP, COUNT = 5, 3
FLAG = 0x5A             # prefill of a caller's if_matching1 bytes: neither 0 nor 1


@pytest.fixture(scope="module")
def ops():
    from pats_amd import ops
    return ops


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_third_level_forms_agree_on_the_counted_problems(ops, inputs, dt):
    inp = (inputs[0][:P_CAP].to(dt), inputs[1][:P_CAP].to(dt)) + tuple(t[:P_CAP] for t in inputs[2:])
    cnt = torch.tensor([COUNT], dtype=torch.int64, device="cuda")
    ref = run(ops, inp, P_CAP)                                  # no count, plain, fresh outputs
    assert len(ref) == 4 and ref[3].dtype == torch.bool
    ref_conf = None
    for counted in (False, True):
        for conf in (False, True):
            for given in (False, True):
                form = (dt, counted, conf, given)
                out = None
                if given:
                    out = (torch.full((P_CAP, 16, 2), SENTINEL, device="cuda"), torch.full((P_CAP, 16, 2), SENTINEL, device="cuda"),
                           torch.full((P_CAP * 16, 2), SENTINEL, device="cuda"),
                           torch.full((P_CAP, 16), FLAG, dtype=torch.uint8, device="cuda"))
                    if conf:
                        out += (torch.full((P_CAP, 16), SENTINEL, device="cuda"),)
                got = run(ops, inp, P_CAP, count=cnt if counted else None, return_confidence=conf, out=out)
                assert len(got) == (5 if conf else 4), form
                if given:                                       # the caller's tensors themselves, if_matching1 as it was given
                    assert all(g is o for g, o in zip(got[:4], out[:4])), form
                    assert not conf or got[4].data_ptr() == out[4].data_ptr(), form
                else:
                    assert got[3].dtype == torch.bool, form
                for k, rows in enumerate((COUNT, COUNT, COUNT * 16)):
                    assert same_bits(got[k][:rows], ref[k][:rows]), (form, k)
                assert torch.equal(got[3][:COUNT].to(torch.bool), ref[3][:COUNT]), form
                if conf:
                    ref_conf = got[4] if ref_conf is None else ref_conf
                    assert same_bits(got[4][:COUNT], ref_conf[:COUNT]), form
                if counted and given:                           # rows past the count are not written
                    assert all(bool((got[k][rows:] == SENTINEL).all()) for k, rows in enumerate((COUNT, COUNT, COUNT * 16))), form
                    assert bool((got[3][COUNT:] == FLAG).all()), form
                    assert not conf or bool((got[4][COUNT:] == SENTINEL).all()), form


_BATCH = {}


def _merge_inputs(ops, mixed):
    """The row table of a two-pair batch (5x6 + 5x6, or 6x9 + 5x6 mixed) and the fine level's trust scores and flags as they
    are BEFORE the merge: the expansion run again on the step's fine-level plans.  Made once per batch kind, left unchanged."""
    if mixed not in _BATCH:
        _, _, _, out = _small_batch(mixed)
        st, rows, co = out["stages"], out["rows"], out["coarse"]
        trust, _, _, _, ifn_L2, _ = ops.est_position_second(st["Z2"], st["sx"], st["sy"], [96, 96], 8, count=rows.chunk_base[-1:])
        live = int(rows.chunk_base[-1].item())
        assert live > 0 and int((~ifn_L2[:live]).sum()) > 0
        _BATCH[mixed] = (rows, (co["H"], co["W"]), trust, ifn_L2, live)
    return _BATCH[mixed]


@pytest.mark.parametrize("merge_new", [True, False])
@pytest.mark.parametrize("mixed", [False, True])
def test_merge_with_a_zeroed_scores_back_equals_the_merge_that_makes_its_own(ops, mixed, merge_new):
    rows, shape, trust, ifn_L2, live = _merge_inputs(ops, mixed)
    cells = rows.table.cells if mixed else rows.pairs * rows.h * rows.w
    zero = torch.zeros((cells, 16, 9), dtype=torch.float64, device="cuda")
    zero = zero if mixed else zero.view(rows.pairs, rows.h * rows.w, 16, 9)
    t_a, f_a, t_b, f_b = trust.clone(), ifn_L2.clone(), trust.clone(), ifn_L2.clone()
    own = ops.merge_patches_batch(merge_new, rows, t_a, shape, f_a)
    given = ops.merge_patches_batch(merge_new, rows, t_b, shape, f_b, scores_back=zero)
    assert own.dtype == torch.bool and own.shape == (rows.rows_cap, 144) and int((~own[:live]).sum()) > 0
    assert torch.equal(own, given)
    assert same_bits(t_a[:live], t_b[:live]) and torch.equal(f_a[:live], f_b[:live])         # the in-place updates


def test_uniform_device_count_crops_equal_the_ragged_crops_of_a_one_shape_table(ops):
    h, w = 5, 6
    left, right = [cu(x) for x in synth.SynthNets(seed=synth.SEED + 40, h=h, w=w).images()]     # _small_batch's first pair
    xs, ys, ap, ifn = cell_inputs(1, h, w, 77)
    table = ops.PairTable([(h, w)], left.device)
    uni = ops.Compute_imgs_ex(xs, ys, ap, ifn, left, right, width=w, height=h, known_count="device")
    rag = ops.Compute_imgs_ragged(xs.reshape(-1), ys.reshape(-1), ap.reshape(-1, 2), ifn.reshape(-1), left.reshape(-1),
                                  right.reshape(-1), table)
    assert len(uni) == len(rag) == 8
    K = int(uni[7].item())
    assert 0 < K < h * w and torch.equal(uni[7], rag[7]) and torch.equal(uni[6], rag[6])
    for k in (0, 1, 5):                                         # the crops and their bounds: the first K_total rows are written
        assert same_bits(uni[k][:K], rag[k][:K]), k
    for k in (2, 3, 4):                                         # per-cell outputs, [1,N,2] against the packed [N,2]
        assert same_bits(uni[k].reshape(-1, 2), rag[k]), k
