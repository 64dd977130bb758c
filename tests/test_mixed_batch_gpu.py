"""Ragged throughput batches (pats_amd.batch.forward_pairs_mixed): pairs of DIFFERENT grids in one batch.  Every pair's
matches must be bit-identical to pipeline.forward_path and to forward_pairs(pairs=1) on that pair alone, and the goldens of
the reference's own chain (tests/golden/pipeline_*.npz) must hold inside a mixed batch.  The stand-in networks are those of
tests/test_batch_gpu.py, made ragged-aware: the pair of a row comes from rows.row_pair (slot order)."""
import numpy as np
import pytest
import torch

from conftest import golden
from pats_amd import synth
from test_batch_gpu import _BatchNets, cu

pytestmark = pytest.mark.gpu


class _MixedNets(_BatchNets):
    """_BatchNets over a MixedPack: nets are given in the CALLER's order and held in slot order; nets.coarse is called once per
    shape group with views into the pack's store (found by address); `kill` = caller indices whose coarse level matches
    nothing (unrelated descriptors, as in test_gpu_parity's chunk-walk edge test)."""

    def __init__(self, nets, pack, kill=()):
        super().__init__([nets[i] for i in pack.caller_of])
        self.pack = pack
        self.kill = {pack.slot_of[i] for i in kill}

    def coarse(self, lefts, rights):
        for lo, hi, h, w, l, _ in self.pack.groups:
            if l.data_ptr() == lefts.data_ptr() and l.shape == lefts.shape:
                break
        else:
            raise AssertionError("coarse called on something that is not a group of the pack")
        d0s, d1s, nss = [], [], []
        for s in range(lo, hi):
            c = self.nets[s].coarse()
            d0, d1 = cu(c["d0"]), cu(c["d1"])
            if s in self.kill:
                d1 = torch.randn(d1.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
                d0 = torch.randn(d0.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
            d0s.append(d0), d1s.append(d1), nss.append(cu(c["ns"]))
            alpha = float(c["alpha"])
        return torch.cat(d0s), torch.cat(d1s), torch.cat(nss), alpha

    def fine(self, rows, new_left, new_right):
        pair_of_row = rows.row_pair.cpu().numpy()
        base = rows.chunk_base.cpu().numpy()
        f0 = np.zeros((rows.rows_cap, 264, 145), np.float32)
        f1 = np.zeros_like(f0)
        sx = np.ones((rows.rows_cap, 1, 144), np.float32)
        sy = np.ones_like(sx)
        self.blocks = []
        for c in range(rows.Cmax):
            r0, r1 = int(base[c]), int(base[c + 1])
            pair = pair_of_row[r0:r1]
            for p in np.unique(pair):
                idx = np.nonzero(pair == p)[0] + r0
                assert (np.diff(idx) == 1).all()
                f = self.nets[p].fine(c, len(idx))
                f0[idx], f1[idx], sx[idx], sy[idx] = f["d0"], f["d1"], f["scale_x"], f["scale_y"]
                self.blocks.append((c, int(p), int(idx[0]), len(idx)))
        return cu(f0), cu(f1), cu(sx), cu(sy)


class _SmallThird(_MixedNets):
    """Third-level tensors over the whole capacity without reading P (the problem count may exceed the capacity)."""

    def third(self, rows, mk0, mk1, b_ids, P_dev):
        cap_ = mk0.shape[0]
        return (torch.zeros((cap_, 128, 65), device="cuda"), torch.zeros((cap_, 128, 65), device="cuda"),
                torch.ones((cap_, 1, 64), device="cuda"))


def _run_mixed(nets, if_local, outdoor, new, kill=(), images=None, net_cls=_MixedNets, **capkw):
    from pats_amd import batch
    imgs = images or [tuple(cu(x) for x in n.images()) for n in nets]
    pack = batch.pack_pairs(imgs)
    cap = batch.MixedCapacities([(n.h, n.w) for n in nets], if_local=if_local, **capkw)
    out = batch.forward_pairs_mixed(pack, net_cls(nets, pack, kill), cap, if_outdoor=outdoor, merge_new=new)
    return pack, cap, out


def _single(n, if_local, outdoor, new):
    from pats_amd import batch
    left, right = [cu(x) for x in n.images()]
    cap = batch.Capacities(1, n.h, n.w, if_local=if_local)
    out = batch.forward_pairs(left, right, _BatchNets([n]), cap, if_outdoor=outdoor, merge_new=new)
    (ml, mr), = batch.split_by_pair(out, cap)
    return ml, mr, out


def _per_chunk_counts(out, slot):
    """(rows, P, M) per chunk of one slot of a mixed result - what the goldens' `chunks` hold for a pair."""
    rows = out["rows"]
    base = rows.chunk_base.cpu().numpy()
    rp = rows.row_pair.cpu().numpy()
    C = rows.Cmax
    n_rows = [int((rp[base[c]:base[c + 1]] == slot).sum()) for c in range(C)]
    P = int(out["P"].item())
    b = out["stages"]["b_ids"][:P].cpu().numpy()
    chunk_b = np.searchsorted(base, b, side="right") - 1
    n_P = np.bincount(chunk_b[rp[b] == slot], minlength=C)[:C].tolist()
    M = int(out["M"].item())
    mrow = out["match_row"][:M].cpu().numpy()
    chunk_m = np.searchsorted(base, mrow, side="right") - 1
    n_M = np.bincount(chunk_m[rp[mrow] == slot], minlength=C)[:C].tolist()
    return n_rows, n_P, n_M


@pytest.mark.parametrize("names", [("pipeline_outdoor.npz", "pipeline_640x480_outdoor.npz"),
                                   ("pipeline_indoor.npz", "pipeline_640x480_indoor.npz")])
def test_goldens_inside_a_mixed_batch(names):
    from pats_amd import batch
    gs = [golden(n) for n in names]
    if_local, outdoor, new = bool(gs[0]["if_local"]), bool(gs[0]["if_outdoor"]), bool(gs[0]["merge_new"])
    assert all((bool(g["if_local"]), bool(g["if_outdoor"]), bool(g["merge_new"])) == (if_local, outdoor, new) for g in gs)
    nets = [synth.SynthNets(seed=int(g["seed"]), h=int(g["h"]), w=int(g["w"])) for g in gs]
    nets.append(synth.SynthNets(seed=synth.SEED + 3040, h=8, w=10))         # a third grid beside the two goldens
    pack, cap, out = _run_mixed(nets, if_local, outdoor, new)
    assert len(pack.groups) == 3
    per_pair = batch.split_by_pair(out, cap)
    for i, g in enumerate(gs):
        ml, mr = (t.cpu().numpy() for t in per_pair[i])
        assert ml.shape == g["matches_l"].shape and ml.shape[0] > 500, names[i]
        np.testing.assert_allclose(ml, g["matches_l"], atol=1e-4, rtol=1e-6)
        np.testing.assert_allclose(mr, g["matches_r"], atol=6e-3, rtol=1e-6)
        chunks = g["chunks"]
        n_rows, n_P, n_M = _per_chunk_counts(out, pack.slot_of[i])
        k = len(chunks)
        assert n_rows[:k] == chunks[:, 0].tolist() and sum(n_rows) == int(chunks[:, 0].sum()), names[i]
        assert n_P[:k] == chunks[:, 1].tolist() and sum(n_P) == int(chunks[:, 1].sum()), names[i]
        assert n_M[:k] == chunks[:, 2].tolist() and sum(n_M) == int(chunks[:, 2].sum()), names[i]
    assert per_pair[2][0].shape[0] > 0


@pytest.mark.parametrize("if_local,outdoor,new", [(True, True, True), (False, False, False)])
def test_mixed_shapes_bit_identical_to_the_pair_alone(if_local, outdoor, new):
    """Six pairs over four grids (15x20 twice, 20x15, 24x32 twice, 32x24: both coarse solvers run), passed in shuffled order:
    every pair's matches equal pipeline.forward_path and forward_pairs(pairs=1) on that pair alone, bit for bit."""
    from pats_amd import batch, pipeline
    from test_gpu_parity import _CudaNets
    shapes = [(24, 32), (15, 20), (32, 24), (20, 15), (15, 20), (24, 32)]
    nets = [synth.SynthNets(seed=synth.SEED + 5000 + 101 * i, h=h, w=w) for i, (h, w) in enumerate(shapes)]
    pack, cap, out = _run_mixed(nets, if_local, outdoor, new)
    assert len(pack.groups) == 4 and pack.caller_of != list(range(6))
    per_pair = batch.split_by_pair(out, cap)
    total = 0
    for i, n in enumerate(nets):
        left, right = [cu(x) for x in n.images()]
        ref = pipeline.forward_path(left, right, _CudaNets(n), if_local=if_local, if_outdoor=outdoor, merge_new=new)
        ml, mr, _ = _single(n, if_local, outdoor, new)
        assert ref["matches_l"].shape[0] > 100, i
        assert torch.equal(per_pair[i][0], ref["matches_l"]) and torch.equal(per_pair[i][1], ref["matches_r"]), i
        assert torch.equal(per_pair[i][0], ml) and torch.equal(per_pair[i][1], mr), i
        total += ml.shape[0]
    assert total == int(out["M"].item())
    assert len({pp[0].shape[0] for pp in per_pair}) >= 5              # the pairs really differ


def test_uniform_batch_through_the_mixed_path_equals_forward_pairs():
    from pats_amd import batch
    nets = [synth.SynthNets(seed=s, h=15, w=20) for s in (synth.SEED + 40, synth.SEED + 1040, synth.SEED + 2040)]
    imgs = [n.images() for n in nets]
    lefts = cu(np.concatenate([i[0] for i in imgs]))
    rights = cu(np.concatenate([i[1] for i in imgs]))
    cap = batch.Capacities(3, 15, 20)
    want = batch.forward_pairs(lefts, rights, _BatchNets(nets), cap)
    pack, mcap, got = _run_mixed(nets, True, True, True)
    assert pack.caller_of == [0, 1, 2] and all(getattr(mcap, k) == getattr(cap, k) for k in vars(cap))
    a, b = want["rows"], got["rows"]
    for k in ("chunk_base", "crop_base", "row_cell", "row_forced", "row_crop", "sum_cycle", "cycle_num", "second", "third"):
        assert torch.equal(getattr(a, k).reshape(-1), getattr(b, k).reshape(-1)), k
    assert torch.equal(a.masks.reshape(-1), b.masks.reshape(-1)) and torch.equal(a.row_slot.reshape(-1), b.row_slot.reshape(-1))
    assert torch.equal(a.row_pair, b.row_pair)
    for k in ("M", "P", "status"):
        assert torch.equal(want[k], got[k]), k
    M = int(want["M"].item())
    for k in ("matches_l", "matches_r", "match_row"):
        assert torch.equal(want[k][:M], got[k][:M]), k
    for p, q in zip(batch.split_by_pair(want, cap), batch.split_by_pair(got, mcap)):
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])


def test_pair_without_coarse_match_inside_a_mixed_batch():
    from pats_amd import batch
    nets = [synth.SynthNets(seed=synth.SEED + 40, h=15, w=20), synth.SynthNets(seed=synth.SEED + 77, h=5, w=6),
            synth.SynthNets(seed=synth.SEED + 3040, h=8, w=10)]
    pack, cap, out = _run_mixed(nets, True, True, True, kill=(1,))
    per_pair = batch.split_by_pair(out, cap)
    assert per_pair[1][0].shape == (0, 2) and per_pair[1][1].shape == (0, 2)
    for i in (0, 2):
        ml, mr, _ = _single(nets[i], True, True, True)
        assert ml.shape[0] > 0 and torch.equal(per_pair[i][0], ml) and torch.equal(per_pair[i][1], mr), i


def test_crops_never_see_a_neighbouring_pair():
    """A 5x6 pair whose crop windows reach past all four borders of its image sits in the middle of the store: a 4x12 pair
    (another width) right before it, a 6x9 pair right after it, both with huge pixels.  Every crop equals the crop
    forward_pairs makes from that pair's image alone (reads outside a pair's image are the reference's zero padding), and the
    matches stay bit-identical."""
    from pats_amd import batch
    nets = [synth.SynthNets(seed=synth.SEED + 4040, h=6, w=9), synth.SynthNets(seed=synth.SEED + 40, h=5, w=6),
            synth.SynthNets(seed=synth.SEED + 3040, h=4, w=12)]
    imgs = [tuple(cu(x) for x in n.images()) for n in nets]
    loud = [tuple(torch.full_like(t, 1e4) for t in imgs[0]), imgs[1], tuple(torch.full_like(t, -1e4) for t in imgs[2])]
    pack, cap, out = _run_mixed(nets, True, True, True, images=loud)
    assert pack.slot_of == [2, 1, 0] and pack.shapes == [(4, 12), (5, 6), (6, 9)]       # the 5x6 pair between the two others
    ml, mr, one = _single(nets[1], True, True, True)
    K = int(one["K_img"][0].item())
    s = pack.slot_of[1]
    cb = out["rows"].crop_base.cpu().tolist()
    assert cb[s + 1] - cb[s] == K and K > 0
    b5 = out["coarse"]["new_left"], out["coarse"]["new_right"]
    for k in range(2):
        assert torch.equal(b5[k][cb[s]:cb[s + 1]], one["crops"][k][:K]), k
    # the windows of this pair do reach past its top / bottom / left / right edge (else the test shows nothing)
    crops = one["crops"][0][:K]
    for edge in (crops[:, :32], crops[:, -32:], crops[:, :, :32], crops[:, :, -32:]):
        assert edge.flatten(1).eq(0).all(1).any()
    per_pair = batch.split_by_pair(out, cap)
    assert torch.equal(per_pair[1][0], ml) and torch.equal(per_pair[1][1], mr)


def test_matches_by_pair_without_P_on_a_ragged_table():
    """ops.matches_by_pair on a ragged row table without P: only the pairs + 1 offsets are written (nothing past them in a
    caller's buffer), equal to the leading part of the summary the batch path reads."""
    from pats_amd import batch, ops
    nets = [synth.SynthNets(seed=synth.SEED + 40, h=15, w=20), synth.SynthNets(seed=synth.SEED + 3040, h=8, w=10),
            synth.SynthNets(seed=synth.SEED + 77, h=5, w=6)]
    pack, cap, out = _run_mixed(nets, True, True, True)
    batch.group_by_pair(out, cap)
    want = out["summary"][:cap.pairs + 1]
    big = torch.full((cap.pairs + 8,), -7, dtype=torch.int64, device="cuda")
    ol, orr = torch.empty_like(out["matches_l"]), torch.empty_like(out["matches_r"])
    got = ops.matches_by_pair(out["rows"], out["matches_l"], out["matches_r"], out["match_row"], out["M"],
                              out=(ol, orr, big[:cap.pairs + 1]))
    assert torch.equal(got[2], want) and torch.equal(big[:cap.pairs + 1], want)
    assert (big[cap.pairs + 1:] == -7).all()                          # untouched past the offsets
    M = int(out["M"].item())
    assert torch.equal(ol[:M], out["by_pair"][0][:M]) and torch.equal(orr[:M], out["by_pair"][1][:M])
    fresh = ops.matches_by_pair(out["rows"], out["matches_l"], out["matches_r"], out["match_row"], out["M"])
    assert len(fresh) == 3 and torch.equal(fresh[2], want)


def test_overflow_in_a_mixed_batch_is_reported():
    from pats_amd import batch
    nets = [synth.SynthNets(seed=synth.SEED + 40, h=15, w=20), synth.SynthNets(seed=synth.SEED + 3040, h=8, w=10)]
    pack, cap, out = _run_mixed(nets, True, True, True, net_cls=_SmallThird, rows_cap=50)
    assert int(out["status"].item()) & 2
    with pytest.raises(RuntimeError, match="rows_cap"):
        batch.split_by_pair(out, cap)
    pack, cap, out = _run_mixed(nets, True, True, True, net_cls=_SmallThird, p_cap_per_pair=16)
    assert int(out["P"].item()) > cap.P_cap
    with pytest.raises(RuntimeError, match="P_cap"):
        batch.split_by_pair(out, cap)
