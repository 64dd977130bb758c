"""Throughput mode of pats_amd.pipeline: PATS.forward's hot path (models/pats.py:18-85 and the three layers' forward
tails) for a BATCH of image pairs, without a single host read between the coarse descriptors and the matches.

The reference runs one pair at a time and, inside it, one chunk at a time (evaluate.py:25, pats.py:33,
first_layer.py:131-146) because it targets a 16-40 GB card, and every boolean-mask indexing on the way is a
device->host sync that sizes the next tensor.  Pairs are independent and the chunks of a pair couple only through the
merge's `scores_back` (pats.py:32,37), so with 288 GB of HBM every stage becomes ONE launch over all pairs and chunks:

  coarse   cost + log_optimal_transport + column mass + area expansion for all pairs        (first_layer.py:110-127)
  plan     cumulative match counts, split_patches, chunk masks, the fine level's row table   (first_layer.py:130-146)
           rows ordered (chunk, pair, cell): chunk c of every pair is one contiguous block   (ops.chunk_rows)
  crops    Compute_imgs for all pairs, (image, patch) order, counts on the device            (utils.py:1343-1393)
  fine     cost + log_optimal_transport2 + ln k + area expansion for all rows                (second_layer.py:100-118)
  merge    merge_patches_new / _old: chunk blocks in order, each over all pairs, tail rows   (second_layer.py:119-122,
           masked                                                                             pats.py:38-39)
  third    surviving cells -> points (pats.py:53-58), cost + OT + Compute_result + label    (third_layer.py:153-170)
           over a CAPACITY with the count on the device
  result   scatter onto the 48x48 sub-cell grid (pats.py:59-67), get_result for all chunks   (pats.py:68-78)

Sizes are capacities fixed on the host (`Capacities`); the counts the reference reads back (matched patches K, rows B,
third-level problems P, matches M) stay on the device and come back WITH the results: `status` / `P` / `M` are read by
the caller when it fetches the matches.  Rows of the table that no chunk uses (padding past the device-side total
`rows.chunk_base[-1]`) are SKIPPED by the fine level's launches (cost build, OT, expansion take the count from the device;
a network callback may do the same with ops.fine_descriptors(count=...)) and are "no match" at the merge; rows that are left
without a cell are not compacted (pats.py:40-52) - they emit nothing, exactly as in pipeline.forward_path.

Network callbacks (`nets`, the out-of-scope backbones + heads; they return GPU tensors - the descriptors mdesc0 / mdesc1, feat0 / feat1 in float32,
float16 or bfloat16 (ops.cost_ot / ops.third_level read them as they are), everything else float32 - no host read required of them;
the backbone maps they gather from with ops.fine_descriptors / ops.third_descriptors may be float16 / bfloat16, and those two
write half descriptors themselves with out_dtype= or a half out=: the float32 values rounded once at the store, no .to() pass):
  nets.coarse(lefts, rights) -> mdesc0 [pairs,D,N], mdesc1 [pairs,D,N], scale [pairs,1,N], alpha
  nets.fine(rows, new_left, new_right) -> mdesc0 [rows_cap,264,145], mdesc1, scale_x [rows_cap,1,144], scale_y
      [, scale_x * scale_y] (what ops.scale_head hands out; formed here if absent)
      rows: ops.ChunkRows (row r shows crop rows.row_crop[r] of new_left / new_right [pairs*N,96,96,3])
      The crops are float32 HWC unless forward_pairs / forward_pairs_mixed get a crop_format (ops.CropFormat): then both
      come in that format - e.g. CropFormat.backbone(torch.bfloat16): [pairs*N,3,96,96] bf16, normalised, the backbone's
      input as it stands (a uint8 format: uint8 left crops, float32 right crops).
  nets.third(rows, mkpts0_c [P_cap,2], mkpts1_c [P_cap,2], b_ids [P_cap], P_dev [1]) ->
      feat0 [P_cap,128,65], feat1 [P_cap,128,65], scale [P_cap,1,64] [, p_s, p_t [P_cap,2] int64: the points rounded to
      the 4-px lattice as ops.third_descriptors returns them; formed here if absent]      (b_ids = row of the table)
"""
import numpy as np
import torch

from . import ops


class Capacities:
    """Host-side sizes of one batch.  p_cap_per_pair bounds the third-level problems of a pair: the merge leaves every
    8-px cell to at most one window per chunk, so 16*h*w cells is the natural size (cells handed over between chunks can
    add a few; the default keeps 25 % headroom; an overflow is reported in the result, never silent)."""

    def __init__(self, pairs, h, w, if_local=True, p_cap_per_pair=None, rows_cap=None):
        self.pairs, self.h, self.w = int(pairs), int(h), int(w)
        self.N = self.h * self.w
        self.chunk_cap = 2 * self.w if if_local else 512                      # first_layer.py:131-135
        self.Cmax = ops.max_chunks(self.h, self.w, self.chunk_cap)
        # worst case: every cell matched, every chunk boundary repeats one grid row.  A caller that knows its data (a dry
        # run of the coarse stage) may pass a tighter rows_cap: the fine level then runs fewer padding rows, and a batch
        # that does not fit is reported through `status` (split_by_pair raises), never truncated silently.
        self.rows_cap = self.pairs * (self.N + (self.Cmax - 1) * self.w) if rows_cap is None else int(rows_cap)
        per_pair = int(1.25 * 16 * self.N) if p_cap_per_pair is None else int(p_cap_per_pair)
        self.P_cap = self.pairs * per_pair


class MixedCapacities:
    """Capacities of a batch whose pairs may have different grids: `shapes` = the pairs' (h, w) (any order).  A list of one
    repeated shape gives exactly Capacities(pairs, h, w, ...).  Otherwise h = w = N = chunk_cap = None and
    Cmax = max_p Cmax_p, rows_cap = sum_p (N_p + (Cmax_p - 1) w_p), P_cap = sum_p int(1.25 * 16 * N_p) (or p_cap_per_pair
    for every pair) - the per-pair worst cases of Capacities added up."""

    def __init__(self, shapes, if_local=True, p_cap_per_pair=None, rows_cap=None):
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.if_local = bool(if_local)
        if not self.shapes:
            raise ValueError("MixedCapacities: no pairs")
        if len(set(self.shapes)) == 1:
            u = Capacities(len(self.shapes), self.shapes[0][0], self.shapes[0][1], if_local, p_cap_per_pair, rows_cap)
            self.pairs, self.h, self.w, self.N = u.pairs, u.h, u.w, u.N
            self.chunk_cap, self.Cmax, self.rows_cap, self.P_cap = u.chunk_cap, u.Cmax, u.rows_cap, u.P_cap
            return
        self.pairs, self.h, self.w, self.N, self.chunk_cap = len(self.shapes), None, None, None, None
        cm = [ops.max_chunks(h, w, 2 * w if if_local else 512) for h, w in self.shapes]
        self.Cmax = max(cm)
        self.rows_cap = (sum(h * w + (c - 1) * w for (h, w), c in zip(self.shapes, cm)) if rows_cap is None else int(rows_cap))
        self.P_cap = sum(int(1.25 * 16 * h * w) if p_cap_per_pair is None else int(p_cap_per_pair) for h, w in self.shapes)


class MixedPack:
    """What pack_pairs returns.  Pairs are sorted stably by grid into SLOTS, so every shape group is a contiguous slot range:
        shapes          (h, w) per slot;  slot_of / caller_of: caller index -> slot, slot -> caller index
        left, right     the flat HWC image stores (slot order; pair s at table.img_base[s] elements)
        table           ops.PairTable of the slots (grids, packed cell ranges, image offsets)
        groups          [(slot_lo, slot_hi, h, w, lefts [g,32h,32w,3], rights)] - views into the stores, for nets.coarse"""


def slot_order(shapes):
    """The slots of a mixed batch: caller indices sorted stably by grid (equal grids keep the caller's order), so that every shape
    group is a contiguous slot range.  Returns caller_of (slot -> caller index)."""
    return sorted(range(len(shapes)), key=lambda i: tuple(shapes[i]))


def pack_pairs(pairs, keep_dtype=False):
    """pairs: [(left, right)] HWC GPU tensors, each [H_p, W_p, 3] or [1, H_p, W_p, 3] with H_p, W_p multiples of 32 (the two
    images of a pair the same size).  Returns a MixedPack for forward_pairs_mixed.  The stores are float32 (.float() of every
    image) - or, with keep_dtype=True, the pairs' own dtype, which must be one of float32, float16, bfloat16 and uint8 and the
    same for every image (nets.coarse then gets views in that dtype; the crops widen it exactly, ops.Compute_imgs_ragged)."""
    if not pairs:
        raise ValueError("pack_pairs: no pairs")
    imgs, shapes = [], []
    for i, (l, r) in enumerate(pairs):
        l = l[0] if l.dim() == 4 else l
        r = r[0] if r.dim() == 4 else r
        if l.dim() != 3 or l.shape[2] != 3 or l.shape != r.shape or l.shape[0] % 32 or l.shape[1] % 32 or not l.is_cuda:
            raise ValueError("pack_pairs: pair %d must be two equal [H,W,3] GPU images with H, W multiples of 32" % i)
        imgs.append((l, r) if keep_dtype else (l.float(), r.float()))
        shapes.append((int(l.shape[0]) // 32, int(l.shape[1]) // 32))
    if keep_dtype:
        dts = {t.dtype for pr in imgs for t in pr}
        if len(dts) != 1 or next(iter(dts)) not in (torch.float32, torch.float16, torch.bfloat16, torch.uint8):
            raise ValueError("pack_pairs: keep_dtype needs every image in one of float32, float16, bfloat16, uint8, got %s"
                             % sorted(str(d) for d in dts))
    caller_of = slot_order(shapes)
    pk = MixedPack()
    pk.caller_of = caller_of
    pk.slot_of = [0] * len(caller_of)
    for s_, i in enumerate(caller_of):
        pk.slot_of[i] = s_
    pk.shapes = [shapes[i] for i in caller_of]
    dev = imgs[0][0].device
    pk.left = torch.cat([imgs[i][0].reshape(-1) for i in caller_of])
    pk.right = torch.cat([imgs[i][1].reshape(-1) for i in caller_of])
    pk.table = ops.PairTable(pk.shapes, dev)
    pk.groups = []
    lo = 0
    while lo < len(caller_of):
        hi = lo
        while hi < len(caller_of) and pk.shapes[hi] == pk.shapes[lo]:
            hi += 1
        h, w = pk.shapes[lo]
        o0, n = int(pk.table.img_base_host[lo]), (hi - lo) * h * w * 1024 * 3
        pk.groups.append((lo, hi, h, w, pk.left[o0:o0 + n].view(hi - lo, 32 * h, 32 * w, 3),
                          pk.right[o0:o0 + n].view(hi - lo, 32 * h, 32 * w, 3)))
        lo = hi
    return pk


def pack_raw_pairs(pairs, size=None, targets=None, canvas=None, dtype=torch.uint8, bgr=False, K=None, intrinsics="ratio", threshold=None):
    """pack_pairs for RAW images: pairs = [(left, right)] decoded uint8 [h0, w0, 3] GPU tensors of any size, each its own tensor.
    What the reference's data set classes do on the CPU - Resize_img's centre crop and resize, the zero pad to a canvas that is a
    multiple of 32 and common to the pair (include/pats_amd.h, "Image front end") - happens in ONE launch that writes every canvas
    straight into the flat stores in slot order (ops.prepare_images; no torch.cat pass).  size / targets / canvas as
    ops.prepare_plan takes them; dtype: the stores' (uint8, float32, float16, bfloat16); bgr: swap the channel order.
    Returns the MixedPack pack_pairs(prepared images, keep_dtype=True) would return, which also carries
        plan                 the ops.PreparePlan (windows, targets, canvases; host)
        K_left, K_right      [pairs,3,3] float64 host arrays: the intrinsics of the prepared images      } with K = [(K_l, K_r)], the raw
        norm [pairs,8]       float32 on the GPU, caller order: the `norm` of verify_by_pair and the rest  } images' 3 x 3, and
        thr [pairs]          float32 on the GPU: threshold / mean focal length; with `threshold` only     } intrinsics "ratio" or "axes"
    (None without K).  ValueError: a canvas that does not hold a target, K without both matrices of every pair."""
    if not pairs:
        raise ValueError("pack_raw_pairs: no pairs")
    for i, pr in enumerate(pairs):
        if len(pr) != 2 or any(not isinstance(t, torch.Tensor) or t.dim() != 3 for t in pr):
            raise ValueError("pack_raw_pairs: pair %d must be two [h, w, 3] tensors" % i)
    plan = ops.prepare_plan([((l.shape[0], l.shape[1]), (r.shape[0], r.shape[1])) for l, r in pairs], size=size, targets=targets,
                            canvas=canvas)
    pk = MixedPack()
    pk.plan, pk.K_left, pk.K_right, pk.norm, pk.thr = plan, None, None, None, None
    if K is not None:
        if len(K) != len(pairs) or any(k is None or len(k) != 2 or k[0] is None or k[1] is None for k in K):
            raise ValueError("pack_raw_pairs: K must hold (K_left, K_right) for every pair")
        prepared = [[ops.prepare_intrinsics(k[s], plan.h0[p, s], plan.w0[p, s], plan.w_t[p, s], plan.h_t[p, s], intrinsics)
                     for p, k in enumerate(K)] for s in range(2)]
        pk.K_left, pk.K_right = np.stack(prepared[0]), np.stack(prepared[1])
    elif threshold is not None:
        raise ValueError("pack_raw_pairs: a threshold needs K")
    dev = pairs[0][0].device
    pk.caller_of, pk.slot_of = list(plan.caller_of), list(plan.slot_of)
    pk.shapes = [plan.shapes[i] for i in pk.caller_of]
    pk.left = torch.empty(plan.elems, dtype=dtype, device=dev)
    pk.right = torch.empty(plan.elems, dtype=dtype, device=dev)
    ops.prepare_images(pairs, plan, pk.left, pk.right, bgr=bgr)
    pk.table = ops.PairTable(pk.shapes, dev)
    pk.groups = []
    lo = 0
    while lo < len(pk.shapes):
        hi = lo
        while hi < len(pk.shapes) and pk.shapes[hi] == pk.shapes[lo]:
            hi += 1
        h, w = pk.shapes[lo]
        o0, n = int(pk.table.img_base_host[lo]), (hi - lo) * h * w * 1024 * 3
        pk.groups.append((lo, hi, h, w, pk.left[o0:o0 + n].view(hi - lo, 32 * h, 32 * w, 3),
                          pk.right[o0:o0 + n].view(hi - lo, 32 * h, 32 * w, 3)))
        lo = hi
    if K is not None:
        pk.norm = torch.from_numpy(ops.prepare_norm(pk.K_left, pk.K_right)).to(dev)
        if threshold is not None:
            pk.thr = torch.from_numpy(ops.prepare_thr(pk.K_left, pk.K_right, threshold)).to(dev)
    return pk


_ONE = {}


def _one(device):
    """The reference's `self.one` (second_layer.py:63): a device-resident 1.0, made once per device."""
    key = str(device)
    if key not in _ONE:
        _ONE[key] = torch.tensor(1.0, device=device)
    return _ONE[key]


def _round4(x, clamp96):
    """third_layer.py:122 / :126-128: round(x / 4).long() * 4 (targets clamped to [0, 96] first)."""
    if clamp96:
        x = torch.clamp(x, 0.0, 96.0)           # == the reference's two torch.where; python scalars: no H2D copy per call
    return torch.round(x / 4.0).long() * 4


def _coarse_tail(lefts, rights, nets, iters, H, W):
    """The first layer's tail (first_layer.py:110-127) for pairs of ONE grid: nets.coarse, cost + OT, column mass, area expansion
    -> est_position_first's (trust, pts, xs, ys, ifn1, ifn2)."""
    mdesc0, mdesc1, scale, alpha = nets.coarse(lefts, rights)
    Z = ops.cost_ot(mdesc0, mdesc1, 1, alpha, scale, iters)
    scales, cflag = ops.colmass_sqrt(Z, return_flags=True)
    return ops.est_position_first(Z, scales, (H, W), 32, col_nomatch=cflag)


def coarse_stage(lefts, rights, nets, cap, iters=100, fine_inputs=True, crop_format=None):
    """(fine_inputs="rows_only": stop after the row table - capacity planning.)
    The first layer's tail for all pairs + the chunk plan / row table + the crops (first_layer.py:110-146,
    utils.py:1343-1393) and - fine_inputs=True - the second layer's descriptors for those rows (nets.fine: backbone on the
    crops + the a15 gather).  Independent of every other batch and HBM-bound (crops, gathers): a caller may run it on a
    stream of its own beside the solver stages of the previous batches (bench.py does)."""
    H, W = int(lefts.shape[1]), int(lefts.shape[2])
    h, w = cap.h, cap.w
    assert (H // 32, W // 32) == (h, w) and lefts.shape[0] == cap.pairs
    trust, pts, xs, ys, ifn1, ifn2 = _coarse_tail(lefts, rights, nets, iters, H, W)
    rows = ops.chunk_rows(ifn1, h, w, cap.chunk_cap, Cmax=cap.Cmax, rows_cap=cap.rows_cap)
    if fine_inputs == "rows_only":
        return {"rows": rows, "ifn1": ifn1}
    new_left, new_right, xsn, ysn, avn, bound5, K_img, K_tot = ops.Compute_imgs_ex(
        xs, ys, pts, ifn1, lefts, rights, width=w, height=h, known_count="device", crop_format=crop_format)
    co = {"rows": rows, "new_left": new_left, "new_right": new_right, "xsn": xsn, "avn": avn, "K_img": K_img,
          "ifn1": ifn1, "H": H, "W": W}
    if fine_inputs:
        co["fine"] = nets.fine(rows, new_left, new_right)
    return co


def _timed(events, tag):
    if events is None:
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    events.setdefault(tag, []).append((e0, e1))
    e0.record()
    return e1


def fine_solve_stage(co, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None):
    """second_layer.py:100-122 + pats.py:38-39,53-58 for every row of a coarse_stage result: cost + OT + expansion, the
    merges in chunk order, the surviving cells' points (VALU-bound)."""
    rows, H, W = co["rows"], co["H"], co["W"]
    fine = co["fine"] if "fine" in co else nets.fine(rows, co["new_left"], co["new_right"])
    f0, f1, sx, sy = fine[:4]
    ns2 = fine[4] if len(fine) > 4 else (sx * sy).contiguous()
    e = _timed(events, "fine")
    if events is not None:                      # the boundary between the pair's two kernels, recorded inside the C call
        em = torch.cuda.Event(enable_timing=True)
        em.record()
        events.setdefault("fine_mid", []).append(em)
        ops.set_cost_ot_mid_event(em)
    live = rows.chunk_base[-1:]                 # rows in use, on the device: the launches cover rows_cap, padding rows are skipped
    Z2, cflag2 = ops.cost_ot(f0, f1, 2, _one(f0.device), ns2, iters, bias_k=2.0 if if_outdoor else 3.0, return_flags=True,
                             count=live)
    if e is not None:
        e.record()
    trust2, pts2, _, _, ifn_L2, _ = ops.est_position_second(Z2, sx, sy, [96, 96], 8, col_nomatch=cflag2, count=live)
    merged = ops.merge_patches_batch(merge_new, rows, trust2, (H, W), ifn_L2)
    mk0, mk1, b_ids, P = ops.third_inputs(merged, pts2, capacity=cap.P_cap, sync=False)
    return {"co": co, "merged": merged, "pts2": pts2, "P": P, "mk0": mk0, "mk1": mk1, "b_ids": b_ids,
            "stages": {"Z2": Z2, "trust2": trust2, "pts2": pts2, "ifn_L2": ifn_L2, "sx": sx, "sy": sy, "f0": f0,
                       "f1": f1, "ns2": ns2, "mk0": mk0, "mk1": mk1, "b_ids": b_ids}}


def third_gather_stage(fs, nets, cap):
    """The third layer's descriptors for the surviving cells (nets.third: backbone maps + the a16 window gather;
    HBM-bound).  Completes a fine_solve_stage result in place."""
    third = nets.third(fs["co"]["rows"], fs["mk0"], fs["mk1"], fs["b_ids"], fs["P"])
    feat0, feat1, scale3 = third[:3]
    p_s, p_t = third[3:5] if len(third) > 3 else (_round4(fs["mk0"], False), _round4(fs["mk1"], True))
    fs.update(feat0=feat0, feat1=feat1, scale3=scale3, p_s=p_s, p_t=p_t)
    fs["stages"].update(feat0=feat0, feat1=feat1, scale3=scale3, p_s=p_s, p_t=p_t)
    return fs


def fine_stage(co, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None):
    return third_gather_stage(fine_solve_stage(co, nets, cap, if_outdoor, merge_new, iters, events), nets, cap)


def third_stage(fs, nets, cap, if_outdoor=True, iters=100, events=None, confidence=False):
    """third_layer.py:153-170 over the capacity with the count on the device, then pats.py:59-78: the scatter onto the
    sub-cell grid and get_result for every chunk of every pair.  confidence: the result gains match_conf [M_cap] float32, the
    third level's per-match confidence (ops.third_level) carried through the scatter and the compaction beside matches_r."""
    co, rows, P = fs["co"], fs["co"]["rows"], fs["P"]
    e = _timed(events, "third")
    # one sequence: with confidence the calls return one tensor more (conf, conf16, match_conf), handed on to the next
    level = ops.third_level(fs["feat0"], fs["feat1"], fs["scale3"], fs["p_s"], fs["p_t"], outdoor=if_outdoor, iters=iters, count=P,
                            return_confidence=bool(confidence))
    m0f, m1f, label, ifm = level[:4]
    if e is not None:
        e.record()
    scattered = ops.refine_scatter(fs["merged"], fs["pts2"], m1f, label, conf=level[4] if confidence else None)
    ifn16, pts16 = scattered[:2]
    result = ops.get_result_chunks(rows, ifn16, co["avn"], pts16, co["xsn"], conf16=scattered[2] if confidence else None)
    ml, mr, mrow, M = result[:4]
    stages = dict(fs["stages"], m0f=m0f, m1f=m1f, label=label, ifm=ifm, pts16=pts16)
    out = {"matches_l": ml, "matches_r": mr, "match_row": mrow}
    if confidence:
        stages.update(conf=level[4], conf16=scattered[2])
        out["match_conf"] = result[4]
    out.update(M=M, P=P, status=rows.status, rows=rows, if_nomatching16=ifn16, merged=fs["merged"], K_img=co["K_img"],
               crops=(co["new_left"], co["new_right"]), coarse=co, stages=stages)
    return out


def fine_third_stage(co, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, confidence=False):
    fs = fine_stage(co, nets, cap, if_outdoor, merge_new, iters, events)
    return third_stage(fs, nets, cap, if_outdoor, iters, events, confidence)


def forward_pairs(lefts, rights, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None,
                  confidence=False):
    """lefts / rights [pairs,H,W,3] HWC, float32 (or float16 / bfloat16 / uint8: nets.coarse gets them as they are, the crops
    widen them exactly).  crop_format: the ops.CropFormat nets.fine receives the crops in (None: float32 HWC).
    nets.coarse / nets.fine / nets.third may return their descriptors in float32, float16 or bfloat16 (ops.cost_ot / ops.third_level
    read them as they are: same matches as on .float() copies); scales and points stay float32.
    Returns a dict of DEVICE tensors:
        matches_l, matches_r [M_cap,2]   the first M rows valid, reference order inside every pair (chunk, patch, sub-cell)
        match_row [M_cap] int32          row of the table per match;  rows.row_cell[match_row] // N = pair
        match_conf [M_cap] float32       confidence=True only: the third level's per-match confidence (ops.third_level), aligned
                                         with matches_l / matches_r; group_by_pair / split_by_pair then carry it along
        M, P [1] int64, status [1] int32 match count, third-level problem count (P > cap.P_cap = overflow), table status
        rows                             the ops.ChunkRows table
        stages                           the intermediate tensors (parity checks; nothing reads them here)
    No host read happens in here."""
    co = coarse_stage(lefts, rights, nets, cap, iters, fine_inputs=False, crop_format=crop_format)
    return fine_third_stage(co, nets, cap, if_outdoor, merge_new, iters, events, confidence)


def coarse_stage_mixed(pack, nets, cap, iters=100, if_local=True, crop_format=None):
    """coarse_stage for a MixedPack: the first layer's tail once per shape group (the coarse solvers are chosen by size, so a
    group is one launch set on one grid - bits independent of the batch), its per-cell outputs packed over the slots, then the
    row table and the crops in ONE launch set over the whole batch (ops.chunk_rows_ragged, ops.Compute_imgs_ragged)."""
    ifn1, xs, ys, pts = [], [], [], []
    for lo, hi, h, w, lefts, rights in pack.groups:
        _, p_, x_, y_, f_, _ = _coarse_tail(lefts, rights, nets, iters, 32 * h, 32 * w)
        ifn1.append(f_.reshape(-1))
        xs.append(x_.reshape(-1))
        ys.append(y_.reshape(-1))
        pts.append(p_.reshape(-1))
    one = len(pack.groups) == 1
    ifn1 = ifn1[0] if one else torch.cat(ifn1)
    xs, ys, pts = (xs[0], ys[0], pts[0]) if one else (torch.cat(xs), torch.cat(ys), torch.cat(pts))
    rows = ops.chunk_rows_ragged(ifn1, pack.table, if_local, Cmax=cap.Cmax, rows_cap=cap.rows_cap)
    new_left, new_right, xsn, ysn, avn, bound5, K_img, K_tot = ops.Compute_imgs_ragged(xs, ys, pts, ifn1, pack.left, pack.right,
                                                                                       pack.table, crop_format=crop_format)
    return {"rows": rows, "new_left": new_left, "new_right": new_right, "xsn": xsn, "avn": avn, "K_img": K_img, "ifn1": ifn1,
            "H": None, "W": None}


def forward_pairs_mixed(pack, nets, cap, if_outdoor=True, merge_new=True, iters=100, events=None, crop_format=None,
                        confidence=False):
    """forward_pairs for pairs of different grids (pack_pairs): the coarse level once per shape group, everything from the row
    table on ONE launch set over the whole batch, no host read.  Same result dict, in SLOT order (rows.row_pair = the slot;
    pack.caller_of[slot] = the caller's index); split_by_pair(out, cap) hands the per-pair lists back in the caller's order.
    Every pair's matches are bit-identical to forward_pairs / pipeline.forward_path on that pair alone.  nets.coarse is called
    once per group with its [g, 32h, 32w, 3] views; nets.fine / nets.third find a row's pair through rows.row_pair.
    crop_format, confidence: as for forward_pairs."""
    if cap.pairs != pack.table.pairs or sorted(cap.shapes) != sorted(pack.shapes):
        raise ValueError("forward_pairs_mixed: the capacities were made for other shapes than the pack holds")
    co = coarse_stage_mixed(pack, nets, cap, iters, cap.if_local, crop_format=crop_format)
    out = fine_third_stage(co, nets, cap, if_outdoor, merge_new, iters, events, confidence)
    out["caller_of"] = pack.caller_of
    return out


def group_by_pair(out, cap, buffers=None, confidence=False):
    """Device side of the hand-over: the batch's matches regrouped by pair (ops.matches_by_pair), no host read.  Adds
    `by_pair` = (matches_l, matches_r, pair_off) and `summary` (int64 [pairs + 4]: the pairs + 1 offsets, then M, P, table status -
    everything the host reads of a step, in ONE buffer) to the result; a caller in a loop passes `buffers` (out_l, out_r,
    summary-sized pair_off) to reuse the outputs.
    confidence (or a result that holds match_conf): match_conf is regrouped with the matches, by_pair = (matches_l, matches_r,
    pair_off, conf) and `buffers` may carry conf's destination as a fourth tensor."""
    if confidence and "match_conf" not in out:
        raise ValueError("group_by_pair: confidence=True needs a result made with confidence=True")
    got = ops.matches_by_pair(out["rows"], out["matches_l"], out["matches_r"], out["match_row"], out["M"], out=buffers, P=out["P"],
                              match_conf=out.get("match_conf"))
    out["by_pair"], out["summary"] = got[:3] + got[4:], got[3]          # got = (matches_l, matches_r, pair_off, summary[, conf])
    return out["by_pair"]


# ---- what the hand-over functions below share; a new per-pair stage calls these instead of copying a neighbour ----
def _overflow_check(o, cap):
    """o = the summary's host copy: raises on the capacity overflows of a step."""
    M, P, status = o[cap.pairs + 1:cap.pairs + 4]
    if status & 1:
        raise RuntimeError("pats_amd.batch: a pair needed more than Cmax = %d chunks" % cap.Cmax)
    if status & 2:
        raise RuntimeError("pats_amd.batch: the row table overflowed rows_cap = %d" % cap.rows_cap)
    if P > cap.P_cap:
        raise RuntimeError("pats_amd.batch: %d third-level problems exceed P_cap = %d" % (P, cap.P_cap))


def _read_topk_summary(out, cap):
    """(summary, top_count) of a topk_by_pair result as host lists.  Device-to-host copies: ONE when topk_by_pair did the regroup
    itself (`topk_summary` holds both), TWO otherwise."""
    if "topk_summary" in out:
        o = out["topk_summary"].cpu().tolist()            # the one synchronisation of a batch
        return o[:cap.pairs + 4], o[cap.pairs + 4:]
    return out["summary"].cpu().tolist(), out["topk"][4].cpu().tolist()


def _caller_order(out, cap, per_slot):
    """per_slot in the caller's order (forward_pairs_mixed: slot s holds the caller's pair caller_of[s])."""
    if "caller_of" not in out:
        return per_slot
    per_caller = [None] * cap.pairs
    for s_, i in enumerate(out["caller_of"]):
        per_caller[i] = per_slot[s_]
    return per_caller


def _caller_of_dev(out, dev):
    """caller_of on the device (made once, kept in the result): index_select with it takes caller order to slot order."""
    if "caller_of_dev" not in out:
        out["caller_of_dev"] = torch.tensor(out["caller_of"], dtype=torch.int64, device=dev)
    return out["caller_of_dev"]


def _slot_of_dev(out, cap, dev):
    """The inverse of caller_of on the device (made once, kept in the result): slot order back to caller order."""
    if "slot_of_dev" not in out:
        slot_of = [0] * cap.pairs
        for s_, i in enumerate(out["caller_of"]):
            slot_of[i] = s_
        out["slot_of_dev"] = torch.tensor(slot_of, dtype=torch.int64, device=dev)
    return out["slot_of_dev"]


def _check_on(fn, out, on):
    if on not in ("all", "topk"):
        raise ValueError("%s: on must be \"all\" or \"topk\", got %r" % (fn, on))
    if on == "topk" and "topk" not in out:
        raise ValueError("%s: on=\"topk\" needs a topk_by_pair result" % fn)


def _lists_on(out, cap, on):
    """The lists a device-side stage works on -> (matches_l, matches_r, conf or None, the segment keywords of the ops call):
    "topk" = the rows of the topk_by_pair result, strided; "all" = the regrouped full lists (regrouped here if they are not yet)."""
    if on == "topk":
        tl, tr, tc, _, tn = out["topk"]
        return tl, tr, tc, {"stride": int(tl.shape[1]), "counts": tn}
    if "by_pair" not in out:
        group_by_pair(out, cap)
    bp = out["by_pair"]
    return bp[0], bp[1], bp[3] if len(bp) > 3 else None, {"pair_off": out["summary"], "pairs": cap.pairs}


def split_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (matches_l, matches_r) lists - (matches_l, matches_r, conf) for a result made with
    confidence=True - from a forward_pairs (or forward_pairs_mixed: in the
    caller's order) result, in the reference's order.  Reads the counts back (the one synchronisation of a batch) and raises on a capacity overflow."""
    if "summary" not in out:
        group_by_pair(out, cap)
    o = out["summary"].cpu().tolist()                 # the one synchronisation of a batch: offsets, M, P, status in one copy
    _overflow_check(o, cap)
    lists = out["by_pair"][:2] + out["by_pair"][3:]           # (matches_l, matches_r[, conf]): pair_off left out
    per_slot = [tuple(t[o[p]:o[p + 1]] for t in lists) for p in range(cap.pairs)]
    return _caller_order(out, cap, per_slot)


def _topk_lists(fn, out, cap):
    """What topk_by_pair and topk_spread_by_pair do in front of their launch -> (matches_l, matches_r, conf, top_count's place or
    None): the regrouped lists, regrouped here if they are not yet - then with ONE int64 buffer of (pairs + 4) + pairs entries,
    group_by_pair's summary and behind it top_count's place, kept as `topk_summary`.  None: the caller regrouped on its own."""
    if "match_conf" not in out:
        raise ValueError("%s: needs a result made with confidence=True" % fn)
    top_count = None
    if "by_pair" not in out:
        ml, mr, mc = out["matches_l"], out["matches_r"], out["match_conf"]
        both = torch.empty((2 * cap.pairs + 4,), dtype=torch.int64, device=ml.device)
        group_by_pair(out, cap, buffers=(torch.empty_like(ml), torch.empty_like(mr), both[:cap.pairs + 4], torch.empty_like(mc)))
        out["topk_summary"] = both
    if "topk_summary" in out:                       # still the buffer behind `summary`?  (a regroup of the caller's own since then
        if out["topk_summary"].data_ptr() == out["summary"].data_ptr():             # has its summary elsewhere)
            top_count = out["topk_summary"][cap.pairs + 4:]
        else:
            del out["topk_summary"]
    ml, mr, _, mc = out["by_pair"]
    return ml, mr, mc, top_count


def _topk_dest(cap, K, dev, top_count):
    """topk_by_pair's five destinations around a top_count that lives in `topk_summary`."""
    K = int(K)
    return (torch.empty((cap.pairs, K, 2), dtype=torch.float32, device=dev), torch.empty((cap.pairs, K, 2), dtype=torch.float32, device=dev),
            torch.empty((cap.pairs, K), dtype=torch.float32, device=dev), torch.empty((cap.pairs, K), dtype=torch.int32, device=dev),
            top_count)


def topk_by_pair(out, cap, K, min_conf=None):
    """Device side, after (or instead of) group_by_pair: each pair's K most confident matches (ops.topk_by_pair: one launch over
    all pairs, no host read; confidence descending, ties by the position in the pair's list; min_conf keeps conf >= min_conf).
    Needs a result made with confidence=True.  Adds `topk` = (top_l [pairs,K,2], top_r [pairs,K,2], top_conf [pairs,K],
    top_idx [pairs,K] int32, top_count [pairs] int64) to the result and returns it; rows in SLOT order for a mixed pack
    (split_topk_by_pair hands them back in the caller's).  If the result is not regrouped yet this does it, with ONE int64 buffer
    of (pairs + 4) + pairs entries - group_by_pair's summary, then top_count - kept as `topk_summary`: the whole hand-over is then
    still one device-to-host copy.  After a group_by_pair of the caller's own, top_count is a tensor of its own.  Nothing is
    removed from the full lists: this is a selection by the third level's confidence alone - no mutual check, no suppression."""
    ml, mr, mc, top_count = _topk_lists("topk_by_pair", out, cap)
    dest = None if top_count is None else _topk_dest(cap, K, ml.device, top_count)
    out["topk"] = ops.topk_by_pair(ml, mr, mc, out["summary"], K, min_conf=min_conf, out=dest, pairs=cap.pairs)
    out.pop("topk_spread", None)                    # the rows are no spread selection any more
    return out["topk"]


def _spread_grid(cap, cell):
    """The grid of `cell`-pixel cells over the largest image of the batch, (ceil(32 h / cell), ceil(32 w / cell)) - for mixed shapes
    the largest h and the largest w: smaller pairs leave cells empty.  ValueError if the kernel's table cannot hold it."""
    if int(cell) != cell or not 1 <= cell <= 65536:
        raise ValueError("topk_spread_by_pair: cell = %r must be an integer number of pixels, 1 .. 65536" % (cell,))
    shapes = cap.shapes if hasattr(cap, "shapes") else [(cap.h, cap.w)]
    H, W = 32 * max(h for h, _ in shapes), 32 * max(w for _, w in shapes)

    def grid(c):
        return -(-H // c), -(-W // c)

    g, most = grid(int(cell)), ops.topk_spread_max_cells()
    if g[0] * g[1] > most:
        fits = next(c for c in range(int(cell) + 1, max(H, W) + 1) if grid(c)[0] * grid(c)[1] <= most)      # 1 x 1 at max(H, W)
        raise ValueError("topk_spread_by_pair: cell = %d makes %d x %d cells on %d x %d pixels, more than max_cells = %d; the "
                         "smallest cell that fits is %d" % (cell, g[0], g[1], H, W, most, fits))
    return g


def topk_spread_by_pair(out, cap, K, cell, min_conf=None, side="left"):
    """topk_by_pair's sibling that spreads the selection over the image (ops.topk_spread_by_pair: one launch over all pairs, no host
    read): a grid of `cell`-pixel cells over the `side` ("left" / "right") image, (ceil(32 h / cell), ceil(32 w / cell)) of them for
    the batch's largest h and w; each cell keeps its most confident match with conf >= min_conf, each pair the K most confident of
    these.  Needs a result made with confidence=True and regroups like topk_by_pair (`topk_summary`).  Stores `topk`, the same
    five-tuple in the same order of the rows - split_topk_by_pair and every on="topk" stage work on it unchanged; top_count =
    min(K, occupied) - and `topk_spread` = (occupied [pairs] int64, cell, (grid0, grid1), side); returns `topk`.  A later plain
    topk_by_pair removes `topk_spread`.  Nothing is removed from the full lists.  ValueError for a grid above
    ops.topk_spread_max_cells(): it names the smallest cell that fits."""
    grid = _spread_grid(cap, cell)
    ml, mr, mc, top_count = _topk_lists("topk_spread_by_pair", out, cap)
    dest = None
    if top_count is not None:
        dest = _topk_dest(cap, K, ml.device, top_count) + (torch.empty((cap.pairs,), dtype=torch.int64, device=ml.device),)
    got = ops.topk_spread_by_pair(ml, mr, mc, out["summary"], K, int(cell), grid, side=side, min_conf=min_conf, out=dest, pairs=cap.pairs)
    out["topk"], out["topk_spread"] = got[:5], (got[5], int(cell), grid, side)
    return out["topk"]


def split_topk_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (l [c,2], r [c,2], conf [c], idx [c]) slices of a topk_by_pair result, c = the pair's
    top_count, in the caller's order for a forward_pairs_mixed result.  Raises on the capacity overflows split_by_pair raises on.
    Device-to-host copies: ONE when topk_by_pair did the regroup itself (`topk_summary`: offsets, M, P, status and the counts in
    one buffer), TWO otherwise (`summary`, then top_count)."""
    if "topk" not in out:
        raise ValueError("split_topk_by_pair: run topk_by_pair first")
    tl, tr, tc, ti, _ = out["topk"]
    o, counts = _read_topk_summary(out, cap)
    _overflow_check(o, cap)
    per_slot = [(tl[p, :counts[p]], tr[p, :counts[p]], tc[p, :counts[p]], ti[p, :counts[p]]) for p in range(cap.pairs)]
    return _caller_order(out, cap, per_slot)


def _pair_seeds(out, cap, seed, dev):
    """The generators' per-pair seeds in slot order: pair i of the CALLER's order gets seed + i (int64, wrapping), built on the device
    once per seed and kept in the result as `pair_seed`."""
    seed = ((int(seed) + (1 << 63)) % (1 << 64)) - (1 << 63)              # the int64 the bits of `seed` spell
    if out.get("pair_seed", (None,))[0] != seed:
        ids = _caller_of_dev(out, dev) if "caller_of" in out else torch.arange(cap.pairs, dtype=torch.int64, device=dev)
        out["pair_seed"] = (seed, ids + seed)                             # slot order
    return out["pair_seed"][1]


def _sample_by_pair(fn, generate, out, cap, H, seed, norm, on, progressive, samples):
    """What hypothesize_by_pair, hypothesize5_by_pair and hypothesize7_by_pair share: the order handling, the per-pair seeds (pair i of the CALLER's order
    gets seed + i, built on the device once per seed and kept in the result), the permutation of norm to slot order and of the
    results back to the caller's.  generate = the ops function."""
    _check_on(fn, out, on)
    if progressive is None:
        progressive = on == "topk"
    dev = out["matches_l"].device
    mixed = "caller_of" in out                                            # slot s holds the caller's pair caller_of[s]
    pair_seed = _pair_seeds(out, cap, seed, dev)
    if mixed and norm is not None:
        norm = norm.index_select(0, _caller_of_dev(out, dev))
    ml, mr, _, seg = _lists_on(out, cap, on)
    hyp = generate(ml, mr, H, pair_seed, norm=norm, progressive=progressive, return_samples=samples, **seg)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, dev)
        hyp = tuple(t.index_select(0, back) for t in hyp) if samples else hyp.index_select(0, back)
    return hyp


def hypothesize_by_pair(out, cap, H, seed=0, norm=None, on="topk", progressive=None, samples=False):
    """Device side, after the matching: H 8-point hypotheses per pair (ops.epipolar_hypotheses_by_pair: one launch, no host read) -
    the `models` of verify_by_pair.  on="topk": drawn from the rows of a prior topk_by_pair result (strided form); on="all": from
    the regrouped full lists (regroups first if the result is not grouped yet, as verify_by_pair does).  progressive (default: on ==
    "topk"): hypothesis h draws from the first max(8, ceil(n (h + 1) / H)) matches of the pair's list, the most confident ones of a
    top-K.  seed: a Python int; pair i of the CALLER's order gets pair_seed = seed + i (int64, wrapping), built on the device once
    per seed and kept in the result - a pair's hypotheses do not depend on its slot in a mixed pack.  norm [pairs,8] or None, in the
    caller's order (permuted to slot order on the device, as verify_by_pair does).
    Returns models [pairs,H,3,3] float32 - or (models, sample_idx [pairs,H,8] int32) with samples=True - in the CALLER's order: they
    go straight into verify_by_pair(out, cap, models, thr, norm=norm, on=...).  Adds `hypotheses` (what is returned) to the result;
    the matches, the regrouped lists and a top-K of the same step are not touched."""
    hyp = _sample_by_pair("hypothesize_by_pair", ops.epipolar_hypotheses_by_pair, out, cap, H, seed, norm, on, progressive, samples)
    out["hypotheses"] = hyp
    return hyp


def hypothesize5_by_pair(out, cap, H, seed=0, norm=None, on="topk", progressive=None, samples=False):
    """Device side, after the matching: H 5-point samples per pair, each solved for the up to ten essential matrices through it
    (ops.epipolar_hypotheses5_by_pair: one launch, no host read).  on, progressive (the pool's minimum is 5 here), seed and norm
    exactly as hypothesize_by_pair takes them - and norm must carry the intrinsics: the solver works in calibrated coordinates.
    Returns models [pairs,10*H,3,3] float32 - or (models, sample_idx [pairs,H,5] int32) with samples=True - in the CALLER's order:
    sample h owns rows 10 h .. 10 h + 9, its solutions first, zero models (which verification ignores) behind.  They go straight
    into verify_by_pair(out, cap, models, thr, norm=norm, on=...).  Adds `hypotheses5` (what is returned) to the result;
    `hypotheses`, the matches, the regrouped lists and a top-K of the same step are not touched."""
    hyp = _sample_by_pair("hypothesize5_by_pair", ops.epipolar_hypotheses5_by_pair, out, cap, H, seed, norm, on, progressive, samples)
    flat = (hyp[0] if samples else hyp).flatten(1, 2)                     # [pairs,H,10,3,3] -> [pairs,10 H,3,3]: a view
    hyp = (flat, hyp[1]) if samples else flat
    out["hypotheses5"] = hyp
    return hyp


def hypothesize7_by_pair(out, cap, H, seed=0, norm=None, on="topk", progressive=None, samples=False):
    """Device side, after the matching: H 7-point samples per pair, each solved for the up to three fundamental matrices through
    it (ops.epipolar_hypotheses7_by_pair: one launch, no host read) - the branch of a caller without intrinsics.  on, progressive
    (the pool's minimum is 7 here), seed and norm exactly as hypothesize_by_pair takes them; norm need not carry any calibration.
    Returns models [pairs,H,3,3,3] float32 - or (models, sample_idx [pairs,H,7] int32) with samples=True - in the CALLER's order:
    models.reshape(pairs, -1, 3, 3) goes straight into verify_by_pair(out, cap, ..., thr, norm=norm, on=...), sample h owning rows
    3 h .. 3 h + 2, its solutions first, zero models (which verification ignores) behind.  Adds `hypotheses7` (what is returned) to
    the result; `hypotheses`, `hypotheses5`, the matches, the regrouped lists and a top-K of the same step are not touched."""
    hyp = _sample_by_pair("hypothesize7_by_pair", ops.epipolar_hypotheses7_by_pair, out, cap, H, seed, norm, on, progressive, samples)
    out["hypotheses7"] = hyp
    return hyp


def _verify(fn, score, key, out, cap, models, thr, norm, min_conf, on, adaptive=None, msac=False, first=None, **more):
    """What the verify functions share; score = the ops function, key = "verified" / "verified_h" / "verified_abs".  adaptive: None
    for the fixed budget, else (confidence, sample_size, models_per_sample, round_models) - `key`_used is stored too.  msac: score is
    an MSAC entry - `key` keeps the standard tuple, `key`_gain = (gains, best_gain) and `key`_score = "msac" are stored too.  first:
    the result (`lifted`) whose first entry is scored in the place of matches_l.  more: what else score takes (moments=)."""
    if adaptive is not None:
        confidence, sample_size, models_per_sample, round_models = adaptive
        if not 0.0 < float(confidence) < 1.0:         # false for a NaN; before any device work
            raise ValueError("%s: confidence = %r must lie strictly between 0 and 1" % (fn, confidence))
        if round_models is None:
            round_models = 320 if models_per_sample == 10 else 256
        more.update(confidence=confidence, sample_size=sample_size, models_per_sample=models_per_sample, round_models=round_models)
    _check_on(fn, out, on)
    if min_conf is not None and "match_conf" not in out:
        raise ValueError("%s: min_conf needs a result made with confidence=True" % fn)
    if "caller_of" in out:                            # mixed pack: slot s holds the caller's pair caller_of[s]
        idx = _caller_of_dev(out, models.device)
        models, thr = models.index_select(0, idx), thr.index_select(0, idx)
        norm = None if norm is None else norm.index_select(0, idx)
    ml, mr, conf, seg = _lists_on(out, cap, on)
    res = score(ml if first is None else out[first][0], mr, models, thr, conf=conf if min_conf is not None else None, min_conf=min_conf, norm=norm,
                **more, **seg)
    out[key], out[key + "_on"] = (res[:-2] if adaptive is not None or msac else res), on
    out[key + "_models"] = models                     # slot order: the refit's source when no moments were asked for
    out.pop(key + "_gain", None)                      # a count verification after an MSAC one leaves no stale gains
    out.pop(key + "_score", None)
    if msac:
        out[key + "_gain"], out[key + "_score"] = res[-2:], "msac"
    if adaptive is not None:
        out[key + "_used"] = res[-2:]
    return res


def verify_by_pair(out, cap, models, thr, norm=None, min_conf=None, on="all", moments=False):
    """Device side, after the matching (and after topk_by_pair for on="topk"): every pair's H candidate epipolar models
    (models [pairs,H,3,3], thr [pairs], norm [pairs,8] or None - all float32 GPU tensors in the CALLER's pair order) tested against
    the pair's matches (ops.epipolar_score_by_pair: no host read).  on="all": the regrouped full lists (regroups first if the
    result is not grouped yet, as topk_by_pair does); on="topk": the rows of a prior topk_by_pair result, in strided form.
    min_conf (needs a result made with confidence=True): only matches with conf >= min_conf take part.
    Adds `verified` = (counts [pairs,H] int32, best [pairs] int32, best_count [pairs] int64, inlier uint8 aligned with the lists
    that were scored - [M_cap] for "all", [pairs*K] for "topk" - [, moments [pairs,9,9] float64]) to the result and returns it; rows
    in SLOT order for a mixed pack (models / thr / norm are permuted to it on the device; split_verified_by_pair hands the pairs
    back in the caller's order).  The matches, the regrouped lists and a top-K of the same step are not touched."""
    return _verify("verify_by_pair", ops.epipolar_score_by_pair, "verified", out, cap, models, thr, norm, min_conf, on, moments=moments)


def verify_msac_by_pair(out, cap, models, thr, norm=None, min_conf=None, on="all", moments=False):
    """verify_by_pair with the winner chosen by MSAC gain instead of by count (ops.epipolar_score_msac_by_pair: no host read) - the
    same arguments.  `verified` keeps verify_by_pair's tuple - counts as there; best, best_count, inlier and moments of the MSAC
    winner - so pose_by_pair, polish_by_pair, fundamental_by_pair and split_verified_by_pair work on it unchanged;
    `verified_gain` = (gains [pairs,H] int64, best_gain [pairs] int64; rows in slot order like `verified`'s) and
    `verified_score` = "msac" are added (a later verify_by_pair on the same result removes the two).  Returns the tuple followed by
    gains, best_gain."""
    return _verify("verify_msac_by_pair", ops.epipolar_score_msac_by_pair, "verified", out, cap, models, thr, norm, min_conf, on, msac=True,
                   moments=moments)


def split_verified_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (l [c,2], r [c,2], inlier [c] bool, best, best_count) of a verify_by_pair result - the
    lists that were scored (the pair's full list for on="all", its top_count top-K rows for on="topk") with the best model's inlier
    mask, views of the device tensors; best / best_count are 0-d device views (their values are not read here).  In the caller's
    order for a forward_pairs_mixed result.  Raises on the capacity overflows split_by_pair raises on.  Device-to-host copies: ONE
    (`summary`; for on="topk" `topk_summary` when topk_by_pair did the regroup itself), TWO for on="topk" otherwise."""
    if "verified" not in out:
        raise ValueError("split_verified_by_pair: run verify_by_pair first")
    best, best_count, inl = out["verified"][1:4]
    if out["verified_on"] == "topk":
        tl, tr = out["topk"][:2]
        o, counts = _read_topk_summary(out, cap)
        _overflow_check(o, cap)
        mask = inl.view(cap.pairs, -1)
        per_slot = [(tl[p, :counts[p]], tr[p, :counts[p]], mask[p, :counts[p]].bool(), best[p], best_count[p]) for p in range(cap.pairs)]
    else:
        o = out["summary"].cpu().tolist()                     # the one synchronisation of a batch
        _overflow_check(o, cap)
        ml, mr = out["by_pair"][:2]
        per_slot = [(ml[o[p]:o[p + 1]], mr[o[p]:o[p + 1]], inl[o[p]:o[p + 1]].bool(), best[p], best_count[p]) for p in range(cap.pairs)]
    return _caller_order(out, cap, per_slot)


def pose_by_pair(out, cap, norm=None, swapped=False, front=False):
    """Device side, after verify_by_pair: each pair's relative pose from its verified inliers (ops.epipolar_pose_by_pair: no host
    read) - the refit of `verified`'s moments if the verification produced them, otherwise its winning model; the nearest
    essential matrix, its four decompositions and the cheirality vote over the lists that verification scored ("all" or "topk").
    norm [pairs,8] or None in the CALLER's order - pass what verify_by_pair was given.  swapped: the lists are in the hand-over's
    (y, x) order and the pose is wanted in the reference's (x, y) frame.
    Returns (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64, front_counts [pairs,4] int32,
    choice [pairs] int32) in the CALLER's order - with front=True followed by front (uint8, aligned with the scored lists like
    `verified`'s inlier mask: slot order) - and stores them as `pose`.  E.float() goes straight back into verify_by_pair as an
    H = 1 model: the local-optimisation round, which polish_by_pair runs `rounds` times in one launch, keeping the best."""
    if "verified" not in out:
        raise ValueError("pose_by_pair: run verify_by_pair first")
    ver, on = out["verified"], out["verified_on"]
    best, best_count, inl = ver[1:4]
    mixed = "caller_of" in out
    if mixed and norm is not None:
        norm = norm.index_select(0, _caller_of_dev(out, inl.device))
    src = {"moments": ver[4]} if len(ver) > 4 else {"models": out["verified_models"], "best": best}
    ml, mr, _, seg = _lists_on(out, cap, on)
    res = ops.epipolar_pose_by_pair(ml, mr, inl, best_count, norm=norm, swapped=swapped, return_front=front, **src, **seg)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, inl.device)
        res = tuple(t.index_select(0, back) for t in res[:6]) + tuple(res[6:])
    out["pose"] = res
    return res


def split_pose_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (R [3,3], t [3], E [3,3], front_count) of a pose_by_pair result, views of the device
    tensors (their values are not read here), in the caller's order.  Raises on the capacity overflows split_verified_by_pair
    raises on, after the same device-to-host copies and no further one."""
    if "pose" not in out:
        raise ValueError("split_pose_by_pair: run pose_by_pair first")
    split_verified_by_pair(out, cap)                  # the overflow checks, with the copies that function makes
    E, R, t, front_count = out["pose"][:4]
    return [(R[i], t[i], E[i], front_count[i]) for i in range(cap.pairs)]


def triangulate_by_pair(out, cap, norm=None, swapped=False, max_reproj=None, max_cos=None, mask="front", depths=False, reproj=False,
                        cos=False):
    """Device side, after pose_by_pair: each pair's masked matches triangulated under its pose (ops.epipolar_triangulate_by_pair:
    no host read) - the midpoint of the two rays' common perpendicular in the LEFT camera's frame, over the lists that verification
    scored ("all" or "topk").  mask="front": the matches the pose's cheirality vote kept (needs pose_by_pair(..., front=True));
    mask="inlier": the verification's inliers.  norm [pairs,8] or None, max_reproj / max_cos [pairs] float32 or None, all in the
    CALLER's order - pass the norm that verify_by_pair and pose_by_pair were given, and the swapped that pose_by_pair was given: the
    pose is in the reference's frame only because of it, and the points come back in that frame the same way.  A match is valid only
    with a squared reprojection error <= max_reproj^2 and a cosine of its triangulation angle <= max_cos.
    Returns (points float32 [n,3], valid uint8 [n], tri_count [pairs] int64, reproj_sum [pairs] float64) - followed by depths
    [n,2], reproj [n], cos_parallax [n] (float32) for depths / reproj / cos = True - and stores them as `points`.  tri_count and
    reproj_sum are in the CALLER's order; the per-match outputs are aligned with the scored lists like `verified`'s inlier mask and the
    pose's front (slot order; split_points_by_pair hands the pairs back in the caller's).  `verified`, `pose`, the lists and a top-K
    of the same step are not touched."""
    if "pose" not in out:
        raise ValueError("triangulate_by_pair: run pose_by_pair first")
    if mask not in ("front", "inlier"):
        raise ValueError("triangulate_by_pair: mask must be \"front\" or \"inlier\", got %r" % (mask,))
    pose, on = out["pose"], out["verified_on"]
    if mask == "front" and len(pose) < 7:
        raise ValueError("triangulate_by_pair: mask=\"front\" needs pose_by_pair(..., front=True)")
    used = pose[6] if mask == "front" else out["verified"][3]
    R, t = pose[1], pose[2]
    mixed = "caller_of" in out
    if mixed:                                                             # the pose is in the caller's order: back to slots
        idx = _caller_of_dev(out, used.device)
        R, t = R.index_select(0, idx), t.index_select(0, idx)
        norm, max_reproj, max_cos = (None if v is None else v.index_select(0, idx) for v in (norm, max_reproj, max_cos))
    ml, mr, _, seg = _lists_on(out, cap, on)
    res = ops.epipolar_triangulate_by_pair(ml, mr, used, R, t, norm=norm, swapped=swapped, max_reproj=max_reproj, max_cos=max_cos,
                                           return_depths=depths, return_reproj=reproj, return_cos=cos, **seg)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, used.device)
        res = res[:2] + tuple(v.index_select(0, back) for v in res[2:4]) + tuple(res[4:])
    out["points"] = res
    return res


def split_points_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (X [c,3], valid [c] bool, tri_count, reproj_sum) of a triangulate_by_pair result - the
    points of the lists that were scored (the pair's full list for on="all", its top_count top-K rows for on="topk"), views of the
    device tensors; tri_count / reproj_sum are 0-d device views (their values are not read here).  In the caller's order.  Raises on
    the capacity overflows split_verified_by_pair raises on, after the device-to-host copies that function makes and no further one."""
    if "points" not in out:
        raise ValueError("split_points_by_pair: run triangulate_by_pair first")
    if out["verified_on"] == "topk":                  # (lo, hi) per slot in the flat numbering of the scored lists
        K = int(out["topk"][0].shape[1])
        o, counts = _read_topk_summary(out, cap)
        _overflow_check(o, cap)
        ext = [(p * K, p * K + counts[p]) for p in range(cap.pairs)]
    else:
        o = out["summary"].cpu().tolist()             # the one synchronisation of a batch
        _overflow_check(o, cap)
        ext = [(o[p], o[p + 1]) for p in range(cap.pairs)]
    X, valid, tri_count, reproj_sum = out["points"][:4]
    per_slot = [(X[lo:hi], valid[lo:hi].bool()) for lo, hi in ext]
    return [xv + (tri_count[i], reproj_sum[i]) for i, xv in enumerate(_caller_order(out, cap, per_slot))]


def pose_error_by_pair(out, cap, T1, T0=None, min_matches=15, min_gt_t=0.0, into=None):
    """Device side, after pose_by_pair: each pair's rotation and translation error against the ground truth
    (ops.pose_error_by_pair: one launch, no host read) - the reference's compute_pose_error behind its estimator.  T1 [pairs,4,4]
    float64 holds the ground truth (R_gt | t_gt), or with T0 the two extrinsics (ground truth T1 inv(T0)); both in the CALLER's
    order, like the pose.  The pose must be in the ground truth's frame: for a data set's extrinsics that is
    pose_by_pair(..., swapped=True).  A pair whose FULL regrouped match list (the reference's kp1.shape[0], not a top-K count) is
    shorter than min_matches is not scored: the lengths are the differences of `summary`, taken on the device (the lists are
    regrouped here if they are not yet).
    Returns (err_R, err_t, err [pairs] float64 in degrees, status [pairs] int32) in the CALLER's order and stores them as
    `pose_error`.  into=(buffer, offset): err is written into buffer[offset:offset + pairs] (float64, on the device) and is that
    view - a data set accumulates over its steps and ops.pose_auc(buffer[:total]) is the one aggregate.  `verified`, `pose`,
    `points`, the lists and a top-K of the same step are not touched."""
    if "pose" not in out:
        raise ValueError("pose_error_by_pair: run pose_by_pair first")
    R, t = out["pose"][1], out["pose"][2]
    if "summary" not in out:
        group_by_pair(out, cap)
    off = out["summary"][:cap.pairs + 1]
    counts = off[1:] - off[:-1]                                           # slot order
    if "caller_of" in out:
        counts = counts.index_select(0, _slot_of_dev(out, cap, counts.device))
    dest = None
    if into is not None:
        buf, at = into[0], int(into[1])
        if (not isinstance(buf, torch.Tensor) or not buf.is_cuda or buf.dim() != 1 or not buf.is_contiguous() or buf.dtype != torch.float64
                or at < 0 or at + cap.pairs > buf.numel()):
            raise ValueError("pose_error_by_pair: into must be (contiguous float64 vector on the device, offset) with offset + pairs <= its length")
        f64 = dict(dtype=torch.float64, device=R.device)
        dest = (torch.empty(cap.pairs, **f64), torch.empty(cap.pairs, **f64), buf[at:at + cap.pairs],
                torch.empty(cap.pairs, dtype=torch.int32, device=R.device))
    res = ops.pose_error_by_pair(R, t, T1, T0=T0, counts=counts, min_matches=min_matches, min_gt_t=min_gt_t, out=dest)
    out["pose_error"] = res
    return res


def hypothesize_h_by_pair(out, cap, H, seed=0, norm=None, on="topk", progressive=None, samples=False):
    """Device side, after the matching: H 4-point HOMOGRAPHY hypotheses per pair (ops.homography_hypotheses_by_pair: one launch, no
    host read) - the `models` of verify_h_by_pair, for pairs that look at a plane or whose camera mostly rotates.  on, progressive
    (the pool's minimum is 4 here), seed and norm exactly as hypothesize_by_pair takes them; the same seed gives a pair the same
    generator key in both branches.
    Returns models [pairs,H,3,3] float32 - or (models, sample_idx [pairs,H,4] int32) with samples=True - in the CALLER's order.  Adds
    `hypotheses_h` (what is returned) to the result; `hypotheses`, `hypotheses5`, the matches, the regrouped lists and a top-K of the
    same step are not touched."""
    hyp = _sample_by_pair("hypothesize_h_by_pair", ops.homography_hypotheses_by_pair, out, cap, H, seed, norm, on, progressive, samples)
    out["hypotheses_h"] = hyp
    return hyp


def verify_h_by_pair(out, cap, models, thr, norm=None, min_conf=None, on="all", moments=False):
    """Device side: every pair's H candidate HOMOGRAPHIES (models [pairs,H,3,3], thr [pairs], norm [pairs,8] or None - float32 GPU
    tensors in the CALLER's pair order) tested against the pair's matches by the forward transfer error
    (ops.homography_score_by_pair: no host read).  on and min_conf as verify_by_pair takes them.
    Adds `verified_h` = (counts [pairs,H] int32, best [pairs] int32, best_count [pairs] int64, inlier uint8 aligned with the lists that
    were scored [, moments [pairs,9,9] float64]) to the result and returns it; rows in SLOT order for a mixed pack, as
    `verified`'s.  `verified_h_on` and `verified_h_models` go with it.  `verified` and `pose` are never touched: a caller runs
    both branches on one result and compares best_count of the two - choosing between the models stays with the caller."""
    return _verify("verify_h_by_pair", ops.homography_score_by_pair, "verified_h", out, cap, models, thr, norm, min_conf, on, moments=moments)


def verify_h_msac_by_pair(out, cap, models, thr, norm=None, min_conf=None, on="all", moments=False):
    """verify_h_by_pair with the winner chosen by MSAC gain (ops.homography_score_msac_by_pair), as verify_msac_by_pair is to
    verify_by_pair: `verified_h` keeps the standard tuple for the MSAC winner - homography_by_pair, polish_h_by_pair and
    pose_h_by_pair work on it unchanged -, `verified_h_gain` = (gains, best_gain) and `verified_h_score` = "msac" are added."""
    return _verify("verify_h_msac_by_pair", ops.homography_score_msac_by_pair, "verified_h", out, cap, models, thr, norm, min_conf, on,
                   msac=True, moments=moments)


def homography_by_pair(out, cap, norm=None, swapped=False, pixel=False):
    """Device side, after verify_h_by_pair: each pair's homography refitted to its verified inliers (ops.homography_refit_by_pair:
    one launch, float64, no host read) - the smallest eigenvector of `verified_h`'s moments if the verification produced them,
    otherwise its winning model.  norm [pairs,8] or None in the CALLER's order - pass what verify_h_by_pair was given.  swapped: the
    lists are in the hand-over's (y, x) order and H is wanted in the reference's (x, y) frame.
    Returns (H [pairs,3,3] float64, eig [pairs,2] float64: the two smallest eigenvalues of the moments) in the CALLER's order - with
    pixel=True followed by H_px [pairs,3,3]: the homography of the stored coordinates - and stores them as `homography`.  H.float()
    goes straight back into verify_h_by_pair as an H = 1 model: the local-optimisation round, which polish_h_by_pair runs `rounds`
    times in one launch, keeping the best."""
    if "verified_h" not in out:
        raise ValueError("homography_by_pair: run verify_h_by_pair first")
    ver = out["verified_h"]
    best, best_count = ver[1:3]
    mixed = "caller_of" in out
    if mixed and norm is not None:
        norm = norm.index_select(0, _caller_of_dev(out, best.device))
    src = {"moments": ver[4]} if len(ver) > 4 else {"models": out["verified_h_models"], "best": best}
    res = ops.homography_refit_by_pair(best_count, norm=norm, swapped=swapped, return_pixel=pixel, **src)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, best.device)
        res = tuple(t.index_select(0, back) for t in res)
    out["homography"] = res
    return res


def pose_h_by_pair(out, cap, thr=None, norm=None, swapped=False, front=False, candidates=False, min_baseline=0.0):
    """Device side, after verify_h_by_pair: each pair's pose from its verified homography (ops.homography_pose_by_pair: no host
    read) - the refit of `verified_h`'s moments if the verification produced them, otherwise its winning model, decomposed into its
    four (R, t, n) candidates, one picked by the matches of the lists that verification scored: how many inliers lie on the visible
    side of the plane and - with thr [pairs] float32 - how many matches of the whole list support the candidate's essential matrix
    (the matches off the plane: what resolves the two-fold ambiguity).  thr, norm [pairs,8] in the CALLER's order - pass the norm
    that verify_h_by_pair was given; swapped as pose_by_pair takes it.  min_baseline: a pair with |t| / d at most this only rotates.
    Returns and stores as `pose_h` (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64, vis [pairs,4]
    int32, choice [pairs] int32) in the CALLER's order - with front=True followed by front (uint8, aligned with the scored lists: slot
    order): the layout of `pose`, so triangulate_by_pair, pose_error_by_pair and split_pose_by_pair read it through
    pose_branch(out, "planar").
    `pose_h_extra` = (n [pairs,3], baseline [pairs] float64, sup [pairs,4] int32, status [pairs] int32: 0 no pose, 1 a pose, 2
    rotation only) - with candidates=True followed by cand_R [pairs,2,3,3], cand_t, cand_n [pairs,2,3] - in the CALLER's order.
    `verified`, `pose` and `homography` are not touched."""
    if "verified_h" not in out:
        raise ValueError("pose_h_by_pair: run verify_h_by_pair first")
    ver, on = out["verified_h"], out["verified_h_on"]
    best, best_count, inl = ver[1:4]
    mixed = "caller_of" in out
    if mixed:
        idx = _caller_of_dev(out, inl.device)
        norm, thr = (None if v is None else v.index_select(0, idx) for v in (norm, thr))
    src = {"moments": ver[4]} if len(ver) > 4 else {"models": out["verified_h_models"], "best": best}
    ml, mr, _, seg = _lists_on(out, cap, on)
    res = ops.homography_pose_by_pair(ml, mr, inl, best_count, norm=norm, thr=thr, swapped=swapped, min_baseline=min_baseline,
                                      return_candidates=candidates, return_front=front, **src, **seg)
    per_pair, per_match = res[:13 if candidates else 10], res[13 if candidates else 10:]
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, inl.device)
        per_pair = tuple(t.index_select(0, back) for t in per_pair)
    out["pose_h"] = per_pair[:6] + tuple(per_match)
    out["pose_h_extra"] = per_pair[6:]
    return out["pose_h"]


def select_pose_by_pair(out, cap, ratio=0.8):
    """Device side, after pose_by_pair and pose_h_by_pair on the same lists: each pair's choice between its epipolar and its planar
    pose (ops.pose_select_by_pair: one launch, no host read) - the planar one when it exists and the homography's best_count is at
    least ratio times the epipolar best_count, or when fewer than 8 epipolar inliers leave no other.  ratio: a float, or a [pairs]
    float32 tensor in the CALLER's order.
    Returns and stores as `pose_selected` (E, R, t, front_count, front_counts [pairs,4], choice [pairs]) of the chosen branch in the
    CALLER's order, zeros / the identity for a pair without a pose - followed by front_sel (uint8, slot order) when both poses were made
    with front=True: the layout of `pose`, read by the consumers through pose_branch(out, "selected").  `pose_selected_extra` =
    (branch [pairs] int32 in the CALLER's order: 0 no pose, 1 epipolar, 2 planar, 3 planar and rotation only; inlier_sel uint8, slot
    order: the chosen branch's inlier mask).  `verified_selected` = (None, best, best_count, inlier_sel) of the chosen branch in
    `verified`'s layout and slot order (0 for a pair without a pose).  `verified`, `verified_h`, `pose` and `pose_h` are not touched."""
    if "pose" not in out or "pose_h" not in out:
        raise ValueError("select_pose_by_pair: run pose_by_pair and pose_h_by_pair first")
    if out["verified_on"] != out["verified_h_on"]:
        raise ValueError("select_pose_by_pair: verified_on = %r and verified_h_on = %r: both branches must have scored the same lists"
                         % (out["verified_on"], out["verified_h_on"]))
    pe, ph_, status = out["pose"], out["pose_h"], out["pose_h_extra"][3]
    bce, ie = out["verified"][2:4]
    bch, ih = out["verified_h"][2:4]
    dev = ie.device
    if not isinstance(ratio, torch.Tensor):
        ratio = torch.full((cap.pairs,), float(ratio), dtype=torch.float32, device=dev)
    per_e, per_h = pe[:4], ph_[:4]
    mixed = "caller_of" in out
    if mixed:                                                             # the poses are in the caller's order: back to slots
        idx = _caller_of_dev(out, dev)
        per_e, per_h = (tuple(t.index_select(0, idx) for t in per) for per in (per_e, per_h))
        status, ratio = status.index_select(0, idx), ratio.index_select(0, idx)
    with_front = len(pe) > 6 and len(ph_) > 6
    _, _, _, seg = _lists_on(out, cap, out["verified_on"])
    res = ops.pose_select_by_pair(per_e + ((pe[6],) if with_front else ()), bce, ie, per_h + ((ph_[6],) if with_front else ()), status,
                                  bch, ih, ratio, **seg)
    E, R, t, front_count, branch = res[:5]
    if mixed:
        back = _slot_of_dev(out, cap, dev)
        E, R, t, front_count, branch = (v.index_select(0, back) for v in (E, R, t, front_count, branch))
    planar, none = (branch >= 2), (branch == 0)                           # caller order, like pose[4:6] and pose_h[4:6]
    counts = torch.where(planar[:, None], ph_[4], pe[4]).masked_fill(none[:, None], 0)
    choice = torch.where(planar, ph_[5], pe[5]).masked_fill(none, 0)
    out["pose_selected"] = (E, R, t, front_count, counts, choice) + tuple(res[6:])
    out["pose_selected_extra"] = (branch, res[5])
    planar_s, none_s = res[4] >= 2, res[4] == 0                           # slot order, like the verifications' results
    out["verified_selected"] = (None, torch.where(planar_s, out["verified_h"][1], out["verified"][1]).masked_fill(none_s, 0),
                                torch.where(planar_s, bch, bce).masked_fill(none_s, 0), res[5])
    return out["pose_selected"]


# branch -> (its pose, its verification, the function that makes them, the key of the lists that were scored, the key of its models)
_BRANCHES = {"planar": ("pose_h", "verified_h", "pose_h_by_pair", "verified_h_on", "verified_h_models"),
             "selected": ("pose_selected", "verified_selected", "select_pose_by_pair", "verified_h_on", None),      # both branches scored the same lists
             "absolute": ("pose_abs", "verified_abs", "pose_abs_by_pair", "verified_abs_on", None)}


def pose_branch(out, branch):
    """The result seen through one branch: a shallow copy of `out` whose `pose` and `verified` (with `verified_on` and
    `verified_models`) are those of branch = "epipolar" (as they are), "planar" (`pose_h`, `verified_h`), "selected"
    (`pose_selected`, `verified_selected`) or "absolute" (`pose_abs`, `verified_abs`: the metric pose of pose_abs_by_pair).  Every consumer of a pose - triangulate_by_pair (mask="front": the branch's front,
    "inlier": its inlier mask), pose_error_by_pair, split_pose_by_pair, split_points_by_pair - then works on the view as it stands:
    the poses share one layout, so there is no second code path.  What a consumer stores (`points`, `pose_error`) goes into the
    view; `out` and the default branch's `points` and `pose_error` are never touched (a view does not inherit them either).  The
    tensors are shared, nothing is copied or launched.  Raises ValueError for an unknown branch and for a branch that has not been
    computed."""
    if branch != "epipolar" and branch not in _BRANCHES:
        raise ValueError("pose_branch: branch must be \"epipolar\", \"planar\", \"selected\" or \"absolute\", got %r" % (branch,))
    view = dict(out)
    view.pop("points", None)
    view.pop("pose_error", None)
    if branch == "epipolar":
        if "pose" not in out:
            raise ValueError("pose_branch: branch=\"epipolar\": run pose_by_pair first")
        return view
    pose_key, ver_key, maker, on_key, models_key = _BRANCHES[branch]
    if pose_key not in out:
        raise ValueError("pose_branch: branch=%r: run %s first" % (branch, maker))
    view["pose"], view["verified"] = out[pose_key], out[ver_key]
    view["verified_on"] = out[on_key]
    view["verified_models"] = out[models_key] if models_key else None
    return view


def _polish(fn, polish, key, verify, store, out, cap, thr, rounds, norm, min_conf, moments=True, first=None, **more):
    """What the polish functions share; polish = the ops function, key = "verified" / "verified_h" / "verified_abs", verify = the
    function that makes it, store = the name the walk is stored under.  moments: polish returns them behind the mask (they join the
    new `key`).  first: the result (`lifted`) whose first entry is walked in the place of matches_l.  more: what else polish takes
    (steps=, with a cost behind counts)."""
    if key not in out:
        raise ValueError("%s: run %s first" % (fn, verify))
    if min_conf is not None and "match_conf" not in out:
        raise ValueError("%s: min_conf needs a result made with confidence=True" % fn)
    on, best = out[key + "_on"], out[key][1]
    if "caller_of" in out:                            # mixed pack: slot s holds the caller's pair caller_of[s]
        idx = _caller_of_dev(out, thr.device)
        thr = thr.index_select(0, idx)
        norm = None if norm is None else norm.index_select(0, idx)
    ml, mr, conf, seg = _lists_on(out, cap, on)
    res = polish(ml if first is None else out[first][0], mr, out[key + "_models"], thr, best=best, rounds=rounds,
                 conf=conf if min_conf is not None else None, min_conf=min_conf, norm=norm, **more, **seg)
    model, best_count, inl = res[:3]
    kept = res[3:4] if moments else ()                # the moments stay with the new `key`; behind them best_round, counts[, cost]
    out[store] = (model,) + res[3 + len(kept):]
    out[key] = (best_count.to(torch.int32)[:, None], torch.zeros_like(best), best_count, inl) + kept
    out[key + "_models"] = model[:, None]
    return out[key]


def polish_by_pair(out, cap, thr, rounds=4, norm=None, min_conf=None):
    """Device side, after any of verify_by_pair / verify_adaptive_by_pair: the local optimisation of each pair's winning model
    (ops.epipolar_polish_by_pair: ONE launch for all rounds, no host read) - `rounds` times "refit the inliers, verify the refit" on
    the lists that verification scored (`verified_on`), starting from `verified_models` and its `best`, and the round with the most
    inliers kept (round 0 is the verified winner: the result never has less support).  thr [pairs], norm [pairs,8] or None in the
    CALLER's order and min_conf - pass what the verification was given; they are permuted to slot order on the device as there.
    Stores `polished` = (model [pairs,3,3] float32, best_round [pairs] int32, counts [pairs, rounds + 1] int32) and REPLACES
    `verified` by the standard tuple of the polished model - (counts [pairs,1] int32, best = 0, best_count, inlier, moments) - and
    `verified_models` by model[:, None], all in SLOT order like the verification's: pose_by_pair and split_verified_by_pair work on
    the polished result unchanged and hand the pairs back in the caller's order.  Returns the new `verified`."""
    return _polish("polish_by_pair", ops.epipolar_polish_by_pair, "verified", "verify_by_pair", "polished", out, cap, thr, rounds, norm, min_conf)


def polish_h_by_pair(out, cap, thr, rounds=4, norm=None, min_conf=None):
    """polish_by_pair for the homography branch, after verify_h_by_pair / verify_h_adaptive_by_pair (ops.homography_polish_by_pair):
    stores `polished_h` and replaces `verified_h` and `verified_h_models` - homography_by_pair works on the result unchanged."""
    return _polish("polish_h_by_pair", ops.homography_polish_by_pair, "verified_h", "verify_h_by_pair", "polished_h", out, cap, thr, rounds, norm,
                   min_conf)


def polish_f_by_pair(out, cap, thr, rounds=4, norm=None, min_conf=None):
    """polish_by_pair for uncalibrated callers, after verify_by_pair / verify_adaptive_by_pair (ops.fundamental_polish_by_pair): the
    refit of every round is fundamental_by_pair's rank-2 F instead of the pose's essential matrix.  Stores `polished_f` and replaces
    `verified` and `verified_models` as polish_by_pair does - fundamental_by_pair works on the result unchanged."""
    return _polish("polish_f_by_pair", ops.fundamental_polish_by_pair, "verified", "verify_by_pair", "polished_f", out, cap, thr, rounds, norm,
                   min_conf)


def fundamental_by_pair(out, cap, norm=None, swapped=False, pixel=False):
    """Device side, after verify_by_pair (or polish_f_by_pair): each pair's fundamental matrix from its verified inliers
    (ops.fundamental_refit_by_pair: one launch, float64, no host read) - the smallest eigenvector of `verified`'s moments if the
    verification produced them, otherwise its winning model, truncated to rank 2.  It picks its inputs exactly as pose_by_pair does
    and needs no intrinsics.  norm [pairs,8] or None in the CALLER's order - pass what verify_by_pair was given.  swapped: the lists
    are in the hand-over's (y, x) order and F is wanted in the reference's (x, y) frame.
    Returns (F [pairs,3,3] float64, eig [pairs,2] float64: the two smallest eigenvalues of the moments, sigma [pairs,3] float64: the
    refit's singular values before the truncation) in the CALLER's order - with pixel=True followed by F_px [pairs,3,3]: the
    fundamental matrix of the stored coordinates - and stores them as `fundamental`.  F.float() goes straight back into
    verify_by_pair as an H = 1 model: the local-optimisation round, which polish_f_by_pair runs `rounds` times in one launch."""
    if "verified" not in out:
        raise ValueError("fundamental_by_pair: run verify_by_pair first")
    ver = out["verified"]
    best, best_count = ver[1:3]
    mixed = "caller_of" in out
    if mixed and norm is not None:
        norm = norm.index_select(0, _caller_of_dev(out, best.device))
    src = {"moments": ver[4]} if len(ver) > 4 else {"models": out["verified_models"], "best": best}
    res = ops.fundamental_refit_by_pair(best_count, norm=norm, swapped=swapped, return_pixel=pixel, **src)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, best.device)
        res = tuple(t.index_select(0, back) for t in res)
    out["fundamental"] = res
    return res


def degensac_by_pair(out, cap, H, thr, seed=0, norm=None, parallax=2.0, min_conf=None, on="topk", samples=False):
    """Device side, after verify_by_pair AND verify_h_by_pair (or their local optimisations) on the same lists: the plane-and-parallax
    stage of the uncalibrated branch (DEGENSAC; no host read).  A dominant plane makes the 7-point
    winner a member of a whole family of fundamental matrices; this stage takes the plane `verified_h` found, draws H pairs of
    matches off it (ops.plane_parallax_hypotheses_by_pair: off the plane at parallax * thr), verifies the H models F = [e]x Hp like
    any others (ops.epipolar_score_by_pair, with moments when `verified` has them) and keeps, per pair, whichever of the standing
    and the new verification has more support (ops.plane_parallax_select_by_pair: a tie keeps the standing one).  There is no
    gate: the stage always runs and only support decides.  thr [pairs], norm [pairs,8] or None in the CALLER's order and min_conf -
    pass what the verifications were given -; seed as the hypothesize functions take it (pair i of the caller's order draws with
    seed + i); on must be what both verifications were computed on.
    REPLACES `verified` by the standard tuple of the kept model - (counts [pairs,1] int32, best = 0, best_count, inlier[, moments])
    - and `verified_models` by model[:, None], in SLOT order, exactly the form polish_f_by_pair leaves: polish_f_by_pair,
    fundamental_by_pair and split_verified_by_pair work on the result unchanged.  Stores and returns `degensac` = (replaced [pairs]
    uint8, overlap [pairs] int32: the standing inliers the plane explains at thr - divide by count_before for the degeneracy share -,
    pool [pairs] int32: the matches off the plane, count_before, count_pp [pairs] int64: the support of the standing and of the
    best plane-and-parallax model[, sample_idx [pairs,H,2] int32 with samples=True]) in the CALLER's order.  Apart from the
    generators' `pair_seed` nothing else of the result is touched."""
    fn = "degensac_by_pair"
    if "verified" not in out:
        raise ValueError("%s: run verify_by_pair first" % fn)
    if "verified_h" not in out or "verified_h_models" not in out:
        raise ValueError("%s: run verify_h_by_pair first (the plane)" % fn)
    _check_on(fn, out, on)
    for key in ("verified", "verified_h"):
        if out[key + "_on"] != on:
            raise ValueError("%s: `%s` was computed on=\"%s\", the stage runs on=\"%s\": its mask is not aligned with these lists" %
                             (fn, key, out[key + "_on"], on))
    if min_conf is not None and "match_conf" not in out:
        raise ValueError("%s: min_conf needs a result made with confidence=True" % fn)
    ver, plane = out["verified"], out["verified_h"]
    dev = ver[1].device
    mixed = "caller_of" in out                            # slot s holds the caller's pair caller_of[s]
    pair_seed = _pair_seeds(out, cap, seed, dev)
    if mixed:
        idx = _caller_of_dev(out, dev)
        thr = thr.index_select(0, idx)
        norm = None if norm is None else norm.index_select(0, idx)
    ml, mr, conf, seg = _lists_on(out, cap, on)
    hyp = ops.plane_parallax_hypotheses_by_pair(ml, mr, H, pair_seed, out["verified_h_models"], plane[1], thr, norm=norm, parallax=parallax,
                                                return_samples=samples, **seg)
    with_moments = len(ver) > 4
    new = ops.epipolar_score_by_pair(ml, mr, hyp[0], thr, conf=conf if min_conf is not None else None, min_conf=min_conf, norm=norm,
                                     moments=with_moments, **seg)
    standing = (out["verified_models"], ver[1], ver[2], ver[3]) + tuple(ver[4:5])
    sel = ops.plane_parallax_select_by_pair(ml, mr, thr, out["verified_h_models"], plane[1], standing, (hyp[0],) + tuple(new[1:]), norm=norm,
                                            **seg)
    model, best_count, inl = sel[:3]
    out["verified"] = (best_count.to(torch.int32)[:, None], torch.zeros_like(ver[1]), best_count, inl) + tuple(sel[3:4] if with_moments else ())
    out["verified_models"] = model[:, None]
    res = (sel[-2], sel[-1], hyp[1], ver[2], new[2]) + tuple(hyp[2:3])
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, dev)
        res = tuple(t.index_select(0, back) for t in res)
    out["degensac"] = res
    return res


def verify_adaptive_by_pair(out, cap, models, thr, confidence, sample_size, models_per_sample=1, round_models=None, norm=None,
                            min_conf=None, on="all", moments=False):
    """verify_by_pair that stops each pair at a RANSAC confidence, on the device (ops.epipolar_score_adaptive_by_pair: no host
    read): the pair's models are tested in rounds of round_models (None: 320 with models_per_sample == 10, else 256) and a pair
    stops once (1 - w^sample_size)^(models seen // models_per_sample) <= 1 - confidence, w = its best inlier ratio so far.
    sample_size = 8 for hypothesize_by_pair's models, 5 with models_per_sample = 10 for hypothesize5_by_pair's.  Everything else -
    the caller's pair order, the slot order of a mixed pack, on, min_conf - as verify_by_pair.
    Stores verify_by_pair's tuple as `verified` (with `verified_on`, `verified_models`): pose_by_pair and split_verified_by_pair
    work on it unchanged; counts are 0 from used[p] on.  Also stores `verified_used` = (used [pairs] int32, participating [pairs]
    int32) and returns the tuple followed by those two, in SLOT order like counts.  A confidence outside (0, 1) raises ValueError."""
    return _verify("verify_adaptive_by_pair", ops.epipolar_score_adaptive_by_pair, "verified", out, cap, models, thr, norm, min_conf, on,
                   adaptive=(confidence, sample_size, models_per_sample, round_models), moments=moments)


def verify_h_adaptive_by_pair(out, cap, models, thr, confidence, sample_size, models_per_sample=1, round_models=None, norm=None,
                              min_conf=None, on="all", moments=False):
    """verify_h_by_pair with the stopping rule of verify_adaptive_by_pair (ops.homography_score_adaptive_by_pair); sample_size = 4
    for hypothesize_h_by_pair's models.  Stores `verified_h` (with `verified_h_on`, `verified_h_models`: homography_by_pair works
    on it unchanged) and `verified_h_used` = (used, participating); returns the tuple followed by those two."""
    return _verify("verify_h_adaptive_by_pair", ops.homography_score_adaptive_by_pair, "verified_h", out, cap, models, thr, norm, min_conf,
                   on, adaptive=(confidence, sample_size, models_per_sample, round_models), moments=moments)


# ---- the absolute-pose branch: lift through depth, P3P, reprojection verification, the metric pose ----
def lift_by_pair(out, cap, depths, norm, on="topk", interp="nearest", max_depth=None, max_jump=None):
    """Device side, after the matching (and after topk_by_pair for on="topk"): each pair's LEFT matches lifted through the left
    image's depth map to metric 3-D points (ops.lift_by_pair: one launch, no host read).  depths: one float32 GPU tensor [h, w] per
    pair (or None), of any sizes, each its own tensor, possibly a strided view - in the CALLER's order, like norm [pairs,8] (or None:
    the points stay in pixels) and max_depth [pairs] float32 (or None); for a mixed pack the table of addresses is permuted to slot
    order on the device.  The map must be sampled where the matches live: axis 0 belongs to the stored component 0 (y), the centre of
    pixel (i, j) lies at (i, j) - the depth of the prepared left image, at its resolution.  interp "nearest" or "bilinear"; max_jump
    (bilinear): a match whose taps differ by more than max_jump times the smallest one lies on a depth edge and is invalid.
    Stores `lifted` = (points [n,3] float32, valid [n] uint8, lift_count [pairs] int64, on) and returns it: the per-match outputs are
    aligned with the lists (slot order, like `verified`'s inlier mask), lift_count is in the CALLER's order.  `verified`, `pose` and
    the lists are not touched."""
    fn = "lift_by_pair"
    _check_on(fn, out, on)
    if interp not in ("nearest", "bilinear"):
        raise ValueError("%s: interp must be \"nearest\" or \"bilinear\", got %r" % (fn, interp))
    if not isinstance(depths, (list, tuple)) or len(depths) != cap.pairs:
        raise ValueError("%s: depths must be a list of %d maps, one per pair, got %s" %
                         (fn, cap.pairs, len(depths) if isinstance(depths, (list, tuple)) else type(depths).__name__))
    for i, d in enumerate(depths):
        if d is not None and (not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.dim() != 2):
            raise ValueError("%s: depths[%d] must be a float32 [h, w] tensor or None, got %s" %
                             (fn, i, "%s %s" % (d.dtype, list(d.shape)) if isinstance(d, torch.Tensor) else type(d).__name__))
    ml, _, _, seg = _lists_on(out, cap, on)
    table = ops.lift_table(depths, device=ml.device)
    tab = table.dev
    mixed = "caller_of" in out
    if mixed:                                                             # caller order -> slot order
        idx = _caller_of_dev(out, ml.device)
        tab = tab.index_select(0, idx)
        norm, max_depth = (None if v is None else v.index_select(0, idx) for v in (norm, max_depth))
    points, valid, lift_count = ops.lift_by_pair(ml, None, norm=norm, max_depth=max_depth, interp=interp, max_jump=max_jump, table=tab, **seg)
    if mixed:
        lift_count = lift_count.index_select(0, _slot_of_dev(out, cap, ml.device))
    out["lifted"], out["lifted_table"] = (points, valid, lift_count, on), table       # the table keeps the maps alive
    return out["lifted"]


def _need_lifted(fn, out):
    if "lifted" not in out:
        raise ValueError("%s: run lift_by_pair first" % fn)
    return out["lifted"]


def hypothesize_p3p_by_pair(out, cap, H, seed=0, norm=None, progressive=None, samples=False):
    """Device side, after lift_by_pair: H 3-point samples per pair over the lists that were lifted, each solved for the up to four
    absolute poses of the RIGHT camera (ops.absolute_hypotheses_by_pair: one launch, no host read).  seed, progressive (default: the
    lift was on="topk"; the pool's minimum is 3) and norm - whose right half normalises the right points: pass what lift_by_pair was
    given - exactly as hypothesize_by_pair takes them.  A sample that holds an invalid lift gives no model: the share of such samples
    is 1 - (lift_count / n)^3.
    Returns models [pairs,4*H,3,4] float32, a view - or (models, sample_idx [pairs,H,3] int32) with samples=True - in the CALLER's
    order: sample h owns rows 4 h .. 4 h + 3, its solutions first, zero models (which verification ignores) behind.  They go
    straight into verify_abs_by_pair.  Adds `hypotheses_p3p` (what is returned) to the result."""
    fn = "hypothesize_p3p_by_pair"
    points, _, _, on = _need_lifted(fn, out)

    def generate(ml, mr, H, pair_seed, **kw):
        return ops.absolute_hypotheses_by_pair(points, mr, H, pair_seed, **kw)

    hyp = _sample_by_pair(fn, generate, out, cap, H, seed, norm, on, progressive, samples)
    flat = (hyp[0] if samples else hyp).flatten(1, 2)                     # [pairs,H,4,3,4] -> [pairs,4 H,3,4]: a view
    hyp = (flat, hyp[1]) if samples else flat
    out["hypotheses_p3p"] = hyp
    return hyp


def verify_abs_by_pair(out, cap, models, thr, norm=None, min_conf=None):
    """Device side, after lift_by_pair: every pair's M candidate absolute poses (models [pairs,M,3,4] float32, thr [pairs] in
    normalised units, norm [pairs,8] or None - GPU tensors in the CALLER's order) tested by reprojection against the lifted matches
    (ops.absolute_score_by_pair: no host read), over the lists that were lifted.  min_conf needs a result made with confidence=True.
    Stores `verified_abs` = (counts [pairs,M] int32, best [pairs] int32, best_count [pairs] int64, inlier uint8 aligned with the
    lists) - rows in SLOT order for a mixed pack, like `verified` -, `verified_abs_on` and `verified_abs_models`, and returns the
    tuple.  `verified`, `verified_h` and `pose` are never touched."""
    fn = "verify_abs_by_pair"
    on = _need_lifted(fn, out)[3]
    return _verify(fn, ops.absolute_score_by_pair, "verified_abs", out, cap, models, thr, norm, min_conf, on, first="lifted")


def polish_abs_by_pair(out, cap, thr, rounds=4, steps=3, norm=None, min_conf=None):
    """Device side, after verify_abs_by_pair: the local optimisation of each pair's winning absolute pose
    (ops.absolute_polish_by_pair: ONE launch for all rounds, no host read) - `rounds` times "refit the pose on its inliers by `steps`
    Gauss-Newton steps on the reprojection error, verify the refit" on the lifted lists that verification scored, starting from
    `verified_abs_models` and its `best`, the best round kept (round 0 is the verified winner: the result never has less support).
    thr [pairs], norm [pairs,8] or None in the CALLER's order and min_conf - pass what verify_abs_by_pair was given; they are permuted
    to slot order on the device as there.
    Stores `polished_abs` = (model [pairs,3,4] float32, best_round [pairs] int32, counts [pairs, rounds + 1] int32, cost
    [pairs, rounds + 1] float64) and REPLACES `verified_abs` by the standard tuple of the polished model - (counts [pairs,1] int32,
    best = 0, best_count, inlier) - and `verified_abs_models` by model[:, None], all in SLOT order like the verification's:
    pose_abs_by_pair and pose_branch(out, "absolute") work on the polished result unchanged and hand the pairs back in the caller's
    order.  `verified`, `verified_h`, `pose` and `lifted` are never touched.  Returns the new `verified_abs`."""
    return _polish("polish_abs_by_pair", ops.absolute_polish_by_pair, "verified_abs", "verify_abs_by_pair", "polished_abs", out, cap, thr, rounds,
                   norm, min_conf, moments=False, first="lifted", steps=steps)


def pose_abs_by_pair(out, cap, swapped=False):
    """Device side, after verify_abs_by_pair: each pair's METRIC pose - the winning P3P model widened exactly to float64 (index
    operations on the device, no host read, no refit).  swapped: the lists are in the hand-over's (y, x) order and the pose is wanted
    in the reference's (x, y) frame: R -> P R P, t -> P t, as pose_by_pair does.  E = [t]_x R scaled to |E|_F = 1.  A pair without an
    inlier has no pose: E, R and t are zero (what every consumer reads as "no pose").
    Stores `pose_abs` in the standard pose layout - (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64 =
    best_count, counts [pairs,4] int32 = (best_count, 0, 0, 0), choice [pairs] int32 = 0) in the CALLER's order, then front = the
    winner's inlier mask (slot order) - and returns it; batch.pose_branch(out, "absolute") is the view every consumer of a pose
    works on.  `pose`, `verified` and `verified_h` are never touched."""
    if "verified_abs" not in out:
        raise ValueError("pose_abs_by_pair: run verify_abs_by_pair first")
    _, best, best_count, inlier = out["verified_abs"]
    models = out["verified_abs_models"]                                   # slot order
    pairs, M = int(models.shape[0]), int(models.shape[1])
    rows = torch.arange(pairs, device=models.device)
    win = models[rows, best.long().clamp(0, M - 1)].double()              # [pairs,3,4]: exact
    none = (best_count <= 0).view(pairs, 1, 1)
    R, t = win[:, :, :3].masked_fill(none, 0.0), win[:, :, 3].masked_fill(none.view(pairs, 1), 0.0)
    if swapped:
        perm = torch.tensor([1, 0, 2], device=models.device)
        R, t = R.index_select(1, perm).index_select(2, perm), t.index_select(1, perm)
    E = torch.linalg.cross(t.unsqueeze(2).expand(-1, -1, 3), R, dim=1)     # column j = t x R[:, j]: [t]_x R, element-wise work only
    nrm = E.flatten(1).norm(dim=1).view(pairs, 1, 1)
    E = torch.where(nrm > 0, E / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(E))
    counts = torch.zeros((pairs, 4), dtype=torch.int32, device=models.device)
    counts[:, 0] = best_count.to(torch.int32)
    res = (E, R.contiguous(), t.contiguous(), best_count.clone(), counts, torch.zeros(pairs, dtype=torch.int32, device=models.device))
    if "caller_of" in out:                                                # slots back to the caller's order
        back = _slot_of_dev(out, cap, models.device)
        res = tuple(v.index_select(0, back) for v in res)
    out["pose_abs"] = res + (inlier,)
    return out["pose_abs"]


# ---- the match-level yardstick: the lifted matches against depth-and-pose ground truth ----
_MATCH_ERROR_MASKS = ("verified", "verified_abs", "verified_h")


def match_error_by_pair(out, cap, T1, T0=None, thr=(1.0, 3.0, 5.0), norm=None, swapped=False, depths_r=None, occl_rel=0.2, size_r=None,
                        min_conf=None, edges=None, mask=None):
    """Device side, after lift_by_pair: every match of the lists that were lifted scored against the ground truth
    (ops.match_error_by_pair: one launch, no host read) - the lifted point carried through the ground-truth pose into the right image,
    err = the distance of the matched right point from it in pixels.  T1 [pairs,4,4] float64 (with T0: the two extrinsics, ground
    truth T1 inv(T0)) as pose_error_by_pair takes them, swapped=True for a data set's extrinsics; norm [pairs,8] - pass what
    lift_by_pair was given -, size_r [pairs,2] float32 (the right images' content) and depths_r (one float32 [h, w] GPU map or None per
    pair: the RIGHT images' depth, for the covisibility test within occl_rel) - all in the CALLER's order; for a mixed pack they are
    permuted to slot order on the device.  thr: ascending pixel thresholds; edges: ascending confidence floors for the sweep and
    min_conf: the gate (both need a result made with confidence=True).  mask: "verified", "verified_abs" or "verified_h" - that
    verification's inlier mask, which must have been computed on the lists that were lifted - or None.
    Stores `match_error` = (err float64, status uint8 - aligned with the lists: slot order, like `lifted` -, tally [pairs,8],
    correct [pairs,n_thr] int64, err_sum [pairs] float64, sweep [pairs,B,1+n_thr] int64 or None, confusion [pairs,4] int64 or None -
    in the CALLER's order) and returns it.  No other entry of the result is touched."""
    fn = "match_error_by_pair"
    if "lifted" not in out:
        raise ValueError("%s: run lift_by_pair first" % fn)
    points, _, _, on = out["lifted"]
    if mask is not None:
        if mask not in _MATCH_ERROR_MASKS:
            raise ValueError("%s: mask must be one of %s or None, got %r" % (fn, ", ".join("\"%s\"" % m for m in _MATCH_ERROR_MASKS), mask))
        if mask not in out:
            raise ValueError("%s: mask=\"%s\" needs that verification's result" % (fn, mask))
        if out[mask + "_on"] != on:
            raise ValueError("%s: `%s` was computed on=\"%s\", the lift on=\"%s\": the mask is not aligned with the lifted lists" %
                             (fn, mask, out[mask + "_on"], on))
    if (min_conf is not None or edges is not None) and "match_conf" not in out:
        raise ValueError("%s: min_conf and edges need a result made with confidence=True" % fn)
    if depths_r is not None and (not isinstance(depths_r, (list, tuple)) or len(depths_r) != cap.pairs):
        raise ValueError("%s: depths_r must be a list of %d maps, one per pair" % (fn, cap.pairs))
    _, mr, conf, seg = _lists_on(out, cap, on)
    dev = points.device
    tab = None if depths_r is None else ops.lift_table(depths_r, device=dev)          # keeps the maps alive until the call returns
    tab_dev = None if tab is None else tab.dev
    mixed = "caller_of" in out
    if mixed:                                                             # caller order -> slot order
        idx = _caller_of_dev(out, dev)
        T1, T0, norm, size_r, tab_dev = (None if v is None else v.index_select(0, idx) for v in (T1, T0, norm, size_r, tab_dev))
    res = ops.match_error_by_pair(points, mr, T1, T0=T0, thr=thr, norm=norm, swapped=swapped, table_r=tab_dev, occl_rel=occl_rel, size_r=size_r,
                                  conf=conf if (min_conf is not None or edges is not None) else None, min_conf=min_conf, edges=edges,
                                  mask=None if mask is None else out[mask][3], **seg)
    if mixed:                                                             # slots back to the caller's order
        back = _slot_of_dev(out, cap, dev)
        res = res[:2] + tuple(None if v is None else v.index_select(0, back) for v in res[2:])
    out["match_error"] = res
    return res


def split_match_error_by_pair(out, cap):
    """Host side, AFTER the step: per-pair (err [c] float64, status [c] uint8, tally [8], correct [n_thr], err_sum) of a
    match_error_by_pair result - the rows of the lists that were lifted (the pair's full list for on="all", its top_count top-K rows
    for on="topk"), views of the device tensors (their values are not read here), in the caller's order.  Raises on the capacity
    overflows split_by_pair raises on, after the device-to-host copies split_verified_by_pair makes and no further one."""
    if "match_error" not in out:
        raise ValueError("split_match_error_by_pair: run match_error_by_pair first")
    err, status, tally, correct, err_sum = out["match_error"][:5]
    if out["lifted"][3] == "topk":                    # (lo, hi) per slot in the flat numbering of the lifted lists
        K = int(out["topk"][0].shape[1])
        o, counts = _read_topk_summary(out, cap)
        _overflow_check(o, cap)
        ext = [(p * K, p * K + counts[p]) for p in range(cap.pairs)]
    else:
        o = out["summary"].cpu().tolist()             # the one synchronisation of a batch
        _overflow_check(o, cap)
        ext = [(o[p], o[p + 1]) for p in range(cap.pairs)]
    per_slot = [(err[lo:hi], status[lo:hi]) for lo, hi in ext]
    return [es + (tally[i], correct[i], err_sum[i]) for i, es in enumerate(_caller_order(out, cap, per_slot))]
