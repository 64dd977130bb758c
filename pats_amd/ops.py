"""Host-side mirror of the reference's operator surface for the OT hot path.

Same names, positional arguments, dtypes and return shapes as the reference's Python functions, so
the parity tests read like the reference's own call sites; each function is a thin shim that
hands raw device pointers to the C-ABI of include/pats_amd.h (libpats_amd.so, hand-written HIP for
gfx950).  PyTorch is used for device memory and streams only.  Tensors must live on a HIP device
("cuda" in torch-ROCm); there is no CPU path and no fallback.

Reference call sites (paths relative to zju3dv/pats):
  log_sinkhorn_iterations / log_optimal_transport / log_optimal_transport2   models/modules.py:137-182
  cost (einsum + scale)            models/first_layer.py:110-114 second_layer.py:100-104 third_layer.py:156-158
  Compute_positions_and_ranges     utils/utils.py:1527-1537
  Iterative_expand_matrix          utils/utils.py:1179-1297
  est_position (first / second)    models/first_layer.py:159-178  models/second_layer.py:240-259
  split_patches                    utils/utils.py:152-181
  Compute_imgs / tensor_resize     utils/utils.py:1343-1393  setup/library.cpp:47-66
  Compute_result / third label     models/third_layer.py:161-170,184-217
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

_L = _lib.lib
_check = _lib.check
_L()   # load libpats_amd.so at import: a missing HIP extension fails here, loudly


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's current HIP stream as the C-ABI's pats_stream_t.  (torch.cuda.current_stream() builds a Stream object per call:
    9 us each, 0.8 ms of a pair walked chunk by chunk; the raw getter is what torch's own extensions use.)"""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("pats_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)"
                           % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("pats_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    return t.contiguous()


def _map(t, name, dtype=torch.float32):
    """A [B,C,H,W] feature map in either memory format -> (tensor whose storage a kernel can walk, channels_last?).
    A torch.channels_last tensor is used AS IT LIES (the channels-last gathers read it in full 64-byte granules);
    anything else is made NCHW-contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("pats_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("pats_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last):
        return t, True
    return t.contiguous(), False


# element types the descriptor gathers take their maps in (include/pats_amd.h pats_map_dtype_t)
_MAP_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _maps_any(tensors, names):
    """The maps of ONE gather call in float32, float16 or bfloat16 -> (maps as _map returns them, pats_map_dtype_t code).
    Half maps are widened to fp32 exactly in the kernels; the cases those kernels do not take fall back to .float() copies,
    which give the same bits: maps of different dtypes in one call, mixed memory formats, and data pointers off the kernels'
    alignment (4 bytes NCHW, 16 bytes channels-last)."""
    for t, name in zip(tensors, names):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype not in _MAP_DTYPES:
            raise RuntimeError("pats_amd: %s must be float32, float16 or bfloat16, got %s" % (name, t.dtype))
    dtypes = {t.dtype for t in tensors}
    if dtypes == {torch.float32}:
        return [_map(t, n) for t, n in zip(tensors, names)], _MAP_DTYPES[torch.float32]
    if len(dtypes) != 1:
        return [_map(t.float(), n) for t, n in zip(tensors, names)], _MAP_DTYPES[torch.float32]
    dt = tensors[0].dtype
    maps = [_map(t, n, dt) for t, n in zip(tensors, names)]
    if len({cl for _, cl in maps}) != 1:
        maps = [(t.contiguous(), False) for t, _ in maps]
    align = 16 if maps[0][1] else 4
    if any(t.data_ptr() % align for t, _ in maps):
        return [_map(t.float(), n) for t, n in zip(tensors, names)], _MAP_DTYPES[torch.float32]
    return maps, _MAP_DTYPES[dt]


def _descs_any(tensors, names):
    """The two descriptor sets of ONE cost / cost_ot / third_level call in float32, float16 or bfloat16 -> (contiguous tensors,
    pats_map_dtype_t code).  Both sets in the same half dtype go to the typed entry points as they lie: the cost builds widen
    every element to fp32 exactly at the load, so every output has the bits of the same call on .float() copies.  Two different
    dtypes in one call, or a data pointer off the element size (all the kernels' loads need), fall back to .float() copies and
    the fp32 entry: same bits."""
    for t, name in zip(tensors, names):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype not in _MAP_DTYPES:
            raise RuntimeError("pats_amd: %s must be float32, float16 or bfloat16, got %s" % (name, t.dtype))
    dtypes = {t.dtype for t in tensors}
    if len(dtypes) == 1 and torch.float32 not in dtypes:
        dt = tensors[0].dtype
        descs = [_dev(t, n, dt) for t, n in zip(tensors, names)]
        if not any(t.data_ptr() % t.element_size() for t in descs):
            return descs, _MAP_DTYPES[dt]
    return [_dev(t.float(), n) for t, n in zip(tensors, names)], _MAP_DTYPES[torch.float32]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_WS = {}
_WS_MAX = 64 << 20
_WS_ON = [False]


class workspace_cache:
    """Context: inside it the scratch block of a C call (up to 64 MB) is kept per (device, stream) and shared by consecutive
    calls instead of being allocated per call - the calls of a stream run in order and none reads its scratch after it returns.
    pipeline.forward_chunks_device uses it (a pair walked chunk by chunk made 300 allocator calls, a third of them these).
    Off by default: it is a host-side saving for many small calls on few streams; the throughput path (big tensors, their own
    allocations) keeps the allocator.  (profiles/r06_ws_cache_ab.txt: an apparent 4x cost to bench.py's masked-stream leg turned
    out to be a first-process-on-the-box effect, not the cache.)"""

    def __enter__(self):
        self.prev = _WS_ON[0]
        _WS_ON[0] = True

    def __exit__(self, *exc):
        _WS_ON[0] = self.prev


def _workspace(nbytes, device):
    """Scratch for ONE C call on the current stream (see workspace_cache)."""
    n = max(int(nbytes), 1)
    if not _WS_ON[0] or n > _WS_MAX or _raw_stream is None or torch.cuda.is_current_stream_capturing():
        return torch.empty(n, dtype=torch.uint8, device=device)
    key = (device.index, _raw_stream(torch.cuda.current_device()))
    t = _WS.get(key)
    if t is None or t.numel() < n:
        t = _WS[key] = torch.empty(min(_WS_MAX, max(2 * n, 1 << 20)), dtype=torch.uint8, device=device)
    return t


def _scalar_dev(x, device):
    """0-d tensor / python float -> device float32[1] without a device sync."""
    if isinstance(x, torch.Tensor):
        return x.detach().reshape(1).to(device=device, dtype=torch.float32)
    return torch.full((1,), float(x), dtype=torch.float32, device=device)


def set_sinkhorn_mode(mode):
    """'auto' | 'log' | 'kernel' (include/pats_amd.h PATS_SINKHORN_*). Returns the previous mode."""
    names = {"auto": 0, "log": 1, "kernel": 2}
    prev = _L().pats_set_sinkhorn_mode(names[mode])
    return {v: k for k, v in names.items()}[prev]


def set_fine_fused(on):
    """Fine level of cost_ot (variant 2, 145 x 145): True = the fused cost -> OT kernel (no score matrix in HBM), False (default)
    = MFMA cost kernel + Sinkhorn kernel.  Same bits; returns the previous setting."""
    return bool(_L().pats_set_fine_fused(1 if on else 0))


def set_third_gather(mode):
    """Kernel of the fp32 third-level gather on NCHW maps: "tile" (default, third_desc_kernel: a tile of neighbouring points per
    workgroup) or "point" (third_desc_point_kernel: one point per workgroup).  Same bits; returns the previous setting."""
    modes = {"tile": 0, "point": 1}
    if mode not in modes:
        raise ValueError("set_third_gather: mode must be 'tile' or 'point'")
    prev = _L().pats_set_third_gather(modes[mode])
    return {v: k for k, v in modes.items()}.get(prev, "tile")


def sinkhorn_fallbacks(reset=True):
    """Problems on the current device whose linear-domain solve left the guard band and were redone
    with log-sum-exp sweeps since the last reset (pats_sinkhorn_fallbacks; synchronises)."""
    import ctypes
    n = ctypes.c_int64(0)
    rc = _L().pats_sinkhorn_fallbacks(ctypes.byref(n), 1 if reset else 0)
    if rc != 0:
        raise RuntimeError(_L().pats_last_error().decode())
    return int(n.value)


def sinkhorn_tail_solves(reset=True):
    """Of sinkhorn_fallbacks(), the 145 x 145 problems whose stabilised linear re-solve failed its guard as well and ended in the
    log-sum-exp sweeps of the same launch, and the third level's 65 x 65 problems whose stabilised re-solve bailed out to the
    log-sum-exp kernel (pats_sinkhorn_tail_solves; synchronises; a counter of its own)."""
    n = ctypes.c_int64(0)
    _check(_L().pats_sinkhorn_tail_solves(ctypes.byref(n), 1 if reset else 0), "sinkhorn_tail_solves")
    return int(n.value)


def set_gnn_redo(mode):
    """'inline' (default) | 'deferred' (include/pats_amd.h pats_set_gnn_redo_mode): in deferred mode the GNN layers queue no gated
    fp32 redo chain; an activation beyond the fp16 range raises a sticky device flag instead and the outputs of that call are not
    valid - read gnn_overflows() where you synchronise anyway and repeat the work under 'inline' if it says True.  Returns the
    previous mode."""
    names = {"inline": 0, "deferred": 1}
    prev = _L().pats_set_gnn_redo_mode(names[mode])
    return {v: k for k, v in names.items()}[prev]


def gnn_overflows(reset=True):
    """True if a GNN layer launched under set_gnn_redo('deferred') on the current device left the fp16 range since the last reset
    (pats_gnn_overflows; synchronises)."""
    n = ctypes.c_int64(0)
    _check(_L().pats_gnn_overflows(ctypes.byref(n), 1 if reset else 0), "gnn_overflows")
    return bool(n.value)


# ------------------------------------------------------------------------------------------------
# cost build
# ------------------------------------------------------------------------------------------------
def cost(mdesc0, mdesc1, out=None):
    """0.1 * (einsum('bdn,bdm->bnm', mdesc0, mdesc1) / D**.5)   (first_layer.py:110-114).
    out: optional preallocated [b, n, m] float32 result (as torch's `out=`).
    mdesc0 / mdesc1: float32, float16 or bfloat16 (see _descs_any); the result is float32 with the bits of the call on
    .float() copies."""
    (d0, d1), code = _descs_any([mdesc0, mdesc1], ["mdesc0", "mdesc1"])
    b, D, n = d0.shape
    if d1.shape[0] != b or d1.shape[1] != D:
        raise RuntimeError("cost: descriptor shapes %s / %s do not match" % (tuple(d0.shape), tuple(d1.shape)))
    m = d1.shape[2]
    if out is None:
        out = torch.empty((b, n, m), dtype=torch.float32, device=d0.device)
    elif tuple(out.shape) != (b, n, m) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != d0.device:
        raise RuntimeError("cost: out must be a contiguous float32 [%d, %d, %d] tensor on %s" % (b, n, m, d0.device))
    if code:
        _check(_L().pats_cost_typed(_ptr(d0), _ptr(d1), code, b, D, n, m, _ptr(out), _stream()), "cost")
    else:
        _check(_L().pats_cost_f32(_ptr(d0), _ptr(d1), b, D, n, m, _ptr(out), _stream()), "cost")
    return out


# ------------------------------------------------------------------------------------------------
# Sinkhorn / OT
# ------------------------------------------------------------------------------------------------
def log_sinkhorn_iterations(Z, log_mu, log_nu, iters: int):
    Z, log_mu, log_nu = _dev(Z, "Z"), _dev(log_mu, "log_mu"), _dev(log_nu, "log_nu")
    b, M, N = Z.shape
    if tuple(log_mu.shape) != (b, M) or tuple(log_nu.shape) != (b, N):
        raise RuntimeError("log_sinkhorn_iterations: marginal shapes do not match Z")
    out = torch.empty_like(Z)
    nb = _L().pats_sinkhorn_workspace_bytes(b, M, N)
    ws = _workspace(nb, Z.device)
    _check(_L().pats_sinkhorn_f32(_ptr(Z), b, M, N, _ptr(log_mu), _ptr(log_nu), int(iters), _ptr(out),
                                  _ptr(ws), nb, _stream()), "log_sinkhorn_iterations")
    return out


def log_optimal_transport(scores, alpha, ns, iters: int):
    scores = _dev(scores, "scores")
    b, m, n = scores.shape
    ns = _dev(ns, "ns")
    if ns.numel() != b * n:
        raise RuntimeError("log_optimal_transport: ns must have %d entries per batch" % n)
    ns = ns.reshape(b, n)
    a = _scalar_dev(alpha, scores.device)
    Z = torch.empty((b, m + 1, n + 1), dtype=torch.float32, device=scores.device)
    nb = _L().pats_ot_workspace_bytes(b, m + 1, n + 1)
    ws = _workspace(nb, scores.device)
    _check(_L().pats_log_optimal_transport_f32(_ptr(scores), b, m, n, _ptr(a), _ptr(ns), int(iters),
                                               _ptr(Z), _ptr(ws), nb, _stream()), "log_optimal_transport")
    return Z


def log_optimal_transport2(scores, one, ns, iters: int, bias_k: float = 0.0):
    """bias_k = 2 (outdoor) / 3 (indoor) folds the caller's dustbin `+= log(k)` of
    second_layer.py:107-112 into the epilogue; 0 returns exactly modules.py:165-182."""
    scores = _dev(scores, "scores")
    b, m, n = scores.shape
    ns = _dev(ns, "ns")
    if ns.numel() != b * (n - 1):
        raise RuntimeError("log_optimal_transport2: ns must have %d entries per batch" % (n - 1))
    ns = ns.reshape(b, n - 1)
    o = _scalar_dev(one, scores.device)
    Z = torch.empty((b, m, n), dtype=torch.float32, device=scores.device)
    nb = _L().pats_ot2_workspace_bytes(b, m, n)
    ws = _workspace(nb, scores.device)
    _check(_L().pats_log_optimal_transport2_f32(_ptr(scores), b, m, n, _ptr(o), _ptr(ns), int(iters),
                                                float(bias_k), _ptr(Z), _ptr(ws), nb, _stream()),
           "log_optimal_transport2")
    return Z


def set_cost_ot_mid_event(event):
    """Measurement hook: the next two-kernel cost_ot call records `event` (a torch.cuda.Event that has been recorded once, so
    that its handle exists; None clears) between its cost-build launch and its Sinkhorn launch."""
    h = None if event is None else ctypes.c_void_p(event.cuda_event)
    _check(_L().pats_set_cost_ot_mid_event(h), "set_cost_ot_mid_event")


def cost_ot(mdesc0, mdesc1, variant, scalar, ns, iters: int, bias_k: float = 0.0, return_flags=False, count=None):
    """descriptors -> log-plan (cost build + OT on one stream, score matrix never returned).
    return_flags (variant 2): also est_position's if_nomatching2 [b, m-1] (bool) from the OT epilogue ->
    (Z, col_nomatch); hand it to est_position_second(col_nomatch=...).
    count (fine level, with return_flags): DEVICE int64 [1] - the tensors are a capacity, only the first `count` problems are
    solved (the rows of the others are left as allocated).
    mdesc0 / mdesc1: float32, float16 or bfloat16 (see _descs_any; Z is float32 with the bits of the call on .float() copies);
    a half `scalar` / `ns` is widened here."""
    (d0, d1), code = _descs_any([mdesc0, mdesc1], ["mdesc0", "mdesc1"])
    b, D, n = d0.shape
    m = d1.shape[2]
    ns = _dev(_widen(ns), "ns").reshape(b, m if variant == 1 else m - 1)
    s = _scalar_dev(scalar, d0.device)
    shape = (b, n + 1, m + 1) if variant == 1 else (b, n, m)
    Z = torch.empty(shape, dtype=torch.float32, device=d0.device)
    nb = _L().pats_cost_ot_workspace_bytes(b, D, n, m, variant)
    ws = _workspace(nb, d0.device)
    if return_flags:
        if variant != 2:
            raise RuntimeError("cost_ot: return_flags needs variant 2 (the coarse level gets them from colmass_sqrt)")
        flags = torch.empty((b, m - 1), dtype=torch.bool, device=d0.device)
        cnt = _dev(count, "count", torch.int64) if count is not None else None
        if code:
            _check(_L().pats_cost_ot_typed(_ptr(d0), _ptr(d1), code, b, _ptr(cnt) if cnt is not None else None, D, n, m,
                                           int(variant), _ptr(s), _ptr(ns), int(iters), float(bias_k), _ptr(Z),
                                           _ptr(flags.view(torch.uint8)), _ptr(ws), nb, _stream()), "cost_ot")
            return Z, flags
        if count is not None:
            _check(_L().pats_cost_ot_flags_counted_f32(_ptr(d0), _ptr(d1), b, _ptr(cnt), D, n, m, int(variant), _ptr(s), _ptr(ns),
                                                       int(iters), float(bias_k), _ptr(Z), _ptr(flags.view(torch.uint8)), _ptr(ws),
                                                       nb, _stream()), "cost_ot")
            return Z, flags
        _check(_L().pats_cost_ot_flags_f32(_ptr(d0), _ptr(d1), b, D, n, m, int(variant), _ptr(s), _ptr(ns), int(iters),
                                           float(bias_k), _ptr(Z), _ptr(flags.view(torch.uint8)), _ptr(ws), nb, _stream()),
               "cost_ot")
        return Z, flags
    if count is not None:
        raise RuntimeError("cost_ot: count needs return_flags=True (the fine level's counted launch)")
    if code:
        _check(_L().pats_cost_ot_typed(_ptr(d0), _ptr(d1), code, b, None, D, n, m, int(variant), _ptr(s), _ptr(ns), int(iters),
                                       float(bias_k), _ptr(Z), None, _ptr(ws), nb, _stream()), "cost_ot")
        return Z
    _check(_L().pats_cost_ot_f32(_ptr(d0), _ptr(d1), b, D, n, m, int(variant), _ptr(s), _ptr(ns),
                                 int(iters), float(bias_k), _ptr(Z), _ptr(ws), nb, _stream()), "cost_ot")
    return Z


# ------------------------------------------------------------------------------------------------
# post-OT
# ------------------------------------------------------------------------------------------------
def colmass_sqrt(Z, return_flags=False):
    """sqrt(exp(Z[:, :-1, :-1]).sum(1) + 1e-8)   (first_layer.py:117-118).
    return_flags: the same pass over the columns also yields est_position's if_nomatching2 (first_layer.py:163,167)
    -> (scales, col_nomatch [b, N-1] bool)."""
    Z = _dev(Z, "Z")
    b, M, N = Z.shape
    out = torch.empty((b, N - 1), dtype=torch.float32, device=Z.device)
    if return_flags:
        flags = torch.empty((b, N - 1), dtype=torch.bool, device=Z.device)
        _check(_L().pats_colmass_flags_f32(_ptr(Z), b, M, N, _ptr(out), _ptr(flags.view(torch.uint8)), _stream()),
               "colmass_sqrt")
        return out, flags
    _check(_L().pats_colmass_sqrt_f32(_ptr(Z), b, M, N, _ptr(out), _stream()), "colmass_sqrt")
    return out


def dustbin_bias_(Z, k):
    """In place: Z[:, :, -1] += log(k); Z[:, -1, :] += log(k)   (second_layer.py:107-112)."""
    if not Z.is_contiguous():
        raise RuntimeError("dustbin_bias_: Z must be contiguous (in-place op)")
    _dev(Z, "Z")
    b, M, N = Z.shape
    _check(_L().pats_dustbin_bias_inplace_f32(_ptr(Z), b, M, N, float(k), _stream()), "dustbin_bias_")
    return Z


def exp(Z):
    Z = _dev(Z, "Z")
    out = torch.empty_like(Z)
    _check(_L().pats_exp_f32(_ptr(Z), Z.numel(), _ptr(out), _stream()), "exp")
    return out


def argmax(Z):
    """(scores.max(2).indices, scores.max(1).indices), first index on ties (first_layer.py:162)."""
    Z = _dev(Z, "Z")
    b, M, N = Z.shape
    r = torch.empty((b, M), dtype=torch.int64, device=Z.device)
    c = torch.empty((b, N), dtype=torch.int64, device=Z.device)
    _check(_L().pats_argmax_f32(_ptr(Z), b, M, N, _ptr(r), _ptr(c), _stream()), "argmax")
    return r, c


# ------------------------------------------------------------------------------------------------
# patch-area expansion
# ------------------------------------------------------------------------------------------------
_POS_CACHE = {}


def Compute_positions_and_ranges(height, width, device):
    """utils/utils.py:1527-1537.  The returned tensors carry the grid as `_pats_grid` so
    Iterative_expand_matrix does not have to read them back from the device.  They depend on (height, width, device)
    only and are built once (treat them as read-only): the per-call host-to-device copies of the first version were
    stream-ordered pageable copies, i.e. the host waited for everything queued before them."""
    key = (int(height), int(width), str(torch.device(device)))
    hit = _POS_CACHE.get(key)
    if hit is not None:
        return hit
    k = torch.arange(height * width)
    positions = torch.stack([(k // width).float(), (k % width).float()], dim=1)
    max_shape = max(height, width)
    kk = torch.arange(max_shape).float()
    ranges = torch.where(kk[None, :] <= kk[:, None], kk[None, :].expand(max_shape, -1),
                         torch.full((max_shape, max_shape), 1e7))
    positions, ranges = positions.to(device), ranges.to(device)
    positions._pats_grid = (int(height), int(width))
    ranges._pats_grid = (int(height), int(width))
    _POS_CACHE[key] = (positions, ranges)
    return positions, ranges


def _grid_of(positions, ranges):
    """(h, w) of the index tables handed to Iterative_expand_matrix.  The expansion kernel does not READ the two tensors: it forms
    positions[k] = (k // w, k % w) and ranges[i] = [0 .. i, 1e7 ...] itself (utils.py:1527-1537 - what every call site of the
    reference passes, first_layer.py:173-175 / second_layer.py:254-256).  The reference does honour other contents (a shifted
    `ranges` changes 311 of 1 152 rectangle bounds of the golden case, tests/golden/positions_ranges.npz), so tensors that do
    not come from Compute_positions_and_ranges above are CHECKED against those tables once (one device comparison) and
    anything else is refused instead of being silently replaced."""
    g = getattr(positions, "_pats_grid", None) or getattr(ranges, "_pats_grid", None)
    if g is not None:
        return g
    # foreign tensors: recover (h, w) from the values (one device read), then hold both to the canonical tables
    if positions.dim() != 2 or positions.shape[1] != 2 or ranges.dim() != 2 or ranges.shape[0] != ranges.shape[1]:
        raise RuntimeError("Iterative_expand_matrix: positions must be [h*w,2] and ranges [max(h,w),max(h,w)]")
    w = int((positions[:, 0] == 0).sum().item())
    if w <= 0 or positions.shape[0] % w != 0:
        raise RuntimeError("Iterative_expand_matrix: positions is not the table of Compute_positions_and_ranges")
    h = positions.shape[0] // w
    cp, cr = Compute_positions_and_ranges(h, w, positions.device)
    if tuple(ranges.shape) != tuple(cr.shape) or not torch.equal(positions.float(), cp) or not torch.equal(ranges.float().to(cr.device), cr):
        raise RuntimeError("Iterative_expand_matrix: only the index tables Compute_positions_and_ranges builds are supported "
                           "(positions[k] = (k // w, k % w), ranges[i] = [0 .. i, 1e7 ...]); the tensors handed in differ")
    try:
        positions._pats_grid = ranges._pats_grid = (h, w)      # checked once
    except Exception:                                          # noqa: BLE001
        pass
    return h, w


def Iterative_expand_matrix(scores_in, scalex, scaley, limitation, ranges, positions,
                            lower_bound=1e-3, upper_bound=1e7, iter_num=15, width=20, height=15,
                            type="distance", input_is_log=False, row_nomatch=None, count=None):
    """utils/utils.py:1179-1297.  Returns (whole_cost, core_cost, average_point, x_scale, y_scale,
    bound) with the reference's shapes/dtypes.  `width`/`height`/`upper_bound`/`type` are accepted
    and ignored exactly as the reference ignores them (it re-derives width/height at :1181)."""
    P = _dev(scores_in, "scores_in")
    b, M, N = P.shape
    sx = _dev(scalex, "scalex").reshape(b, -1)
    sy = _dev(scaley, "scaley").reshape(b, -1)
    if sx.shape[1] != N - 1 or sy.shape[1] != N - 1:
        raise RuntimeError("Iterative_expand_matrix: scale tensors must have %d entries" % (N - 1))
    h, w = _grid_of(positions, ranges)
    if isinstance(limitation, torch.Tensor):
        lim3 = getattr(limitation, "_pats_lim3", None)
        if lim3 is None:
            lim3 = int(limitation[3].item())
    else:
        lim3 = int(limitation[3])
    m = M - 1
    dev = P.device
    whole = torch.empty((b, m), dtype=torch.float32, device=dev)
    core = torch.empty((b, m), dtype=torch.float32, device=dev)
    avg = torch.empty((b, m, 2), dtype=torch.float32, device=dev)
    xs = torch.empty((b, m), dtype=torch.float32, device=dev)
    ys = torch.empty((b, m), dtype=torch.float32, device=dev)
    bound = torch.empty((b, m, 4), dtype=torch.int64, device=dev)
    rn = _ptr(row_nomatch.view(torch.uint8)) if row_nomatch is not None else _ptr(None)
    if count is not None:           # not in the reference's signature: a device-side batch count (throughput mode)
        _check(_L().pats_iterative_expand_counted_f32(_ptr(P), int(bool(input_is_log)), b, _ptr(_dev(count, "count", torch.int64)),
                                                      M, N, _ptr(sx), _ptr(sy), lim3, h, w, float(lower_bound), int(iter_num),
                                                      _ptr(whole), _ptr(core), _ptr(avg), _ptr(xs), _ptr(ys), _ptr(bound), rn,
                                                      _stream()), "Iterative_expand_matrix")
        return whole, core, avg, xs, ys, bound
    _check(_L().pats_iterative_expand_f32(_ptr(P), int(bool(input_is_log)), b, M, N, _ptr(sx), _ptr(sy),
                                          lim3, h, w, float(lower_bound), int(iter_num), _ptr(whole),
                                          _ptr(core), _ptr(avg), _ptr(xs), _ptr(ys), _ptr(bound), rn,
                                          _stream()), "Iterative_expand_matrix")
    return whole, core, avg, xs, ys, bound


def _est_position(scores, scale_x, scale_y, H, W, patch_scale, iter_num, lower_bound, col_nomatch=None, count=None):
    """est_position (first_layer.py:159-178 / second_layer.py:240-259) without a separate argmax pass: the row flag
    `scores.max(2).indices[:, :-1] == h*w` comes out of the expansion kernel (which holds every row anyway), the
    column flag from the caller (OT epilogue / colmass pass) or, failing that, from one pass over the columns."""
    b, M, N = scores.shape
    h, w = H // patch_scale, W // patch_scale
    if col_nomatch is None:
        col_nomatch = torch.empty((b, N - 1), dtype=torch.bool, device=scores.device)
        _check(_L().pats_colmass_flags_f32(_ptr(_dev(scores, "scores")), b, M, N, _ptr(None),
                                           _ptr(col_nomatch.view(torch.uint8)), _stream()), "est_position")
    if_nomatching1 = torch.empty((b, M - 1), dtype=torch.bool, device=scores.device)
    positions1, ranges1 = Compute_positions_and_ranges(h, w, scores.device)
    limitation1 = [0, h, 0, w]
    trust_score, _, average_point1, x_scale, y_scale, _ = Iterative_expand_matrix(
        scores, scale_x.reshape(b, -1, 1), scale_y.reshape(b, -1, 1), limitation1, ranges1, positions1,
        height=h, width=w, iter_num=iter_num, lower_bound=lower_bound, input_is_log=True, row_nomatch=if_nomatching1, count=count)
    return trust_score, average_point1, x_scale, y_scale, if_nomatching1, col_nomatch


def est_position_first(scores, scale_src, image_shape, patch_scale, col_nomatch=None):
    """FirstLayer.est_position (first_layer.py:159-178): scores is the LOG plan; exp() is fused
    into the expansion kernel's load.  col_nomatch: if_nomatching2 when the caller already has it
    (colmass_sqrt(return_flags=True))."""
    H, W = image_shape
    return _est_position(scores, scale_src, scale_src, H, W, patch_scale, 15, 1e-5, col_nomatch)


def est_position_second(scores, scale_x, scale_y, image_shape, patch_scale, col_nomatch=None, count=None):
    """SecondLayer.est_position (second_layer.py:240-259).  col_nomatch: if_nomatching2 from
    cost_ot(..., return_flags=True).  count: device-side batch count (throughput mode), as for cost_ot."""
    H, W = image_shape
    return _est_position(scores, scale_x, scale_y, H, W, patch_scale, 8, 1e-3, col_nomatch, count)


# ------------------------------------------------------------------------------------------------
# chunk planner (host)
# ------------------------------------------------------------------------------------------------
def split_patches(sum_cycle, height, width, max_once_used=350):
    """utils/utils.py:152-181.  One D->H copy of the cumsum (none if it already is a CPU tensor /
    numpy array, e.g. one row of a batch fetched once for many pairs), then host C++."""
    if isinstance(sum_cycle, np.ndarray):
        sc = np.ascontiguousarray(sum_cycle, dtype=np.int32)
    else:
        sc = sum_cycle.detach().to("cpu", torch.int32).contiguous().numpy()
    if sc.shape[0] != height * width:
        raise RuntimeError("split_patches: sum_cycle must have height*width entries")
    second = np.zeros((height + 1, 2), np.int64)
    third = np.zeros((height + 1, 2), np.int64)
    n = _L().pats_split_patches(sc.ctypes.data_as(ctypes.c_void_p), int(height), int(width),
                                int(max_once_used), second.ctypes.data_as(ctypes.c_void_p),
                                third.ctypes.data_as(ctypes.c_void_p))
    if n < 1:
        _check(-n, "split_patches")
    return n, second[:n].tolist(), third[:n].tolist()


def split_patches_device(sum_cycle, height, width, max_once_used=350):
    """split_patches (utils/utils.py:152-181) for a batch of pairs WITHOUT leaving the device:
    sum_cycle [pairs, height*width] int32 -> (cycle_num [pairs] int32, second_layer_set [pairs,height+1,2],
    third_layer_set [pairs,height+1,2] int64), rows past cycle_num zeroed.  No host read."""
    sc = _dev(sum_cycle, "sum_cycle", torch.int32)
    pairs = sc.shape[0]
    if sc.dim() != 2 or sc.shape[1] != height * width:
        raise RuntimeError("split_patches_device: sum_cycle must be [pairs, height*width]")
    second = torch.empty((pairs, height + 1, 2), dtype=torch.int64, device=sc.device)
    third = torch.empty((pairs, height + 1, 2), dtype=torch.int64, device=sc.device)
    num = torch.empty((pairs,), dtype=torch.int32, device=sc.device)
    _check(_L().pats_split_patches_device(_ptr(sc), pairs, int(height), int(width), int(max_once_used), _ptr(second),
                                          _ptr(third), _ptr(num), _stream()), "split_patches_device")
    return num, second, third


# ------------------------------------------------------------------------------------------------
# subdivision gather
# ------------------------------------------------------------------------------------------------
# element types the crops take images in and write crops in (include/pats_amd.h pats_img_dtype_t)
_IMG_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.uint8: 3}
_LAYOUTS = {"hwc": 0, "chw": 1}


class CropFormat:
    """The format the subdivision gather writes its crops in (pats_crop_format_t).
        dtype   torch.float32 / float16 / bfloat16, or torch.uint8 for the left crops of uint8 images (exact copies; the
                right crops then come out float32, like the reference's new_left / new_right, utils.py:1352-1385)
        layout  "hwc" [K,96,96,3] or "chw" [K,3,96,96] (= crops.permute(0,3,1,2).contiguous())
        mean, std  three floats each, or None: per-channel (x - mean[c]) / std[c] in fp32 (torchvision's Normalize)
    Every crop is computed in fp32 as the float32 kernels compute it, then normalised, then rounded ONCE to dtype
    (round-to-nearest-even).  CropFormat() is today's output: float32 HWC, not normalised."""

    BACKBONE_MEAN = (0.485, 0.456, 0.406)          # second_layer.py:56
    BACKBONE_STD = (0.229, 0.224, 0.225)

    def __init__(self, dtype=torch.float32, layout="hwc", mean=None, std=None):
        if dtype not in _IMG_DTYPES:
            raise ValueError("CropFormat: dtype must be float32, float16, bfloat16 or uint8, got %r" % (dtype,))
        if layout not in _LAYOUTS:
            raise ValueError("CropFormat: layout must be 'hwc' or 'chw', got %r" % (layout,))
        if (mean is None) != (std is None):
            raise ValueError("CropFormat: mean and std go together")
        if mean is not None:
            mean, std = tuple(float(m) for m in mean), tuple(float(v) for v in std)
            if len(mean) != 3 or len(std) != 3:
                raise ValueError("CropFormat: mean and std need 3 values each, got %d and %d" % (len(mean), len(std)))
            if not all(np.isfinite(mean)) or not all(np.isfinite(std)) or any(v == 0.0 for v in std):
                raise ValueError("CropFormat: mean and std must be finite and std non-zero")
            if dtype == torch.uint8:
                raise ValueError("CropFormat: uint8 crops cannot be normalised")
        self.dtype, self.layout, self.mean, self.std = dtype, layout, mean, std

    @classmethod
    def backbone(cls, dtype=torch.float32):
        """What the reference's fine backbone reads (second_layer.py:56,66-68): chw, Normalize(mean, std) of the 0..255 values."""
        return cls(dtype, "chw", cls.BACKBONE_MEAN, cls.BACKBONE_STD)

    @property
    def normalize(self):
        return self.mean is not None

    def is_default(self):
        return self.dtype == torch.float32 and self.layout == "hwc" and not self.normalize

    def shape(self, rows):
        return (rows, 96, 96, 3) if self.layout == "hwc" else (rows, 3, 96, 96)

    def _c(self):
        f = _lib.CropFormat()
        f.dtype, f.layout, f.normalize = _IMG_DTYPES[self.dtype], _LAYOUTS[self.layout], int(self.normalize)
        for c in range(3):
            f.mean[c] = self.mean[c] if self.normalize else 0.0
            f.std[c] = self.std[c] if self.normalize else 1.0
        return f

    def __eq__(self, other):
        return isinstance(other, CropFormat) and (self.dtype, self.layout, self.mean, self.std) == \
            (other.dtype, other.layout, other.mean, other.std)

    def __repr__(self):
        return "CropFormat(dtype=%s, layout=%r, mean=%r, std=%r)" % (self.dtype, self.layout, self.mean, self.std)


def _crop_images(left, right, names):
    """The images of ONE crop call -> (left, right, pats_img_dtype_t code).  float32 / float16 / bfloat16 / uint8 images of
    one dtype go to the kernels as they are (a non-contiguous view is made contiguous, in its dtype); images of other dtypes,
    or of two different dtypes, take the float32 path on .float() copies, as every crop call did before the typed kernels."""
    for t, n in zip((left, right), names):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % n)
    if left.dtype == right.dtype and left.dtype in _IMG_DTYPES:
        return _dev(left, names[0], left.dtype), _dev(right, names[1], right.dtype), _IMG_DTYPES[left.dtype]
    return _dev(left.float(), names[0]), _dev(right.float(), names[1]), 0


def _crop_formats(crop_format, code, left_dtype=None):
    """(left format, right format, dtype to convert the left crops to afterwards or None).  crop_format None: float32 HWC -
    except the host-count path of Compute_imgs (left_dtype given), whose new_left keeps left.dtype as it always did."""
    if crop_format is None:
        lf = rf = CropFormat()
        if left_dtype is not None and left_dtype != torch.float32:
            if left_dtype in _IMG_DTYPES and (left_dtype != torch.uint8 or code == 3):
                lf = CropFormat(left_dtype)
            else:
                return lf, rf, left_dtype
        return lf, rf, None
    if not isinstance(crop_format, CropFormat):
        raise TypeError("crop_format must be an ops.CropFormat or None")
    if crop_format.dtype == torch.uint8:
        if code != 3:
            raise RuntimeError("Compute_imgs: uint8 crops need uint8 images")
        return crop_format, CropFormat(torch.float32, crop_format.layout), None
    return crop_format, crop_format, None


def _crop_out(t, fmt, rows, name, device):
    """A crop output: allocated, or the caller's tensor (dtype and per-crop shape of the format, >= rows crops, contiguous,
    16-byte aligned) cut to `rows` crops."""
    if t is None:
        return torch.empty(fmt.shape(rows), dtype=fmt.dtype, device=device)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
        raise RuntimeError("Compute_imgs: %s must be a GPU tensor on %s" % (name, device))
    if t.dtype != fmt.dtype or tuple(t.shape[1:]) != fmt.shape(rows)[1:] or t.shape[0] < rows:
        raise RuntimeError("Compute_imgs: %s must be %s of shape [>= %d, %s], got %s %s" % (
            name, fmt.dtype, rows, ",".join(str(d) for d in fmt.shape(rows)[1:]), t.dtype, tuple(t.shape)))
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise RuntimeError("Compute_imgs: %s must be contiguous and 16-byte aligned" % name)
    return t[:rows]


def tensor_resize(input_tensor, bound, validate=True):
    """tensor_resize.tensor_resize(input, bound)  (setup/library.cpp:47-66,92-93).
    input [n,C,Hp,Wp] float32, bound [K,5] int64 -> new [K,C,96,96] float32 on input.device.
    A float16 / bfloat16 input is widened to fp32 exactly in the kernel (library.cpp:50-62 resizes a half input into a
    float32 result): the result is float32 and bit-identical to the call on input.float().
    Raises RuntimeError for an empty or out-of-range crop like the reference (validate=True)."""
    if not isinstance(input_tensor, torch.Tensor):
        raise TypeError("input_tensor must be a torch.Tensor")
    if input_tensor.dtype not in _MAP_DTYPES:
        raise RuntimeError("pats_amd: input_tensor must be float32, float16 or bfloat16, got %s" % input_tensor.dtype)
    inp = _dev(input_tensor, "input_tensor", input_tensor.dtype)
    bnd = _dev(bound, "bound", torch.int64)
    if inp.dim() != 4 or bnd.dim() != 2 or bnd.shape[1] != 5:
        raise RuntimeError("tensor_resize: expected input [n,C,H,W] and bound [K,5]")
    n_img, C, Hp, Wp = inp.shape
    K = bnd.shape[0]
    out = torch.empty((K, C, 96, 96), dtype=torch.float32, device=inp.device)
    status = torch.zeros((1,), dtype=torch.int32, device=inp.device) if validate else None
    if inp.dtype == torch.float32:
        _check(_L().pats_tensor_resize_f32(_ptr(inp), n_img, C, Hp, Wp, _ptr(bnd), K, _ptr(out),
                                           _ptr(status), _stream()), "tensor_resize")
    else:
        fmt = CropFormat(torch.float32, "chw")._c()
        _check(_L().pats_tensor_resize_typed(_ptr(inp), _IMG_DTYPES[inp.dtype], n_img, C, Hp, Wp, _ptr(bnd), K, None,
                                             ctypes.byref(fmt), _ptr(out), _ptr(status), _stream()), "tensor_resize")
    if validate and K > 0 and int(status.item()) != 0:
        # library.cpp:56-60: narrow() outside the tensor / an empty crop into upsample_bilinear2d is a
        # c10::Error there (RuntimeError / IndexError in Python).  One host read per call (the reference
        # makes five per crop); validate=False skips it and leaves such crops zero-filled.
        raise RuntimeError("tensor_resize: a crop is empty or outside the %dx%d input (start/length out of range, "
                           "or image index >= %d)" % (Hp, Wp, n_img))
    return out


def Compute_imgs(x_scale, y_scale, average_point, if_nomatching, left, right, sequence_num=0,
                 output_path=None, if_view=False, margin=128, width=20, height=15, patch_scale=32, known_count=None,
                 validate=False, crop_format=None, out=None):
    """utils/utils.py:1343-1393 - same 5-tuple as the reference."""
    return Compute_imgs_ex(x_scale, y_scale, average_point, if_nomatching, left, right, sequence_num,
                           output_path, if_view, margin, width, height, patch_scale, known_count, validate,
                           crop_format, out)[:5]


def Compute_imgs_ex(x_scale, y_scale, average_point, if_nomatching, left, right, sequence_num=0,
                    output_path=None, if_view=False, margin=128, width=20, height=15, patch_scale=32,
                    known_count=None, validate=False, crop_format=None, out=None):
    """Compute_imgs plus the [K,5] bound tensor the reference hands to tensor_resize (utils.py:1382).
    utils/utils.py:1343-1393, any batch of images (PATS.forward uses 1, first_layer.py:135; a batch
    yields the crops of all images in (image, patch) order - `sequence = img * 10000 + patch`, :1374-1377).
    Returns (new_left [K,96,96,3], new_right [K,96,96,3], x_scale_new [1,N,2], y_scale_new
    [1,N,2], average_new [1,N,2], bound5 [K,5]).  One host read (K) sizes the outputs, as the reference's
    boolean-mask indexing does - unless the caller already knows the matched patches per image
    (`known_count`, e.g. the last entry of the cumsum it fetched for split_patches): then no sync;
    validate=True checks those counts against the device-side ones (one host read).
    known_count="device" never touches the host: outputs are sized for the capacity n_img*N, only the first
    K_total rows are written, and the tuple gains (K_img [n_img], K_total [1]) int64 DEVICE tensors.
    Images: float32, float16, bfloat16 or uint8 (the loaders' cv2 images), left and right of one dtype, are read as they are
    and widened to fp32 exactly in the kernels - the crops equal those of images.float() bit for bit; images of other dtypes
    or of two dtypes are converted with .float() first, as before.
    crop_format: an ops.CropFormat for both sides' crops (dtype, hwc / chw, normalisation; CropFormat.backbone(dtype) is the
    fine backbone's input).  None: float32 HWC - on the host-count path new_left keeps left.dtype, as it always did.
    out: optional (left_out, right_out), either may be None - tensors of the format's dtype and per-crop shape with at least
    as many crops as the call writes (K, or the capacity n_img*N with known_count="device"); the crops are written into them
    (e.g. buf[0], buf[1] of one [2, cap, 3, 96, 96] buffer whose view(2 * cap, 3, 96, 96) the backbone reads)."""
    if margin != 128 or patch_scale != 32:
        raise RuntimeError("Compute_imgs: margin=128 / patch_scale=32 are what the path uses")
    nb = left.shape[0]                          # images in the batch; crops come out ordered (image, patch)
    dev = x_scale.device
    Np = width * height
    xs = _dev(x_scale.float(), "x_scale").reshape(nb, Np)
    ys = _dev(y_scale.float(), "y_scale").reshape(nb, Np)
    ap = _dev(average_point.float(), "average_point").reshape(nb, Np, 2)
    ifn = _as_flags(if_nomatching, "if_nomatching").reshape(nb, Np)         # bool viewed as bytes: no copy kernel
    leftf, rightf, code = _crop_images(left, right, ("left", "right"))
    H, W = leftf.shape[1], leftf.shape[2]
    on_device = isinstance(known_count, str) and known_count == "device"
    lfmt, rfmt, left_to = _crop_formats(crop_format, code, None if on_device else left.dtype)
    lout, rout = (None, None) if out is None else out
    counts = None
    if known_count is not None and not on_device:
        if isinstance(known_count, torch.Tensor):
            known_count = known_count.tolist()          # a (GPU) tensor of counts: one host read, like int(tensor)
        counts = [int(k) for k in np.atleast_1d(np.asarray(known_count)).ravel()]
        if len(counts) != nb:
            raise RuntimeError("Compute_imgs: known_count needs one entry per image")
    # all images in one launch: block i offsets its compacted bounds by the matches of the images before it
    bound5, Kd, Kt, xsn, ysn, avn = _imgs_bounds(None, xs, ys, ap, ifn, nb, (nb, Np), height, width)
    status = torch.zeros((1,), dtype=torch.int32, device=dev) if validate else None
    if on_device:
        new_left, new_right = _crops(None, leftf, rightf, code, nb, H, W, height, width, margin, bound5, nb * Np, Kt, lfmt, rfmt,
                                     lout, rout, status)
        if validate and int(status.item()) != 0:
            raise RuntimeError("Compute_imgs: a right crop is empty or outside the padded image")
        return new_left, new_right, xsn, ysn, avn, bound5, Kd, Kt
    if counts is None:
        counts = [int(k) for k in Kd.tolist()]                  # the host read
    elif validate:
        got = [int(k) for k in Kd.tolist()]
        if got != counts:
            raise RuntimeError("Compute_imgs: known_count %s does not match the matched patches per image %s" % (counts, got))
    K = sum(counts)
    new_left, new_right = _crops(None, leftf, rightf, code, nb, H, W, height, width, margin, bound5, K, None, lfmt, rfmt,
                                 lout if left_to is None else None, rout, status)
    if validate and K > 0 and int(status.item()) != 0:
        raise RuntimeError("Compute_imgs: a right crop is empty or outside the padded image")
    if left_to is not None:                 # a left image of another dtype (e.g. float64): converted back, as before
        new_left = new_left.to(left_to)
        if lout is not None:
            new_left = _crop_out(lout, CropFormat(left_to), K, "out[0]", dev).copy_(new_left)
    return new_left, new_right, xsn, ysn, avn, bound5[:K]


def _imgs_bounds(table, xs, ys, ap, ifn, pairs, cell_ext, height=0, width=0):
    """The crop bounds of a batch - what Compute_imgs_ex and Compute_imgs_ragged share: (bound5 [cells,5], K_img [pairs], K_total
    [1], xsn, ysn, avn [cell_ext, 2]) allocated and written.  cell_ext: (nb, Np) for nb uniform images, (sum N,) for a PairTable."""
    dev = xs.device
    bound5 = torch.empty((xs.numel(), 5), dtype=torch.int64, device=dev)
    Kd = torch.empty((pairs,), dtype=torch.int64, device=dev)
    Kt = torch.empty((1,), dtype=torch.int64, device=dev)
    xsn = torch.empty(cell_ext + (2,), dtype=torch.float32, device=dev)
    ysn = torch.empty(cell_ext + (2,), dtype=torch.float32, device=dev)
    avn = torch.empty(cell_ext + (2,), dtype=torch.float32, device=dev)
    if table is None:
        entry, head, grid, what = "pats_compute_imgs_bounds_batch_f32", (), (cell_ext[0], cell_ext[1], height, width), "Compute_imgs(bounds)"
    else:
        entry, head, grid, what = "pats_compute_imgs_bounds_ragged_f32", (table.ref(),), (), "Compute_imgs_ragged(bounds)"
    _check(getattr(_L(), entry)(*head, _ptr(xs), _ptr(ys), _ptr(ap), _ptr(ifn), *grid, _ptr(bound5), _ptr(Kd), _ptr(Kt), _ptr(xsn),
                                _ptr(ysn), _ptr(avn), _stream()), what)
    return bound5, Kd, Kt, xsn, ysn, avn


# the crop entries (left, right, what a failure names) of the float32 HWC forms; every other image dtype or format is "typed"
_CROPS = {"typed": ("pats_left_crops_typed", "pats_tensor_resize_hwc_typed", "Compute_imgs(left)", "Compute_imgs(right)"),
          "host": ("pats_left_crops_f32", "pats_tensor_resize_hwc_f32", "Compute_imgs(left)", "Compute_imgs(right)"),
          "counted": ("pats_left_crops_counted_f32", "pats_tensor_resize_hwc_counted_f32", "Compute_imgs(left)", "Compute_imgs(right)"),
          "ragged": ("pats_left_crops_ragged_f32", "pats_tensor_resize_hwc_ragged_f32", "Compute_imgs_ragged(left)",
                     "Compute_imgs_ragged(right)")}


def _crops(table, left, right, code, nb, H, W, height, width, margin, bound5, rows, K_dev, lfmt, rfmt, lout, rout, status):
    """Both sides' crops of `rows` bounds (K_dev: the device count of those that exist, or None) into fresh tensors or the
    caller's lout / rout -> (new_left, new_right).  table: a PairTable, or None for nb uniform images."""
    dev = bound5.device
    new_left = _crop_out(lout, lfmt, rows, "out[0]", dev)
    new_right = _crop_out(rout, rfmt, rows, "out[1]", dev)
    tab = table.ref() if table is not None else None
    if code != 0 or not lfmt.is_default() or not rfmt.is_default():
        form, lc, rc = "typed", lfmt._c(), rfmt._c()
        largs = (tab, _ptr(left), code, nb, H, W, height, width, _ptr(bound5), rows, _ptr(K_dev), ctypes.byref(lc), _ptr(new_left))
        rargs = (tab, _ptr(right), code, nb, H, W, margin, _ptr(bound5), rows, _ptr(K_dev), ctypes.byref(rc), _ptr(new_right),
                 _ptr(status))
    elif table is not None:
        form = "ragged"
        largs = (tab, _ptr(left), _ptr(bound5), rows, _ptr(K_dev), _ptr(new_left))
        rargs = (tab, _ptr(right), margin, _ptr(bound5), rows, _ptr(K_dev), _ptr(new_right), _ptr(status))
    else:
        form, count_arg = ("counted", (_ptr(K_dev),)) if K_dev is not None else ("host", ())
        largs = (_ptr(left), nb, H, W, _ptr(bound5), rows, *count_arg, height, width, _ptr(new_left))
        rargs = (_ptr(right), nb, H, W, margin, _ptr(bound5), rows, *count_arg, _ptr(new_right), _ptr(status))
    lentry, rentry, lwhat, rwhat = _CROPS[form]
    _check(getattr(_L(), lentry)(*largs, _stream()), lwhat)
    _check(getattr(_L(), rentry)(*rargs, _stream()), rwhat)
    return new_left, new_right


# ------------------------------------------------------------------------------------------------
# third level
# ------------------------------------------------------------------------------------------------
def Compute_result(scores, W, T, scale_x, scale_y, p_s, p_t, device=None, outdoor=True,
                   input_is_log=False, return_confidence=False):
    """ThirdLayer.Compute_result (third_layer.py:184-217) + the label rule (:161-170).
    Returns (mkpts0_f, mkpts1_f, whole_loss, label, if_matching1[, conf]).  return_confidence: conf [P,16] float32, the plan
    mass inside each centre cell's 5x5 window over the mass of its whole row (third_level has the definition)."""
    if W != 8 or T != 5:
        raise RuntimeError("Compute_result: the path uses W=8, T=5 (third_layer.py:108-111)")
    S = _dev(scores, "scores")
    P = S.shape[0]
    if tuple(S.shape[1:]) != (65, 65):
        raise RuntimeError("Compute_result: scores must be [P,65,65]")
    sx = _dev(scale_x, "scale_x").reshape(P, 64)
    sy = _dev(scale_y, "scale_y").reshape(P, 64)
    ps = _dev(p_s.to(torch.int64), "p_s", torch.int64).reshape(P, 2)
    pt = _dev(p_t.to(torch.int64), "p_t", torch.int64).reshape(P, 2)
    dev = S.device
    m0 = torch.empty((P, 16, 2), dtype=torch.float32, device=dev)
    m1 = torch.empty((P, 16, 2), dtype=torch.float32, device=dev)
    wl = torch.empty((P, 16), dtype=torch.float32, device=dev)
    label = torch.empty((P * 16, 2), dtype=torch.float32, device=dev)
    ifm = torch.empty((P, 16), dtype=torch.uint8, device=dev)
    ws = torch.empty((1,), dtype=torch.int32, device=dev)          # whole_loss' cross-problem count: no allocation in the call
    if return_confidence:
        conf = torch.empty((P, 16), dtype=torch.float32, device=dev)
        _check(_L().pats_compute_result_ws_conf_f32(_ptr(S), int(bool(input_is_log)), P, _ptr(sx), _ptr(sy), _ptr(ps),
                                                    _ptr(pt), int(bool(outdoor)), _ptr(m0), _ptr(m1), _ptr(wl),
                                                    _ptr(label), _ptr(ifm), _ptr(conf), _ptr(ws), 4, _stream()), "Compute_result")
        return m0, m1, wl, label, ifm.bool(), conf
    _check(_L().pats_compute_result_ws_f32(_ptr(S), int(bool(input_is_log)), P, _ptr(sx), _ptr(sy), _ptr(ps),
                                           _ptr(pt), int(bool(outdoor)), _ptr(m0), _ptr(m1), _ptr(wl),
                                           _ptr(label), _ptr(ifm), _ptr(ws), 4, _stream()), "Compute_result")
    return m0, m1, wl, label, ifm.bool()


def _third_conf(out, P, dev):
    """third_level's conf [P,16]: a fresh tensor, or the fifth tensor of the caller's `out` checked."""
    if out is None or len(out) == 4:
        return torch.empty((P, 16), dtype=torch.float32, device=dev)
    c = _dev(out[4], "out[4]")
    if tuple(c.shape) != (P, 16) or c.data_ptr() != out[4].data_ptr():
        raise RuntimeError("third_level: out[4] (conf) must be a contiguous [P,16] float32 tensor")
    return c


def _third_out(out, P, dev, n=4):
    """The four output tensors of third_level: fresh ones, or the caller's `out` checked (if_matching1 as uint8 storage).
    n = 5: `out` may carry conf as a fifth tensor (_third_conf checks it)."""
    if out is not None and n == 5 and len(out) == 5:
        return _third_out(tuple(out[:4]), P, dev)
    if out is None:
        return (torch.empty((P, 16, 2), dtype=torch.float32, device=dev), torch.empty((P, 16, 2), dtype=torch.float32, device=dev),
                torch.empty((P * 16, 2), dtype=torch.float32, device=dev), torch.empty((P, 16), dtype=torch.uint8, device=dev))
    if len(out) != 4:
        raise RuntimeError("third_level: out must be (mkpts0_f, mkpts1_f, label, if_matching1)")
    m0, m1, label = (_dev(t, "out[%d]" % i) for i, t in enumerate(out[:3]))
    ifm = _as_flags(out[3], "out[3]")
    shapes = ((P, 16, 2), (P, 16, 2), (P * 16, 2), (P, 16))
    if any(tuple(t.shape) != s or t.data_ptr() != o.data_ptr() for t, o, s in zip((m0, m1, label, ifm), out, shapes)):
        raise RuntimeError("third_level: out must be contiguous [P,16,2], [P,16,2], [P*16,2] float32 and [P,16] uint8 / bool tensors")
    return m0, m1, label, ifm


def third_level(feat_f0_unfold, feat_f1_unfold, scale, mkpts0_c, mkpts1_c, outdoor=True, iters=100,
                return_plan=False, count=None, out=None, return_confidence=False):
    """The third layer's whole OT step in one launch (third_layer.py:153-170):
        scale_x = scale_y = sqrt(scale + 1e-8)
        scores  = exp(log_optimal_transport2(0.1 * einsum(f0, f1) / 128**.5, 1, scale, 100))
        mkpts0_f, mkpts1_f, _ = Compute_result(scores, 8, 5, scale_x, scale_y, mkpts0_c, mkpts1_c)
        label / if_matching1 as :161-170
    Returns (mkpts0_f, mkpts1_f, label, if_matching1[, Z][, conf]).  The 65x65 plans stay on chip.
    return_confidence: conf [P,16] float32 is appended (behind Z).  For problem p and centre cell k (row r of the plan
    S = exp(Z)): conf = (sum of S[r, c] over the 5x5 window around argmax_c S[r, :64], zero outside the 8x8 grid) / (sum of
    S[r, :] over all 65 columns) - the two terms of third_layer.py:212-213 - for all 16 cells, whatever label / if_matching1
    say; a problem the guard sends to a re-solve gets the confidence of the re-solved plan.  The other outputs keep their bits;
    `out` may carry conf as a fifth tensor; with `count`, rows past it are not written.
    count: a DEVICE int64 [1] holding the number of problems that exist (throughput mode: the tensors are sized for a
    capacity, nothing is read back); rows past it are not written, and sqrt(scale + 1e-8) is formed in the kernel.
    out: optional (mkpts0_f [P,16,2], mkpts1_f [P,16,2], label [P*16,2], if_matching1 [P,16] uint8 or bool) to write into; the same
    four tensors are returned, if_matching1 as it was given.
    feat_f*_unfold: float32, float16 or bfloat16 (see _descs_any); every output is float32 / bool with the bits of the call on
    .float() copies.  A half `scale` is widened here."""
    (f0, f1), code = _descs_any([feat_f0_unfold, feat_f1_unfold], ["feat_f0_unfold", "feat_f1_unfold"])
    P, D, n = f0.shape
    if n != 65 or tuple(f1.shape) != (P, D, 65):
        raise RuntimeError("third_level: descriptors must be [P,D,65]")
    sc = _dev(_widen(scale), "scale").reshape(P, 64)
    ps = _dev(mkpts0_c.to(torch.int64), "mkpts0_c", torch.int64).reshape(P, 2)
    pt = _dev(mkpts1_c.to(torch.int64), "mkpts1_c", torch.int64).reshape(P, 2)
    dev = f0.device
    counted = count is not None
    if counted:                     # the kernel forms sqrt(scale + 1e-8) itself and writes no plan
        if return_plan:
            raise RuntimeError("third_level: return_plan is not available with a device-side count")
        cnt, sxy, Z = _dev(count, "count", torch.int64).reshape(1), None, None
    else:
        cnt, sxy = None, torch.sqrt(sc + 1e-8)
        Z = torch.empty((P, 65, 65), dtype=torch.float32, device=dev) if return_plan else None
    m0, m1, label, ifm = _third_out(out, P, dev, 5 if return_confidence else 4)
    conf = _third_conf(out, P, dev) if return_confidence else None
    # one argument list; the form picks the entry and splices in what only it takes (dtype code, count, plan, conf)
    entry = _THIRD_LEVEL[2 if return_confidence else 1 if code else 0][counted]
    args = [_ptr(f0), _ptr(f1)]
    if return_confidence or code:
        args += (code, P, _ptr(cnt))
    elif counted:
        args += (P, _ptr(cnt))
    else:
        args.append(P)
    args += (D, _ptr(sc), _ptr(sxy), _ptr(sxy), _ptr(ps), _ptr(pt), int(iters), int(bool(outdoor)), _ptr(m0), _ptr(m1), _ptr(label),
             _ptr(ifm))
    if entry != "pats_third_level_counted_f32":
        args.append(_ptr(Z))
    if return_confidence:
        args.append(_ptr(conf))
    _check(getattr(_L(), entry)(*args, _stream()), "third_level")
    if out is not None:
        res = tuple(out[:4])
    else:                           # the counted form hands out a view of the flags, the other a bool copy, as they always did
        res = (m0, m1, label, ifm.view(torch.bool) if counted else ifm.bool())
    if return_plan:
        res += (Z,)
    return res + (conf,) if return_confidence else res


# third_level's entry by (0 fp32 / 1 typed / 2 typed with confidence) and [no count, device count]
_THIRD_LEVEL = (("pats_third_level_f32", "pats_third_level_counted_f32"), ("pats_third_level_typed",) * 2,
                ("pats_third_level_typed_conf",) * 2)


def _widen(t):
    """title / rubbish / kenc in half precision: small, widened here (exactly) to the float32 the kernels read."""
    return t.float() if isinstance(t, torch.Tensor) and t.dtype in (torch.float16, torch.bfloat16) else t


def _out_dtype(outs, out_dtype, who):
    """The element type a gather writes: that of `out` when given (all of `outs` must agree, and out_dtype must not
    contradict them), else out_dtype, else float32."""
    if out_dtype is not None and not isinstance(out_dtype, torch.dtype):
        raise TypeError("%s: out_dtype must be a torch.dtype" % who)
    dts = {t.dtype for t in outs if isinstance(t, torch.Tensor)}
    if len(dts) > 1:
        raise RuntimeError("%s: out[0] and out[1] must have one dtype, got %s" % (who, " and ".join(sorted(map(str, dts)))))
    dt = dts.pop() if dts else (out_dtype if out_dtype is not None else torch.float32)
    if out_dtype is not None and out_dtype != dt:
        raise RuntimeError("%s: out_dtype %s conflicts with out's dtype %s" % (who, out_dtype, dt))
    if dt not in _MAP_DTYPES:
        raise RuntimeError("%s: the output must be float32, float16 or bfloat16, got %s" % (who, dt))
    return dt


def fine_descriptors(desc0_, title, rubbish, out=None, count=None, out_dtype=None):
    """second_layer.py:71-86: desc0_ = the three maps of ResNet2.forward2 on the stacked crops
    ([2B,64,48,48], [2B,64,24,24], [2B,128,12,12]); title [B,8] = compress_1(desc_l); rubbish [B,264]
    = compress_2(desc_l).  Returns desc [2,B,264,145] (desc[0], desc[1] feed the GNN).
    Maps in torch.channels_last memory format (all three) take the channels-last gather: same bits, 0.67x the HBM bytes.
    Maps in float16 / bfloat16 are widened to fp32 exactly in the kernel: desc is float32 and bit-identical to the call on
    [m.float() for m in desc0_]; title / rubbish may be half too (widened here).
    out_dtype (or the dtype of `out`, which decides when given): torch.float32 (default), float16 or bfloat16.  A half desc is
    the float32 desc rounded once, to nearest even, at the kernel's store - bit-identical to fine_descriptors(...).to(dtype)
    without the pass over it - and is what cost_ot takes as it lies."""
    odt = _out_dtype([out] if out is not None else [], out_dtype, "fine_descriptors")
    maps, dtype = _maps_any(list(desc0_), ["desc0_[%d]" % i for i in range(len(desc0_))])
    if len({cl for _, cl in maps}) != 1:       # mixed formats: fall back to the NCHW kernel on contiguous copies
        maps = [(t.contiguous(), False) for t, _ in maps]
    (f0, nhwc), (f1, _), (f2, _) = maps
    B = f0.shape[0] // 2
    if tuple(f0.shape[1:]) != (64, 48, 48) or tuple(f1.shape) != (2 * B, 64, 24, 24) or \
            tuple(f2.shape) != (2 * B, 128, 12, 12):
        raise RuntimeError("fine_descriptors: unexpected feature-map shapes")
    ti = _dev(_widen(title), "title").reshape(B, 8)
    ru = _dev(_widen(rubbish), "rubbish").reshape(B, 264)
    desc = torch.empty((2, B, 264, 145), dtype=odt, device=f0.device) if out is None else _dev(out, "out", odt)
    if tuple(desc.shape) != (2, B, 264, 145) or (out is not None and desc.data_ptr() != out.data_ptr()):
        raise RuntimeError("fine_descriptors: out must be a contiguous [2,B,264,145] tensor")
    cnt = _dev(count, "count", torch.int64) if count is not None else None      # device-side row count: B is a capacity
    if odt == torch.float32:
        _check(_L().pats_fine_descriptors_typed(_ptr(f0), _ptr(f1), _ptr(f2), dtype, int(bool(nhwc)), _ptr(ti), _ptr(ru), B,
                                                _ptr(cnt), _ptr(desc), _stream()), "fine_descriptors")
    else:
        _check(_L().pats_fine_descriptors_typed_out(_ptr(f0), _ptr(f1), _ptr(f2), dtype, int(bool(nhwc)), _ptr(ti), _ptr(ru), B,
                                                    _ptr(cnt), _ptr(desc), _MAP_DTYPES[odt], _stream()), "fine_descriptors")
    return desc


def third_descriptors(feat_f0, feat_f1, mkpts0_c, mkpts1_c, b_ids, kenc, rubbish, count=None, out=None, out_dtype=None):
    """third_layer.py:121-146.  Returns (feat_f0_unfold, feat_f1_unfold [P,128,65], mkpts0_c,
    mkpts1_c [P,2] int64 rounded to the 4-px lattice as the reference reassigns them).
    count: DEVICE int64 [1], the number of points that exist (the tensors are a capacity; rows past it are not written);
    out: optional (o0, o1) to write into.
    Maps in torch.channels_last memory format take the channels-last gather: same bits, under half the HBM bytes.
    Maps in float16 / bfloat16 are widened to fp32 exactly in the kernel: the outputs are float32 and bit-identical to the
    call on feat_f0.float(), feat_f1.float(); kenc / rubbish may be half too (widened here).
    out_dtype (or the dtype of out[0] and out[1], which must agree and decide when given): torch.float32 (default), float16 or
    bfloat16.  Half outputs are the float32 outputs rounded once, to nearest even, at the kernel's store - bit-identical to
    converting them afterwards - and are what third_level takes as they lie; the rounded points do not change.  Half outputs
    of channels-last maps must be 16-byte aligned (fresh tensors are); NCHW ones may sit at any element offset."""
    odt = _out_dtype(list(out) if out is not None else [], out_dtype, "third_descriptors")
    ((f0, nhwc), (f1, nhwc1)), dtype = _maps_any([feat_f0, feat_f1], ["feat_f0", "feat_f1"])
    if nhwc != nhwc1:
        f0, f1, nhwc = f0.contiguous(), f1.contiguous(), False
    B = f0.shape[0]
    if tuple(f0.shape[1:]) != (128, 52, 52) or f1.shape != f0.shape:
        raise RuntimeError("third_descriptors: feature maps must be [B,128,52,52]")
    m0 = _dev(mkpts0_c.float(), "mkpts0_c").reshape(-1, 2)
    m1 = _dev(mkpts1_c.float(), "mkpts1_c").reshape(-1, 2)
    P = m0.shape[0]
    bi = _dev(b_ids.to(torch.int64), "b_ids", torch.int64).reshape(P)
    ke = _dev(_widen(kenc), "kenc").reshape(128, 64)
    ru = _dev(_widen(rubbish), "rubbish").reshape(B, 128, 144)
    dev = f0.device
    if out is not None:
        o0, o1 = _dev(out[0], "out[0]", odt), _dev(out[1], "out[1]", odt)
        if tuple(o0.shape) != (P, 128, 65) or o1.shape != o0.shape or o0.data_ptr() != out[0].data_ptr():
            raise RuntimeError("third_descriptors: out must be two contiguous [P,128,65] tensors")
    else:
        o0 = torch.empty((P, 128, 65), dtype=odt, device=dev)
        o1 = torch.empty((P, 128, 65), dtype=odt, device=dev)
    ps = torch.empty((P, 2), dtype=torch.int64, device=dev)
    pt = torch.empty((P, 2), dtype=torch.int64, device=dev)
    cnt = _dev(count, "count", torch.int64).reshape(1) if count is not None else None
    if odt == torch.float32:
        _check(_L().pats_third_descriptors_typed(_ptr(f0), _ptr(f1), dtype, int(bool(nhwc)), _ptr(m0), _ptr(m1), _ptr(bi),
                                                 _ptr(ke), _ptr(ru), P, _ptr(cnt), B, _ptr(o0), _ptr(o1), _ptr(ps), _ptr(pt),
                                                 _stream()), "third_descriptors")
    else:
        _check(_L().pats_third_descriptors_typed_out(_ptr(f0), _ptr(f1), dtype, int(bool(nhwc)), _ptr(m0), _ptr(m1), _ptr(bi),
                                                     _ptr(ke), _ptr(ru), P, _ptr(cnt), B, _ptr(o0), _ptr(o1), _MAP_DTYPES[odt],
                                                     _ptr(ps), _ptr(pt), _stream()), "third_descriptors")
    return o0, o1, ps, pt


# ------------------------------------------------------------------------------------------------
# the steps either side of the OT path
# ------------------------------------------------------------------------------------------------
def _as_flags(t, name):
    """bool / uint8 tensor -> contiguous uint8 view sharing storage when it already is contiguous bool."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("pats_amd: %s must be a GPU tensor (no CPU fallback)" % name)
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError("pats_amd: %s must be bool or uint8, got %s" % (name, t.dtype))
    return t.contiguous()


def _merge_tensors(trust_score, if_nomatching1_L2, rows, who=None):
    """-> whether the merges' in-place tensors are what the C entries take: trust_score float32 and if_nomatching1_L2 bool, both
    contiguous and [rows,144].  With `who`, a wrong dtype or layout (or a trust_score off the GPU) raises that wrapper's message
    for the tensor instead, and only the extents are answered."""
    for t, name, dtype, kind in ((trust_score, "trust_score", torch.float32, "float32 GPU"),
                                 (if_nomatching1_L2, "if_nomatching1_L2", torch.bool, "bool")):
        if t.dtype != dtype or not t.is_contiguous() or (who and t is trust_score and not t.is_cuda):
            if who:
                raise RuntimeError("%s: %s must be a contiguous %s tensor (it is updated in place)" % (who, name, kind))
            return False
    return trust_score.numel() == rows * 144 and if_nomatching1_L2.numel() == rows * 144


def _merge_scores_back(scores_back, cells=None):
    """-> whether scores_back is what the merges take: float64, contiguous, [cells,16,9] (None: any extent)"""
    return scores_back.dtype == torch.float64 and scores_back.is_contiguous() and (cells is None or scores_back.numel() == cells * 144)


def _merge(merge_new, patch_num, trust_score, original_image_shape, if_nomatching1_L1, if_nomatching1_L2,
           scores_back, validate):
    B = trust_score.shape[0]
    shaped = _merge_tensors(trust_score, if_nomatching1_L2, B, "merge_patches")
    if not _merge_scores_back(scores_back):
        raise RuntimeError("merge_patches: scores_back must be a contiguous float64 tensor (it is updated in place)")
    if not shaped or int(patch_num) != B:
        raise RuntimeError("merge_patches: trust_score / if_nomatching1_L2 must be [patch_num,144]")
    H, W = int(original_image_shape[0]), int(original_image_shape[1])
    l1 = _as_flags(if_nomatching1_L1, "if_nomatching1_L1")
    bt = l1.shape[0]
    if l1.numel() != bt * (H // 32) * (W // 32) or scores_back.numel() != l1.numel() * 144:
        raise RuntimeError("merge_patches: if_nomatching1_L1 must be [batch, H/32*W/32], scores_back [batch, H/32*W/32, 16, 9]")
    if validate and int((l1 == 0).sum()) != B:          # the reference's masked assignment raises here (:160 / :209)
        raise IndexError("merge_patches: %d unmasked coarse patches but %d rows of trust_score" % (int((l1 == 0).sum()), B))
    dev = trust_score.device
    out = torch.empty((B, 144), dtype=torch.bool, device=dev)
    nws = _L().pats_merge_workspace_bytes(B, H, W, bt)
    ws = _workspace(nws, dev)
    _check(_L().pats_merge_patches(1 if merge_new else 0, B, _ptr(trust_score), H, W, bt, _ptr(l1),
                                   _ptr(if_nomatching1_L2.view(torch.uint8)), _ptr(scores_back), _ptr(out.view(torch.uint8)),
                                   _ptr(ws), nws, _stream()), "merge_patches")
    return out


def merge_patches_new(patch_num, trust_score, original_image_shape, if_nomatching1_L1, if_nomatching1_L2, scores_back,
                      validate=True):
    """SecondLayer.merge_patches_new (second_layer.py:193-240).  trust_score, if_nomatching1_L2 and
    scores_back are updated in place as in the reference; returns (if_nomatching [B,144], scores_back)."""
    out = _merge(True, patch_num, trust_score, original_image_shape, if_nomatching1_L1, if_nomatching1_L2,
                 scores_back, validate)
    return out, scores_back


def merge_patches_old(patch_num, trust_score, original_image_shape, if_nomatching1_L1, if_nomatching1_L2, scores_back,
                      validate=True):
    """SecondLayer.merge_patches_old (second_layer.py:137-191); hands back a zeroed scores_back (:191)."""
    out = _merge(False, patch_num, trust_score, original_image_shape, if_nomatching1_L1, if_nomatching1_L2,
                 scores_back, validate)
    return out, torch.zeros_like(scores_back)


def third_inputs(if_nomatching, pts, capacity=None, sync=True):
    """pats.py:53-58: (mkpts0_c [P,2], mkpts1_c [P,2], b_ids [P]) of the surviving L2 cells - the arguments
    PATS.forward passes to ThirdLayer (third_input[:, :2] * 2, third_input[:, 2:4] * 2, third_input[:, -1]).
    One host read of P (the reference's boolean-mask indexing syncs at the same point).
    sync=False makes none: returns (mkpts0_c [cap,2], mkpts1_c [cap,2], b_ids [cap], P [1] int64 DEVICE count) with
    `capacity` rows (default B*144), only the first min(P, cap) written."""
    f = _as_flags(if_nomatching, "if_nomatching")
    B = f.shape[0]
    p = _dev(pts, "pts").reshape(B, 144, 2)
    if f.numel() != B * 144:
        raise RuntimeError("third_inputs: if_nomatching must be [B,144]")
    dev = p.device
    cap = B * 144 if capacity is None else int(capacity)
    mk0 = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    mk1 = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    bi = torch.empty((cap,), dtype=torch.int64, device=dev)
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)                  # always written by the scan
    nws = _L().pats_compact_workspace_bytes(B * 144)
    ws = _workspace(nws, dev)
    _check(_L().pats_third_inputs_f32(_ptr(f), _ptr(p), B, _ptr(mk0), _ptr(mk1), _ptr(bi), cap, _ptr(cnt), _ptr(ws), nws,
                                      _stream()), "third_inputs")
    if not sync:
        return mk0, mk1, bi, cnt
    P = int(cnt.item())
    return mk0[:P], mk1[:P], bi[:P]


def refine_scatter(if_nomatching, pts, mkpts1_f, label, conf=None):
    """pats.py:59-67: (if_nomatching16 [B,2304] bool, pts16 [B,2304,2]) on the 48x48 sub-cell grid.
    `label` is ThirdLayer's [P*16,2] tensor (column 0 is read) or a 1-D [P*16] tensor.
    conf (third_level's [P,16] confidence): a third element conf16 [B,2304] float32 is returned, scattered by the permutation
    pts16 gets, 0 where if_nomatching16 is set."""
    f = _as_flags(if_nomatching, "if_nomatching")
    B = f.shape[0]
    p = _dev(pts, "pts").reshape(B, 144, 2)
    mk = _dev(mkpts1_f, "mkpts1_f").reshape(-1, 16, 2)
    P = mk.shape[0]
    lb = _dev(label, "label")
    stride = 2 if lb.dim() == 2 else 1
    if lb.numel() != P * 16 * stride:
        raise RuntimeError("refine_scatter: label must be [P*16,2] or [P*16]")
    dev = p.device
    f16 = torch.empty((B, 2304), dtype=torch.bool, device=dev)
    p16 = torch.empty((B, 2304, 2), dtype=torch.float32, device=dev)
    nws = _L().pats_compact_workspace_bytes(B * 144)
    ws = _workspace(nws, dev)
    entry, cf_arg, c16_arg, res = "pats_refine_scatter_f32", (), (), (f16, p16)
    if conf is not None:            # the confidence form: conf behind the label's stride, conf16 behind pts16
        cf = _dev(conf, "conf")
        if cf.numel() != P * 16:
            raise RuntimeError("refine_scatter: conf must be [P,16]")
        c16 = torch.empty((B, 2304), dtype=torch.float32, device=dev)
        entry, cf_arg, c16_arg, res = "pats_refine_scatter_conf_f32", (_ptr(cf),), (_ptr(c16),), (f16, p16, c16)
    _check(getattr(_L(), entry)(_ptr(f), _ptr(p), _ptr(mk), _ptr(lb), stride, *cf_arg, B, P, _ptr(f16.view(torch.uint8)), _ptr(p16),
                                *c16_arg, _ptr(ws), nws, _stream()), "refine_scatter")
    return res


def get_result(batch_size, if_nomatching, average_point, scale, patch_size, left_choice, layer_num=2, validate=True,
               sync=True):
    """utils.get_result (utils.py:189-213) for the two-level call of pats.py:73: returns (matches_l,
    matches_r) [M,2].  scale[1] may be the reference's [K,n1,2] tensor or a [K,2] / [K,1,2] tensor holding
    one scale per row (what pats.py:70 repeats over the sub-cells).
    sync=False makes no host read: returns (matches_l [cap,2], matches_r [cap,2], M [1] int64 DEVICE count),
    only the first M rows written (throughput mode; the reference reads M when it masks)."""
    if layer_num != 2 or len(if_nomatching) != 2:
        raise RuntimeError("get_result: only the reference's layer_num=2 call is implemented")
    f0, f1 = _as_flags(if_nomatching[0], "if_nomatching[0]"), _as_flags(if_nomatching[1], "if_nomatching[1]")
    z0, z1 = [int(v) for v in patch_size[0]], [int(v) for v in patch_size[1]]
    n0, n1 = z0[1] * z0[2], z1[1] * z1[2]
    bs, rows1 = int(batch_size), f1.shape[0]
    if f0.numel() != bs * n0 or f1.numel() != rows1 * n1:
        raise RuntimeError("get_result: if_nomatching shapes do not match patch_size")
    a0, a1 = _dev(average_point[0], "average_point[0]"), _dev(average_point[1], "average_point[1]")
    s0, s1 = _dev(scale[0], "scale[0]"), _dev(scale[1], "scale[1]")
    if a0.numel() != bs * n0 * 2 or s0.numel() != bs * n0 * 2 or a1.numel() != rows1 * n1 * 2:
        raise RuntimeError("get_result: average_point / scale shapes do not match")
    if s1.numel() == rows1 * n1 * 2:
        stride = 2
    elif s1.numel() == rows1 * 2:
        stride = 0
    else:
        raise RuntimeError("get_result: scale[1] must be [K,n1,2] or [K,2]")
    c0, c1 = _as_flags(left_choice[0], "left_choice[0]"), _as_flags(left_choice[1], "left_choice[1]")
    if c0.numel() != bs or c1.numel() != rows1:
        raise RuntimeError("get_result: left_choice shapes do not match")
    if validate and int((f0 == 0).sum()) != rows1:
        raise IndexError("get_result: %d surviving level-0 cells but %d level-1 rows" % (int((f0 == 0).sum()), rows1))
    dev = a0.device
    cap = rows1 * n1
    ml = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    mr = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)                  # always written by the scan
    nws = _L().pats_get_result_workspace_bytes(bs * n0, rows1, n1)
    ws = _workspace(nws, dev)
    ps0, ps1 = (ctypes.c_int * 3)(*z0), (ctypes.c_int * 3)(*z1)
    _check(_L().pats_get_result_f32(bs, _ptr(f0), _ptr(f1), rows1, _ptr(a0), _ptr(a1), _ptr(s0), _ptr(s1), stride, ps0, ps1,
                                    _ptr(c0), _ptr(c1), _ptr(ml), _ptr(mr), cap, _ptr(cnt), _ptr(ws), nws, _stream()),
           "get_result")
    if not sync:
        return ml, mr, cnt
    M = int(cnt.item())
    return ml[:M], mr[:M]


# ------------------------------------------------------------------------------------------------
# throughput mode: the chunk loop of PATS.forward for a batch of pairs, no host read (csrc/batch.hip)
# ------------------------------------------------------------------------------------------------
class ChunkRows:
    """The row table pats_chunk_rows_device / pats_chunk_rows_ragged build (include/pats_amd.h): device tensors only.
    row_pair [rows_cap] (pair of the row, -1 past the total) and cell_base [pairs + 1] (pair p owns the packed cells
    cell_base[p] .. cell_base[p + 1]) serve both kinds of batch; `table` is the PairTable of a ragged batch (h = w = None
    there) and None for a uniform one."""
    __slots__ = ("pairs", "h", "w", "Cmax", "rows_cap", "sum_cycle", "cycle_num", "second", "third", "masks", "chunk_base",
                 "crop_base", "row_cell", "row_forced", "row_crop", "row_slot", "status", "table", "_row_pair", "_cell_base")

    @property
    def row_pair(self):
        if getattr(self, "_row_pair", None) is None:          # uniform table: row_cell // N, formed on first use
            N = self.h * self.w
            self._row_pair = torch.where(self.row_cell >= 0, torch.div(self.row_cell, N, rounding_mode="floor"),
                                         torch.full_like(self.row_cell, -1))
        return self._row_pair

    @property
    def cell_base(self):
        if getattr(self, "_cell_base", None) is None:
            self._cell_base = torch.arange(self.pairs + 1, dtype=torch.int64, device=self.row_cell.device) * (self.h * self.w)
        return self._cell_base


class PairTable:
    """The shapes of a ragged batch (pats_pair_table_t): grids (h_p, w_p) in batch order, packed cell ranges and the offsets
    of the pairs' [32 h_p, 32 w_p, 3] images in a flat store - host copies (validated by every call) and device tensors."""

    def __init__(self, shapes, device):
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.pairs = len(self.shapes)
        self.shape_host = np.ascontiguousarray(np.array(self.shapes, np.int32).reshape(self.pairs, 2))
        n = self.shape_host[:, 0].astype(np.int64) * self.shape_host[:, 1]
        self.cell_base_host = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        self.img_base_host = np.concatenate([[0], np.cumsum(n * 1024 * 3)])[:-1].astype(np.int64)
        self.cells = int(self.cell_base_host[-1])
        self.hmax = int(self.shape_host[:, 0].max()) if self.pairs else 0
        self.shape = torch.from_numpy(self.shape_host).to(device)
        self.cell_base = torch.from_numpy(self.cell_base_host).to(device)
        self.img_base = torch.from_numpy(self.img_base_host).to(device)
        self.ct = _lib.PairTable(self.pairs, self.shape_host.ctypes.data, self.cell_base_host.ctypes.data, self.shape.data_ptr(),
                                 self.cell_base.data_ptr(), self.img_base.data_ptr())

    def ref(self):
        return ctypes.byref(self.ct)


def max_chunks(height, width, max_once_used):
    """Upper bound of split_patches' chunk count: a chunk closes when the cumulative match count passes a multiple of
    max_once_used (utils.py:157), at most once per grid row."""
    return min(height + 1, (height * width - 1) // int(max_once_used) + 1)


def _chunk_rows_table(table, pairs, h, w, hmax, cell_ext, Cmax, rows_cap, dev):
    """A ChunkRows with every tensor the planner writes allocated - what chunk_rows and chunk_rows_ragged share.  cell_ext: the
    extents of a per-cell tensor, (pairs, N) for a uniform batch and (sum N,) for a ragged one (`table` its PairTable)."""
    r = ChunkRows()
    r.table, r.pairs, r.h, r.w, r.Cmax, r.rows_cap = table, pairs, h, w, Cmax, rows_cap
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    r.sum_cycle = torch.empty(cell_ext, dtype=i32, device=dev)
    r.cycle_num = torch.empty((pairs,), dtype=i32, device=dev)
    r.second = torch.empty((pairs, hmax + 1, 2), dtype=i64, device=dev)
    r.third = torch.empty((pairs, hmax + 1, 2), dtype=i64, device=dev)
    r.masks = torch.empty((Cmax,) + cell_ext, dtype=torch.bool, device=dev)
    r.chunk_base = torch.empty((Cmax + 1,), dtype=i64, device=dev)
    r.crop_base = torch.empty((pairs + 1,), dtype=i64, device=dev)
    r.row_cell = torch.empty((rows_cap,), dtype=i32, device=dev)
    # a ragged table is told each row's pair; a uniform one forms row_cell // N and the cell ranges on first use (ChunkRows)
    r._row_pair = torch.empty((rows_cap,), dtype=i32, device=dev) if table is not None else None
    r._cell_base = table.cell_base if table is not None else None
    r.row_forced = torch.empty((rows_cap,), dtype=u8, device=dev)
    r.row_crop = torch.empty((rows_cap,), dtype=i32, device=dev)
    r.row_slot = torch.empty((Cmax, r.sum_cycle.numel()), dtype=i32, device=dev)
    r.status = torch.empty((1,), dtype=i32, device=dev)
    return r


def _chunk_rows_plan(r, head, what):
    """The planner's call on a _chunk_rows_table: `head` = the arguments in front of the outputs; r.row_pair goes behind row_cell
    for a ragged table."""
    entry, pair_arg = ("pats_chunk_rows_device", ()) if r.table is None else ("pats_chunk_rows_ragged", (_ptr(r._row_pair),))
    dev = r.status.device
    nws = _L().pats_chunk_rows_workspace_bytes(r.pairs, r.Cmax)
    ws = _workspace(nws, dev)
    _check(getattr(_L(), entry)(*head, r.Cmax, r.rows_cap, _ptr(r.sum_cycle), _ptr(r.cycle_num), _ptr(r.second), _ptr(r.third),
                                _ptr(r.masks.view(torch.uint8)), _ptr(r.chunk_base), _ptr(r.crop_base), _ptr(r.row_cell), *pair_arg,
                                _ptr(r.row_forced), _ptr(r.row_crop), _ptr(r.row_slot), _ptr(r.status), _ptr(ws), nws, _stream()), what)
    return r


def chunk_rows(if_nomatching1, height, width, max_once_used, Cmax=None, rows_cap=None):
    """first_layer.py:130-146 + pats.py:33-39 for a batch of pairs on the device: cumulative match counts, chunk plans,
    chunk masks and the fine level's row table in (chunk, pair, cell) order.  if_nomatching1 [pairs, h*w] bool."""
    f = _as_flags(if_nomatching1, "if_nomatching1")
    pairs, N = f.shape[0], height * width
    if f.numel() != pairs * N:
        raise RuntimeError("chunk_rows: if_nomatching1 must be [pairs, height*width]")
    Cmax = max_chunks(height, width, max_once_used) if Cmax is None else int(Cmax)
    rows_cap = pairs * (N + (Cmax - 1) * width) if rows_cap is None else int(rows_cap)
    r = _chunk_rows_table(None, pairs, int(height), int(width), height, (pairs, N), Cmax, rows_cap, f.device)
    return _chunk_rows_plan(r, (_ptr(f), pairs, int(height), int(width), int(max_once_used)), "chunk_rows")


def merge_patches_batch(merge_new, rows, trust_score, original_image_shape, if_nomatching1_L2, scores_back=None):
    """SecondLayer.merge_patches_new / _old (second_layer.py:137-238) for every chunk of every pair of a ChunkRows table,
    chunk blocks in order, pats.py:38-39 applied.  trust_score / if_nomatching1_L2 [rows_cap,144] are updated in place;
    scores_back [pairs, N, 16, 9] float64 (zeros if None, pats.py:32).  Returns if_nomatching [rows_cap,144] bool."""
    table = rows.table
    if table is None:
        H, W = int(original_image_shape[0]), int(original_image_shape[1])
        on_grid, cells, sb_shape = H // 32 == rows.h and W // 32 == rows.w, rows.pairs * rows.h * rows.w, (rows.pairs, rows.h * rows.w, 16, 9)
        entry, what, sizer, size_args = "pats_merge_patches_batch", "merge_patches_batch", "pats_merge_batch_workspace_bytes", (rows.pairs, H, W)
        head, pair_arg = (1 if merge_new else 0, rows.Cmax, rows.pairs, H, W, rows.rows_cap), ()
    else:                           # ragged: the table carries the grids (original_image_shape is not read), row_pair the rows' pairs
        on_grid, cells, sb_shape = True, table.cells, (table.cells, 16, 9)
        entry, what, sizer, size_args = "pats_merge_patches_ragged", "merge_patches_ragged", "pats_merge_ragged_workspace_bytes", (cells,)
        head, pair_arg = (table.ref(), 1 if merge_new else 0, rows.Cmax, rows.rows_cap), (_ptr(rows.row_pair),)
    if not _merge_tensors(trust_score, if_nomatching1_L2, rows.rows_cap, "merge_patches_batch") or not on_grid:
        raise RuntimeError("merge_patches_batch: tensors must be [rows_cap,144]" + (" on the table's grid" if table is None else ""))
    dev = trust_score.device
    fresh = scores_back is None
    if fresh:
        scores_back = torch.empty(sb_shape, dtype=torch.float64, device=dev)            # cleared by the call
    elif not _merge_scores_back(scores_back, cells):
        raise RuntimeError("merge_patches_batch: scores_back must be a contiguous float64 [%s, 16, 9] tensor"
                           % ("pairs, N" if table is None else "sum N"))
    out = torch.empty((rows.rows_cap, 144), dtype=torch.bool, device=dev)
    nws = getattr(_L(), sizer)(*size_args)
    ws = _workspace(nws, dev)
    _check(getattr(_L(), entry)(*head, _ptr(rows.chunk_base), _ptr(rows.row_cell), *pair_arg, _ptr(rows.row_slot), _ptr(rows.row_forced),
                                _ptr(trust_score), _ptr(if_nomatching1_L2.view(torch.uint8)), _ptr(scores_back), int(fresh),
                                _ptr(out.view(torch.uint8)), _ptr(ws), nws, _stream()), what)
    return out


def merge_patches_chunk(merge_new, rows, c, row_origin, trust_score, original_image_shape, if_nomatching1_L2, scores_back,
                        first=False):
    """merge_patches_new / _old for chunk `c` of a ChunkRows table on that chunk's own tensors (trust_score / if_nomatching1_L2
    [B,144] = table rows row_origin .. row_origin + B, updated in place): PATS.forward's chunk loop walked chunk by chunk
    (pats.py:33-39) with one launch per chunk and no host read.  scores_back [pairs,N,16,9] float64 is handed from call to
    call (first=True clears it, pats.py:32).  Returns if_nomatching [B,144] bool (pats.py:38-39 applied)."""
    B = trust_score.shape[0]
    H, W = int(original_image_shape[0]), int(original_image_shape[1])
    if not _merge_tensors(trust_score, if_nomatching1_L2, B):
        raise RuntimeError("merge_patches_chunk: trust_score / if_nomatching1_L2 must be contiguous [B,144] float32 / bool")
    if not _merge_scores_back(scores_back, rows.pairs * rows.h * rows.w):
        raise RuntimeError("merge_patches_chunk: scores_back must be a contiguous float64 [pairs, N, 16, 9] tensor")
    dev = trust_score.device
    out = torch.empty((B, 144), dtype=torch.bool, device=dev)
    nws = _L().pats_merge_batch_workspace_bytes(rows.pairs, H, W)
    ws = _workspace(nws, dev)
    _check(_L().pats_merge_patches_chunks(1 if merge_new else 0, rows.Cmax, int(c), int(c) + 1, rows.pairs, H, W, int(row_origin), B,
                                          _ptr(rows.chunk_base), _ptr(rows.row_cell), _ptr(rows.row_slot), _ptr(rows.row_forced),
                                          _ptr(trust_score), _ptr(if_nomatching1_L2.view(torch.uint8)), _ptr(scores_back),
                                          int(bool(first)), _ptr(out.view(torch.uint8)), _ptr(ws), nws, _stream()),
           "merge_patches_chunk")
    return out


def _carve(device, *sizes):
    """One allocation for several internal tensors of a fused call: returns (arena, [device addresses])."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (int(n) + 255) & ~255
    arena = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    base = arena.data_ptr()
    return arena, [ctypes.c_void_p(base + o) for o in offs]


def chunk_fine_tail(f0, f1, one, ns, scale_x, scale_y, iters, bias_k, merge_new, rows, c, row_origin, image_shape, scores_back, first,
                    wait_before_merge=None, record_after_merge=None):
    """Everything between the fine network callback and the third one for ONE chunk of a pair walked chunk by chunk, in one C
    call (pats_chunk_fine_tail_f32, csrc/chunk_walk.cpp): second_layer.py:100-122 (cost build, log_optimal_transport2 + ln k,
    est_position, the chunk's merge through the row table `rows`) and pats.py:37-39,53-58 (tail rows, the third level's inputs over
    the capacity 144 B).  Returns (merged [B,144] bool, points [B,144,2], mkpts0_c [144 B,2], mkpts1_c, b_ids [144 B], P [1] int64
    on the device); the log plan, flags and the other expansion outputs stay internal.
    wait_before_merge / record_after_merge: torch.cuda.Event objects (already recorded once, so that their handles exist) - the
    stream waits for the first right before the merge and re-records the second right behind it.
    float16 / bfloat16 descriptors are widened with .float() here (the chunk walk's C entry reads float32 only)."""
    d0, d1 = _dev(_widen(f0), "f0"), _dev(_widen(f1), "f1")
    B = d0.shape[0]
    if tuple(d0.shape) != (B, 264, 145) or d1.shape != d0.shape:
        raise RuntimeError("chunk_fine_tail: descriptors must be [B,264,145]")
    nsv, sx, sy = _dev(ns, "ns").reshape(B, 144), _dev(scale_x, "scale_x").reshape(B, 144), _dev(scale_y, "scale_y").reshape(B, 144)
    H, W = int(image_shape[0]), int(image_shape[1])
    dev = d0.device
    merged = torch.empty((B, 144), dtype=torch.bool, device=dev)
    pts = torch.empty((B, 144, 2), dtype=torch.float32, device=dev)
    mk = torch.empty((2, B * 144, 2), dtype=torch.float32, device=dev)
    bi = torch.empty((B * 144,), dtype=torch.int64, device=dev)
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)
    nws = _L().pats_chunk_fine_tail_workspace_bytes(B, rows.pairs, H, W)
    n1 = B * 144
    arena, (Z, cflag, trust, core, xs, ys, bound, rflag, ws) = _carve(dev, B * 145 * 145 * 4, n1, n1 * 4, n1 * 4, n1 * 4, n1 * 4, n1 * 4 * 8,
                                                                      n1, nws)
    _check(_L().pats_chunk_fine_tail_f32(_ptr(d0), _ptr(d1), B, _ptr(_scalar_dev(one, dev)), _ptr(nsv), int(iters), float(bias_k), _ptr(sx),
                                         _ptr(sy), 1 if merge_new else 0, rows.Cmax, int(c), rows.pairs, H, W, int(row_origin),
                                         _ptr(rows.chunk_base), _ptr(rows.row_cell), _ptr(rows.row_slot), _ptr(rows.row_forced),
                                         _ptr(scores_back), int(bool(first)), Z, cflag, trust, core, _ptr(pts), xs, ys, bound, rflag,
                                         _ptr(merged.view(torch.uint8)), _ptr(mk[0]), _ptr(mk[1]), _ptr(bi), _ptr(cnt),
                                         ctypes.c_void_p(wait_before_merge.cuda_event if wait_before_merge is not None else 0),
                                         ctypes.c_void_p(record_after_merge.cuda_event if record_after_merge is not None else 0),
                                         ws, nws, _stream()),
           "chunk_fine_tail")
    return merged, pts, mk[0], mk[1], bi, cnt


def chunk_third_tail(feat0, feat1, P, scale, p_s, p_t, iters, outdoor, merged, points, chunk_mask, h, w, pts_new, scales):
    """Everything behind the third network callback for ONE chunk, in one C call (pats_chunk_third_tail_f32): third_layer.py:153-170
    over the capacity 144 B with the count P on the device, pats.py:59-67 (scatter onto the sub-cell grid) and :68-78 (get_result with
    the chunk's mask [h w] as the level-0 flags; pts_new / scales = Compute_imgs' [1, h w, 2] tensors).  Returns (matches_l, matches_r
    [2304 B, 2], M [1] int64 on the device): the first M rows are the chunk's matches in the reference's order.
    float16 / bfloat16 descriptors are widened with .float() here (the chunk walk's C entry reads float32 only)."""
    a, b = _dev(_widen(feat0), "feat0"), _dev(_widen(feat1), "feat1")
    Pc = a.shape[0]
    B = merged.shape[0]
    if tuple(a.shape) != (Pc, 128, 65) or b.shape != a.shape or Pc != B * 144:
        raise RuntimeError("chunk_third_tail: descriptors must be [144 B,128,65]")
    sc = _dev(scale, "scale").reshape(Pc, 64)
    ps = _dev(p_s.to(torch.int64), "p_s", torch.int64).reshape(Pc, 2)
    pt = _dev(p_t.to(torch.int64), "p_t", torch.int64).reshape(Pc, 2)
    dev = a.device
    ml = torch.empty((B * 2304, 2), dtype=torch.float32, device=dev)
    mr = torch.empty((B * 2304, 2), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)
    nws = _L().pats_chunk_third_tail_workspace_bytes(B, int(h), int(w))
    arena, (m0, m1, label, ifm, f16, p16, mrow, ws) = _carve(dev, Pc * 32 * 4, Pc * 32 * 4, Pc * 32 * 4, Pc * 16, B * 2304, B * 2304 * 8,
                                                             B * 2304 * 4, nws)
    _check(_L().pats_chunk_third_tail_f32(_ptr(a), _ptr(b), Pc, _ptr(_dev(P, "P", torch.int64)), _ptr(sc), _ptr(ps), _ptr(pt), int(iters),
                                          int(bool(outdoor)), _ptr(_as_flags(merged, "merged")), _ptr(_dev(points, "points")), B,
                                          _ptr(_as_flags(chunk_mask, "chunk_mask")), int(h), int(w), _ptr(_dev(pts_new, "pts_new")),
                                          _ptr(_dev(scales, "scales")), _ptr(_ones(B, dev)), m0, m1, label, ifm, f16, p16, _ptr(ml), _ptr(mr),
                                          mrow, _ptr(cnt), ws, nws, _stream()), "chunk_third_tail")
    return ml, mr, cnt


_ONES = {}


def _ones(n, device):
    key = (int(n), str(device))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((int(n),), dtype=torch.uint8, device=device)
    return t


def get_result_chunks(rows, if_nomatching16, pts_new, pts16, scales, patch_size=((32, None, None), (2, 48, 48)), conf16=None):
    """get_result (utils.py:189-213) for every (chunk, pair) of a ChunkRows table in one call, as PATS.forward issues it per
    chunk (pats.py:68-73): pts_new / scales = Compute_imgs' per-pair [pairs,N,2] tensors, pts16 [rows_cap,2304,2] /
    if_nomatching16 [rows_cap,2304] from refine_scatter.  No host read.  Returns (matches_l [cap,2], matches_r [cap,2],
    match_row [cap] int32, M [1] int64 device): the first M rows are valid, match_row -> rows.row_cell // N = pair.
    conf16 (refine_scatter's [rows_cap,2304]): a fifth element match_conf [cap] float32, compacted into the matches' slots."""
    f16 = _as_flags(if_nomatching16, "if_nomatching16")
    if conf16 is not None:
        conf16 = _dev(conf16, "conf16")
        if conf16.numel() != f16.numel():
            raise RuntimeError("get_result_chunks: conf16 must have if_nomatching16's shape")
    table = rows.table
    z1 = [int(v) for v in patch_size[1]]
    n1 = z1[1] * z1[2]
    if table is not None and int(patch_size[0][0]) != 32:
        raise RuntimeError("get_result_chunks: the level-0 patch size of the path is 32")
    if f16.numel() != rows.rows_cap * n1:
        raise RuntimeError("get_result_chunks: if_nomatching16 must be [rows_cap, %d]" % n1)
    a0, a1, s0 = _dev(pts_new, "pts_new"), _dev(pts16, "pts16"), _dev(scales, "scales")
    cells = table.cells if table is not None else rows.pairs * rows.h * rows.w
    if a0.numel() != cells * 2 or s0.numel() != cells * 2 or a1.numel() != rows.rows_cap * n1 * 2:
        raise RuntimeError("get_result_chunks: pts_new / scales must be [%s,2], pts16 [rows_cap,%d,2]"
                           % ("sum N" if table is not None else "pairs,N", n1))
    dev = a0.device
    cap = rows.rows_cap * n1
    ml = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    mr = torch.empty((cap, 2), dtype=torch.float32, device=dev)
    mrow = torch.empty((cap,), dtype=torch.int32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int64, device=dev)
    nws = _L().pats_get_result_workspace_bytes(rows.Cmax * cells, rows.rows_cap, n1)
    ws = _workspace(nws, dev)
    ps1 = (ctypes.c_int * 3)(*z1)
    if table is None:               # the uniform entries take the pair count and the level-0 patch size, the ragged ones the table
        head, sizes, what = (rows.Cmax, rows.pairs), ((ctypes.c_int * 3)(int(patch_size[0][0]), rows.h, rows.w), ps1), "get_result_chunks"
    else:
        head, sizes, what = (table.ref(), rows.Cmax), (ps1,), "get_result_chunks_ragged"
    conf_arg, mc_arg, res = (), (), (ml, mr, mrow, cnt)
    if conf16 is not None:
        mc = torch.empty((cap,), dtype=torch.float32, device=dev)
        conf_arg, mc_arg, res = (_ptr(conf16),), (_ptr(mc),), (ml, mr, mrow, cnt, mc)
    entry = _GET_RESULT_CHUNKS[table is not None][conf16 is not None]
    _check(getattr(_L(), entry)(*head, _ptr(rows.masks.view(torch.uint8)), _ptr(f16), rows.rows_cap, _ptr(a0), _ptr(a1), _ptr(s0), *conf_arg,
                                *sizes, _ptr(_ones(rows.Cmax * rows.pairs, dev)), _ptr(_ones(rows.rows_cap, dev)), _ptr(ml), _ptr(mr),
                                *mc_arg, _ptr(mrow), cap, _ptr(cnt), _ptr(ws), nws, _stream()), what)
    return res


# the entries of get_result_chunks and matches_by_pair by [ragged][confidence]
_GET_RESULT_CHUNKS = (("pats_get_result_chunks_f32", "pats_get_result_chunks_conf_f32"),
                      ("pats_get_result_chunks_ragged_f32", "pats_get_result_chunks_ragged_conf_f32"))
_MATCHES_BY_PAIR = (("pats_matches_by_pair_summary_f32", "pats_matches_by_pair_summary_conf_f32"),
                    ("pats_matches_by_row_pair_summary_f32", "pats_matches_by_row_pair_summary_conf_f32"))


def matches_by_pair(rows, matches_l, matches_r, match_row, M, out=None, P=None, match_conf=None):
    """The matches of a batch (get_result_chunks) grouped by pair ON THE DEVICE: (matches_l, matches_r) with every pair's
    list contiguous in the reference's order, and pair_off [pairs + 1] int64 (pair p = rows pair_off[p] .. pair_off[p + 1]).
    What batch.split_by_pair reads back is then only pair_off.  out: optional (out_l, out_r, pair_off) to write into.
    P (device int64 [1], the step's third-level problem count): pair_off is then the first pairs + 1 entries of a pairs + 4
    buffer whose tail is (M, P, table status) - returned as a fourth element: the whole hand-over in ONE device-to-host copy.
    match_conf (get_result_chunks' fifth element): regrouped with the matches and returned as the LAST element; out may then
    carry its destination as a fourth tensor (out_l, out_r, pair_off, conf)."""
    dev = matches_l.device
    n_off = rows.pairs + 1 + (3 if P is not None else 0)
    if out is None:
        out = (torch.empty_like(matches_l), torch.empty_like(matches_r), torch.empty((n_off,), dtype=torch.int64, device=dev))
    ol, orr, off = out[:3]
    if off.numel() != n_off or not off.is_contiguous():
        raise RuntimeError("matches_by_pair: pair_off must be a contiguous int64 tensor of %d entries" % n_off)
    nws = _L().pats_matches_by_pair_workspace_bytes(rows.Cmax, rows.pairs)
    ws = _workspace(nws, dev)
    mc_arg, oc_arg, res = (), (), ((ol, orr, off) if P is None else (ol, orr, off[:rows.pairs + 1], off))
    if match_conf is not None:
        mc = _dev(match_conf, "match_conf").reshape(-1)
        oc = out[3] if len(out) > 3 else torch.empty_like(mc)
        if mc.numel() != matches_l.shape[0] or oc.numel() != mc.numel() or oc.dtype != torch.float32 or not oc.is_contiguous():
            raise RuntimeError("matches_by_pair: match_conf and its destination must be contiguous float32 [cap] tensors")
        mc_arg, oc_arg, res = (_ptr(mc),), (_ptr(oc),), res + (oc,)
    # the pair of a row: row_pair[row] in a ragged batch (there is no global N), row_cell[row] // N in a uniform one
    pair_args = (_ptr(rows.row_pair),) if rows.table is not None else (_ptr(rows.row_cell),)
    grid_arg = () if rows.table is not None else (rows.h * rows.w,)
    if P is None and match_conf is None and rows.table is None:
        entry, tail = "pats_matches_by_pair_f32", ()                # the one entry without the summary's two pointers
    else:                           # without P the call writes the pairs + 1 offsets only (null status): the buffer holds no more
        entry = _MATCHES_BY_PAIR[rows.table is not None][match_conf is not None]
        tail = (_ptr(_dev(P, "P", torch.int64)), _ptr(rows.status)) if P is not None else (None, None)
    _check(getattr(_L(), entry)(_ptr(matches_l), _ptr(matches_r), *mc_arg, _ptr(match_row), _ptr(M), *pair_args, _ptr(rows.chunk_base),
                                rows.Cmax, rows.pairs, *grid_arg, _ptr(ol), _ptr(orr), *oc_arg, _ptr(off), *tail, _ptr(ws), nws,
                                _stream()), "matches_by_pair")
    return res


# ---- what the per-pair hand-over stages below (top-K, epipolar score / hypotheses / pose) check alike; fn = the public
# function's name, the prefix of every message.  A new per-pair stage calls these instead of copying a neighbour. ----
def _bp_layout(fn, named, types=()):
    """Contiguity and dtype of the (tensor, name) pairs that are tensors - float32 unless `types` {name: dtype} says otherwise.
    The FIRST check of a stage: a bad layout or type is refused the same way with or without a GPU."""
    types = dict(types)
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            continue
        if not t.is_contiguous():
            raise RuntimeError("%s: %s must be contiguous" % (fn, name))
        want = types.get(name, torch.float32)
        if t.dtype != want:
            raise RuntimeError("%s: %s must be %s, got %s" % (fn, name, str(want).replace("torch.", ""), t.dtype))


def _bp_one_form(fn, pair_off, stride, counts):
    """Exactly one segment form: pair_off (ragged), or stride and counts (strided)."""
    if (pair_off is None) == (counts is None) or (stride is None) != (counts is None):
        raise RuntimeError("%s: give either pair_off, or stride and counts" % fn)


# What tells the families of the hypothesis, verification and local-optimisation stages apart, as data: the name and width of the
# first list; whether it and matches_r must have the same shape (else the same number of rows: lifted points are flat beside a top-K's
# [pairs,K,2]) and what the refusal of the two says; the shape of a model, as a tuple and as the messages write it with
# the family's letter for the model count; whether a local optimisation returns moments, or takes steps and returns cost.
_Family = collections.namedtuple("_Family", "first width same_shape lists model models letter moments cost")
_EPI = _Family("matches_l", 2, True, "matches_l / matches_r must be [cap,2]", (3, 3), "[pairs,H,3,3]", "H", True, False)
_ABS = _Family("points", 3, False, "points must be [cap,3] and matches_r [cap,2]", (3, 4), "[pairs,M,3,4]", "M", False, True)


def _bp_flat(t, width):
    """A GPU list [cap,width] (or top-K's [pairs,K,width]) as the flat [cap,width] list it is - None for any other shape."""
    shape = t.shape
    if len(shape) < 2 or shape[-1] != width:
        return None
    return t if len(shape) == 2 else t.reshape(-1, width)             # a view costs a microsecond: these calls take few


def _bp_vector(t, name, dtype=torch.float32):
    """A per-pair (or per-match) GPU tensor as the vector of its elements; a [n] tensor as it is."""
    t = _dev(t, name, dtype)
    return t if t.dim() == 1 else t.reshape(-1)


def _bp_matches(fn, first, matches_r, fam=_EPI):
    """The family's first list and the right matches as flat GPU lists -> (first [cap,width], mr [cap,2], cap)."""
    a, mr = _dev(first, fam.first), _dev(matches_r, "matches_r")
    fa, fr = _bp_flat(a, fam.width), _bp_flat(mr, 2)
    if fa is None or fr is None or (a.shape != mr.shape if fam.same_shape else fa.shape[0] != fr.shape[0]):
        raise RuntimeError("%s: %s" % (fn, fam.lists))
    return fa, fr, fa.shape[0]


def _bp_segments(fn, pair_off, stride, counts, pairs, cap):
    """The pairs' segments (one form: _bp_one_form) -> (seg, pairs, stride, pair_off pointer, counts pointer): seg is the GPU int64
    tensor behind the one pointer that is not null; stride is 0 for the ragged form.  pairs=None: as many as seg describes."""
    if counts is None:
        seg = _dev(pair_off, "pair_off", torch.int64)
        if seg.dim() != 1:
            raise RuntimeError("%s: pair_off must be an int64 vector" % fn)
        pairs = seg.numel() - 1 if pairs is None else int(pairs)
        if pairs < 1 or seg.numel() < pairs + 1:
            raise RuntimeError("%s: pair_off holds %d entries, %d pairs need %d" % (fn, seg.numel(), pairs, pairs + 1))
        return seg, pairs, 0, _ptr(seg), None
    seg = _dev(counts, "counts", torch.int64).reshape(-1)
    pairs = seg.numel() if pairs is None else int(pairs)
    stride = int(stride)
    if pairs < 1 or seg.numel() != pairs:
        raise RuntimeError("%s: counts must hold one int64 per pair" % fn)
    if stride < 1 or pairs * stride > cap:
        raise RuntimeError("%s: stride = %d: pairs * stride must lie in 1 .. cap = %d" % (fn, stride, cap))
    return seg, pairs, stride, None, _ptr(seg)


def _bp_norm(fn, norm, pairs):
    """The optional normalisation as a GPU [pairs,8] tensor, or None."""
    if norm is None:
        return None
    norm = _dev(norm, "norm")
    if tuple(norm.shape) != (pairs, 8):
        raise RuntimeError("%s: norm must be [pairs,8]" % fn)
    return norm


def _bp_candidates(fn, fam, first, matches_r, models, thr, pair_off, stride, counts, pairs):
    """The lists, the candidate models and the segments of a verification or a local optimisation, checked -> (first, mr, models, thr
    as GPU tensors, H = the models per pair, seg = the C arguments (pair_off, stride, counts_in, pairs, cap))."""
    a, mr, cap = _bp_matches(fn, first, matches_r, fam)
    models, thr = _dev(models, "models"), _bp_vector(thr, "thr")
    if models.dim() != 4 or tuple(models.shape[2:]) != fam.model:
        raise RuntimeError("%s: models must be %s" % (fn, fam.models))
    H = int(models.shape[1])
    _, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    if models.shape[0] != pairs or thr.numel() != pairs:
        raise RuntimeError("%s: models %s and thr [pairs] must hold %d pairs" % (fn, fam.models, pairs))
    if not 1 <= H <= epipolar_max_h():
        raise RuntimeError("%s: %s = %d, must lie in 1 .. %d" % (fn, fam.letter, H, epipolar_max_h()))
    return a, mr, models, thr, H, (off_p, stride, counts_p, pairs, cap)


def _bp_conf_norm(fn, conf, cap, norm, pairs):
    """The optional confidence list as a flat GPU [cap] tensor and the optional normalisation -> (conf, norm)."""
    if conf is not None:
        conf = _bp_vector(conf, "conf")
        if conf.numel() != cap:
            raise RuntimeError("%s: conf must be [cap]" % fn)
    return conf, _bp_norm(fn, norm, pairs)


def _bp_gated_call(first, mr, conf, inlier, min_conf, cap):
    """What a verification or a local optimisation hands to C for its per-match arguments and its gate -> ((first, matches_r, conf),
    (use_min_conf, min_conf), inlier), pointers: with cap == 0 the placeholders stand in for the empty tensors."""
    if cap == 0:
        first = mr = _bp_placeholder(first.device)
        inlier = _bp_placeholder(first.device, torch.uint8)
        conf = None if conf is None else first
    return (_ptr(first), _ptr(mr), _ptr(conf)), (0 if min_conf is None else 1, 0.0 if min_conf is None else float(min_conf)), _ptr(inlier)


def _bp_refit_source(fn, pairs, moments, models, best):
    """The source of a refit -> (moments, models, best, H): moments as a GPU [pairs,9,9] float64 tensor and no models (H = 1), or,
    without moments, models [pairs,H,3,3] and best [pairs]."""
    if moments is not None:
        moments = _dev(moments, "moments", torch.float64)
        if tuple(moments.shape) != (pairs, 9, 9):
            raise RuntimeError("%s: moments must be [pairs,9,9]" % fn)
        return moments, None, None, 1
    models, best = _dev(models, "models"), _dev(best, "best", torch.int32).reshape(-1)
    if models.dim() != 4 or tuple(models.shape[2:]) != (3, 3) or models.shape[0] != pairs or best.numel() != pairs:
        raise RuntimeError("%s: models must be [pairs,H,3,3] and best [pairs]" % fn)
    H = int(models.shape[1])
    if not 1 <= H <= epipolar_max_h():
        raise RuntimeError("%s: H = %d, must lie in 1 .. %d" % (fn, H, epipolar_max_h()))
    return moments, models, best, H


def _bp_outputs(fn, want, out, dev, lone=False):
    """The destinations `want` = [(name, dtype, shape)] describes: allocated when out is None, else out checked against it.
    lone: a tensor is taken as the 1-tuple of it."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dt, device=dev) for _, dt, shape in want)
    if lone and isinstance(out, torch.Tensor):
        out = (out,)
    if len(out) != len(want):
        raise RuntimeError("%s: out must be (%s)" % (fn, ", ".join(n for n, _, _ in want)))
    for t, (name, dt, shape) in zip(out, want):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("%s: %s must be a contiguous GPU %s tensor of shape %s" % (fn, name, dt, list(shape)))
    return tuple(out)


def _bp_placeholder(dev, dtype=torch.float32):
    """Empty tensors have no address: with cap == 0 a stage passes these 8 bytes for its [cap] arguments (the call is valid and
    touches none of them)."""
    return torch.empty((8 // dtype.itemsize,), dtype=dtype, device=dev)


def topk_max_k():
    """The largest K topk_by_pair takes (pats_topk_by_pair_max_k)."""
    return int(_L().pats_topk_by_pair_max_k())


def _topk_inputs(fn, matches_l, matches_r, conf, pair_off, K, pairs):
    """What topk_by_pair and topk_spread_by_pair check of the arguments they share -> (matches_l, matches_r, conf as GPU tensors,
    the pair_off tensor, its pointer, pairs, cap, K, the five outputs they share as _bp_outputs takes them)."""
    for t, name in ((matches_l, "matches_l"), (matches_r, "matches_r"), (conf, "conf"), (pair_off, "pair_off")):
        if isinstance(t, torch.Tensor) and t.is_cuda and not t.is_contiguous():
            raise RuntimeError("%s: %s must be contiguous" % (fn, name))
    ml, mr, cf = _dev(matches_l, "matches_l"), _dev(matches_r, "matches_r"), _dev(conf, "conf").reshape(-1)
    K, cap = int(K), int(cf.numel())
    pair_off, pairs, _, off_p, _ = _bp_segments(fn, pair_off, None, None, pairs, cap)
    if ml.dim() != 2 or ml.shape[1] != 2 or ml.shape != mr.shape or ml.shape[0] != cap:
        raise RuntimeError("%s: matches_l / matches_r must be [cap,2] and conf [cap]" % fn)
    if not 1 <= K <= topk_max_k():
        raise RuntimeError("%s: K = %d, must lie in 1 .. %d" % (fn, K, topk_max_k()))
    want = (("top_l", torch.float32, (pairs, K, 2)), ("top_r", torch.float32, (pairs, K, 2)), ("top_conf", torch.float32, (pairs, K)),
            ("top_idx", torch.int32, (pairs, K)), ("top_count", torch.int64, (pairs,)))
    return ml, mr, cf, pair_off, off_p, pairs, cap, K, want


def topk_by_pair(matches_l, matches_r, conf, pair_off, K, min_conf=None, out=None, pairs=None):
    """Each pair's K most confident matches out of matches_by_pair's regrouped lists, ON THE DEVICE: one launch for the whole
    batch, no host read (pats_topk_by_pair_f32; include/pats_amd.h holds the definition).  matches_l / matches_r [cap,2], conf
    [cap] float32, pair_off the [pairs + 1] int64 view matches_by_pair returns - or, with pairs= given, a longer buffer that
    starts with those offsets (the summary buffer).  min_conf: keep only matches with conf >= min_conf (inclusive).
    Returns (top_l [pairs,K,2], top_r [pairs,K,2], top_conf [pairs,K], top_idx [pairs,K] int32, top_count [pairs] int64): rank j
    of pair p is the match at position top_idx[p,j] of the pair's list, by confidence descending, ties by position ascending
    (+inf and a positive NaN rank first); past top_count[p] top_idx is -1 and the rest 0.0.  out: the five destinations."""
    fn = "topk_by_pair"
    ml, mr, cf, pair_off, off_p, pairs, cap, K, want = _topk_inputs(fn, matches_l, matches_r, conf, pair_off, K, pairs)
    dev = ml.device
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_topk_by_pair_workspace_bytes(pairs, K)
    ws = _workspace(nws, dev) if nws else None
    if cap == 0:
        ml = mr = cf = _bp_placeholder(dev)
    _check(_L().pats_topk_by_pair_f32(_ptr(ml), _ptr(mr), _ptr(cf), off_p, pairs, cap, K, 0 if min_conf is None else 1,
                                      0.0 if min_conf is None else float(min_conf), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                      _ptr(out[3]), _ptr(out[4]), _ptr(ws), nws, _stream()), fn)
    return out


def topk_spread_max_cells():
    """The largest grid0 * grid1 topk_spread_by_pair takes (pats_topk_spread_by_pair_max_cells)."""
    return int(_L().pats_topk_spread_by_pair_max_cells())


def topk_spread_by_pair(matches_l, matches_r, conf, pair_off, K, cell, grid, side="left", min_conf=None, out=None, pairs=None):
    """topk_by_pair's sibling that spreads the selection over the image, ON THE DEVICE: a grid of grid = (grid0, grid1) square cells
    of `cell` pixels lies over the points of one side ("left": matches_l, "right": matches_r; grid0 along component 0 of the stored
    points), every cell keeps its most confident match with conf >= min_conf, and the K most confident of these winners are the
    pair's selection (pats_topk_spread_by_pair_f32; include/pats_amd.h holds the definition).  One launch for the whole batch, no
    host read.  The inputs are topk_by_pair's; grid0 * grid1 <= topk_spread_max_cells(), a point outside the grid counts for the
    edge cell.  Returns topk_by_pair's five tensors - top_count = min(K, occupied) - and occupied [pairs] int64, the cells of each
    pair that hold a match.  out: the six destinations."""
    fn = "topk_spread_by_pair"
    ml, mr, cf, pair_off, off_p, pairs, cap, K, want = _topk_inputs(fn, matches_l, matches_r, conf, pair_off, K, pairs)
    if side not in ("left", "right"):
        raise RuntimeError("topk_spread_by_pair: side must be \"left\" or \"right\", got %r" % (side,))
    try:
        grid0, grid1 = (int(x) for x in grid)
        whole = (grid0, grid1) == tuple(grid)
    except (TypeError, ValueError):
        whole = False
    if not whole or grid0 < 1 or grid1 < 1:
        raise RuntimeError("topk_spread_by_pair: grid must be two positive integers (grid0, grid1), got %r" % (grid,))
    if int(cell) != cell:
        raise RuntimeError("topk_spread_by_pair: cell must be an integer number of pixels, got %r" % (cell,))
    dev = ml.device
    out = _bp_outputs(fn, want + (("occupied", torch.int64, (pairs,)),), out, dev)
    nws = _L().pats_topk_spread_by_pair_workspace_bytes(pairs, K, grid0, grid1)
    ws = _workspace(nws, dev) if nws else None
    if cap == 0:
        ml = mr = cf = _bp_placeholder(dev)
    _check(_L().pats_topk_spread_by_pair_f32(_ptr(ml), _ptr(mr), _ptr(cf), off_p, pairs, cap, K, 0 if min_conf is None else 1,
                                             0.0 if min_conf is None else float(min_conf), 0 if side == "left" else 1, int(cell),
                                             grid0, grid1, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(out[4]),
                                             _ptr(out[5]), _ptr(ws), nws, _stream()), fn)
    return out


def _score_checked(fn, fam, first, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, out, pairs, moments=False,
                   adaptive=None, msac=False):
    """What every verification checks and allocates; the caller lays out its own C call from what comes back -> (head, out, (pairs, H,
    cap)): head = the C arguments every score entry starts with (the lists and conf, the segments, models, H, thr, norm, the gate,
    counts, best, best_count, inlier), out = the destinations.  moments, adaptive, msac: the outputs they add, and adaptive's checks."""
    _bp_layout(fn, [(first, fam.first), (matches_r, "matches_r"), (models, "models"), (thr, "thr"), (pair_off, "pair_off"),
                    (counts, "counts"), (conf, "conf"), (norm, "norm")], {"pair_off": torch.int64, "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if min_conf is not None and conf is None:
        raise RuntimeError("%s: min_conf needs conf" % fn)
    if adaptive is not None:
        confidence, s, g, B = float(adaptive[0]), int(adaptive[1]), int(adaptive[2]), int(adaptive[3])
        if not 0.0 < confidence < 1.0:                   # false for a NaN
            raise RuntimeError("%s: confidence = %r must lie strictly between 0 and 1" % (fn, confidence))
        if not (1 <= s <= 16 and 1 <= g <= 16):
            raise RuntimeError("%s: sample_size = %d and models_per_sample = %d must lie in 1 .. 16" % (fn, s, g))
        if B < 64 or B % 64:
            raise RuntimeError("%s: round_models = %d must be a positive multiple of 64" % (fn, B))
    a, mr, models, thr, H, seg = _bp_candidates(fn, fam, first, matches_r, models, thr, pair_off, stride, counts, pairs)
    pairs, cap = seg[3:]
    if adaptive is not None and -(-H // B) > 256:
        raise RuntimeError("%s: round_models = %d gives %d rounds for H = %d (at most 256)" % (fn, B, -(-H // B), H))
    conf, norm = _bp_conf_norm(fn, conf, cap, norm, pairs)
    want = [("counts", torch.int32, (pairs, H)), ("best", torch.int32, (pairs,)), ("best_count", torch.int64, (pairs,)),
            ("inlier", torch.uint8, (cap,))]
    if moments:
        want.append(("moments", torch.float64, (pairs, 9, 9)))
    if adaptive is not None:
        want += [("used", torch.int32, (pairs,)), ("participating", torch.int32, (pairs,))]
    if msac:
        want += [("gains", torch.int64, (pairs, H)), ("best_gain", torch.int64, (pairs,))]
    out = _bp_outputs(fn, want, out, a.device)
    lists, gate, inl = _bp_gated_call(a, mr, conf, out[3], min_conf, cap)
    return lists + seg + (_ptr(models), H, _ptr(thr), _ptr(norm)) + gate + (_ptr(out[0]), _ptr(out[1]), _ptr(out[2]), inl), out, (pairs, H, cap)


def _score_by_pair(fn, entry, workspace_bytes, matches_l, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, moments, out,
                   pairs, adaptive=None, msac=False):
    """The C call of the six epipolar and homography verifications behind _score_checked's head: moments, the workspace, the stream
    and what an adaptive or an MSAC entry appends.  entry and its workspace query are the library's functions, looked up by the
    callers by plain attribute: these calls take microseconds and a formatted name would show.  adaptive: None for the fixed budget,
    else (confidence, sample_size, models_per_sample, round_models) - four more arguments, two more outputs.  msac: the MSAC entries
    - two more outputs, gains and best_gain."""
    head, out, sizes = _score_checked(fn, _EPI, matches_l, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, out, pairs,
                                      moments, adaptive, msac)
    nws = workspace_bytes(*sizes)
    ws = _workspace(nws, out[0].device) if nws else None
    more = (_ptr(out[-2]), _ptr(out[-1])) if msac or adaptive is not None else ()
    if adaptive is not None:
        more = (float(adaptive[0]), int(adaptive[1]), int(adaptive[2]), int(adaptive[3])) + more
    _check(entry(*head, _ptr(out[4]) if moments else None, _ptr(ws), nws, _stream(), *more), fn)
    return out


def _hypotheses_checked(fn, fam, K, slots, first, matches_r, H, seed, pair_off, stride, counts, norm, progressive, return_samples,
                        return_counts, out, pairs):
    """What every minimal-sample generator checks and allocates - K = the sample size, slots = the models per sample (1, the 10 and 3
    of the 5- and 7-point generators, P3P's 4) -; the caller lays out its own C call -> (head, out, (pairs, H)): head = the C arguments every
    generator starts with (the lists, the segments, H, seed, norm, progressive, models, sample_idx - and n_models where slots > 1: the
    one-model entries have none), out = the destinations."""
    _bp_layout(fn, [(first, fam.first), (matches_r, "matches_r"), (seed, "seed"), (pair_off, "pair_off"), (counts, "counts"),
                    (norm, "norm")], {"pair_off": torch.int64, "counts": torch.int64, "seed": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if not isinstance(seed, torch.Tensor):
        raise RuntimeError("%s: seed must be an int64 GPU tensor [pairs]" % fn)
    a, mr, cap = _bp_matches(fn, first, matches_r, fam)
    H = int(H)
    seed = _bp_vector(seed, "seed", torch.int64)
    _, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    if seed.numel() != pairs:
        raise RuntimeError("%s: seed must hold one int64 per pair (%d), got %d" % (fn, pairs, seed.numel()))
    if not 1 <= H <= epipolar_max_h() // slots:
        raise RuntimeError("%s: H = %d, must lie in 1 .. %d%s" % (fn, H, epipolar_max_h() // slots, " (%d H models)" % slots if slots > 1 else ""))
    norm = _bp_norm(fn, norm, pairs)
    want = [("models", torch.float32, (pairs, H) + ((slots,) if slots > 1 else ()) + fam.model)]
    if return_samples:
        want.append(("sample_idx", torch.int32, (pairs, H, K)))
    if return_counts:
        want.append(("n_models", torch.int32, (pairs, H)))
    out = _bp_outputs(fn, want, out, a.device, lone=True)
    if cap == 0:
        a = mr = _bp_placeholder(a.device)
    n_models = (_ptr(out[-1]) if return_counts else None,) if slots > 1 else ()
    return (_ptr(a), _ptr(mr), off_p, stride, counts_p, pairs, cap, H, _ptr(seed), _ptr(norm), 1 if progressive else 0, _ptr(out[0]),
            _ptr(out[1]) if return_samples else None) + n_models, out, (pairs, H)


def _hypotheses_by_pair(fn, K, slots, entry, workspace_bytes, matches_l, matches_r, H, seed, pair_off, stride, counts, norm, progressive,
                        return_samples, return_counts, out, pairs):
    """The C call of the epipolar and homography generators behind _hypotheses_checked's head: the workspace and the stream."""
    head, out, sizes = _hypotheses_checked(fn, _EPI, K, slots, matches_l, matches_r, H, seed, pair_off, stride, counts, norm, progressive,
                                           return_samples, return_counts, out, pairs)
    nws = workspace_bytes(*sizes)
    ws = _workspace(nws, out[0].device) if nws else None
    _check(entry(*head, _ptr(ws), nws, _stream()), fn)
    return out if len(out) > 1 else out[0]


def epipolar_max_h():
    """The largest number of models per pair epipolar_score_by_pair takes (pats_epipolar_max_h)."""
    return int(_L().pats_epipolar_max_h())


def epipolar_score_by_pair(matches_l, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None,
                           norm=None, moments=False, out=None, pairs=None):
    """H candidate epipolar models per pair against every match of the pair, ON THE DEVICE, no host read
    (pats_epipolar_score_by_pair_f32; include/pats_amd.h holds the definition): match i is an inlier of the 3x3 model E iff
    r^2 <= thr^2 den with a = E x_l, b = E^T x_r, r = x_r . a, den = a0^2 + a1^2 + b0^2 + b1^2 > 0 (squared Sampson error).
    matches_l / matches_r [cap,2] float32 (also [pairs,K,2]: top-K outputs are taken as the flat [pairs*K,2] lists they are),
    models [pairs,H,3,3], thr [pairs] float32.  The pairs' segments in exactly one of two forms: pair_off (int64 [pairs + 1] - or,
    with pairs= given, a longer buffer that starts with the offsets) or stride + counts (int64 [pairs]: pair p = rows
    p * stride .. + counts[p], the layout of topk_by_pair's outputs).  norm [pairs,8] = (c0_l, c1_l, s0_l, s1_l, c0_r, c1_r, s0_r,
    s1_r): x = ((p0 - c0) * s0, (p1 - c1) * s1, 1); without it x = (p0, p1, 1).  min_conf (needs conf [cap]): only matches with
    conf >= min_conf take part.  A pair whose thr is NaN or negative has no inliers.
    Returns (counts [pairs,H] int32, best [pairs] int32 - the lowest index of the largest count -, best_count [pairs] int64,
    inlier [cap] uint8 - 1 where the match is an inlier of its pair's best model, 0 everywhere else) and, with moments=True,
    moments [pairs,9,9] float64 = the sum of q q^T over those inliers, q = vec(x_r x_l^T): torch.linalg.eigh of it is the
    least-squares refit.  out: the four (five) destinations."""
    return _score_by_pair("epipolar_score_by_pair", _L().pats_epipolar_score_by_pair_f32, _L().pats_epipolar_workspace_bytes, matches_l,
                          matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, moments, out, pairs)


def msac_gain_one():
    """The gain of a perfect inlier in the units of epipolar_score_msac_by_pair's gains (pats_msac_gain_one: 1 << 20)."""
    return int(_L().pats_msac_gain_one())


def epipolar_score_msac_by_pair(matches_l, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None,
                                norm=None, moments=False, out=None, pairs=None):
    """epipolar_score_by_pair with the winner chosen by MSAC gain, ON THE DEVICE, no host read
    (pats_epipolar_score_msac_by_pair_f32; include/pats_amd.h, "Per-pair MSAC scoring", holds the definition): an inlier of model h
    adds 2^20 - min(floor(2^20 r^2 / (thr^2 den)), 2^20) to gains[p, h], every other match 0; best is the lowest index of the largest
    gain.  The arguments are epipolar_score_by_pair's.
    Returns epipolar_score_by_pair's tuple - counts bit for bit its counts; best, best_count, inlier and moments those of the MSAC
    winner - followed by gains [pairs,H] int64 and best_gain [pairs] int64 (gains / msac_gain_one() ~ the sum over the inliers of
    1 - e^2 / thr^2).  out: the six (seven) destinations."""
    return _score_by_pair("epipolar_score_msac_by_pair", _L().pats_epipolar_score_msac_by_pair_f32, _L().pats_epipolar_workspace_bytes,
                          matches_l, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, moments, out, pairs, msac=True)


def epipolar_hypotheses_by_pair(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False,
                                return_samples=False, out=None, pairs=None):
    """H 8-point hypotheses per pair, ON THE DEVICE, one launch, no host read (pats_epipolar_hypotheses_by_pair_f32;
    include/pats_amd.h holds the definition): for every pair and every h eight distinct matches of the pair are drawn by a
    counter-based generator and the unit null vector of their 8x9 constraint matrix is written as a row-major 3x3 model - the input
    of epipolar_score_by_pair.  matches_l / matches_r [cap,2] float32 (also [pairs,K,2]: top-K outputs are taken as the flat lists
    they are); the pairs' segments in exactly one of two forms, as for epipolar_score_by_pair: pair_off (int64 [pairs + 1] - or,
    with pairs= given, a longer buffer that starts with the offsets) or stride + counts (int64 [pairs]).  seed: int64 GPU tensor
    [pairs], one generator seed per pair.  norm [pairs,8]: the verification's normalisation.  progressive: hypothesis h draws from
    the first max(8, ceil(n (h + 1) / H)) matches of the pair's list (a confidence-sorted top-K) instead of all n.
    Returns models [pairs,H,3,3] float32 - exact zeros for a pair with fewer than 8 matches and for a sample with a non-finite
    coordinate - or, with return_samples=True, (models, sample_idx [pairs,H,8] int32: the draws as positions inside the pair's
    list, -1 for a pair with fewer than 8 matches).  out: the destination(s), a tensor or a tuple."""
    return _hypotheses_by_pair("epipolar_hypotheses_by_pair", 8, 1, _L().pats_epipolar_hypotheses_by_pair_f32,
                               _L().pats_epipolar_hypotheses_workspace_bytes, matches_l, matches_r, H, seed, pair_off, stride, counts, norm,
                               progressive, return_samples, False, out, pairs)


def epipolar_hypotheses5_by_pair(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False,
                                 return_samples=False, return_counts=False, out=None, pairs=None):
    """H 5-point samples per pair, ON THE DEVICE, one launch, no host read (pats_epipolar_hypotheses5_by_pair_f32;
    include/pats_amd.h holds the definition): for every pair and every h five distinct matches of the pair are drawn by the
    hypotheses' counter-based generator and the real essential matrices through them - at most ten - are written as row-major 3x3
    unit models into the sample's lowest slots, exact zeros behind them.  The arguments are those of epipolar_hypotheses_by_pair;
    10 * H may not exceed epipolar_max_h().  The models live in the frame of the normalised points: norm must carry the intrinsics.
    progressive: sample h draws from the first max(5, ceil(n (h + 1) / H)) matches of the pair's list instead of all n.
    Returns models [pairs,H,10,3,3] float32 - models.view(pairs, 10 * H, 3, 3) is a `models` of epipolar_score_by_pair; all ten
    slots zero for a pair with fewer than 5 matches, a sample with a non-finite coordinate and a degenerate sample - or a tuple
    (models[, sample_idx [pairs,H,5] int32 with return_samples=True: the draws as positions inside the pair's list, -1 for a pair
    with fewer than 5 matches][, n_models [pairs,H] int32 with return_counts=True: the non-zero slots]).  out: the destination(s), a
    tensor or a tuple in that order."""
    return _hypotheses_by_pair("epipolar_hypotheses5_by_pair", 5, 10, _L().pats_epipolar_hypotheses5_by_pair_f32,
                               _L().pats_epipolar_hypotheses5_workspace_bytes, matches_l, matches_r, H, seed, pair_off, stride, counts, norm,
                               progressive, return_samples, return_counts, out, pairs)


def epipolar_hypotheses7_by_pair(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False,
                                 return_samples=False, return_counts=False, out=None, pairs=None):
    """H 7-point samples per pair, ON THE DEVICE, one launch, no host read (pats_epipolar_hypotheses7_by_pair_f32;
    include/pats_amd.h, "Per-pair 7-point hypotheses", holds the definition): for every pair and every h seven distinct matches of
    the pair are drawn by the hypotheses' counter-based generator and the real fundamental matrices through them - at most three,
    rank 2 by construction - are written as row-major 3x3 unit models into the sample's lowest slots, exact zeros behind them.  The
    arguments are those of epipolar_hypotheses_by_pair; 3 * H may not exceed epipolar_max_h().  No calibration is needed: norm is
    the verification's normalisation, whatever it is.  progressive: sample h draws from the first max(7, ceil(n (h + 1) / H))
    matches of the pair's list instead of all n.
    Returns models [pairs,H,3,3,3] float32 - models.view(pairs, 3 * H, 3, 3) is a `models` of epipolar_score_by_pair; all three
    slots zero for a pair with fewer than 7 matches and a sample with a non-finite coordinate - or a tuple (models[, sample_idx
    [pairs,H,7] int32 with return_samples=True: the draws as positions inside the pair's list, -1 for a pair with fewer than 7
    matches][, n_models [pairs,H] int32 with return_counts=True: the non-zero slots]).  out: the destination(s), a tensor or a tuple
    in that order."""
    return _hypotheses_by_pair("epipolar_hypotheses7_by_pair", 7, 3, _L().pats_epipolar_hypotheses7_by_pair_f32,
                               _L().pats_epipolar_hypotheses7_workspace_bytes, matches_l, matches_r, H, seed, pair_off, stride, counts, norm,
                               progressive, return_samples, return_counts, out, pairs)


def plane_parallax_pool_max():
    """The number of off-plane matches plane_parallax_hypotheses_by_pair draws from at most (pats_plane_parallax_pool_max)."""
    return int(_L().pats_plane_parallax_pool_max())


def _pp_plane(fn, models_h, best_h, pairs):
    """The plane of the plane-and-parallax entries, checked -> (models_h [pairs,Mh,3,3], best_h [pairs] as GPU tensors, Mh)."""
    models_h, best_h = _dev(models_h, "models_h"), _bp_vector(best_h, "best_h", torch.int32)
    if models_h.dim() != 4 or tuple(models_h.shape[2:]) != (3, 3) or models_h.shape[0] != pairs or best_h.numel() != pairs:
        raise RuntimeError("%s: models_h must be [pairs,Mh,3,3] and best_h [pairs], %d pairs" % (fn, pairs))
    Mh = int(models_h.shape[1])
    if not 1 <= Mh <= epipolar_max_h():
        raise RuntimeError("%s: Mh = %d, must lie in 1 .. %d" % (fn, Mh, epipolar_max_h()))
    return models_h, best_h, Mh


def plane_parallax_hypotheses_by_pair(matches_l, matches_r, H, seed, models_h, best_h, thr, pair_off=None, stride=None, counts=None,
                                      norm=None, parallax=2.0, return_samples=False, out=None, pairs=None):
    """H plane-and-parallax hypotheses per pair, ON THE DEVICE, one launch, no host read (pats_plane_parallax_hypotheses_by_pair_f32;
    include/pats_amd.h, "Per-pair plane-and-parallax hypotheses and hand-over", holds the definition): the matches of the pair that
    are finite and off the plane Hp = models_h[p, best_h[p]] at parallax * thr[p] - by the homography verification's own test - form
    the pair's pool in segment order; for every h two of them are drawn by the hypotheses' generator and F = [e]x Hp, e the
    intersection of the two lines x'_i x Hp x_i, is written as a unit model with the branch's sign rule.  matches_l / matches_r, the
    segments, seed and norm as epipolar_hypotheses7_by_pair takes them; models_h [pairs,Mh,3,3] float32, best_h [pairs] int32 and
    thr [pairs] float32 as homography_score_by_pair (or homography_polish_by_pair) took and left them; parallax >= 1.
    Returns (models [pairs,H,3,3] float32 - nine exact zeros where there is no plane (a zero Hp), fewer than two pool members, two
    coinciding lines or a non-finite value -, pool [pairs] int32: the pool's size, of which the first plane_parallax_pool_max()
    members are drawn from) and, with return_samples=True, sample_idx [pairs,H,2] int32: the draws as positions inside the pair's
    list, -1 where nothing was drawn.  out: the destinations, a tuple in that order."""
    fn = "plane_parallax_hypotheses_by_pair"
    _bp_layout(fn, [(matches_l, "matches_l"), (matches_r, "matches_r"), (seed, "seed"), (pair_off, "pair_off"), (counts, "counts"),
                    (norm, "norm"), (models_h, "models_h"), (best_h, "best_h"), (thr, "thr")],
               {"pair_off": torch.int64, "counts": torch.int64, "seed": torch.int64, "best_h": torch.int32})
    _bp_one_form(fn, pair_off, stride, counts)
    if not isinstance(seed, torch.Tensor):
        raise RuntimeError("%s: seed must be an int64 GPU tensor [pairs]" % fn)
    parallax = float(parallax)
    if not (math.isfinite(parallax) and parallax >= 1.0):
        raise RuntimeError("%s: parallax = %r must be a finite number >= 1" % (fn, parallax))
    a, mr, cap = _bp_matches(fn, matches_l, matches_r)
    H = int(H)
    seed = _bp_vector(seed, "seed", torch.int64)
    _, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    if seed.numel() != pairs:
        raise RuntimeError("%s: seed must hold one int64 per pair (%d), got %d" % (fn, pairs, seed.numel()))
    if not 1 <= H <= epipolar_max_h():
        raise RuntimeError("%s: H = %d, must lie in 1 .. %d" % (fn, H, epipolar_max_h()))
    norm = _bp_norm(fn, norm, pairs)
    models_h, best_h, Mh = _pp_plane(fn, models_h, best_h, pairs)
    thr = _bp_vector(thr, "thr")
    if thr.numel() != pairs:
        raise RuntimeError("%s: thr must hold one float32 per pair (%d), got %d" % (fn, pairs, thr.numel()))
    want = [("models", torch.float32, (pairs, H, 3, 3)), ("pool", torch.int32, (pairs,))]
    if return_samples:
        want.append(("sample_idx", torch.int32, (pairs, H, 2)))
    out = _bp_outputs(fn, want, out, a.device)
    if cap == 0:
        a = mr = _bp_placeholder(a.device)
    nws = _L().pats_plane_parallax_hypotheses_workspace_bytes(pairs, H)
    ws = _workspace(nws, out[0].device) if nws else None
    _check(_L().pats_plane_parallax_hypotheses_by_pair_f32(_ptr(a), _ptr(mr), off_p, stride, counts_p, pairs, cap, H, _ptr(seed), _ptr(norm),
                                                           _ptr(models_h), Mh, _ptr(best_h), _ptr(thr), parallax, _ptr(out[0]),
                                                           _ptr(out[2]) if return_samples else None, _ptr(out[1]), _ptr(ws), nws,
                                                           _stream()), fn)
    return out


def plane_parallax_select_by_pair(matches_l, matches_r, thr, models_h, best_h, standing, candidate, pair_off=None, stride=None,
                                  counts=None, norm=None, out=None, pairs=None):
    """The hand-over of the plane-and-parallax stage, ON THE DEVICE, one launch, no host read (pats_plane_parallax_select_by_pair;
    include/pats_amd.h holds the definition): standing and candidate are two verifications of the same lists, each a tuple (models
    [pairs,H,3,3] float32, best [pairs] int32, best_count [pairs] int64, inlier [cap] uint8[, moments [pairs,9,9] float64]) as
    epipolar_score_by_pair took and left them - the standing one of the pair's fundamental matrices, the candidate of
    plane_parallax_hypotheses_by_pair's models.  A pair keeps the standing one unless the candidate's best_count is STRICTLY larger.
    The lists, the segments, thr and norm as the verifications took them; models_h, best_h: the plane.
    Returns (model [pairs,3,3] float32, best_count [pairs] int64, inlier [cap] uint8[, moments [pairs,9,9] float64 - when both
    tuples carry moments], replaced [pairs] uint8, overlap [pairs] int32: the standing inliers that are inliers of the plane at thr,
    the standing model's degeneracy measure).  out: the destinations, a tuple in that order."""
    fn = "plane_parallax_select_by_pair"
    sides = []
    for side, name in ((standing, "standing"), (candidate, "candidate")):
        if not isinstance(side, (tuple, list)) or len(side) not in (4, 5):
            raise RuntimeError("%s: %s must be (models, best, best_count, inlier[, moments])" % (fn, name))
        sides.append(tuple(side) + (None,) * (5 - len(side)))
    (ma, ba, ca, ia, qa), (mb, bb, cb, ib, qb) = sides
    _bp_layout(fn, [(matches_l, "matches_l"), (matches_r, "matches_r"), (thr, "thr"), (pair_off, "pair_off"), (counts, "counts"),
                    (norm, "norm"), (models_h, "models_h"), (best_h, "best_h"), (ma, "standing models"), (ba, "standing best"),
                    (ca, "standing best_count"), (ia, "standing inlier"), (qa, "standing moments"), (mb, "candidate models"),
                    (bb, "candidate best"), (cb, "candidate best_count"), (ib, "candidate inlier"), (qb, "candidate moments")],
               {"pair_off": torch.int64, "counts": torch.int64, "best_h": torch.int32, "standing best": torch.int32,
                "candidate best": torch.int32, "standing best_count": torch.int64, "candidate best_count": torch.int64,
                "standing inlier": torch.uint8, "candidate inlier": torch.uint8, "standing moments": torch.float64,
                "candidate moments": torch.float64})
    _bp_one_form(fn, pair_off, stride, counts)
    a, mr, cap = _bp_matches(fn, matches_l, matches_r)
    _, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    norm = _bp_norm(fn, norm, pairs)
    models_h, best_h, Mh = _pp_plane(fn, models_h, best_h, pairs)
    thr = _bp_vector(thr, "thr")
    if thr.numel() != pairs:
        raise RuntimeError("%s: thr must hold one float32 per pair (%d), got %d" % (fn, pairs, thr.numel()))
    args, with_moments = [], qa is not None and qb is not None
    for name, (m, b, c, i, q) in (("standing", sides[0]), ("candidate", sides[1])):
        _, m, b, Hx = _bp_refit_source("%s: %s" % (fn, name), pairs, None, m, b)
        c, i = _bp_vector(c, name + " best_count", torch.int64), _bp_vector(i, name + " inlier", torch.uint8)
        if c.numel() != pairs or i.numel() != cap:
            raise RuntimeError("%s: %s best_count must be [pairs] and inlier [cap]" % (fn, name))
        if with_moments:
            q = _dev(q, name + " moments", torch.float64)
            if tuple(q.shape) != (pairs, 9, 9):
                raise RuntimeError("%s: %s moments must be [pairs,9,9]" % (fn, name))
        if cap == 0:
            i = _bp_placeholder(a.device, torch.uint8)
        args += [_ptr(m), Hx, _ptr(b), _ptr(c), _ptr(i), _ptr(q) if with_moments else None]
    want = [("model", torch.float32, (pairs, 3, 3)), ("best_count", torch.int64, (pairs,)), ("inlier", torch.uint8, (cap,))]
    if with_moments:
        want.append(("moments", torch.float64, (pairs, 9, 9)))
    want += [("replaced", torch.uint8, (pairs,)), ("overlap", torch.int32, (pairs,))]
    out = _bp_outputs(fn, want, out, a.device)
    inl = out[2]
    if cap == 0:
        a = mr = _bp_placeholder(a.device)
        inl = _bp_placeholder(a.device, torch.uint8)
    _check(_L().pats_plane_parallax_select_by_pair(_ptr(a), _ptr(mr), off_p, stride, counts_p, pairs, cap, _ptr(norm), _ptr(models_h), Mh,
                                                   _ptr(best_h), _ptr(thr), *args, _ptr(out[0]), _ptr(out[1]), _ptr(inl),
                                                   _ptr(out[3]) if with_moments else None, _ptr(out[-2]), _ptr(out[-1]), _stream()), fn)
    return out


def epipolar_pose_by_pair(matches_l, matches_r, inlier, best_count, moments=None, models=None, best=None, pair_off=None, stride=None,
                          counts=None, norm=None, swapped=False, return_front=False, return_refit=False, out=None, pairs=None):
    """Each pair's relative pose from its verified inliers, ON THE DEVICE, no host read (pats_epipolar_pose_by_pair_f64;
    include/pats_amd.h holds the definition): the least-squares refit of `moments` (its eigenvector for the smallest eigenvalue;
    without moments the winning model models[p, best[p]]), the nearest essential matrix E, the four (R, t) decompositions and the
    cheirality vote of the pair's used matches - inlier != 0, finite - that picks one.  matches_l / matches_r [cap,2] float32 (also
    [pairs,K,2]), the segments (pair_off, or stride + counts) and norm exactly as epipolar_score_by_pair took them; inlier [cap]
    uint8, best_count [pairs] int64 and moments [pairs,9,9] float64 (or best [pairs] int32 with the models) are its outputs.
    swapped: the points are in the hand-over's (y, x) order; R, t, E come back in the reference's (x, y) frame.
    Returns (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64, front_counts [pairs,4] int32,
    choice [pairs] int32), then front [cap] uint8 with return_front=True, then e_refit [pairs,9] float64 with return_refit=True.
    A pair without a pose (best_count < 8, a non-finite moment, a refit of rank below 2) has E = 0, R = I, t = 0 and no count.
    out: the destinations, in that order."""
    fn = "epipolar_pose_by_pair"
    _bp_layout(fn, [(matches_l, "matches_l"), (matches_r, "matches_r"), (inlier, "inlier"), (best_count, "best_count"),
                    (moments, "moments"), (models, "models"), (best, "best"), (pair_off, "pair_off"), (counts, "counts"), (norm, "norm")],
               {"inlier": torch.uint8, "best_count": torch.int64, "moments": torch.float64, "best": torch.int32, "pair_off": torch.int64,
                "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if moments is None and (models is None or best is None):
        raise RuntimeError("epipolar_pose_by_pair: give moments, or models and best")
    ml, mr, cap = _bp_matches(fn, matches_l, matches_r)
    inl = _dev(inlier, "inlier", torch.uint8).reshape(-1)
    if inl.numel() != cap:
        raise RuntimeError("epipolar_pose_by_pair: inlier must be [cap]")
    bc = _dev(best_count, "best_count", torch.int64).reshape(-1)
    seg, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    if bc.numel() != pairs:
        raise RuntimeError("epipolar_pose_by_pair: best_count must hold one int64 per pair (%d), got %d" % (pairs, bc.numel()))
    moments, models, best, H = _bp_refit_source(fn, pairs, moments, models, best)
    norm = _bp_norm(fn, norm, pairs)
    dev = ml.device
    want = [("E", torch.float64, (pairs, 3, 3)), ("R", torch.float64, (pairs, 3, 3)), ("t", torch.float64, (pairs, 3)),
            ("front_count", torch.int64, (pairs,)), ("front_counts", torch.int32, (pairs, 4)), ("choice", torch.int32, (pairs,))]
    if return_front:
        want.append(("front", torch.uint8, (cap,)))
    if return_refit:
        want.append(("e_refit", torch.float64, (pairs, 9)))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_epipolar_pose_workspace_bytes(pairs, cap)
    ws = _workspace(nws, dev) if nws else None
    front = out[6] if return_front else None
    refit = out[-1] if return_refit else None
    if cap == 0:
        ml = mr = _bp_placeholder(dev)
        inl = _bp_placeholder(dev, torch.uint8)
        front = None
    _check(_L().pats_epipolar_pose_by_pair_f64(_ptr(ml), _ptr(mr), _ptr(inl), off_p, stride, counts_p, pairs, cap, _ptr(bc),
                                               _ptr(moments), _ptr(models), H, _ptr(best), _ptr(norm), 1 if swapped else 0, _ptr(out[0]),
                                               _ptr(out[1]), _ptr(out[2]), _ptr(out[4]), _ptr(out[5]), _ptr(out[3]), _ptr(front),
                                               _ptr(refit), _ptr(ws), nws, _stream()), fn)
    return out


def epipolar_triangulate_by_pair(matches_l, matches_r, mask, R, t, pair_off=None, stride=None, counts=None, norm=None, swapped=False,
                                 max_reproj=None, max_cos=None, return_depths=False, return_reproj=False, return_cos=False, out=None,
                                 pairs=None):
    """Each pair's masked matches triangulated under its pose, ON THE DEVICE, no host read (pats_epipolar_triangulate_by_pair_f64;
    include/pats_amd.h holds the definition): the midpoint of the common perpendicular of a match's two rays in the LEFT camera's
    frame, the two depths, the squared reprojection error and the cosine of the triangulation angle, float64 throughout.
    matches_l / matches_r [cap,2] float32 (also [pairs,K,2]), the segments (pair_off, or stride + counts) and norm exactly as
    epipolar_pose_by_pair took them; mask [cap] uint8 - its front, or the verification's inlier; R [pairs,3,3], t [pairs,3]
    float64 its outputs, with the `swapped` it was given.  max_reproj / max_cos [pairs] float32: a match is valid only with
    e2 <= max_reproj^2 and cos <= max_cos (a NaN limit: no valid match in that pair).
    Returns (points [cap,3] float32, valid [cap] uint8, tri_count [pairs] int64, reproj_sum [pairs] float64), then depths [cap,2]
    with return_depths=True, reproj [cap] with return_reproj=True, cos_parallax [cap] with return_cos=True (float32).  A row that is
    not valid holds zeros everywhere; a pair without a pose (t = 0) or with a non-finite one has no valid match.
    out: the destinations, in that order."""
    fn = "epipolar_triangulate_by_pair"
    _bp_layout(fn, [(matches_l, "matches_l"), (matches_r, "matches_r"), (mask, "mask"), (R, "R"), (t, "t"), (pair_off, "pair_off"),
                    (counts, "counts"), (norm, "norm"), (max_reproj, "max_reproj"), (max_cos, "max_cos")],
               {"mask": torch.uint8, "R": torch.float64, "t": torch.float64, "pair_off": torch.int64, "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    ml, mr, cap = _bp_matches(fn, matches_l, matches_r)
    msk = _dev(mask, "mask", torch.uint8).reshape(-1)
    if msk.numel() != cap:
        raise RuntimeError("epipolar_triangulate_by_pair: mask must be [cap]")
    seg, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    R, t = _dev(R, "R", torch.float64), _dev(t, "t", torch.float64)
    if tuple(R.shape) != (pairs, 3, 3) or tuple(t.shape) != (pairs, 3):
        raise RuntimeError("epipolar_triangulate_by_pair: R must be [pairs,3,3] and t [pairs,3]")
    norm = _bp_norm(fn, norm, pairs)
    lims = []
    for lim, name in ((max_reproj, "max_reproj"), (max_cos, "max_cos")):
        if lim is not None:
            lim = _dev(lim, name).reshape(-1)
            if lim.numel() != pairs:
                raise RuntimeError("epipolar_triangulate_by_pair: %s must hold one float32 per pair (%d), got %d" % (name, pairs, lim.numel()))
        lims.append(lim)
    dev = ml.device
    want = [("points", torch.float32, (cap, 3)), ("valid", torch.uint8, (cap,)), ("tri_count", torch.int64, (pairs,)),
            ("reproj_sum", torch.float64, (pairs,))]
    more = {}
    for flag, name, shape in ((return_depths, "depths", (cap, 2)), (return_reproj, "reproj", (cap,)), (return_cos, "cos_parallax", (cap,))):
        if flag:
            more[name] = len(want)
            want.append((name, torch.float32, shape))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_epipolar_triangulate_workspace_bytes(pairs, cap)
    ws = _workspace(nws, dev) if nws else None
    points, valid = out[0], out[1]
    per_match = {name: out[k] for name, k in more.items()}
    if cap == 0:
        ml = mr = points = _bp_placeholder(dev)
        msk = valid = _bp_placeholder(dev, torch.uint8)
        per_match = {}
    _check(_L().pats_epipolar_triangulate_by_pair_f64(_ptr(ml), _ptr(mr), off_p, stride, counts_p, pairs, cap, _ptr(msk), _ptr(norm), _ptr(R),
                                                      _ptr(t), 1 if swapped else 0, _ptr(lims[0]), _ptr(lims[1]), _ptr(points),
                                                      _ptr(per_match.get("depths")), _ptr(per_match.get("reproj")),
                                                      _ptr(per_match.get("cos_parallax")), _ptr(valid), _ptr(out[2]), _ptr(out[3]), _ptr(ws),
                                                      nws, _stream()), fn)
    return out


def pose_error_by_pair(R, t, T1, T0=None, counts=None, min_matches=15, min_gt_t=0.0, out=None):
    """Each pair's rotation and translation error against the ground truth, ON THE DEVICE, one launch, no host read
    (pats_pose_error_by_pair_f64; include/pats_amd.h holds the definition): the reference's angle_error_mat, angle_error_vec with the
    fold at 90 degrees and their maximum, in degrees, float64.  R [pairs,3,3], t [pairs,3] float64 as epipolar_pose_by_pair returns
    them; T1 [pairs,4,4] float64 the ground truth (R_gt | t_gt) in its upper 3 x 4 - or, with T0 [pairs,4,4] given, the two
    extrinsics, and the ground truth is the rigid T1 inv(T0).  Estimate and ground truth must be in the SAME frame: with a data
    set's extrinsics call epipolar_pose_by_pair(..., swapped=True).  counts [pairs] int64: a pair with fewer than min_matches matches
    is not scored.  min_gt_t: a ground-truth translation of at most this length has no direction, err_t = 0.
    Returns (err_R, err_t, err [pairs] float64, status [pairs] int32): status 0 evaluated, 1 too few matches, 2 no pose (t = 0 or a
    non-finite entry), 3 a non-finite ground truth - the lowest that applies; for status != 0 the errors are +inf, the reference's
    value for a pair it cannot score.  No output ever holds a NaN.  out: the four destinations - views are fine, so `err` can be a
    slice of a running buffer that pose_auc aggregates."""
    fn = "pose_error_by_pair"
    f64 = torch.float64
    _bp_layout(fn, [(R, "R"), (t, "t"), (T1, "T1"), (T0, "T0"), (counts, "counts")], {"R": f64, "t": f64, "T1": f64, "T0": f64, "counts": torch.int64})
    R, t, T1 = _dev(R, "R", f64), _dev(t, "t", f64), _dev(T1, "T1", f64)
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise RuntimeError("pose_error_by_pair: R must be [pairs,3,3] with pairs >= 1")
    pairs = int(R.shape[0])
    if tuple(t.shape) != (pairs, 3):
        raise RuntimeError("pose_error_by_pair: t must be [pairs,3]")
    if tuple(T1.shape) != (pairs, 4, 4):
        raise RuntimeError("pose_error_by_pair: T1 must be [pairs,4,4]")
    if T0 is not None:
        T0 = _dev(T0, "T0", f64)
        if tuple(T0.shape) != (pairs, 4, 4):
            raise RuntimeError("pose_error_by_pair: T0 must be [pairs,4,4]")
    if counts is not None:
        counts = _dev(counts, "counts", torch.int64)
        if tuple(counts.shape) != (pairs,):
            raise RuntimeError("pose_error_by_pair: counts must hold one int64 per pair (%d)" % pairs)
    want = [("err_R", f64, (pairs,)), ("err_t", f64, (pairs,)), ("err", f64, (pairs,)), ("status", torch.int32, (pairs,))]
    out = _bp_outputs(fn, want, out, R.device)
    _check(_L().pats_pose_error_by_pair_f64(_ptr(R), _ptr(t), _ptr(T1), _ptr(T0), _ptr(counts), pairs, int(min_matches), float(min_gt_t),
                                            _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _stream()), fn)
    return out


def pose_auc_max_n():
    """The longest error list pose_auc takes (pats_pose_auc_max_n)."""
    return int(_L().pats_pose_auc_max_n())


def pose_auc(errors, thresholds=(5.0, 10.0, 20.0), return_sorted=False, out=None):
    """The AUC of the recall curve over a list of pose errors at each threshold, ON THE DEVICE, one launch, no host read
    (pats_pose_auc_f64; include/pats_amd.h holds the definition): the reference's error_auc - sorted errors behind a leading 0,
    recall i / n, the trapezoids up to the threshold, divided by it.  errors [n] float64, 0 <= n <= pose_auc_max_n() - the `err` of
    pose_error_by_pair accumulated over a data set; +inf (a pair that was not scored) never counts, a NaN is taken as +inf, -0.0 as +0.0.
    thresholds: 1 .. 8 finite positive numbers (host values).
    Returns (auc [n_thr] float64, below [n_thr] int64: the errors strictly below each threshold), followed by sorted [n] float64 -
    the sorted list - with return_sorted=True.  out: the destinations, in that order."""
    fn = "pose_auc"
    _bp_layout(fn, [(errors, "errors")], {"errors": torch.float64})
    errors = _dev(errors, "errors", torch.float64)
    if errors.dim() != 1:
        raise RuntimeError("pose_auc: errors must be a float64 vector")
    n = int(errors.numel())
    thr = [float(v) for v in thresholds]
    n_thr = len(thr)
    want = [("auc", torch.float64, (n_thr,)), ("below", torch.int64, (n_thr,))]
    if return_sorted:
        want.append(("sorted", torch.float64, (n,)))
    if n_thr < 1:
        raise RuntimeError("pose_auc: thresholds must hold 1 .. 8 numbers")
    out = _bp_outputs(fn, want, out, errors.device)
    srt = out[2] if return_sorted and n > 0 else None
    if n == 0:
        errors = _bp_placeholder(errors.device, torch.float64)
    _check(_L().pats_pose_auc_f64(_ptr(errors), n, (ctypes.c_double * n_thr)(*thr), n_thr, _ptr(out[0]), _ptr(out[1]), _ptr(srt),
                                  _stream()), fn)
    return out


def homography_hypotheses_by_pair(matches_l, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False,
                                  return_samples=False, out=None, pairs=None):
    """H 4-point homography hypotheses per pair, ON THE DEVICE, one launch, no host read (pats_homography_hypotheses_by_pair_f32;
    include/pats_amd.h, "Per-pair homographies", holds the definition): for every pair and every h four distinct matches of the pair
    are drawn by the hypotheses' counter-based generator and the unit null vector of their 8x9 DLT matrix is written as a row-major
    3x3 model H, x_r ~ H x_l - the input of homography_score_by_pair.  The arguments are those of epipolar_hypotheses_by_pair.
    progressive: hypothesis h draws from the first max(4, ceil(n (h + 1) / H)) matches of the pair's list instead of all n.
    Returns models [pairs,H,3,3] float32 - exact zeros for a pair with fewer than 4 matches and for a sample with a non-finite
    coordinate - or, with return_samples=True, (models, sample_idx [pairs,H,4] int32: the draws as positions inside the pair's
    list, -1 for a pair with fewer than 4 matches).  out: the destination(s), a tensor or a tuple."""
    return _hypotheses_by_pair("homography_hypotheses_by_pair", 4, 1, _L().pats_homography_hypotheses_by_pair_f32,
                               _L().pats_homography_hypotheses_workspace_bytes, matches_l, matches_r, H, seed, pair_off, stride, counts, norm,
                               progressive, return_samples, False, out, pairs)


def homography_score_by_pair(matches_l, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None,
                             norm=None, moments=False, out=None, pairs=None):
    """H candidate homographies per pair against every match of the pair, ON THE DEVICE, no host read
    (pats_homography_score_by_pair_f32; include/pats_amd.h, "Per-pair homographies", holds the definition): match i is an inlier of
    the 3x3 model H iff d0^2 + d1^2 <= thr^2 a2^2 with a = H x_l, d = (a0 - r0 a2, a1 - r1 a2), a2^2 > 0 - the squared forward
    transfer error against thr^2 without the division.  The arguments, the segment forms, norm, min_conf and thr are those of
    epipolar_score_by_pair; an all-zero model has no inliers.
    Returns (counts [pairs,H] int32, best [pairs] int32 - the lowest index of the largest count -, best_count [pairs] int64,
    inlier [cap] uint8 - 1 where the match is an inlier of its pair's best model, 0 everywhere else) and, with moments=True,
    moments [pairs,9,9] float64 = the sum of A_i^T A_i + B_i^T B_i over those inliers (the two DLT rows of a match): the input of
    homography_refit_by_pair.  out: the four (five) destinations."""
    return _score_by_pair("homography_score_by_pair", _L().pats_homography_score_by_pair_f32, _L().pats_homography_score_workspace_bytes,
                          matches_l, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, moments, out, pairs)


def homography_score_msac_by_pair(matches_l, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None,
                                  norm=None, moments=False, out=None, pairs=None):
    """homography_score_by_pair with the winner chosen by MSAC gain (pats_homography_score_msac_by_pair_f32): the arguments and the
    outputs of epipolar_score_msac_by_pair, the squared forward transfer error d0^2 + d1^2 against thr^2 a2^2 as the test."""
    return _score_by_pair("homography_score_msac_by_pair", _L().pats_homography_score_msac_by_pair_f32,
                          _L().pats_homography_score_workspace_bytes, matches_l, matches_r, models, thr, pair_off, stride, counts, conf,
                          min_conf, norm, moments, out, pairs, msac=True)


def homography_refit_by_pair(best_count, moments=None, models=None, best=None, norm=None, swapped=False, return_pixel=False, out=None):
    """Each pair's homography refitted to its verified inliers, ON THE DEVICE, one launch, float64, no host read
    (pats_homography_refit_by_pair_f64; include/pats_amd.h, "Per-pair homographies", holds the definition): the unit eigenvector of
    `moments` for its smallest eigenvalue - without moments the winning model models[p, best[p]] promoted.  best_count [pairs] int64
    and moments [pairs,9,9] float64 (or best [pairs] int32 with the models [pairs,H,3,3] float32) are homography_score_by_pair's
    outputs; norm [pairs,8] what it was given.  swapped: the points are in the hand-over's (y, x) order; H and H_px come back in the
    reference's (x, y) frame.
    Returns (H [pairs,3,3] float64 - Frobenius norm 1, the component of largest magnitude positive: H.float() is a model for
    homography_score_by_pair -, eig [pairs,2] float64: the two smallest eigenvalues of the moments, ascending; 0 without moments),
    then H_px [pairs,3,3] float64 with return_pixel=True: the homography of the stored coordinates, N_r^-1 H N_l rescaled (H itself
    without norm).  A pair without a model (best_count < 4, a non-finite moment) has zeros everywhere.  out: the destinations."""
    fn = "homography_refit_by_pair"
    _bp_layout(fn, [(best_count, "best_count"), (moments, "moments"), (models, "models"), (best, "best"), (norm, "norm")],
               {"best_count": torch.int64, "moments": torch.float64, "best": torch.int32})
    if moments is None and (models is None or best is None):
        raise RuntimeError("homography_refit_by_pair: give moments, or models and best")
    bc = _dev(best_count, "best_count", torch.int64).reshape(-1)
    pairs = int(bc.numel())
    if pairs < 1:
        raise RuntimeError("homography_refit_by_pair: best_count must hold one int64 per pair")
    moments, models, best, H = _bp_refit_source(fn, pairs, moments, models, best)
    norm = _bp_norm(fn, norm, pairs)
    dev = bc.device
    want = [("H", torch.float64, (pairs, 3, 3)), ("eig", torch.float64, (pairs, 2))]
    if return_pixel:
        want.append(("H_px", torch.float64, (pairs, 3, 3)))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_homography_refit_workspace_bytes(pairs)
    ws = _workspace(nws, dev) if nws else None
    _check(_L().pats_homography_refit_by_pair_f64(_ptr(bc), _ptr(moments), _ptr(models), H, _ptr(best), _ptr(norm), pairs,
                                                  1 if swapped else 0, _ptr(out[0]), _ptr(out[2]) if return_pixel else None, _ptr(out[1]),
                                                  _ptr(ws), nws, _stream()), fn)
    return out


def homography_pose_by_pair(matches_l, matches_r, inlier, best_count, moments=None, models=None, best=None, pair_off=None, stride=None,
                            counts=None, norm=None, thr=None, swapped=False, min_baseline=0.0, return_candidates=False,
                            return_front=False, out=None, pairs=None):
    """Each pair's pose from its verified homography, ON THE DEVICE, no host read (pats_homography_pose_by_pair_f64;
    include/pats_amd.h, "Per-pair pose from a homography and the E-or-H decision", holds the definition): the homography refit's
    G = h_refit (the smallest eigenvector of `moments`; without moments the winning model models[p, best[p]]) decomposed into its
    four (R, t, n) candidates, one picked by the pair's matches - how many used matches (inlier != 0, finite) lie on the visible side
    of the plane, then, with thr [pairs] float32 given, how many matches of the whole segment support the candidate's essential
    matrix.  matches_l / matches_r [cap,2] float32 (also [pairs,K,2]), the segments (pair_off, or stride + counts) and norm exactly as
    homography_score_by_pair took them; inlier [cap] uint8, best_count [pairs] int64 and moments [pairs,9,9] float64 (or best [pairs]
    int32 with the models) are its outputs.  swapped as epipolar_pose_by_pair takes it.  min_baseline: a pair whose baseline
    |t| / d is at most this is taken as rotating only.
    Returns (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64, vis [pairs,4] int32, choice [pairs] int32,
    n [pairs,3], baseline [pairs] float64, sup [pairs,4] int32, status [pairs] int32: 0 no pose, 1 a pose, 2 rotation only (t = n = 0)),
    then cand_R [pairs,2,3,3], cand_t, cand_n [pairs,2,3] float64 with return_candidates=True, then front [cap] uint8 with
    return_front=True.  A pair without a pose has E = 0, R = I, t = n = 0 and no count.  out: the destinations, in that order."""
    fn = "homography_pose_by_pair"
    _bp_layout(fn, [(matches_l, "matches_l"), (matches_r, "matches_r"), (inlier, "inlier"), (best_count, "best_count"),
                    (moments, "moments"), (models, "models"), (best, "best"), (pair_off, "pair_off"), (counts, "counts"), (norm, "norm"),
                    (thr, "thr")],
               {"inlier": torch.uint8, "best_count": torch.int64, "moments": torch.float64, "best": torch.int32, "pair_off": torch.int64,
                "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if moments is None and (models is None or best is None):
        raise RuntimeError("homography_pose_by_pair: give moments, or models and best")
    min_baseline = float(min_baseline)
    if not min_baseline >= 0.0:                       # false for a NaN
        raise RuntimeError("homography_pose_by_pair: min_baseline = %r must be a number >= 0" % min_baseline)
    ml, mr, cap = _bp_matches(fn, matches_l, matches_r)
    inl = _dev(inlier, "inlier", torch.uint8).reshape(-1)
    if inl.numel() != cap:
        raise RuntimeError("homography_pose_by_pair: inlier must be [cap]")
    bc = _dev(best_count, "best_count", torch.int64).reshape(-1)
    seg, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    if bc.numel() != pairs:
        raise RuntimeError("homography_pose_by_pair: best_count must hold one int64 per pair (%d), got %d" % (pairs, bc.numel()))
    moments, models, best, H = _bp_refit_source(fn, pairs, moments, models, best)
    norm = _bp_norm(fn, norm, pairs)
    if thr is not None:
        thr = _dev(thr, "thr").reshape(-1)
        if thr.numel() != pairs:
            raise RuntimeError("homography_pose_by_pair: thr must hold one float32 per pair (%d), got %d" % (pairs, thr.numel()))
    dev = ml.device
    f64, i32 = torch.float64, torch.int32
    want = [("E", f64, (pairs, 3, 3)), ("R", f64, (pairs, 3, 3)), ("t", f64, (pairs, 3)), ("front_count", torch.int64, (pairs,)),
            ("vis", i32, (pairs, 4)), ("choice", i32, (pairs,)), ("n", f64, (pairs, 3)), ("baseline", f64, (pairs,)),
            ("sup", i32, (pairs, 4)), ("status", i32, (pairs,))]
    if return_candidates:
        want += [("cand_R", f64, (pairs, 2, 3, 3)), ("cand_t", f64, (pairs, 2, 3)), ("cand_n", f64, (pairs, 2, 3))]
    if return_front:
        want.append(("front", torch.uint8, (cap,)))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_homography_pose_workspace_bytes(pairs, cap)
    ws = _workspace(nws, dev) if nws else None
    cand = out[10:13] if return_candidates else (None, None, None)
    front = out[-1] if return_front else None
    if cap == 0:
        ml = mr = _bp_placeholder(dev)
        inl = _bp_placeholder(dev, torch.uint8)
        front = None
    _check(_L().pats_homography_pose_by_pair_f64(_ptr(ml), _ptr(mr), _ptr(inl), off_p, stride, counts_p, pairs, cap, _ptr(bc),
                                                 _ptr(moments), _ptr(models), H, _ptr(best), _ptr(norm), _ptr(thr), 1 if swapped else 0,
                                                 min_baseline, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[6]), _ptr(out[7]),
                                                 _ptr(out[4]), _ptr(out[8]), _ptr(out[5]), _ptr(out[9]), _ptr(out[3]), _ptr(cand[0]),
                                                 _ptr(cand[1]), _ptr(cand[2]), _ptr(front), _ptr(ws), nws, _stream()), fn)
    return out


def pose_select_by_pair(pose_e, best_count_e, inlier_e, pose_h, status_h, best_count_h, inlier_h, ratio, pair_off=None, stride=None,
                        counts=None, out=None, pairs=None):
    """Each pair's choice between its epipolar and its planar pose, ON THE DEVICE, one launch, no host read
    (pats_pose_select_by_pair; include/pats_amd.h, "Per-pair pose from a homography and the E-or-H decision", holds the rule).
    pose_e = (E, R, t, front_count[, front]) of epipolar_pose_by_pair with the verification's best_count_e [pairs] int64 and
    inlier_e [cap] uint8; pose_h the same of homography_pose_by_pair with its status_h [pairs] int32, best_count_h and inlier_h;
    ratio [pairs] float32; the segments (pair_off, or stride + counts) as both stages took them.  The planar pose is chosen when it
    exists and best_count_h >= ratio * best_count_e, or when fewer than 8 epipolar inliers leave no other.
    Returns (E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64, front_count [pairs] int64, branch [pairs] int32: 0 no pose,
    1 epipolar, 2 planar, 3 planar and rotation only, inlier_sel [cap] uint8), then front_sel [cap] uint8 when both poses carry a
    front: the chosen branch's values, its mask bytes over each pair's segment and 0 elsewhere.  out: the destinations, in that order."""
    fn = "pose_select_by_pair"
    if len(pose_e) not in (4, 5) or len(pose_h) not in (4, 5):
        raise RuntimeError("pose_select_by_pair: pose_e and pose_h must be (E, R, t, front_count[, front])")
    with_front = len(pose_e) == 5 and len(pose_h) == 5
    names_e = ("E_e", "R_e", "t_e", "front_count_e", "front_e")[:len(pose_e)]
    names_h = ("E_h", "R_h", "t_h", "front_count_h", "front_h")[:len(pose_h)]
    named = list(zip(pose_e, names_e)) + list(zip(pose_h, names_h)) + [
        (best_count_e, "best_count_e"), (inlier_e, "inlier_e"), (status_h, "status_h"), (best_count_h, "best_count_h"),
        (inlier_h, "inlier_h"), (ratio, "ratio"), (pair_off, "pair_off"), (counts, "counts")]
    types = {"front_count_e": torch.int64, "front_count_h": torch.int64, "front_e": torch.uint8, "front_h": torch.uint8,
             "best_count_e": torch.int64, "best_count_h": torch.int64, "inlier_e": torch.uint8, "inlier_h": torch.uint8,
             "status_h": torch.int32, "pair_off": torch.int64, "counts": torch.int64}
    types.update({n: torch.float64 for n in ("E_e", "R_e", "t_e", "E_h", "R_h", "t_h")})
    _bp_layout(fn, named, types)
    _bp_one_form(fn, pair_off, stride, counts)
    ie, ih = _dev(inlier_e, "inlier_e", torch.uint8).reshape(-1), _dev(inlier_h, "inlier_h", torch.uint8).reshape(-1)
    cap = int(ie.numel())
    if ih.numel() != cap:
        raise RuntimeError("pose_select_by_pair: inlier_e and inlier_h must both be [cap]")
    seg, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    per_pair = {"E": (pairs, 3, 3), "R": (pairs, 3, 3), "t": (pairs, 3), "front_count": (pairs,), "front": (cap,)}
    got = {}
    for tensors, names in ((pose_e, names_e), (pose_h, names_h)):
        for x, name in zip(tensors, names):
            x = _dev(x, name, types[name])
            if name.startswith("front_") and not name.startswith("front_count"):
                x = x.reshape(-1)
            if tuple(x.shape) != per_pair[name[:-2]]:
                raise RuntimeError("pose_select_by_pair: %s must be %s" % (name, list(per_pair[name[:-2]])))
            got[name] = x
    vec = {}
    for x, name, dt in ((best_count_e, "best_count_e", torch.int64), (best_count_h, "best_count_h", torch.int64),
                        (status_h, "status_h", torch.int32), (ratio, "ratio", torch.float32)):
        x = _dev(x, name, dt).reshape(-1)
        if x.numel() != pairs:
            raise RuntimeError("pose_select_by_pair: %s must hold one value per pair (%d), got %d" % (name, pairs, x.numel()))
        vec[name] = x
    dev = ie.device
    want = [("E", torch.float64, (pairs, 3, 3)), ("R", torch.float64, (pairs, 3, 3)), ("t", torch.float64, (pairs, 3)),
            ("front_count", torch.int64, (pairs,)), ("branch", torch.int32, (pairs,)), ("inlier_sel", torch.uint8, (cap,))]
    if with_front:
        want.append(("front_sel", torch.uint8, (cap,)))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_pose_select_workspace_bytes(pairs, cap)
    ws = _workspace(nws, dev) if nws else None
    fe, fh, sel, fsel = got.get("front_e"), got.get("front_h"), out[5], out[6] if with_front else None
    if not with_front:
        fe = fh = None
    if cap == 0:
        ie = ih = sel = _bp_placeholder(dev, torch.uint8)
        fe = fh = fsel = None
    _check(_L().pats_pose_select_by_pair(off_p, stride, counts_p, pairs, cap, _ptr(got["R_e"]), _ptr(got["t_e"]), _ptr(got["E_e"]),
                                         _ptr(got["front_count_e"]), _ptr(fe), _ptr(vec["best_count_e"]), _ptr(ie), _ptr(got["R_h"]),
                                         _ptr(got["t_h"]), _ptr(got["E_h"]), _ptr(got["front_count_h"]), _ptr(fh), _ptr(vec["status_h"]),
                                         _ptr(vec["best_count_h"]), _ptr(ih), _ptr(vec["ratio"]), _ptr(out[1]), _ptr(out[2]),
                                         _ptr(out[0]), _ptr(out[3]), _ptr(out[4]), _ptr(out[5] if cap else sel), _ptr(fsel), _ptr(ws),
                                         nws, _stream()), fn)
    return out


def fundamental_refit_by_pair(best_count, moments=None, models=None, best=None, norm=None, swapped=False, return_pixel=False,
                              return_refit=False, out=None):
    """Each pair's fundamental matrix from its verified inliers, ON THE DEVICE, one launch, float64, no host read
    (pats_fundamental_refit_by_pair_f64; include/pats_amd.h, "Per-pair fundamental matrices", holds the definition): the unit
    eigenvector of `moments` for its smallest eigenvalue - without moments the winning model models[p, best[p]] promoted -
    truncated to rank 2, F = U diag(s1, s2, 0) V^T, rescaled to Frobenius norm 1.  best_count [pairs] int64 and moments [pairs,9,9]
    float64 (or best [pairs] int32 with the models [pairs,H,3,3] float32) are epipolar_score_by_pair's outputs; norm [pairs,8] what
    it was given.  swapped: the points are in the hand-over's (y, x) order; F and F_px come back in the reference's (x, y) frame.
    Returns (F [pairs,3,3] float64 - the component of largest magnitude positive: F.float() is a model for epipolar_score_by_pair -,
    eig [pairs,2] float64: the two smallest eigenvalues of the moments, ascending; 0 without moments -, sigma [pairs,3] float64: the
    singular values of the refit before the truncation, descending), then F_px [pairs,3,3] float64 with return_pixel=True: the
    fundamental matrix of the stored coordinates, N_r^T F N_l rescaled (F itself without norm), then f_refit [pairs,9] float64 with
    return_refit=True: the refit before the truncation.  A pair without a model (best_count < 8, a non-finite moment, a refit of
    rank below 2) has zeros everywhere.  out: the destinations, in that order."""
    fn = "fundamental_refit_by_pair"
    _bp_layout(fn, [(best_count, "best_count"), (moments, "moments"), (models, "models"), (best, "best"), (norm, "norm")],
               {"best_count": torch.int64, "moments": torch.float64, "best": torch.int32})
    if moments is None and (models is None or best is None):
        raise RuntimeError("fundamental_refit_by_pair: give moments, or models and best")
    bc = _dev(best_count, "best_count", torch.int64).reshape(-1)
    pairs = int(bc.numel())
    if pairs < 1:
        raise RuntimeError("fundamental_refit_by_pair: best_count must hold one int64 per pair")
    moments, models, best, H = _bp_refit_source(fn, pairs, moments, models, best)
    norm = _bp_norm(fn, norm, pairs)
    dev = bc.device
    want = [("F", torch.float64, (pairs, 3, 3)), ("eig", torch.float64, (pairs, 2)), ("sigma", torch.float64, (pairs, 3))]
    if return_pixel:
        want.append(("F_px", torch.float64, (pairs, 3, 3)))
    if return_refit:
        want.append(("f_refit", torch.float64, (pairs, 9)))
    out = _bp_outputs(fn, want, out, dev)
    nws = _L().pats_fundamental_refit_workspace_bytes(pairs)
    ws = _workspace(nws, dev) if nws else None
    _check(_L().pats_fundamental_refit_by_pair_f64(_ptr(bc), _ptr(moments), _ptr(models), H, _ptr(best), _ptr(norm), pairs,
                                                   1 if swapped else 0, _ptr(out[0]), _ptr(out[3]) if return_pixel else None, _ptr(out[1]),
                                                   _ptr(out[2]), _ptr(out[-1]) if return_refit else None, _ptr(ws), nws, _stream()), fn)
    return out


def epipolar_score_adaptive_by_pair(matches_l, matches_r, models, thr, confidence, sample_size, models_per_sample=1, round_models=256,
                                    pair_off=None, stride=None, counts=None, conf=None, min_conf=None, norm=None, moments=False,
                                    out=None, pairs=None):
    """epipolar_score_by_pair with plain RANSAC's stopping rule, ON THE DEVICE, no host read
    (pats_epipolar_score_adaptive_by_pair_f32; include/pats_amd.h, "Per-pair adaptive verification", holds the definition): a
    pair's models are tested in rounds of round_models (a positive multiple of 64, at most 256 rounds); after round r, with c the
    largest count so far, k = T_r // models_per_sample samples seen and w = c / participating, the pair stops iff
    (1 - w^sample_size)^k <= 1 - confidence - float64, a fixed order of multiplications, reproducible on the host bit for bit.
    sample_size: 8, 5 or 4 for the three samplers; models_per_sample: 10 for the 5-point models.  Every other argument as
    epipolar_score_by_pair takes it.
    Returns epipolar_score_by_pair's tuple - counts are exactly 0 from used[p] on; best, best_count, inlier and moments are what the
    fixed budget gives with models[p, used[p]:] zeroed - followed by used [pairs] int32 (the models tested; H for a pair that never
    stopped) and participating [pairs] int32 (the matches that took part).  out: the six (seven) destinations."""
    return _score_by_pair("epipolar_score_adaptive_by_pair", _L().pats_epipolar_score_adaptive_by_pair_f32,
                          _L().pats_epipolar_score_adaptive_workspace_bytes, matches_l, matches_r, models, thr, pair_off, stride, counts, conf,
                          min_conf, norm, moments, out, pairs,
                          adaptive=(confidence, sample_size, models_per_sample, round_models))


def homography_score_adaptive_by_pair(matches_l, matches_r, models, thr, confidence, sample_size, models_per_sample=1, round_models=256,
                                      pair_off=None, stride=None, counts=None, conf=None, min_conf=None, norm=None, moments=False,
                                      out=None, pairs=None):
    """homography_score_by_pair with the stopping rule of epipolar_score_adaptive_by_pair
    (pats_homography_score_adaptive_by_pair_f32): the same arguments, the same rule, the same outputs, the forward transfer error as
    the test.  sample_size is 4 for the 4-point hypotheses."""
    return _score_by_pair("homography_score_adaptive_by_pair", _L().pats_homography_score_adaptive_by_pair_f32,
                          _L().pats_homography_score_adaptive_workspace_bytes, matches_l, matches_r, models, thr, pair_off, stride, counts, conf,
                          min_conf, norm, moments, out, pairs,
                          adaptive=(confidence, sample_size, models_per_sample, round_models))


# ------------------------------------------------------------------------------------------------
# ragged batches: pairs of different grids in one throughput batch (PairTable; per-cell tensors packed over cells)
# ------------------------------------------------------------------------------------------------
def chunk_rows_ragged(if_nomatching1, table, if_local=True, Cmax=None, rows_cap=None):
    """chunk_rows for a ragged batch: if_nomatching1 = the pairs' [N_p] flags packed [sum N] (batch order); each pair is planned on
    its own grid with the chunk cap of first_layer.py:131-135.  Cmax / rows_cap default to the worst case of the batch."""
    f = _as_flags(if_nomatching1, "if_nomatching1").reshape(-1)
    if f.numel() != table.cells:
        raise RuntimeError("chunk_rows_ragged: if_nomatching1 must hold the %d packed cells of the table" % table.cells)
    caps = [(2 * w if if_local else 512) for _, w in table.shapes]
    cm = [max_chunks(h, w, c) for (h, w), c in zip(table.shapes, caps)]
    Cmax = max(cm) if Cmax is None else int(Cmax)
    rows_cap = sum(h * w + (c - 1) * w for (h, w), c in zip(table.shapes, cm)) if rows_cap is None else int(rows_cap)
    r = _chunk_rows_table(table, table.pairs, None, None, table.hmax, (table.cells,), Cmax, rows_cap, f.device)
    return _chunk_rows_plan(r, (table.ref(), _ptr(f), int(bool(if_local))), "chunk_rows_ragged")


def Compute_imgs_ragged(x_scale, y_scale, average_point, if_nomatching, left_store, right_store, table, margin=128,
                        crop_format=None, out=None):
    """Compute_imgs_ex(known_count="device") for a ragged batch: the per-cell inputs packed [sum N] ([sum N, 2] for the point),
    left_store / right_store the flat HWC stores the table's img_base points into (img_base counts elements, so the stores may
    hold any of the images' dtypes of Compute_imgs_ex).  Returns (new_left, new_right [sum N,96,96,3], xsn, ysn, avn [sum N,2],
    bound5 [sum N,5], K_img [pairs], K_total [1]) - device tensors, the first K_total crops valid.  crop_format / out: as for
    Compute_imgs_ex (None: float32 HWC)."""
    if margin != 128:
        raise RuntimeError("Compute_imgs_ragged: margin=128 is what the path uses")
    cells = table.cells
    xs = _dev(x_scale.float(), "x_scale").reshape(-1)
    ys = _dev(y_scale.float(), "y_scale").reshape(-1)
    ap = _dev(average_point.float(), "average_point").reshape(-1)
    ifn = _as_flags(if_nomatching, "if_nomatching").reshape(-1)
    if xs.numel() != cells or ys.numel() != cells or ap.numel() != 2 * cells or ifn.numel() != cells:
        raise RuntimeError("Compute_imgs_ragged: per-cell inputs must hold the %d packed cells of the table" % cells)
    lf, rt, code = _crop_images(left_store, right_store, ("left_store", "right_store"))
    lfmt, rfmt, _ = _crop_formats(crop_format, code)
    lout, rout = (None, None) if out is None else out
    need = int(table.img_base_host[-1]) + table.shapes[-1][0] * table.shapes[-1][1] * 1024 * 3 if table.pairs else 0
    if lf.numel() < need or rt.numel() < need:
        raise RuntimeError("Compute_imgs_ragged: the image stores hold %d / %d elements, the table needs %d" % (lf.numel(), rt.numel(), need))
    bound5, Kd, Kt, xsn, ysn, avn = _imgs_bounds(table, xs, ys, ap, ifn, table.pairs, (cells,))
    new_left, new_right = _crops(table, lf, rt, code, 0, 0, 0, 0, 0, margin, bound5, cells, Kt, lfmt, rfmt, lout, rout, None)
    return new_left, new_right, xsn, ysn, avn, bound5, Kd, Kt


def masked_stream(cus):
    """A torch stream (torch.cuda.ExternalStream over a HIP stream of this library) whose kernels may only run on the
    compute units listed in `cus` (indices 0..255 on MI355X) - see pats_stream_create_cu_mask.  The stream lives as long as
    the process (it is not destroyed: torch may still hold references to it)."""
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    words = (n_cu + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for c in cus:
        if not 0 <= int(c) < n_cu:
            raise RuntimeError("masked_stream: CU %d outside 0..%d" % (c, n_cu - 1))
        mask[int(c) // 32] |= 1 << (int(c) % 32)
    handle = ctypes.c_void_p()
    _check(_L().pats_stream_create_cu_mask(mask, words, ctypes.byref(handle)), "masked_stream")
    return torch.cuda.ExternalStream(handle.value)


def profile_marker(tag=0):
    """An empty, uniquely named kernel on the current stream: brackets a region of a kernel trace."""
    _check(_L().pats_profile_marker(int(tag), _stream()), "profile_marker")


def attention(query, key, value, return_prob=True):
    """models/modules.py:84-88: returns (x [b,dim,heads,n], prob [b,heads,n,m]) like the reference;
    return_prob=False skips materialising prob (MultiHeadedAttention discards it, :103) and returns
    (x, None)."""
    q, k, v = _dev(query, "query"), _dev(key, "key"), _dev(value, "value")
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape or k.shape[:3] != q.shape[:3]:
        raise RuntimeError("attention: query [b,dim,heads,n], key/value [b,dim,heads,m]")
    b, dim, heads, n = q.shape
    m = k.shape[3]
    out = torch.empty((b, dim, heads, n), dtype=torch.float32, device=q.device)
    prob = torch.empty((b, heads, n, m), dtype=torch.float32, device=q.device) if return_prob else None
    _check(_L().pats_attention_f32(_ptr(q), _ptr(k), _ptr(v), b, dim, heads, n, m, _ptr(out), _ptr(prob), _stream()),
           "attention")
    return out, prob


# ------------------------------------------------------------------------------------------------
# the GNN layer around the attention core
# ------------------------------------------------------------------------------------------------
class _PropagationWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("wq_t", "bq", "wk_t", "bk", "wv_t", "bv", "wm_t", "bm", "w1_t", "b1",
                                               "bn_a", "bn_b", "w2_t", "b2")]


class PropagationParams:
    """Device-resident weights of one AttentionalPropagation layer (modules.py:107-113) in the layout the C-ABI takes
    (Conv1d matrices transposed, BatchNorm folded for eval mode).  Build it once per layer:
        PropagationParams(layer.state_dict())          # a reference module's own parameters, or any dict with its names
    """

    def __init__(self, state, device="cuda", eps=1e-5, prefix=""):
        def get(name):
            t = state[prefix + name]
            t = torch.from_numpy(np.asarray(t)) if not isinstance(t, torch.Tensor) else t
            return t.detach().to(device=device, dtype=torch.float32)

        def mat_t(name):                              # [C_out, C_in, 1] -> [C_in][C_out]
            w = get(name)
            return w.reshape(w.shape[0], -1).t().contiguous()
        self.eps = float(eps)
        self._packed = {}
        self.C = get("attn.merge.bias").shape[0]
        self.t = {"wq_t": mat_t("attn.proj.0.weight"), "bq": get("attn.proj.0.bias").contiguous(),
                  "wk_t": mat_t("attn.proj.1.weight"), "bk": get("attn.proj.1.bias").contiguous(),
                  "wv_t": mat_t("attn.proj.2.weight"), "bv": get("attn.proj.2.bias").contiguous(),
                  "wm_t": mat_t("attn.merge.weight"), "bm": get("attn.merge.bias").contiguous(),
                  "w1_t": mat_t("mlp.0.weight"), "b1": get("mlp.0.bias").contiguous(),
                  "w2_t": mat_t("mlp.3.weight"), "b2": get("mlp.3.bias").contiguous()}
        gamma, beta = get("mlp.1.weight"), get("mlp.1.bias")
        scale = gamma / torch.sqrt(get("mlp.1.running_var") + self.eps)
        self.bn = {False: (scale.contiguous(), (beta - get("mlp.1.running_mean") * scale).contiguous()),   # eval: folded
                   True: (gamma.contiguous(), beta.contiguous())}                                       # train: gamma / beta

    def packed(self, heads=4):
        """The Conv1d matrices split into fp16 hi + lo halves in MFMA fragment order (pats_propagation_pack_f32), made once and
        kept beside the weights; None if the library has no packed form for this shape."""
        key = int(heads)
        if key not in self._packed:
            nb = _L().pats_propagation_packed_bytes(self.C, key)
            buf = None
            if nb:
                buf = torch.empty((nb,), dtype=torch.uint8, device=self.t["wq_t"].device)
                w = self.struct(False)
                with torch.cuda.device(buf.device):
                    _check(_L().pats_propagation_pack_f32(ctypes.byref(w), self.C, key, _ptr(buf), nb, _stream()), "propagation_pack")
            self._packed[key] = buf
        return self._packed[key]

    def struct(self, bn_train):
        a, b = self.bn[bool(bn_train)]
        w = _PropagationWeights()
        for k, v in self.t.items():
            setattr(w, k, v.data_ptr())
        w.bn_a, w.bn_b = a.data_ptr(), b.data_ptr()
        return w


def attentional_propagation(x, source, params, heads=4, bn_train=False, residual=None, count=None, out=None, count_off=0):
    """AttentionalPropagation.forward(x, source) (modules.py:114-117) -> delta [b,C,n]; with `residual` (= x in
    AttentionalGNN.forward, :131-133) the sum residual + delta.  bn_train: BatchNorm on batch statistics - what the
    third layer's GNN does under PATS.eval() (pats.py:112-120).  Six GEMM launches + the attention kernel.
    count: optional device int64 [1]; rows >= clamp(count - count_off, 0, b) are not problems.  Honoured by the one-kernel layers
    (the fine level's [b, 264, 145] and the third level's [b, 128, 65], eval mode), also when an overflow sends the call to the
    gated composition: rows past it are zeros (fine) / left untouched (third).  Any other shape: ignored, every row is computed.
    bn_train with a count is refused (the batch statistics would take in the padding rows)."""
    if bn_train and count is not None:
        raise RuntimeError("attentional_propagation: bn_train=True with a device-side count is not supported "
                           "(the batch statistics would take in the rows past the count)")
    x, source = _dev(x, "x"), _dev(source, "source")
    b, C, n = x.shape
    m = source.shape[2]
    if source.shape[0] != b or source.shape[1] != C or C != params.C:
        raise RuntimeError("attentional_propagation: x %s / source %s / weights C=%d do not match"
                           % (tuple(x.shape), tuple(source.shape), params.C))
    res = _dev(residual, "residual") if residual is not None else None
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.dtype != torch.float32 or not out.is_cuda:
        raise RuntimeError("attentional_propagation: out must be a contiguous float32 GPU tensor shaped like x")
    nb = _L().pats_attentional_propagation_workspace_bytes(b, C, n, m)
    ws = _workspace(nb, x.device)
    w = params.struct(bn_train)
    pk = params.packed(heads)      # the third level's shape: one fused kernel (gnn_fused.hip); any other: packed-weights convolutions
    if pk is not None and count is not None:
        _check(_L().pats_attentional_propagation_packed_counted_f32(_ptr(x), _ptr(source), b, _ptr(_dev(count, "count", torch.int64)),
                                                                    int(count_off), C,
                                                                    int(heads), n, m, ctypes.byref(w), _ptr(pk), int(bool(bn_train)),
                                                                    float(params.eps), _ptr(res), _ptr(out), _ptr(ws), nb, _stream()),
               "attentional_propagation")
        return out
    if pk is not None:
        _check(_L().pats_attentional_propagation_packed_f32(_ptr(x), _ptr(source), b, C, int(heads), n, m, ctypes.byref(w), _ptr(pk),
                                                            int(bool(bn_train)), float(params.eps), _ptr(res), _ptr(out), _ptr(ws),
                                                            nb, _stream()), "attentional_propagation")
        return out
    _check(_L().pats_attentional_propagation_f32(_ptr(x), _ptr(source), b, C, int(heads), n, m, ctypes.byref(w),
                                                 int(bool(bn_train)), float(params.eps), _ptr(res), _ptr(out), _ptr(ws), nb,
                                                 _stream()), "attentional_propagation")
    return out


UNSUPPORTED = 2            # include/pats_amd.h PATS_ERR_UNSUPPORTED
GNN_STACK_ROWS = 4096     # rows of a descriptor set per pats_attentional_gnn_packed_f32 call (its workspace is ~1.9 MB a row)


def _gnn_packed_stack(desc0, desc1, layers, names, heads, count=None, out=None):
    """The whole stack in the fine level's one-kernel form (csrc/gnn_fine.hip), or None if the library has no such form for
    this shape (anything but [b, 264, 145], 4 heads)."""
    b, C, n = desc0.shape
    if tuple(desc1.shape) != (b, C, n) or b == 0 or not _L().pats_attentional_gnn_packed_workspace_bytes(1, C, int(heads), n):
        return None
    packed = [p.packed(heads) for p in layers]
    if any(pk is None for pk in packed) or any(p.C != C for p in layers):
        return None
    L = len(layers)
    structs = [p.struct(False) for p in layers]
    w_arr = (ctypes.c_void_p * max(L, 1))(*[ctypes.addressof(w) for w in structs])
    pk_arr = (ctypes.c_void_p * max(L, 1))(*[pk.data_ptr() for pk in packed])
    cross = (ctypes.c_int * max(L, 1))(*[1 if nm == "cross" else 0 for nm in names])
    out0, out1 = out if out is not None else (torch.empty_like(desc0), torch.empty_like(desc1))
    for lo in range(0, b, GNN_STACK_ROWS):
        hi = min(b, lo + GNN_STACK_ROWS)
        nb = _L().pats_attentional_gnn_packed_workspace_bytes(hi - lo, C, int(heads), n)
        ws = _workspace(nb, desc0.device)
        rc = _L().pats_attentional_gnn_packed_f32(_ptr(desc0[lo:hi]), _ptr(desc1[lo:hi]), hi - lo, _ptr(count), lo, C, int(heads), n, L, w_arr,
                                                  pk_arr, cross,
                                                  float(layers[0].eps) if L else 1e-5, _ptr(out0[lo:hi]), _ptr(out1[lo:hi]), _ptr(ws), nb,
                                                  _stream())
        if rc == UNSUPPORTED:
            return None
        _check(rc, "attentional_gnn_packed")
    return out0, out1


GNN_LAYER_ROWS = 32768    # rows per pass of the layer-by-layer path over a big batch (a layer's workspace is ~7 tensors)


def attentional_gnn(desc0, desc1, layers, names, heads=4, bn_train=False, count=None, out=None):
    """AttentionalGNN.forward (modules.py:127-134): layers = [PropagationParams, ...], names = ['self', 'cross', ...].
    At the fine level's shape ([b, 264, 145], eval-mode BatchNorm) the whole stack runs in the one-kernel layer's own descriptor
    form (pats_attentional_gnn_packed_f32); any other shape: layer by layer (eval mode: in blocks of GNN_LAYER_ROWS rows - rows are
    independent problems, a cross layer couples row i of one set with row i of the other only).
    count: optional device int64 [1] - only rows < count are problems (throughput mode: the launches cover a capacity); honoured
    by the one-kernel layers (fine and third level's shapes, eval mode), rows past it are zeros (fine) / left untouched (third),
    also after an overflow redo; any other shape ignores it.  bn_train with a count is refused.
    out: optional (out0, out1), contiguous float32 GPU tensors shaped like the inputs."""
    if bn_train and count is not None:
        raise RuntimeError("attentional_gnn: bn_train=True with a device-side count is not supported "
                           "(the batch statistics would take in the rows past the count)")
    layers, names = list(layers), list(names)
    desc0, desc1 = _dev(desc0, "desc0"), _dev(desc1, "desc1")
    if out is not None and (len(out) != 2 or any(tuple(o.shape) != tuple(desc0.shape) or not o.is_contiguous() for o in out)):
        raise RuntimeError("attentional_gnn: out must be two contiguous tensors shaped like the descriptors")
    if count is not None:
        count = _dev(count, "count", torch.int64)
    if not bn_train and len(layers) == len(names):
        got = _gnn_packed_stack(desc0, desc1, layers, names, heads, count, out)
        if got is not None:
            return got
    b = desc0.shape[0]
    if len(layers) == 0:
        if out is not None:
            out[0].copy_(desc0)
            out[1].copy_(desc1)
            return out[0], out[1]
        return desc0, desc1
    # batch statistics couple all rows of a launch: no blocking there
    step = b if (bn_train or b <= GNN_LAYER_ROWS) else GNN_LAYER_ROWS
    if not bn_train and tuple(desc0.shape[1:]) == (264, 145):
        step = min(step, 2 * GNN_STACK_ROWS)     # (the fine level's kernels keep 0.5 MB of projections per problem in the workspace)
    if step == b and out is None:
        res = None
    else:
        res = out if out is not None else (torch.empty_like(desc0), torch.empty_like(desc1))
    # Eval-mode BatchNorm and no device-side count: a layer treats every problem on its own and both descriptor sets go through the SAME
    # weights, so the two sets run as ONE batch of 2 b problems - one launch chain a layer instead of two ('cross': the sources are the
    # sets swapped).  Same kernels, same per-problem arithmetic: the same bits; at the coarse level of one pair (2 x [448, 300]) the
    # 18 layers were 432 launches of ~23 us for almost no work (6 of a pair's 26.6 ms with the heads inside).
    if not bn_train and count is None:
        for lo in range(0, max(b, 1), max(step, 1)):
            hi = min(b, lo + step)
            bb = hi - lo
            X = torch.cat([desc0[lo:hi], desc1[lo:hi]])
            for p, name in zip(layers, names):
                src = torch.cat([X[bb:], X[:bb]]) if name == "cross" else X
                X = attentional_propagation(X, src, p, heads, False, residual=X)
            if res is None:
                return X[:bb], X[bb:]
            res[0][lo:hi].copy_(X[:bb])
            res[1][lo:hi].copy_(X[bb:])
        return res[0], res[1]
    for lo in range(0, max(b, 1), max(step, 1)):
        hi = min(b, lo + step)
        c0, c1 = desc0[lo:hi], desc1[lo:hi]
        for li, (p, name) in enumerate(zip(layers, names)):
            src0, src1 = (c1, c0) if name == "cross" else (c0, c1)
            last = li == len(layers) - 1 and res is not None
            n0 = attentional_propagation(c0, src0, p, heads, bn_train, residual=c0, count=count, count_off=lo, out=res[0][lo:hi] if last else None)
            n1 = attentional_propagation(c1, src1, p, heads, bn_train, residual=c1, count=count, count_off=lo, out=res[1][lo:hi] if last else None)
            c0, c1 = n0, n1
        if res is None:
            return c0, c1
    return res[0], res[1]


# ------------------------------------------------------------------------------------------------
# the descriptor heads either side of the GNN: Conv1d(k=1) alone (final_proj) and chained (MLP / KeypointEncoder)
# ------------------------------------------------------------------------------------------------
def _pad8(t, dim):
    """Zero channels up to a multiple of 8 along `dim` (the contraction's operand slabs are 8 channels)."""
    k = t.shape[dim]
    if k % 8 == 0:
        return t
    shape = list(t.shape)
    shape[dim] = (-k) % 8
    return torch.cat([t, t.new_zeros(shape)], dim=dim).contiguous()


def conv1d(x, weight, bias=None, in_scale=None, in_shift=None, residual=None, weight_t=None):
    """nn.Conv1d(kernel_size=1) as the path uses it (final_proj: first_layer.py:34-36,105, second_layer.py:40-42,91;
    the layers of MLP, modules.py:57-69): x [b,K,n], weight [M,K,1] or [M,K] (the module's own layout), bias [M] or
    None -> [b,M,n].  in_scale / in_shift [K]: x is max(0, x * scale + shift) while it is staged - the BatchNorm1d + ReLU
    of the previous MLP layer, folded.  residual [b,M,n] is added to the result.
    weight_t: the weight already in the C-ABI's layout ([K8][M]: transposed, input channels zero-padded to a multiple of
    8 - MLPParams keeps it), so that no transpose / pad kernel runs per call."""
    x = _dev(x, "x")
    weight = _dev(weight, "weight")
    b, K, n = x.shape
    w2 = weight.reshape(weight.shape[0], -1)
    M = w2.shape[0]
    if w2.shape[1] != K:
        raise RuntimeError("conv1d: weight %s does not take %d input channels" % (tuple(weight.shape), K))
    if weight_t is not None:
        w_t = _dev(weight_t, "weight_t")
        if tuple(w_t.shape) != (K + (-K) % 8, M):
            raise RuntimeError("conv1d: weight_t must be [%d,%d]" % (K + (-K) % 8, M))
    else:
        w_t = _pad8(w2.t().contiguous(), 0)             # [K][M], zero rows for the padding channels
    xp = _pad8(x, 1)
    sc = sh = None
    if in_scale is not None:
        sc = _pad8(_dev(in_scale, "in_scale").reshape(-1), 0)      # padded channels: max(0, 0 * 0 + 0) = 0
        sh = _pad8(_dev(in_shift, "in_shift").reshape(-1), 0)
        if sc.numel() != xp.shape[1] or sh.numel() != xp.shape[1]:
            raise RuntimeError("conv1d: in_scale / in_shift must have %d entries" % K)
    bs = _dev(bias, "bias").reshape(-1) if bias is not None else None
    if bs is not None and bs.numel() != M:
        raise RuntimeError("conv1d: bias must have %d entries" % M)
    res = _dev(residual, "residual") if residual is not None else None
    if res is not None and tuple(res.shape) != (b, M, n):
        raise RuntimeError("conv1d: residual %s is not [%d,%d,%d]" % (tuple(res.shape), b, M, n))
    y = torch.empty((b, M, n), dtype=torch.float32, device=x.device)
    if b == 0 or n == 0:
        return y
    nb = _L().pats_conv1x1_workspace_bytes()
    ws = _workspace(nb, x.device)
    _check(_L().pats_conv1x1_f32(_ptr(w_t), _ptr(bs), _ptr(xp), b, xp.shape[1], M, n, _ptr(sc), _ptr(sh), _ptr(res), _ptr(y),
                                 _ptr(ws), nb, _stream()), "conv1d")
    return y


def bn_fold(h, gamma, beta, eps=1e-5):
    """BatchNorm1d in train mode, folded: (scale, shift) [C] each with scale = gamma / sqrt(var + eps) and
    shift = beta - mean * scale over the batch statistics of h [b,C,n] (biased variance, what F.batch_norm
    normalises with).  Feed them to the next conv1d as in_scale / in_shift."""
    h, gamma, beta = _dev(h, "h"), _dev(gamma, "gamma").reshape(-1), _dev(beta, "beta").reshape(-1)
    b, C, n = h.shape
    if gamma.numel() != C or beta.numel() != C:
        raise RuntimeError("bn_fold: gamma / beta must have %d entries" % C)
    scale = torch.empty((C,), dtype=torch.float32, device=h.device)
    shift = torch.empty_like(scale)
    nb = _L().pats_bn_fold_workspace_bytes(C)
    ws = _workspace(nb, h.device)
    _check(_L().pats_bn_fold_f32(_ptr(h), b, C, n, _ptr(gamma), _ptr(beta), float(eps), _ptr(scale), _ptr(shift), _ptr(ws), nb,
                                 _stream()), "bn_fold")
    return scale, shift


class MLPParams:
    """The parameters of one `MLP(channels)` (modules.py:57-69: Conv1d [BatchNorm1d ReLU] ... Conv1d) from the
    nn.Sequential's own state_dict ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var",
    "3.weight", ...), device-resident.  `prefix` selects a sub-module, e.g. "encoder." for a KeypointEncoder."""

    def __init__(self, state, device="cuda", eps=1e-5, prefix=""):
        def get(name):
            t = state[prefix + name]
            t = torch.from_numpy(np.asarray(t)) if not isinstance(t, torch.Tensor) else t
            return t.detach().to(device=device, dtype=torch.float32).contiguous()
        self.eps = float(eps)
        idx = sorted({int(k[len(prefix):].split(".")[0]) for k in state if k.startswith(prefix) and k[len(prefix):].split(".")[0].isdigit()})
        convs = [i for i in idx if get("%d.weight" % i).dim() == 3]
        self.layers = []
        for li, i in enumerate(convs):
            wgt = get("%d.weight" % i)
            layer = {"weight": wgt, "bias": get("%d.bias" % i), "bn": None,
                     "weight_t": _pad8(wgt.reshape(wgt.shape[0], -1).t().contiguous(), 0)}       # once, not per call
            if li + 1 < len(convs) and (prefix + "%d.running_var" % (i + 1)) in state:        # do_bn, not after the last Conv1d
                g, bta = get("%d.weight" % (i + 1)), get("%d.bias" % (i + 1))
                rm, rv = get("%d.running_mean" % (i + 1)), get("%d.running_var" % (i + 1))
                sc = g / torch.sqrt(rv + self.eps)
                layer["bn"] = {"gamma": g, "beta": bta, "eval": (sc.contiguous(), (bta - rm * sc).contiguous())}
            self.layers.append(layer)


def mlp(x, params, bn_train=False):
    """MLP.forward (modules.py:57-69): Conv1d -> BatchNorm1d -> ReLU -> ... -> Conv1d.  One GEMM launch per Conv1d; each
    BatchNorm + ReLU rides on the next layer's operand staging (eval: folded running statistics; bn_train: batch
    statistics, pats_bn_fold_f32).  An MLP built with do_bn=False would need a ReLU-only fold: scale 1, shift 0."""
    sc = sh = None
    h = _dev(x, "x")
    for i, layer in enumerate(params.layers):
        h = conv1d(h, layer["weight"], layer["bias"], sc, sh, weight_t=layer.get("weight_t"))
        if i + 1 < len(params.layers):
            bn = layer["bn"]
            if bn is None:
                sc = torch.ones((h.shape[1],), dtype=torch.float32, device=h.device)
                sh = torch.zeros_like(sc)
            elif bn_train:
                sc, sh = bn_fold(h, bn["gamma"], bn["beta"], params.eps)
            else:
                sc, sh = bn["eval"]
    return h


def keypoint_encoder(kpts, params, bn_train=False):
    """KeypointEncoder.forward (modules.py:77-82): kpts [n,2] -> [1, feature_dim, n] (first_layer.py:81,99 adds it to the
    coarse descriptors, third_layer.py:139-140 to the 8x8 windows).  `params` = MLPParams(kenc.state_dict(), prefix="encoder.")."""
    kpts = _dev(kpts, "kpts")
    inputs = kpts.transpose(0, 1).reshape(1, 2, -1).contiguous()
    return mlp(inputs, params, bn_train)


def scale_head(desc1, height, width, weights, biases, return_heads=False):
    """The scale head of a layer -> `ns` [b,1,h*w] of its OT problems:
        exp(sigmoid(proj(desc1[:, :, :h*w].reshape(b, C, h, w))) * log(256) - log(256) / 2),  proj = nn.Conv2d(C, 1, 3, padding=1)
    first_layer.py:106-107 (weights = [scalex_proj.weight]); second_layer.py:92-98 (weights = [scalex_proj.weight,
    scaley_proj.weight]: the product scale_x * scale_y); third_layer.py:151-152 ([scale_proj.weight]).  desc1 [b,C,ld]
    with ld = h*w or h*w + 1 (the dustbin feature column is skipped like `[:, :, :-1]`).  return_heads: also the list of
    the heads on their own ([b,1,h*w] each: scale_x, scale_y of second_layer.py:92-97, which est_position takes separately)."""
    desc1 = _dev(desc1, "desc1")
    b, C, ld = desc1.shape
    if not isinstance(weights, (list, tuple)):
        weights, biases = [weights], [biases]
    heads = len(weights)
    wt = torch.cat([_dev(wg, "weight").reshape(1, C, 3, 3) for wg in weights], dim=0).contiguous()
    bs = torch.cat([_dev(bi, "bias").reshape(1) for bi in biases]).contiguous()
    out = torch.empty((b, 1, height * width), dtype=torch.float32, device=desc1.device)
    per = torch.empty((b, heads, height * width), dtype=torch.float32, device=desc1.device) if return_heads else None
    _check(_L().pats_scale_head_f32(_ptr(desc1), b, C, ld, int(height), int(width), _ptr(wt), _ptr(bs), heads, _ptr(out),
                                    _ptr(per), _stream()), "scale_head")
    if return_heads:
        return out, [per[:, i:i + 1, :] for i in range(heads)]
    return out


def _polish_checked(fn, fam, first, matches_r, models, thr, best, rounds, pair_off, stride, counts, conf, min_conf, norm, out, pairs,
                    steps=None):
    """What every local optimisation checks and allocates; the caller lays out its own C call from what comes back -> (lists, seg,
    models, thr_norm, gate, walk, inlier, out): tuples of C arguments - (first, matches_r, conf), (pair_off, stride, counts_in, pairs,
    cap), (models, H), (thr, norm), (use_min_conf, min_conf), (best, rounds) or, for a family with a cost, (best, rounds, steps) -, the
    pointer of the mask, and the destinations."""
    _bp_layout(fn, [(first, fam.first), (matches_r, "matches_r"), (models, "models"), (thr, "thr"), (best, "best"),
                    (pair_off, "pair_off"), (counts, "counts"), (conf, "conf"), (norm, "norm")],
               {"best": torch.int32, "pair_off": torch.int64, "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if min_conf is not None and conf is None:
        raise RuntimeError("%s: min_conf needs conf" % fn)
    walk = (int(rounds), int(steps)) if fam.cost else (int(rounds),)
    rounds = walk[0]
    if not 1 <= rounds <= 16:
        raise RuntimeError("%s: rounds = %d, must lie in 1 .. 16" % (fn, rounds))
    if fam.cost and not 1 <= walk[1] <= 8:
        raise RuntimeError("%s: steps = %d, must lie in 1 .. 8" % (fn, walk[1]))
    a, mr, models, thr, H, seg = _bp_candidates(fn, fam, first, matches_r, models, thr, pair_off, stride, counts, pairs)
    pairs, cap = seg[3:]
    if best is None:
        if H != 1:
            raise RuntimeError("%s: best may be left out with %s == 1 only, got %s = %d" % (fn, fam.letter, fam.letter, H))
    else:
        best = _bp_vector(best, "best", torch.int32)
        if best.numel() != pairs:
            raise RuntimeError("%s: best must hold one int32 per pair (%d), got %d" % (fn, pairs, best.numel()))
    conf, norm = _bp_conf_norm(fn, conf, cap, norm, pairs)
    want = [("model", torch.float32, (pairs,) + fam.model), ("best_count", torch.int64, (pairs,)), ("inlier", torch.uint8, (cap,))]
    if fam.moments:
        want.append(("moments", torch.float64, (pairs, 9, 9)))
    want += [("best_round", torch.int32, (pairs,)), ("counts", torch.int32, (pairs, rounds + 1))]
    if fam.cost:
        want.append(("cost", torch.float64, (pairs, rounds + 1)))
    out = _bp_outputs(fn, want, out, a.device)
    lists, gate, inl = _bp_gated_call(a, mr, conf, out[2], min_conf, cap)
    return lists, seg, (_ptr(models), H), (_ptr(thr), _ptr(norm)), gate, (_ptr(best),) + walk, inl, out


def _polish_by_pair(fn, entry, workspace_bytes, matches_l, matches_r, models, thr, best, rounds, pair_off, stride, counts, conf, min_conf,
                    norm, out, pairs):
    """The C call of the three epipolar and homography local optimisations from _polish_checked's pieces (entry and its workspace
    query are looked up by the callers, as for _score_by_pair)."""
    lists, seg, models, thr_norm, gate, walk, inl, out = _polish_checked(fn, _EPI, matches_l, matches_r, models, thr, best, rounds, pair_off,
                                                                         stride, counts, conf, min_conf, norm, out, pairs)
    nws = workspace_bytes(seg[3], models[1], seg[4])    # pairs, H, cap
    ws = _workspace(nws, out[0].device) if nws else None
    _check(entry(*lists, *seg, *thr_norm, *gate, *models, *walk, _ptr(out[0]), _ptr(out[1]), inl, _ptr(out[3]), _ptr(out[4]),
                 _ptr(out[5]), _ptr(ws), nws, _stream()), fn)
    return out


def epipolar_polish_by_pair(matches_l, matches_r, models, thr, best=None, rounds=4, pair_off=None, stride=None, counts=None, conf=None,
                            min_conf=None, norm=None, out=None, pairs=None):
    """Local optimisation of each pair's winning epipolar model, ON THE DEVICE, one launch, no host read
    (pats_epipolar_polish_by_pair_f32; include/pats_amd.h, "Per-pair local optimisation", holds the definition): starting from
    m_0 = models[p, best[p]], `rounds` times "refit the current model's inliers (epipolar_pose_by_pair's E, cast to float32), verify the
    refit (epipolar_score_by_pair with that one model)", and the round with the most inliers - the lowest among equals, round 0 being
    the input - is returned.  Every value equals what that chain of calls gives, bit for bit.  matches_l / matches_r, the segment
    forms (pair_off, or stride + counts), conf / min_conf, norm and thr exactly as epipolar_score_by_pair takes them; models
    [pairs,H,3,3] float32 and best [pairs] int32 are its input and output (best may be left out with H == 1); 1 <= rounds <= 16.
    Returns (model [pairs,3,3] float32, best_count [pairs] int64, inlier [cap] uint8, moments [pairs,9,9] float64 - the best round's,
    what epipolar_pose_by_pair takes -, best_round [pairs] int32, counts [pairs, rounds + 1] int32: the support of every round, a walk
    that stopped early on a repeated model padded with its count).  out: the six destinations."""
    return _polish_by_pair("epipolar_polish_by_pair", _L().pats_epipolar_polish_by_pair_f32, _L().pats_epipolar_polish_workspace_bytes,
                           matches_l, matches_r, models, thr, best, rounds, pair_off, stride, counts, conf, min_conf, norm, out, pairs)


def homography_polish_by_pair(matches_l, matches_r, models, thr, best=None, rounds=4, pair_off=None, stride=None, counts=None, conf=None,
                              min_conf=None, norm=None, out=None, pairs=None):
    """epipolar_polish_by_pair for homographies (pats_homography_polish_by_pair_f32): the same arguments, the same outputs, the
    forward transfer error of homography_score_by_pair as the test and homography_refit_by_pair's H, cast to float32, as the refit;
    moments and best_count are what homography_refit_by_pair takes."""
    return _polish_by_pair("homography_polish_by_pair", _L().pats_homography_polish_by_pair_f32,
                           _L().pats_homography_polish_workspace_bytes, matches_l, matches_r, models, thr, best, rounds, pair_off, stride,
                           counts, conf, min_conf, norm, out, pairs)


def fundamental_polish_by_pair(matches_l, matches_r, models, thr, best=None, rounds=4, pair_off=None, stride=None, counts=None, conf=None,
                               min_conf=None, norm=None, out=None, pairs=None):
    """epipolar_polish_by_pair for uncalibrated callers (pats_fundamental_polish_by_pair_f32): the same arguments, the same outputs,
    the same Sampson test, and fundamental_refit_by_pair's F - the refit truncated to rank 2, not projected onto the essential
    matrices -, cast to float32, as the refit; moments and best_count are what fundamental_refit_by_pair takes."""
    return _polish_by_pair("fundamental_polish_by_pair", _L().pats_fundamental_polish_by_pair_f32,
                           _L().pats_fundamental_polish_workspace_bytes, matches_l, matches_r, models, thr, best, rounds, pair_off, stride,
                           counts, conf, min_conf, norm, out, pairs)


# ---- the image front end (csrc/prepare.hip; include/pats_amd.h, "Image front end") ----------------------------------------------
# pats_prepare_image_t
_PREPARE_IMAGE = np.dtype([("src", np.uint64), ("dst", np.int64), ("scale_x", np.float64), ("scale_y", np.float64)] +
                          [(n, np.int32) for n in ("h0", "w0", "y0", "x0", "h_c", "w_c", "h_t", "w_t", "H", "W", "side", "bgr")], align=True)
assert _PREPARE_IMAGE.itemsize == 80


def prepare_images_max_side():
    """The largest source or canvas side prepare_images takes (pats_prepare_images_max_side)."""
    return int(_L().pats_prepare_images_max_side())


def prepare_target(h0, w0, size):
    """(w_t, h_t) of an [h0, w0] image whose longer side becomes `size`, with the reference's truncations (yfcc.py:35-37)."""
    s = size / max(h0, w0)
    return int(w0 * s), int(h0 * s)


def prepare_window(h0, w0, w_t, h_t):
    """The centre crop to the target's aspect (Resize_img's slices) -> (y0, x0, h_c, w_c)."""
    if w0 / w_t < h0 / h_t:
        gap = int((h0 - w0 / w_t * h_t) / 2)
        return gap, 0, h0 - 2 * gap, w0
    gap = int((w0 - h0 / h_t * w_t) / 2)
    return 0, gap, h0, w0 - 2 * gap


class PreparePlan:
    """What prepare_plan returns - host data only, every array in CALLER order:
        h0, w0, y0, x0, h_c, w_c, h_t, w_t   [pairs,2] int64 (left, right): the raw size, the crop window, the target
        canvas                               [pairs,2] int64 (H, W): the pair's canvas;  shapes: its grid (H / 32, W / 32)
        caller_of, slot_of                   the slots of the pack: caller indices sorted stably by grid (batch.slot_order)
        dst                                  [pairs] int64: the offset in elements of the pair's canvas in either flat store
                                             (PairTable.img_base of its slot);  elems: the length of a store"""


def prepare_plan(sizes, size=None, targets=None, canvas=None):
    """The host half of the image front end, no GPU: sizes = [((h0, w0) left, (h0, w0) right)] per pair.  Give either `size` (the
    longer side of every target, prepare_target) or `targets`: one (w_t, h_t) for every image, or [((w_t, h_t), (w_t, h_t))] per
    pair.  canvas: None = per pair the maximum of its images' ceil32 targets in each axis (yfcc.py:43-60), or one fixed (H, W) -
    multiples of 32 - for all pairs (scannet.py:52-53); ValueError if a target does not fit it.  Returns a PreparePlan."""
    if not sizes:
        raise ValueError("prepare_plan: no pairs")
    if (size is None) == (targets is None):
        raise ValueError("prepare_plan: give either size or targets")
    n = len(sizes)
    if targets is not None and not isinstance(targets[0], (tuple, list)):
        targets = [((int(targets[0]), int(targets[1])),) * 2] * n
    if targets is not None and len(targets) != n:
        raise ValueError("prepare_plan: %d targets for %d pairs" % (len(targets), n))
    if canvas is not None and (canvas[0] < 32 or canvas[1] < 32 or canvas[0] % 32 or canvas[1] % 32):
        raise ValueError("prepare_plan: the canvas (%d, %d) must be positive multiples of 32" % tuple(canvas))
    pl = PreparePlan()
    names = ("h0", "w0", "y0", "x0", "h_c", "w_c", "h_t", "w_t")
    for name in names:
        setattr(pl, name, np.zeros((n, 2), np.int64))
    pl.canvas = np.zeros((n, 2), np.int64)
    for p in range(n):
        for side in range(2):
            h0, w0 = int(sizes[p][side][0]), int(sizes[p][side][1])
            if h0 < 1 or w0 < 1:
                raise ValueError("prepare_plan: pair %d has an empty image" % p)
            w_t, h_t = prepare_target(h0, w0, size) if targets is None else (int(targets[p][side][0]), int(targets[p][side][1]))
            if w_t < 1 or h_t < 1:
                raise ValueError("prepare_plan: pair %d: the target %d x %d (h x w) is empty" % (p, h_t, w_t))
            for name, v in zip(names, (h0, w0) + prepare_window(h0, w0, w_t, h_t) + (h_t, w_t)):
                getattr(pl, name)[p, side] = v
        H, W = (-(-int(pl.h_t[p].max()) // 32) * 32, -(-int(pl.w_t[p].max()) // 32) * 32) if canvas is None else (int(canvas[0]), int(canvas[1]))
        if pl.h_t[p].max() > H or pl.w_t[p].max() > W:
            raise ValueError("prepare_plan: pair %d: the target %d x %d does not fit the canvas %d x %d"
                             % (p, pl.h_t[p].max(), pl.w_t[p].max(), H, W))
        pl.canvas[p] = (H, W)
    pl.shapes = [(int(H) // 32, int(W) // 32) for H, W in pl.canvas]
    pl.caller_of = sorted(range(n), key=lambda i: pl.shapes[i])        # batch.slot_order
    pl.slot_of = [0] * n
    pl.dst = np.zeros(n, np.int64)
    off = 0
    for s, i in enumerate(pl.caller_of):
        pl.slot_of[i], pl.dst[i] = s, off
        off += int(pl.canvas[i, 0] * pl.canvas[i, 1]) * 3
    pl.elems = off
    return pl


def prepare_intrinsics(K, h0, w0, w_t, h_t, mode="ratio"):
    """The raw image's K [3,3] -> K' float64 of the prepared image, in numpy float64 and the reference's operation order.
    "ratio": Get_resize_ratio as yfcc.py:39-42 applies it (the float gap, not the crop's integer gap); "axes": scale_intrinsics as
    scannet.py:54-55 applies it.  include/pats_amd.h, "Image front end", states both."""
    K = np.array(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError("prepare_intrinsics: K must be 3 x 3")
    if mode == "ratio":
        w, h, w_new, h_new = float(w0), float(h0), float(w_t), float(h_t)
        h_w = h_new / w_new
        add = np.zeros(2, np.float64)
        if w / w_new < h / h_new:
            r = w_new / w
            add[1] = (h - w * h_w) / 2
        else:
            r = h_new / h
            add[0] = (w - h / h_w) / 2
        K = r * K
        K[2, 2] = 1
        K[0:2, 2] -= add * r
        return K
    if mode == "axes":
        return np.dot(np.diag([1.0 / (float(w0) / w_t), 1.0 / (float(h0) / h_t), 1.0]), K)
    raise ValueError("prepare_intrinsics: mode must be \"ratio\" or \"axes\", got %r" % (mode,))


def prepare_norm(K_left, K_right):
    """K'_l, K'_r [pairs,3,3] float64 -> norm [pairs,8] float32 (cy_l, cx_l, 1 / fy_l, 1 / fx_l, cy_r, cx_r, 1 / fy_r, 1 / fx_r), each
    formed in float64 and rounded once: the `norm` of the per-pair stages (a host array)."""
    cols = []
    for K in (np.asarray(K_left, np.float64), np.asarray(K_right, np.float64)):
        cols += [K[:, 1, 2], K[:, 0, 2], 1.0 / K[:, 1, 1], 1.0 / K[:, 0, 0]]
    return np.stack(cols, 1).astype(np.float32)


def prepare_thr(K_left, K_right, threshold):
    """thr [pairs] float32 = threshold / mean(K'_l[0,0], K'_r[1,1], K'_l[0,0], K'_r[1,1]) (metrics.py:36-37), a host array."""
    K_left, K_right = np.asarray(K_left, np.float64), np.asarray(K_right, np.float64)
    return np.array([threshold / np.mean([a[0, 0], b[1, 1], a[0, 0], b[1, 1]]) for a, b in zip(K_left, K_right)]).astype(np.float32)


class PrepareTable:
    """The per-image table of one prepare_images call (pats_prepare_image_t, 2 * pairs entries: pair p's left image at 2 p, its
    right at 2 p + 1): `host` the numpy records, `dev` the same bytes on the GPU; `srcs` keeps the images it points to alive."""


def prepare_table(srcs, plan, bgr=False):
    """The table of prepare_images for these source tensors: srcs = [(left, right)] raw uint8 [h0, w0, 3] GPU tensors in the plan's
    pair order, each its own tensor (no copy is made: the table holds their addresses).  Build it once and hand it to prepare_images
    (table=) to call that without an allocation or an upload - under graph capture, say."""
    fn = "prepare_images"
    if len(srcs) != len(plan.dst):
        raise RuntimeError("%s: %d source pairs for a plan of %d" % (fn, len(srcs), len(plan.dst)))
    host = np.zeros(2 * len(srcs), _PREPARE_IMAGE)
    dev = None
    for p, pr in enumerate(srcs):
        if len(pr) != 2:
            raise RuntimeError("%s: pair %d must be (left, right)" % (fn, p))
        for side, t in enumerate(pr):
            name = "pair %d %s" % (p, ("left", "right")[side])
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch.Tensor" % (fn, name))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:       # layout first: refused the same way without a GPU
                raise RuntimeError("%s: %s must be a uint8 [h, w, 3] image, got %s %s" % (fn, name, t.dtype, list(t.shape)))
            if not t.is_contiguous():
                raise RuntimeError("%s: %s must be contiguous" % (fn, name))
            if not t.is_cuda:
                raise RuntimeError("pats_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
            if (int(t.shape[0]), int(t.shape[1])) != (int(plan.h0[p, side]), int(plan.w0[p, side])):
                raise RuntimeError("%s: %s is %d x %d, the plan was made for %d x %d"
                                   % (fn, name, t.shape[0], t.shape[1], plan.h0[p, side], plan.w0[p, side]))
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError("%s: %s is on %s, the others on %s" % (fn, name, t.device, dev))
            e = host[2 * p + side]
            e["src"], e["dst"], e["side"], e["bgr"] = t.data_ptr(), plan.dst[p], side, 1 if bgr else 0
            for k in ("h0", "w0", "y0", "x0", "h_c", "w_c", "h_t", "w_t"):
                e[k] = getattr(plan, k)[p, side]
            e["H"], e["W"] = plan.canvas[p]
            e["scale_x"] = 1.0 / (float(e["w_t"]) / float(e["w_c"]))
            e["scale_y"] = 1.0 / (float(e["h_t"]) / float(e["h_c"]))
    tab = PrepareTable()
    tab.host, tab.srcs, tab.bgr = host, srcs, bool(bgr)
    tab.dev = torch.from_numpy(host.view(np.uint8)).to(dev)
    return tab


def prepare_images(srcs, plan, left, right, bgr=False, table=None):
    """The device half of the image front end, ONE launch (pats_prepare_images_u8; include/pats_amd.h, "Image front end", holds the
    definition): every raw image of srcs = [(left, right)] (uint8 [h0, w0, 3] GPU tensors of any size, each its own tensor) is
    cropped to the plan's window, resampled to its target with OpenCV's fixed-point bilinear arithmetic (the 2 x 2 mean at an exact
    halving) and written with its zero pad as the pair's canvas into the flat stores left / right at plan.dst - every element of
    every canvas, so the stores may be torch.empty.  left / right: contiguous GPU tensors of at least plan.elems elements, both
    uint8, float32, float16 or bfloat16.  bgr: output channel c reads source channel 2 - c.  table: a prepare_table(srcs, plan, bgr)
    made earlier - the call then allocates and uploads nothing.  Returns (left, right)."""
    fn = "prepare_images"
    if table is None:
        table = prepare_table(srcs, plan, bgr)
    elif len(table.host) != 2 * len(plan.dst) or table.bgr != bool(bgr):
        raise RuntimeError("%s: the table was made for another plan or bgr setting" % fn)
    for t, name in ((left, "left"), (right, "right")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor" % (fn, name))
        if not t.is_cuda:
            raise RuntimeError("pats_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
        if t.dtype not in _IMG_DTYPES or t.dtype != left.dtype:
            raise RuntimeError("%s: left and right must share one of float32, float16, bfloat16, uint8, got %s" % (fn, t.dtype))
        if not t.is_contiguous() or t.numel() < plan.elems:
            raise RuntimeError("%s: %s must be contiguous and hold at least %d elements" % (fn, name, plan.elems))
    _check(_L().pats_prepare_images_u8(ctypes.c_void_p(table.host.ctypes.data), _ptr(table.dev), len(table.host), _ptr(left), left.numel(),
                                       _ptr(right), right.numel(), _IMG_DTYPES[left.dtype], _stream()), fn)
    return left, right


# ---- the absolute-pose branch (csrc/absolute.hip; include/pats_amd.h, "Per-pair absolute pose from depth") ----------------------
_INTERP = {"nearest": 0, "bilinear": 1, 0: 0, 1: 1}


class DepthTable:
    """The per-pair table of one lift_by_pair call: `host` the numpy [pairs,4] int64 rows (address, h, w, row stride in elements),
    `dev` the same on the GPU; `maps` keeps the depth maps it points to alive."""


def lift_table(depths, device=None):
    """The table of lift_by_pair for these depth maps: one float32 GPU tensor [h, w] per pair, of any sizes, each its own tensor -
    a strided view is taken as it lies (its rows must be dense: stride(1) == 1) - or None for a pair without a map (every match of
    it is invalid, as for a map with h or w = 0).  No copy is made: the table holds the addresses.  Build it once and hand it to
    lift_by_pair (table=) to call that without an upload."""
    fn = "lift_by_pair"
    host = np.zeros((len(depths), 4), np.int64)
    dev = device
    for p, t in enumerate(depths):
        if t is None:
            continue
        name = "depths[%d]" % p
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor or None" % (fn, name))
        if t.dtype != torch.float32 or t.dim() != 2:                        # layout first: refused the same way without a GPU
            raise RuntimeError("%s: %s must be a float32 [h, w] map, got %s %s" % (fn, name, t.dtype, list(t.shape)))
        if not t.is_cuda:
            raise RuntimeError("pats_amd: %s is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % (name, t.device))
        if dev is None:
            dev = t.device
        elif t.device != torch.device(dev):
            raise RuntimeError("%s: %s is on %s, the others on %s" % (fn, name, t.device, dev))
        h, w = int(t.shape[0]), int(t.shape[1])
        if h < 1 or w < 1:
            continue                                                          # an empty map has no address
        if (w > 1 and t.stride(1) != 1) or (h > 1 and t.stride(0) < w):
            raise RuntimeError("%s: %s must have dense rows that do not overlap (strides %s)" % (fn, name, list(t.stride())))
        host[p] = (t.data_ptr(), h, w, t.stride(0) if h > 1 else w)
    if dev is None:
        raise RuntimeError("%s: no depth map to take the device from; pass device=" % fn)
    tab = DepthTable()
    tab.host, tab.maps = host, list(depths)
    tab.dev = torch.from_numpy(host).to(dev)
    return tab


def lift_by_pair(matches, depths, pair_off=None, stride=None, counts=None, norm=None, max_depth=None, interp="nearest", max_jump=None,
                 out=None, pairs=None, table=None):
    """One side's matches lifted through that image's depth map to metric 3-D points, ON THE DEVICE, one launch, no host read
    (pats_lift_by_pair_f32; include/pats_amd.h holds the definition).  matches [cap,2] float32 (also [pairs,K,2]) in the hand-over's
    (c0, c1) = (y, x) order, un-normalised pixels; the segments as every per-pair stage takes them (pair_off, or stride + counts);
    depths: the per-pair maps as lift_table takes them - or None with table= a lift_table(...) made earlier (or its [pairs,4] int64
    GPU tensor, rows in the order of the segments).  norm [pairs,8]: its left half normalises the point.  interp "nearest" or
    "bilinear" (0 / 1); max_depth [pairs] float32 and max_jump (a float, bilinear only: (max tap - min tap) > max_jump * min tap marks
    a depth edge) invalidate matches.
    Returns (points [cap,3] float32 = (x0 d, x1 d, d), NaN for an invalid match and 0 outside the segments; valid [cap] uint8;
    lift_count [pairs] int64).  out: the three destinations."""
    fn = "lift_by_pair"
    _bp_layout(fn, [(matches, "matches"), (pair_off, "pair_off"), (counts, "counts"), (norm, "norm"), (max_depth, "max_depth")],
               {"pair_off": torch.int64, "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if interp not in _INTERP or isinstance(interp, bool):
        raise RuntimeError("%s: interp must be \"nearest\" (0) or \"bilinear\" (1), got %r" % (fn, interp))
    ml = _bp_flat(_dev(matches, "matches"), 2)
    if ml is None:
        raise RuntimeError("%s: matches must be [cap,2]" % fn)
    cap = int(ml.shape[0])
    seg, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    dev = ml.device
    if table is None:
        if depths is None or len(depths) != pairs:
            raise RuntimeError("%s: depths must hold one map (or None) per pair (%d), got %s" % (fn, pairs, "None" if depths is None else len(depths)))
        table = lift_table(depths, device=dev)
    tab = table.dev if isinstance(table, DepthTable) else table
    tab = _dev(tab, "table", torch.int64)
    if tuple(tab.shape) != (pairs, 4):
        raise RuntimeError("%s: the depth table must be [pairs,4] int64 (%d pairs), got %s" % (fn, pairs, list(tab.shape)))
    norm = _bp_norm(fn, norm, pairs)
    if max_depth is not None:
        max_depth = _dev(max_depth, "max_depth").reshape(-1)
        if max_depth.numel() != pairs:
            raise RuntimeError("%s: max_depth must hold one float32 per pair (%d), got %d" % (fn, pairs, max_depth.numel()))
    want = [("points", torch.float32, (cap, 3)), ("valid", torch.uint8, (cap,)), ("lift_count", torch.int64, (pairs,))]
    out = _bp_outputs(fn, want, out, dev)
    points, valid = out[0], out[1]
    if cap == 0:
        ml = points = _bp_placeholder(dev)
        valid = _bp_placeholder(dev, torch.uint8)
    _check(_L().pats_lift_by_pair_f32(_ptr(ml), off_p, stride, counts_p, pairs, cap, _ptr(norm), _ptr(tab), _ptr(max_depth), _INTERP[interp],
                                      0 if max_jump is None else 1, 0.0 if max_jump is None else float(max_jump), _ptr(points),
                                      _ptr(valid), _ptr(out[2]), _stream()), fn)
    return out


def absolute_hypotheses_by_pair(points, matches_r, H, seed, pair_off=None, stride=None, counts=None, norm=None, progressive=False,
                                return_samples=False, return_counts=False, out=None, pairs=None):
    """H P3P samples per pair, each solved for the up to four absolute poses (R, t) with x_r ~ R X + t, ON THE DEVICE, one launch, no
    host read (pats_absolute_hypotheses_by_pair_f32; include/pats_amd.h holds the definition).  points [cap,3] float32 = lift_by_pair's,
    matches_r [cap,2] the right list (norm's right half normalises it), seed [pairs] int64, the segments and progressive as
    epipolar_hypotheses_by_pair takes them (the pool's minimum is 3).  A sample with an invalid (NaN) point gives no model.
    Returns models [pairs,H,4,3,4] float32 - row-major [R | t], the kept solutions first by ascending camera distance of the first
    sample point, zero models behind - then sample_idx [pairs,H,3] int32 with return_samples=True and n_models [pairs,H] int32 with
    return_counts=True.  out: the destinations, in that order."""
    fn = "absolute_hypotheses_by_pair"
    head, out, _ = _hypotheses_checked(fn, _ABS, 3, 4, points, matches_r, H, seed, pair_off, stride, counts, norm, progressive,
                                       return_samples, return_counts, out, pairs)
    _check(_L().pats_absolute_hypotheses_by_pair_f32(*head, _stream()), fn)
    return out if len(out) > 1 else out[0]


def absolute_score_by_pair(points, matches_r, models, thr, pair_off=None, stride=None, counts=None, conf=None, min_conf=None, norm=None,
                           out=None, pairs=None):
    """M candidate absolute poses per pair against every lifted match of the pair by REPROJECTION, ON THE DEVICE, no host read
    (pats_absolute_score_by_pair_f32; include/pats_amd.h holds the definition): with Y = R X + t a match is an inlier iff it takes
    part (X and x_r finite, conf >= min_conf), Y2 > 0 and (Y0 - r0 Y2)^2 + (Y1 - r1 Y2)^2 <= thr^2 Y2^2.  points [cap,3] float32,
    matches_r [cap,2], models [pairs,M,3,4] float32 (row-major [R | t]; M <= epipolar_max_h()), thr [pairs] float32 in normalised
    units; the segments, conf / min_conf and norm (its right half) as epipolar_score_by_pair takes them.
    Returns (counts [pairs,M] int32, best [pairs] int32 - the lowest index among the largest counts -, best_count [pairs] int64,
    inlier [cap] uint8 = the winner's mask).  Bit-reproducible.  out: the four destinations."""
    fn = "absolute_score_by_pair"
    head, out, _ = _score_checked(fn, _ABS, points, matches_r, models, thr, pair_off, stride, counts, conf, min_conf, norm, out, pairs)
    _check(_L().pats_absolute_score_by_pair_f32(*head, _stream()), fn)
    return out


def absolute_polish_by_pair(points, matches_r, models, thr, best=None, rounds=4, steps=3, pair_off=None, stride=None, counts=None, conf=None,
                            min_conf=None, norm=None, out=None, pairs=None):
    """Local optimisation of each pair's winning absolute pose, ON THE DEVICE, one launch, no host read
    (pats_absolute_polish_by_pair_f32; include/pats_amd.h, "Per-pair absolute local optimisation", holds the definition): starting from
    m_0 = models[p, best[p]], `rounds` times "refit the current model on its inliers - `steps` Gauss-Newton steps on the reprojection
    error in float64, R made orthonormal, the result cast to float32 -, verify the refit (absolute_score_by_pair with that one
    model)", and the round with the most inliers - among equals the smallest squared error, then the lowest round; round 0 is the
    input - is returned.  points / matches_r, the segment forms (pair_off, or stride + counts), conf / min_conf, norm and thr exactly
    as absolute_score_by_pair takes them; models [pairs,M,3,4] float32 and best [pairs] int32 are its input and output (best may be
    left out with M == 1); 1 <= rounds <= 16, 1 <= steps <= 8.
    Returns (model [pairs,3,4] float32, best_count [pairs] int64, inlier [cap] uint8, best_round [pairs] int32, counts
    [pairs, rounds + 1] int32 and cost [pairs, rounds + 1] float64: the support and the inliers' summed squared reprojection error of
    every round, a walk that stopped early on a repeated model padded with its last values).  Bit-reproducible.  out: the six
    destinations."""
    fn = "absolute_polish_by_pair"
    lists, seg, models, thr_norm, gate, walk, inl, out = _polish_checked(fn, _ABS, points, matches_r, models, thr, best, rounds, pair_off, stride,
                                                                         counts, conf, min_conf, norm, out, pairs, steps)
    _check(_L().pats_absolute_polish_by_pair_f32(*lists, *seg, *models, *thr_norm, *gate, *walk, _ptr(out[0]),
                                                 _ptr(out[1]), inl, _ptr(out[3]), _ptr(out[4]), _ptr(out[5]), _stream()), fn)
    return out


# ---- the match-level yardstick (csrc/match_error.hip; include/pats_amd.h, "Per-pair match error against ground truth") -----------
def match_error_by_pair(points, matches_r, T1, T0=None, thr=(1.0, 3.0, 5.0), norm=None, swapped=False, depths_r=None, table_r=None,
                        occl_rel=0.2, size_r=None, conf=None, min_conf=None, edges=None, mask=None, pair_off=None, stride=None, counts=None,
                        out=None, pairs=None):
    """Each pair's matches scored against depth-and-pose ground truth, ON THE DEVICE, one launch, no host read
    (pats_match_error_by_pair_f64; include/pats_amd.h holds the definition): the lifted left point is carried through the ground-truth
    pose into the right image, and err is the distance of the matched right point from that projection, in pixels, float64.
    points [cap,3] float32 = lift_by_pair's, matches_r [cap,2] the right list in un-normalised pixels, the segments (pair_off, or
    stride + counts) as the lift took them; norm [pairs,8]: what the lift was given (its right half takes the projection back to
    pixels).  T1 / T0 [pairs,4,4] float64 as pose_error_by_pair takes them; swapped: they are in the reference's (x, y) frame.
    depths_r: the RIGHT images' depth maps as lift_table takes them - or table_r= a lift_table(...) made earlier (or its [pairs,4]
    int64 GPU tensor) -: a match must then be covisible, abs(depth - map) <= occl_rel * map at the nearest tap.  size_r [pairs,2]
    float32: (h, w) of the right image's content, a projection outside it is not scored.  conf [cap] with min_conf: the
    verification's gate.  thr: 1 .. 8 ascending pixel thresholds (host values).  edges: 1 .. 64 ascending confidence floors (host
    values; needs conf).  mask [cap] uint8: e.g. a verification's inlier mask.
    Returns (err [cap] float64 - NaN for a match that is not scored, 0 outside the segments -, status [cap] uint8 - 1 scored, 0 takes
    no part, 2 no depth, 3 behind the camera, 4 out of view, 5 no right depth, 6 not covisible -, tally [pairs,8] int64 the rows per
    status, correct [pairs,n_thr] int64 the scored matches within each threshold, err_sum [pairs] float64, sweep [pairs,B,1+n_thr]
    int64 - per confidence floor the scored matches at or above it and those of them within each threshold; None without edges -,
    confusion [pairs,4] int64 - (mask & good, mask & !good, !mask & good, !mask & !good) with good = err <= thr[0]; None without
    mask).  Bit-reproducible.  out: the destinations that are not None, in that order."""
    fn = "match_error_by_pair"
    f64 = torch.float64
    _bp_layout(fn, [(points, "points"), (matches_r, "matches_r"), (T1, "T1"), (T0, "T0"), (norm, "norm"), (size_r, "size_r"), (conf, "conf"),
                    (mask, "mask"), (pair_off, "pair_off"), (counts, "counts")],
               {"T1": f64, "T0": f64, "mask": torch.uint8, "pair_off": torch.int64, "counts": torch.int64})
    _bp_one_form(fn, pair_off, stride, counts)
    if min_conf is not None and conf is None:
        raise RuntimeError("%s: min_conf needs conf" % fn)
    if edges is not None and conf is None:
        raise RuntimeError("%s: edges need conf" % fn)
    if depths_r is not None and table_r is not None:
        raise RuntimeError("%s: give depths_r or table_r, not both" % fn)
    thr = [float(v) for v in thr]
    edges = None if edges is None else [float(v) for v in edges]
    n_thr, B = len(thr), 0 if edges is None else len(edges)
    if not 1 <= n_thr <= 8:
        raise RuntimeError("%s: thr must hold 1 .. 8 numbers, got %d" % (fn, n_thr))
    if edges is not None and not 1 <= B <= 64:
        raise RuntimeError("%s: edges must hold 1 .. 64 numbers, got %d" % (fn, B))
    X, mr, cap = _bp_matches(fn, points, matches_r, _ABS)
    _, pairs, stride, off_p, counts_p = _bp_segments(fn, pair_off, stride, counts, pairs, cap)
    dev = X.device
    T1 = _dev(T1, "T1", f64)
    if tuple(T1.shape) != (pairs, 4, 4):
        raise RuntimeError("%s: T1 must be [pairs,4,4]" % fn)
    if T0 is not None:
        T0 = _dev(T0, "T0", f64)
        if tuple(T0.shape) != (pairs, 4, 4):
            raise RuntimeError("%s: T0 must be [pairs,4,4]" % fn)
    conf, norm = _bp_conf_norm(fn, conf, cap, norm, pairs)
    if size_r is not None:
        size_r = _dev(size_r, "size_r")
        if tuple(size_r.shape) != (pairs, 2):
            raise RuntimeError("%s: size_r must be [pairs,2]" % fn)
    if mask is not None:
        mask = _dev(mask, "mask", torch.uint8).reshape(-1)
        if mask.numel() != cap:
            raise RuntimeError("%s: mask must be [cap]" % fn)
    tab = None
    if depths_r is not None:
        if len(depths_r) != pairs:
            raise RuntimeError("%s: depths_r must hold one map (or None) per pair (%d), got %d" % (fn, pairs, len(depths_r)))
        table_r = lift_table(depths_r, device=dev)
    if table_r is not None:
        tab = _dev(table_r.dev if isinstance(table_r, DepthTable) else table_r, "table_r", torch.int64)
        if tuple(tab.shape) != (pairs, 4) or not tab.is_contiguous():
            raise RuntimeError("%s: the right depth table must be a contiguous [pairs,4] int64 tensor (%d pairs), got %s" % (fn, pairs, list(tab.shape)))
    want = [("err", f64, (cap,)), ("status", torch.uint8, (cap,)), ("tally", torch.int64, (pairs, 8)), ("correct", torch.int64, (pairs, n_thr)),
            ("err_sum", f64, (pairs,))]
    if edges is not None:
        want.append(("sweep", torch.int64, (pairs, B, 1 + n_thr)))
    if mask is not None:
        want.append(("confusion", torch.int64, (pairs, 4)))
    out = _bp_outputs(fn, want, out, dev)
    sweep = out[5] if edges is not None else None
    confusion = out[-1] if mask is not None else None
    err, status = out[0], out[1]
    if cap == 0:
        X = mr = _bp_placeholder(dev)
        err = _bp_placeholder(dev, f64)
        status = _bp_placeholder(dev, torch.uint8)
        conf = None if conf is None else X
        mask = None if mask is None else status
    _check(_L().pats_match_error_by_pair_f64(_ptr(X), _ptr(mr), _ptr(conf), off_p, stride, counts_p, pairs, cap, _ptr(norm), _ptr(T1), _ptr(T0),
                                             1 if swapped else 0, _ptr(tab), float(occl_rel), _ptr(size_r), 0 if min_conf is None else 1,
                                             0.0 if min_conf is None else float(min_conf), (ctypes.c_double * n_thr)(*thr), n_thr,
                                             None if edges is None else (ctypes.c_float * B)(*edges), B, _ptr(mask), _ptr(err), _ptr(status),
                                             _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(sweep), _ptr(confusion), _stream()), fn)
    return tuple(out[:5]) + (sweep, confusion)
