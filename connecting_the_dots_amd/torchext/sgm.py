# Wraps include/ctd_hip.h: ctd_sgm_* (csrc/sgm.hip).
import torch

from .. import _lib
from ._common import _call, _check, _ptr, _same_device, _stream, _workspace
from .costvol_ops import costvol
from .ncc import xcorrvol_batch


# Semi-global cost aggregation (additive; include/ctd_hip.h states the rule word for word)
_SGM_RULE = """
    The rule (include/ctd_hip.h), f32 add / sub / min only.  C = vol (maximise=False: costs) or -vol (maximise=True:
    scores).  Along a direction (dy, dx) with q = (y - dy, x - dx):
      q outside the image:  L(p,d) = C(p,d)
      otherwise:            m = min_k L(q,k);  t = min(L(q,d), m + p2, L(q,d-1) + p1, L(q,d+1) + p1);
                            L(p,d) = C(p,d) + (t - m)
    S = the sum of L over right, left, down, up (paths=4) or right, left, down, down-right, down-left, up, up-right,
    up-left (paths=8), added in that order; idx = argmin_d S (first index), best = S[idx].  S and best are in cost sign
    (lower is better) also with maximise=True.  0 <= p1 <= p2, both finite; D <= 256."""


def sgm_aggregate(vol, p1, p2, paths=8, maximise=False, return_volume=False):
    """Additive: semi-global path aggregation of a materialised volume -> (idx int64, best f32[, S f32]).
    vol [N,D,H,W] | [D,H,W] f32 (never written); idx and best [N,H,W] | [H,W]; S shaped as vol.  `S` composes with
    `match_validity(S, idx, maximise=False)`."""
    _check(vol, "vol", (torch.float32,))
    p1, p2 = float(p1), float(p2)
    if not (0.0 <= p1 <= p2 < float("inf")):
        raise RuntimeError("sgm_aggregate: need 0 <= p1 <= p2, both finite")
    if paths not in (4, 8):
        raise RuntimeError("sgm_aggregate: paths must be 4 or 8")
    squeeze = vol.dim() == 3
    v = vol.unsqueeze(0) if squeeze else vol
    if v.dim() != 4 or v.numel() == 0:
        raise RuntimeError("sgm_aggregate expects a non-empty vol [N,D,H,W] or [D,H,W]")
    dev = _same_device(v)
    N, D, H, W = v.shape
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    L = _lib.lib()
    S = torch.empty_like(v) if return_volume else None
    ws = None if return_volume else _workspace(L.ctd_sgm_workspace_bytes(N, D, H, W, paths, 0), dev)
    _call(L.ctd_sgm_aggregate_f32, "sgm_aggregate", _ptr(v), 1 if maximise else 0, p1, p2, paths, _ptr(S), _ptr(idx),
          _ptr(best), N, D, H, W, _ptr(ws), ws.numel() if ws is not None else 0, dev.index, _stream(dev))
    out = (idx, best) + ((S,) if return_volume else ())
    return tuple(t[0] for t in out) if squeeze else out


def costvol_sgm(im, pattern, n_disps, block_size, type, eps, p1, p2, paths=8, algo=None):
    """Additive: `costvol(im, pattern, n_disps, block_size, type, eps, algo)` aggregated by `sgm_aggregate` ->
    (idx int64, best f32), each shaped as im."""
    return sgm_aggregate(costvol(im, pattern, n_disps, block_size, type, eps, algo), p1, p2, paths, False)


def xcorrvol_sgm(in0, in1, n_disps, block_size, p1, p2, paths=8, algo=None):
    """Additive: the NCC volume of `xcorrvol_batch(in0, in1, n_disps, block_size, algo)` aggregated by `sgm_aggregate`
    with maximise=True -> (idx int64, best f32), [N,H,W] for in0 [N,C,H,W] and [H,W] for in0 [C,H,W]; best is in cost
    sign (the aggregated -NCC)."""
    _check(in0, "in0", (torch.float32,))
    squeeze = in0.dim() == 3
    vol = xcorrvol_batch(in0.unsqueeze(0) if squeeze else in0, in1, n_disps, block_size, algo)
    out = sgm_aggregate(vol, p1, p2, paths, True)
    return tuple(t[0] for t in out) if squeeze else out


sgm_aggregate.__doc__ += _SGM_RULE
