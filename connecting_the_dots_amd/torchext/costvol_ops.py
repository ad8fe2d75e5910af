# Wraps include/ctd_hip.h: ctd_costvol_* and ctd_costvol_argmin_* (csrc/costvol_*.hip).
import torch

from .. import _lib
from ._common import _check, _cost_pair, _loss_type, _photo_fast, _ptr, _stream, _subpixel_mode, _workspace
from .subpixel import costvol_subpixel
from .validity import _validity_kwargs, costvol_validity


def costvol(im, pattern, n_disps, block_size, type='sad', eps=0.1, algo=None):
    """Additive: SAD / MSE / soft-census block cost volume between frames and the pattern shifted by d
    (SURVEY 8a/A6): cost[f,d] = photometric_loss(P_d, im[f]) with P_d[h,x] = P[h, clamp(x-d)].
    im [N,H,W] | [H,W] f32, pattern [H,W] | [N,H,W] -> [N,D,H,W] | [D,H,W]; argmin over d is the best match."""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    ty = _loss_type(type)
    a, stride, dev = _cost_pair(im, pattern, "costvol", batch=False)
    squeeze = im.dim() == 2
    N, H, W = a.shape
    D = int(n_disps)
    out = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    L = _lib.lib()
    if _photo_fast(a, block_size, algo):
        # SAD / MSE, block 9: the separable path stages padded operand planes in a workspace (0 bytes: other kernels)
        nws = L.ctd_costvol_workspace_bytes(N, H, W, D, int(block_size), ty, 1 if stride else 0)
        ws = _workspace(nws, dev) if nws else None
        st = L.ctd_costvol_fast_f32(_ptr(a), _ptr(pattern), stride, _ptr(out), N, H, W, D, int(block_size),
                                    ty, float(eps), _ptr(ws), nws, dev.index, _stream(dev))
    else:
        st = L.ctd_costvol_f32(_ptr(a), _ptr(pattern), stride, _ptr(out), N, H, W, D, int(block_size),
                               ty, float(eps), dev.index, _stream(dev))
    _lib.check(st, "costvol")
    return out[0] if squeeze else out


def costvol_argmin(im, pattern, n_disps, block_size, type='census_sad', eps=0.1, rerank_rel=1e-5, return_rescored=False,
                   subpixel=None, validity=None):
    """Additive: the disparity of least SAD / MSE / soft-census block cost without the cost volume.
    im [N,H,W] | [H,W] f32, pattern [H,W] | [N,H,W] (as `costvol`) -> (idx int64, best f32), each [N,H,W] | [H,W].
    idx equals torch.argmin(costvol(..., algo="exact"), 1) bit for bit (first index on ties): the fast volume kernel
    ranks its costs, and every pixel whose best two fast costs b1 <= b2 miss  b2 - b1 > rerank_rel * (b1 + b2) + 2e-6
    is re-scored in the reference order (include/ctd_hip.h, ctd_costvol_argmin_f32).  best is the reference-order cost
    of idx on re-scored pixels and the fast one (within 1e-5 |b| + 1e-6) elsewhere.
    rerank_rel: 1e-5 = the fast kernels' stated bound (the default); larger re-scores more; < 0 = plain argmin of the
    fast costs, nothing re-scored (indices may then differ from the exact volume's on near-ties).
    return_rescored: also return the sorted int64 flat indices (f*H*W + h*W + w) of the re-scored pixels.
    Block sizes the kernels do not cover (odd, > 9) fall back to costvol(algo="exact") + torch.argmin (all pixels then
    count as re-scored).
    subpixel: None (default) | "equiangular" | "parabola": also return (disp, refined) of
    `costvol_subpixel(im, pattern, idx, ...)` at the end of the tuple (no accuracy gain for the census types).
    validity: None (default) | dict(lr_tol=..., min_gap=...): also return (flags, idx_r, gap) of
    `costvol_validity(im, pattern, idx, ...)` at the end of the tuple (after the sub-pixel outputs)."""
    if validity is not None:
        kw = _validity_kwargs(validity, "costvol_argmin")
        out = costvol_argmin(im, pattern, n_disps, block_size, type, eps, rerank_rel, return_rescored, subpixel)
        return tuple(out) + costvol_validity(im, pattern, out[0], n_disps, block_size, type, eps, **kw)
    if subpixel is not None:
        _subpixel_mode(subpixel, "costvol_argmin")
        out = costvol_argmin(im, pattern, n_disps, block_size, type, eps, rerank_rel, return_rescored)
        return tuple(out) + costvol_subpixel(im, pattern, out[0], n_disps, block_size, type, eps, subpixel)
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    ty = _loss_type(type)
    rerank_rel = float(rerank_rel)
    if rerank_rel != rerank_rel:
        raise RuntimeError("costvol_argmin: rerank_rel is NaN")
    a, stride, dev = _cost_pair(im, pattern, "costvol_argmin", batch=False)
    squeeze = im.dim() == 2
    N, H, W = a.shape
    D, bs = int(n_disps), int(block_size)
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    L = _lib.lib()
    nws = L.ctd_costvol_argmin_workspace_bytes(N, H, W, D, bs, ty, 1 if stride else 0)
    ws = _workspace(nws, dev) if nws else None
    st = L.ctd_costvol_argmin_f32(_ptr(a), _ptr(pattern), stride, _ptr(idx), _ptr(best), N, H, W, D, bs, ty, float(eps),
                                  rerank_rel, _ptr(ws), nws, dev.index, _stream(dev))
    if st == 3:                                        # CTD_ERR_UNSUPPORTED: the reference-order volume, then its argmin
        vol = costvol(a, pattern, D, bs, type, eps, algo="exact")
        idx = vol.argmin(1)
        best = vol.gather(1, idx.unsqueeze(1)).squeeze(1)
        rescored = torch.arange(N * H * W, device=dev)
    else:
        _lib.check(st, "costvol_argmin")
        if return_rescored:
            if ws is None:
                rescored = torch.empty(0, dtype=torch.int64, device=dev)
            else:
                n = int(ws[:4].view(torch.int32)[0]) & 0xFFFFFFFF   # workspace layout: u32 count, the list from byte 256 (ctd_hip.h)
                rescored = (ws[256:256 + 4 * n].view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sort()[0]
    if squeeze:
        idx, best = idx[0], best[0]
    return (idx, best, rescored) if return_rescored else (idx, best)
