# Wraps include/ctd_hip.h: ctd_photometric_* and ctd_pattern_loss_* (csrc/photometric*.hip, csrc/pattern_loss.hip).
import torch

from .. import _lib
from ._common import _PHOTO_TYPES, _call, _check, _loss_type, _photo_fast, _ptr, _same_device, _stream, _workspace


# Photometric block loss (reference: PhotometricLossFunction, functions.py:79-118)
def _photo_args(es, ta):
    _check(es, "es")
    _check(ta, "ta")
    if es.dim() != 4 or es.shape != ta.shape or es.dtype != ta.dtype:
        raise RuntimeError("photometric_loss expects es and ta of the same [B,C,H,W] shape and dtype")
    return _same_device(es, ta)


class PhotometricLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, es, ta, block_size, type, eps, algo=None):
        dev = _photo_args(es, ta)
        ctx.save_for_backward(es, ta)
        ctx.block_size = block_size
        ctx.type = type
        ctx.eps = eps
        ctx.fast = _photo_fast(es, block_size, algo)
        B, C, H, W = es.shape
        out = torch.empty((B, 1, H, W), dtype=es.dtype, device=dev)
        L = _lib.lib()
        fn = L.ctd_photometric_fwd_f32 if es.dtype == torch.float32 else L.ctd_photometric_fwd_f64
        if ctx.fast:
            fn = L.ctd_photometric_fwd_fast_f32
        _call(fn, "photometric_loss_forward", _ptr(es), _ptr(ta), _ptr(out), B, C, H, W, int(block_size), int(type),
              float(eps), dev.index, _stream(dev))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        es, ta = ctx.saved_tensors
        grad_out = grad_out.contiguous()                      # functions.py:99
        _check(grad_out, "grad_out")
        dev = es.device
        B, C, H, W = es.shape
        # the gather backward writes every element: no zero-fill needed (the reference scatters into at::zeros)
        grad_es = torch.empty_like(es)
        L = _lib.lib()
        fn = L.ctd_photometric_bwd_f32 if es.dtype == torch.float32 else L.ctd_photometric_bwd_f64
        if ctx.fast:
            fn = L.ctd_photometric_bwd_fast_f32
        _call(fn, "photometric_loss_backward", _ptr(es), _ptr(ta), _ptr(grad_out), _ptr(grad_es), B, C, H, W,
              int(ctx.block_size), int(ctx.type), float(ctx.eps), dev.index, _stream(dev))
        return grad_es, None, None, None, None, None


def photometric_loss(es, ta, block_size, type='mse', eps=0.1, algo=None):
    """[B,C,H,W] x2 -> [B,1,H,W]: mean over a block_size^2 replicate-clamped block, summed over channels, of
    (es-ta)^2 | |es-ta| | soft-census squared / absolute difference.  Gradient flows to `es` only.
    algo (additive): 'fast' (default, or env CTD_PHOTO_ALGO) = tolerance-level kernels, ~10x faster for the census
    types; 'exact' = reference operation order, bit-identical to the reference CPU build."""
    return PhotometricLossFunction.apply(es, ta, block_size, _loss_type(type), eps, algo)


class PatternLossFunction(torch.autograd.Function):
    """Additive: the whole of RectifiedPatternSimilarityLoss.tforward (networks.py:358-378) as one
    forward and one backward kernel -- warp, block loss (block 9), masked mean.  Tolerance level (fast kernels).
    Returns (val, pattern_proj, terms) with terms = [sum(mask*diff), sum(mask), val] for cross-rank reduction."""

    @staticmethod
    def forward(ctx, disp, im, mask, pattern, type, eps):
        for t, name in ((disp, "disp"), (im, "im"), (pattern, "pattern")) + (((mask, "mask"),) if mask is not None else ()):
            _check(t, name, (torch.float32,))
        dev = _same_device(disp, im, pattern, *(() if mask is None else (mask,)))
        if disp.dim() != 4 or disp.shape[1] != 1 or im.shape != disp.shape or (mask is not None and mask.shape != disp.shape):
            raise RuntimeError("pattern_loss expects disp, im (and mask) of the same [B,1,H,W] shape")
        B, _, H, W = disp.shape
        if pattern.numel() != H * W:
            raise RuntimeError("pattern_loss expects a single-channel pattern with H*W elements")
        L = _lib.lib()
        proj = torch.empty_like(disp)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        ws = _workspace(L.ctd_pattern_loss_workspace_bytes(B, H, W), dev)
        _call(L.ctd_pattern_loss_fwd_f32, "pattern_loss_forward", _ptr(disp), _ptr(im), _ptr(mask), _ptr(pattern),
              _ptr(proj), _ptr(terms), B, H, W, int(type), float(eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
        ctx.save_for_backward(disp, im, pattern, terms, *(() if mask is None else (mask,)))
        ctx.has_mask = mask is not None
        ctx.type, ctx.eps = int(type), float(eps)
        return terms[2].clone(), proj, terms

    @staticmethod
    def backward(ctx, grad_val, grad_proj, grad_terms):
        saved = ctx.saved_tensors
        disp, im, pattern, terms = saved[:4]
        mask = saved[4] if ctx.has_mask else None
        dev = disp.device
        B, _, H, W = disp.shape
        # the kernel applies go[p] = gv * mask[p] / den; gradients arriving at the numerator (cross-rank ratio of
        # sums, sharding.reduce_ratio) or at terms[2] fold into the same scalar.  den does not depend on disp.
        gv = torch.zeros(1, dtype=torch.float32, device=dev)
        if grad_val is not None:
            gv = gv + grad_val.reshape(1)
        if grad_terms is not None:
            gv = gv + grad_terms[2:3] + grad_terms[0:1] * terms[1:2]
        gp = grad_proj.contiguous() if grad_proj is not None else None
        grad_disp = torch.empty_like(disp)
        _call(_lib.lib().ctd_pattern_loss_bwd_f32, "pattern_loss_backward", _ptr(disp), _ptr(im), _ptr(mask),
              _ptr(pattern), _ptr(terms), _ptr(gv), _ptr(gp), _ptr(grad_disp), B, H, W, ctx.type, ctx.eps, dev.index,
              _stream(dev))
        return grad_disp, None, None, None, None, None


def pattern_loss(disp, im, mask, pattern, type='census_sad', eps=0.5):
    """Fused pattern similarity loss: (val, pattern_proj, terms); gradient flows to `disp` only."""
    return PatternLossFunction.apply(disp, im, mask, pattern, _loss_type(type), eps)


class PatternLossMultiFunction(torch.autograd.Function):
    """Additive: the pattern similarity loss of all pyramid levels in one forward and one backward
    launch.  apply(type, eps, n, disp_0..disp_{n-1}, im_0.., mask_0.. (None allowed), pattern_0..) ->
    (vals [n], terms [n,3], proj_0..proj_{n-1})."""

    @staticmethod
    def _levels(n, disps, ims, masks, patterns, projs=None, grad_projs=None, grad_disps=None):
        arr = (_lib.PatternLevel * n)()
        for l in range(n):
            B, _, H, W = disps[l].shape
            arr[l] = _lib.PatternLevel(_ptr(disps[l]), _ptr(ims[l]), _ptr(masks[l]), _ptr(patterns[l]),
                                       _ptr(projs[l]) if projs else None, _ptr(grad_projs[l]) if grad_projs else None,
                                       _ptr(grad_disps[l]) if grad_disps else None, B, H, W)
        return arr

    @staticmethod
    def forward(ctx, type, eps, n, *tensors):
        disps, ims, masks, patterns = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n], tensors[3 * n:4 * n]
        for l in range(n):
            for t, name in ((disps[l], "disp"), (ims[l], "im"), (patterns[l], "pattern")) + (
                    ((masks[l], "mask"),) if masks[l] is not None else ()):
                _check(t, "%s[%d]" % (name, l), (torch.float32,))
            if disps[l].dim() != 4 or disps[l].shape[1] != 1 or ims[l].shape != disps[l].shape or (
                    masks[l] is not None and masks[l].shape != disps[l].shape):
                raise RuntimeError("pattern_loss_multi: level %d expects disp, im (and mask) of one [B,1,H,W] shape" % l)
            if patterns[l].numel() != disps[l].shape[2] * disps[l].shape[3]:
                raise RuntimeError("pattern_loss_multi: level %d pattern must have H*W elements" % l)
        dev = _same_device(*disps, *ims, *patterns, *[m for m in masks if m is not None])
        L = _lib.lib()
        projs = [torch.empty_like(d) for d in disps]
        terms = torch.empty((n, 3), dtype=torch.float32, device=dev)
        levels = PatternLossMultiFunction._levels(n, disps, ims, masks, patterns, projs)
        ws = _workspace(L.ctd_pattern_loss_multi_workspace_bytes(n, levels), dev)
        _call(L.ctd_pattern_loss_multi_fwd_f32, "pattern_loss_multi_forward", n, levels, _ptr(terms), int(type),
              float(eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
        ctx.save_for_backward(terms, *disps, *ims, *patterns, *[m for m in masks if m is not None])
        ctx.n, ctx.type, ctx.eps = n, int(type), float(eps)
        ctx.has_mask = [m is not None for m in masks]
        return (terms[:, 2].clone(), terms) + tuple(projs)

    @staticmethod
    def backward(ctx, grad_vals, grad_terms, *grad_projs):
        n = ctx.n
        saved = ctx.saved_tensors
        terms = saved[0]
        disps, ims, patterns = saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:1 + 3 * n]
        rest = list(saved[1 + 3 * n:])
        masks = [rest.pop(0) if h else None for h in ctx.has_mask]
        dev = terms.device
        # gradients arriving at the numerators / ratios fold into one scalar per level (see PatternLossFunction)
        gv = torch.zeros(n, dtype=torch.float32, device=dev)
        if grad_vals is not None:
            gv = gv + grad_vals
        if grad_terms is not None:
            gv = gv + grad_terms[:, 2] + grad_terms[:, 0] * terms[:, 1]
        gv = gv.contiguous()
        gps = [g.contiguous() if g is not None else None for g in grad_projs]
        grad_disps = [torch.empty_like(d) for d in disps]
        levels = PatternLossMultiFunction._levels(n, disps, ims, masks, patterns, None, gps, grad_disps)
        _call(_lib.lib().ctd_pattern_loss_multi_bwd_f32, "pattern_loss_multi_backward", n, levels, _ptr(terms),
              _ptr(gv), ctx.type, ctx.eps, dev.index, _stream(dev))
        return (None, None, None) + tuple(grad_disps) + (None,) * (3 * n)


def pattern_loss_multi(disps, ims, masks, patterns, type='census_sad', eps=0.5):
    """Fused pattern similarity loss of several pyramid levels (lists of per-level tensors; masks may hold None)
    in one launch each way: (vals [n], terms [n,3], [pattern_proj per level])."""
    ty = _loss_type(type)
    n = len(disps)
    if not (len(ims) == len(masks) == len(patterns) == n) or n < 1 or n > 8:
        raise RuntimeError("pattern_loss_multi expects 1..8 levels with one disp, im, mask and pattern each")
    out = PatternLossMultiFunction.apply(ty, eps, n, *[d.contiguous() for d in disps],
                                         *[i.contiguous() for i in ims],
                                         *[None if m is None else m.contiguous() for m in masks], *patterns)
    return out[0], out[1], list(out[2:])


def photometric_loss_pytorch(es, ta, block_size, type='mse', eps=0.1):
    """Stock-PyTorch formulation of the same loss (replicate pad + unfold), kept as the independent
    second opinion the reference ships next to its kernels (functions.py:120-147)."""
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')
    p = block_size // 2
    B, C, H, W = es.shape

    def windows(x):
        xp = torch.nn.functional.pad(x, (p, p, p, p), mode='replicate')
        return torch.nn.functional.unfold(xp, kernel_size=block_size).view(B, C, -1, H, W)

    ew, tw = windows(es), windows(ta)
    if type in ('mse', 'sad'):
        diff = ew - tw
    else:
        def soft(d):
            return 0.5 * (1 + d / torch.sqrt(d * d + eps))
        diff = soft(ew - es.unsqueeze(2)) - soft(tw - ta.unsqueeze(2))
    term = diff * diff if type.endswith('mse') else diff.abs()
    return term.reshape(B, -1, H, W).sum(dim=1, keepdim=True) / block_size ** 2
