# Wraps include/ctd_hip_band.h and include/ctd_hip_band_validity.h (csrc/band_match.hip, csrc/band_validity.hip).
import torch

from .. import _lib
from ._common import _call, _check, _cost_pair, _loss_type, _ncc_pair, _ptr, _stream, _subpixel_mode
from .subpixel import _pattern_planes_check, _pattern_planes_workspace, costvol_subpixel, xcorrvol_subpixel
from .validity import _validity_outputs, _validity_params


# Band-limited matching: the best score within a per-pixel disparity range (additive; include/ctd_hip_band.h states
# the definition word for word)
_BAND_RULE = """
    The definition (include/ctd_hip_band.h), on the reference-order volume V (NCC: xcorrvol(algo="exact"), higher is
    better; costs: costvol(algo="exact"), lower is better): lo and hi are inclusive and clipped to [0, D-1],
    lo' = max(lo, 0), hi' = min(hi, D-1); idx is the first index of the best V[f,d,h,w] over d in [lo', hi'], -1 when
    lo' > hi'; best is V[f,idx,h,w] bit for bit, NaN where idx == -1.  No volume is read or written, any band width up
    to D is legal, and a band of [0, D-1] everywhere returns the indices of torch.argmax / argmin of V."""


def disparity_band(prior, radius, n_disps):
    """Additive: the search range [lo, hi] (int32, shaped as `prior`, inclusive) of the band matchers around a
    disparity prior -- a network's prediction, the previous frame's disparity, an upsampled coarse match.
    prior f32 (any device, CPU included: pure torch); radius a float or a tensor broadcastable to prior.
      lo = clamp(ceil(prior - radius), 0, D), hi = clamp(floor(prior + radius), -1, D - 1),
    each one float32 subtraction / addition before the rounding.  A non-finite prior or a radius that is negative or NaN
    gives lo = D, hi = -1: an empty band (idx -1, best NaN)."""
    if not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32:
        raise RuntimeError("disparity_band: prior must be a float32 tensor")
    D = int(n_disps)
    r = torch.as_tensor(radius, dtype=torch.float32, device=prior.device)
    r = r.expand(prior.shape) if r.dim() else r
    empty = ~torch.isfinite(prior) | ~(r >= 0)
    lo = torch.ceil(prior - r).clamp(0, D)
    hi = torch.floor(prior + r).clamp(-1, D - 1)
    lo = torch.where(empty, torch.full_like(lo, D), lo).to(torch.int32)
    hi = torch.where(empty, torch.full_like(hi, -1), hi).to(torch.int32)
    return lo.contiguous(), hi.contiguous()


def _band_range(lo, hi, shape, dev, who):
    for t, name in ((lo, "lo"), (hi, "hi")):
        _check(t, name, (torch.int32,))
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s: %s must be int32 shaped %s" % (who, name, tuple(shape)))
        if t.device != dev:
            raise RuntimeError("%s: %s is on another device" % (who, name))


def _ncc_band_inputs(in0, in1, lo, hi, who):
    """checks of the NCC band ops -> (a0 [N,1,H,W], output shape, in1 frame stride, device)"""
    _check(in0, "in0", (torch.float32,))
    _check(in1, "in1", (torch.float32,))
    a0, shape, stride1, dev = _ncc_pair(in0, in1, "%s expects in0 [N,1,H,W] or [1,H,W] and in1 [1,H,W] or [N,1,H,W]" % who,
                                        "%s: in1 does not match in0" % who)
    _band_range(lo, hi, shape, dev, who)
    return a0, shape, stride1, dev


def _cost_band_inputs(im, pattern, lo, hi, type, who):
    """checks of the cost band ops -> (a [N,H,W], type code, pattern frame stride, device)"""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    ty = _loss_type(type, who)
    a, stride, dev = _cost_pair(im, pattern, who)
    _band_range(lo, hi, im.shape, dev, who)
    return a, ty, stride, dev


def xcorrvol_argmax_band(in0, in1, lo, hi, n_disps, block_size, prepared=None, subpixel=None):
    """Additive: NCC matching within a per-pixel disparity range, without a volume (C == 1).
    in0 [N,1,H,W] | [1,H,W]; in1 [1,H,W] | [N,1,H,W] as `xcorrvol_argmax` takes them; lo, hi int32 [N,H,W] | [H,W]
    (see `disparity_band`).  Returns (idx int64, best f32), shaped as lo.
    `prepared`: a `prepare_pattern` handle of the same in1 and frame count keeps the pattern's window statistics -- the
    planes `xcorrvol_subpixel` and `xcorrvol_band_validity` keep there too, filled by whichever op runs first -- so
    later calls skip the pattern half.
    subpixel: None (default) | "parabola" | "equiangular": also return (disp f32, refined u8) of
    `xcorrvol_subpixel(in0, in1, idx, ...)` at the end of the tuple (the fit runs through the volume's scores at
    idx - 1 and idx + 1 whether or not they lie in the band; idx == -1 gives NaN / 0)."""
    who = "xcorrvol_argmax_band"
    if subpixel is not None:
        _subpixel_mode(subpixel, who)
        out = xcorrvol_argmax_band(in0, in1, lo, hi, n_disps, block_size, prepared)
        return tuple(out) + xcorrvol_subpixel(in0, in1, out[0], n_disps, block_size, subpixel, prepared)
    a0, shape, stride1, dev = _ncc_band_inputs(in0, in1, lo, hi, who)
    N, _, H, W = a0.shape
    D, bs = int(n_disps), int(block_size)
    idx = torch.empty(shape, dtype=torch.int64, device=dev)
    best = torch.empty(shape, dtype=torch.float32, device=dev)
    L = _lib.lib()
    nws = L.ctd_xcorrvol_argmax_band_workspace_bytes(N, H, W, D, bs, 1 if stride1 else 0)
    ws, flag = _pattern_planes_workspace(prepared, who, in1, N, H, W, D, bs, nws, dev)
    st = L.ctd_xcorrvol_argmax_band_f32(_ptr(a0), _ptr(in1), stride1, _ptr(lo), _ptr(hi), _ptr(idx), _ptr(best), N, H, W,
                                        D, bs, flag, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _pattern_planes_check(st, who, prepared, flag, H, W, D, bs)
    return idx, best


def costvol_argmin_band(im, pattern, lo, hi, n_disps, block_size, type='census_sad', eps=0.1, subpixel=None):
    """Additive: SAD / MSE / soft-census block matching within a per-pixel disparity range, without a volume.
    im [N,H,W] | [H,W] f32, pattern [H,W] | [N,H,W] as `costvol_argmin` takes them; lo, hi int32 shaped as im (see
    `disparity_band`).  Returns (idx int64, best f32), shaped as im.
    subpixel: None (default) | "equiangular" | "parabola": also return (disp, refined) of
    `costvol_subpixel(im, pattern, idx, ...)` at the end of the tuple."""
    who = "costvol_argmin_band"
    if subpixel is not None:
        _subpixel_mode(subpixel, who)
        out = costvol_argmin_band(im, pattern, lo, hi, n_disps, block_size, type, eps)
        return tuple(out) + costvol_subpixel(im, pattern, out[0], n_disps, block_size, type, eps, subpixel)
    a, ty, stride, dev = _cost_band_inputs(im, pattern, lo, hi, type, who)
    N, H, W = a.shape
    idx = torch.empty(im.shape, dtype=torch.int64, device=dev)
    best = torch.empty(im.shape, dtype=torch.float32, device=dev)
    _call(_lib.lib().ctd_costvol_argmin_band_f32, who, _ptr(a), _ptr(pattern), stride, _ptr(lo), _ptr(hi), _ptr(idx),
          _ptr(best), N, H, W, int(n_disps), int(block_size), ty, float(eps), dev.index, _stream(dev))
    return idx, best


xcorrvol_argmax_band.__doc__ += _BAND_RULE
costvol_argmin_band.__doc__ += _BAND_RULE


_BAND_VALIDITY_RULE = """
    The definition (include/ctd_hip_band_validity.h), on the reference-order volume V of the band functions: pixel
    (f,h,w) *holds* d when lo' <= d <= hi' (lo' = max(lo, 0), hi' = min(hi, D-1)).
      idx, best    exactly those of the band function (-1 / NaN on an empty band)
      idx_r[f,h,x] first index of the best V[f,d,h,x+d] over those d in [0, min(D, W-x)) that pixel x+d holds; -1 when no
                   pixel holds a disparity that lands on column x; ties go to the smaller d (-0.0 and +0.0 tie)
      gap[f,h,w]   s1 - s2 (NCC) | s2 - s1 (costs), s1 = V[idx], s2 = the best V[d] over held d with |d - idx| >= 2; +inf
                   when no such d is held, NaN when idx == -1.  A band of width <= 3 around idx always passes UNIQUE.
      flags bit 0 IN_PATTERN: idx >= 0 and w - idx >= 0;  bit 1 LR_OK: bit 0 and |idx_r[f,h,w-idx] - idx| <= lr_tol;
            bit 2 UNIQUE: idx >= 0 and gap > min_gap;  valid = (flags == 7).
    With lo = 0, hi = D-1 everywhere flags, idx_r and gap are those of `match_validity` on V with the returned idx.
    Every output is exact (the reference's bits) and the same on every run; no volume is read or written.  Unlike
    `xcorrvol_validity` / `costvol_validity` on a band function's idx, the pattern side sees only what the bands hold."""


def xcorrvol_band_validity(in0, in1, lo, hi, n_disps, block_size, lr_tol=1, min_gap=0.0, prepared=None, subpixel=None):
    """Additive: `xcorrvol_argmax_band` with the validity of its matches within the band -> (idx int64, best f32,
    flags u8, idx_r int64, gap f32), each shaped as lo.  Inputs, `prepared` (the handle's planes now serve three ops:
    `xcorrvol_subpixel`, `xcorrvol_argmax_band` and this one) and `subpixel` (appends (disp, refined)) as there.
    Use: disparity_filter(idx.float(), flags == 7)."""
    who = "xcorrvol_band_validity"
    if subpixel is not None:
        _subpixel_mode(subpixel, who)
        out = xcorrvol_band_validity(in0, in1, lo, hi, n_disps, block_size, lr_tol, min_gap, prepared)
        return tuple(out) + xcorrvol_subpixel(in0, in1, out[0], n_disps, block_size, subpixel, prepared)
    lr_tol, min_gap = _validity_params(lr_tol, min_gap, who)
    a0, shape, stride1, dev = _ncc_band_inputs(in0, in1, lo, hi, who)
    N, _, H, W = a0.shape
    D, bs = int(n_disps), int(block_size)
    idx = torch.empty(shape, dtype=torch.int64, device=dev)
    best = torch.empty(shape, dtype=torch.float32, device=dev)
    flags, idx_r, gap = _validity_outputs(idx)
    L = _lib.lib()
    nws = L.ctd_xcorrvol_argmax_band_workspace_bytes(N, H, W, D, bs, 1 if stride1 else 0)
    ws, flag = _pattern_planes_workspace(prepared, who, in1, N, H, W, D, bs, nws, dev)
    st = L.ctd_xcorrvol_band_validity_f32(_ptr(a0), _ptr(in1), stride1, _ptr(lo), _ptr(hi), _ptr(idx), _ptr(best),
                                          _ptr(flags), _ptr(idx_r), _ptr(gap), N, H, W, D, bs, lr_tol, min_gap, flag,
                                          _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _pattern_planes_check(st, who, prepared, flag, H, W, D, bs)
    return idx, best, flags, idx_r, gap


def costvol_band_validity(im, pattern, lo, hi, n_disps, block_size, type='census_sad', eps=0.1, lr_tol=1, min_gap=0.0,
                          subpixel=None):
    """Additive: `costvol_argmin_band` with the validity of its matches within the band -> (idx int64, best f32,
    flags u8, idx_r int64, gap f32), each shaped as im.  Inputs and `subpixel` (appends (disp, refined)) as there."""
    who = "costvol_band_validity"
    if subpixel is not None:
        _subpixel_mode(subpixel, who)
        out = costvol_band_validity(im, pattern, lo, hi, n_disps, block_size, type, eps, lr_tol, min_gap)
        return tuple(out) + costvol_subpixel(im, pattern, out[0], n_disps, block_size, type, eps, subpixel)
    lr_tol, min_gap = _validity_params(lr_tol, min_gap, who)
    a, ty, stride, dev = _cost_band_inputs(im, pattern, lo, hi, type, who)
    N, H, W = a.shape
    idx = torch.empty(im.shape, dtype=torch.int64, device=dev)
    best = torch.empty(im.shape, dtype=torch.float32, device=dev)
    flags, idx_r, gap = _validity_outputs(idx)
    _call(_lib.lib().ctd_costvol_band_validity_f32, who, _ptr(a), _ptr(pattern), stride, _ptr(lo), _ptr(hi), _ptr(idx),
          _ptr(best), _ptr(flags), _ptr(idx_r), _ptr(gap), N, H, W, int(n_disps), int(block_size), ty, float(eps),
          lr_tol, min_gap, dev.index, _stream(dev))
    return idx, best, flags, idx_r, gap


xcorrvol_band_validity.__doc__ += _BAND_VALIDITY_RULE
costvol_band_validity.__doc__ += _BAND_VALIDITY_RULE
