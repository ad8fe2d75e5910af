"""Band-limited semi-global matching (include/ext/ctd_hip_band_sgm.h, csrc/band_sgm.hip): the band matchers' scores
as a band volume of `slots` planes, and semi-global aggregation within every pixel's own disparity range.

    lo, hi = torchext.disparity_band(prior, 2, D)
    idx, best = bandsgm.costvol_band_sgm(im, pattern, lo, hi, D, 9, 'sad', 0.1, p1, p2)      # one call
    vol_b = bandsgm.costvol_band_volume(im, pattern, lo, hi, D, 9, 'sad', 0.1)               # or in two steps
    idx, best, S_b = bandsgm.band_sgm_aggregate(vol_b, lo, hi, D, p1, p2, return_volume=True)
    S = bandsgm.band_volume_expand(S_b, lo, hi, D, float('inf'))                             # for match_validity

The header's prototypes are bound here, onto the library handle of `_lib.lib()` at first use; this table is not one of
`_lib.TABLES`.  No fallback to torch: a missing kernel is an error.
"""
import ctypes

import torch

from . import _lib
from .torchext._common import _call, _check, _ptr, _same_device, _stream, _workspace
from .torchext.band import _cost_band_inputs, _ncc_band_inputs
from .torchext.subpixel import _pattern_planes_check, _pattern_planes_workspace

_c_int, _c_long, _c_float, _c_size_t, _vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

HEADER = "ext/ctd_hip_band_sgm.h"

# mirrors include/ext/ctd_hip_band_sgm.h one to one, in the header's order (tests/test_band_sgm_host.py)
TABLE = {
    "ctd_xcorrvol_band_volume_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 7 + [_vp, _c_size_t, _c_int,
                                                                                             _vp]),
    "ctd_costvol_band_volume_f32": (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp] + [_c_int] * 7 + [_c_float, _c_int, _vp]),
    "ctd_band_sgm_workspace_bytes": (_c_size_t, [_c_int] * 7),
    "ctd_band_sgm_aggregate_f32": (_c_int, [_vp, _vp, _vp, _c_int, _c_float, _c_float, _c_int, _vp, _vp, _vp] +
                                   [_c_int] * 5 + [_vp, _c_size_t, _c_int, _vp]),
}

MAX_SLOTS = 64

_bound = None


def lib():
    """the handle of `_lib.lib()` with this module's prototypes bound"""
    global _bound
    if _bound is None:
        l = _lib.lib()
        for name, (res, args) in TABLE.items():
            fn = getattr(l, name)           # AttributeError here means header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _bound = l
    return _bound


_BAND_SGM_RULE = """
    The rule (include/ext/ctd_hip_band_sgm.h).  lo' = max(lo, 0), hi'' = min(hi, D-1, lo' + slots - 1); pixel p *holds* d
    when lo' <= d <= hi'', in slot k = d - lo'; n(p) is the number it holds.  A band wider than `slots` is truncated to
    its first `slots` disparities.  A band volume Vb [N,slots,H,W] is the reference-order volume V[f,lo'+k,h,w] bit for
    bit in the held slots and NaN elsewhere.  Aggregation: C = Vb (costs) or -Vb (maximise=True); along a direction with
    predecessor q,
      q outside the image or n(q) = 0:  L(p,d) = C(p,d)
      otherwise:  m = min L(q,k) over what q holds;
                  t = min(L(q,d), m + p2, L(q,d-1) + p1, L(q,d+1) + p1), each L(q,.) term only where q holds it;
                  L(p,d) = C(p,d) + (t - m)
    summed over the directions in the order of `torchext.sgm_aggregate`; idx = lo' + the first argmin slot of S, best = S
    there (cost sign); an empty band gives idx -1, best NaN; unheld slots of S_b are NaN.  Where no band is empty this is
    `sgm_aggregate` on the full volume with +inf outside each band.  1 <= slots <= 64; 0 <= p1 <= p2, both finite."""


def band_width(lo, hi, n_disps):
    """The widest clipped band, max over pixels of min(hi, D-1) - max(lo, 0) + 1 (0 when every band is empty), as an
    int: one device-to-host sync.  It is what `slots=None` stands for."""
    for t, name in ((lo, "lo"), (hi, "hi")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise RuntimeError("band_width: %s must be an int32 tensor" % name)
    if lo.shape != hi.shape or lo.numel() == 0:
        return 0
    D = int(n_disps)
    w = hi.clamp(-1, D - 1).to(torch.int64) - lo.clamp(0, D).to(torch.int64) + 1
    return max(int(w.max()), 0)


def _slots(slots, lo, hi, n_disps, who):
    s = max(band_width(lo, hi, n_disps), 1) if slots is None else slots
    if isinstance(s, bool) or not isinstance(s, int) or s < 1:
        raise RuntimeError("%s: slots must be an integer >= 1" % who)
    if s > MAX_SLOTS:
        raise RuntimeError("%s: slots %d exceeds %d%s" % (who, s, MAX_SLOTS, " (the widest band; pass slots= to truncate)"
                                                           if slots is None else ""))
    return s


def xcorrvol_band_volume(in0, in1, lo, hi, n_disps, block_size, slots=None, prepared=None):
    """The NCC scores of every pixel's band as a band volume -> Vb f32 [N,slots,H,W] ([slots,H,W] for in0 [1,H,W]).
    in0, in1, lo, hi and `prepared` as `torchext.xcorrvol_argmax_band` takes them; slots=None: `band_width(lo, hi, D)`."""
    who = "xcorrvol_band_volume"
    a0, shape, stride1, dev = _ncc_band_inputs(in0, in1, lo, hi, who)
    N, _, H, W = a0.shape
    D, bs = int(n_disps), int(block_size)
    s = _slots(slots, lo, hi, D, who)
    vb = torch.empty((N, s, H, W) if len(shape) == 3 else (s, H, W), dtype=torch.float32, device=dev)
    L = lib()
    nws = L.ctd_xcorrvol_argmax_band_workspace_bytes(N, H, W, D, bs, 1 if stride1 else 0)
    ws, flag = _pattern_planes_workspace(prepared, who, in1, N, H, W, D, bs, nws, dev)
    st = L.ctd_xcorrvol_band_volume_f32(_ptr(a0), _ptr(in1), stride1, _ptr(lo), _ptr(hi), _ptr(vb), N, s, H, W, D, bs,
                                        flag, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _pattern_planes_check(st, who, prepared, flag, H, W, D, bs)
    return vb


def costvol_band_volume(im, pattern, lo, hi, n_disps, block_size, type='census_sad', eps=0.1, slots=None):
    """The block costs of every pixel's band as a band volume -> Vb f32 [N,slots,H,W] ([slots,H,W] for im [H,W]).
    im, pattern, lo, hi, type and eps as `torchext.costvol_argmin_band` takes them; slots=None: `band_width(lo, hi, D)`."""
    who = "costvol_band_volume"
    a, ty, stride, dev = _cost_band_inputs(im, pattern, lo, hi, type, who)
    N, H, W = a.shape
    D = int(n_disps)
    s = _slots(slots, lo, hi, D, who)
    vb = torch.empty((N, s, H, W) if im.dim() == 3 else (s, H, W), dtype=torch.float32, device=dev)
    _call(lib().ctd_costvol_band_volume_f32, who, _ptr(a), _ptr(pattern), stride, _ptr(lo), _ptr(hi), _ptr(vb), N, s, H, W,
          D, int(block_size), ty, float(eps), dev.index, _stream(dev))
    return vb


def _band_volume_inputs(vol_b, lo, hi, who, cuda=True):
    """vol_b [N,slots,H,W] | [slots,H,W] f32 with lo, hi int32 [N,H,W] | [H,W] -> (vol_b as 4-D, lo, hi as 3-D, squeeze)"""
    if cuda:
        _check(vol_b, "vol_b", (torch.float32,))
        _check(lo, "lo", (torch.int32,))
        _check(hi, "hi", (torch.int32,))
    elif not all(isinstance(t, torch.Tensor) for t in (vol_b, lo, hi)) or vol_b.dtype != torch.float32 or \
            lo.dtype != torch.int32 or hi.dtype != torch.int32:
        raise RuntimeError("%s expects vol_b f32 and lo, hi int32 tensors" % who)
    squeeze = vol_b.dim() == 3
    v = vol_b.unsqueeze(0) if squeeze else vol_b
    if v.dim() != 4 or v.numel() == 0:
        raise RuntimeError("%s expects a non-empty vol_b [N,slots,H,W] or [slots,H,W]" % who)
    want = (v.shape[0], v.shape[2], v.shape[3])
    if tuple(lo.shape) != (want[1:] if squeeze else want) or lo.shape != hi.shape:
        raise RuntimeError("%s: lo and hi must be int32 shaped %s" % (who, tuple(want[1:] if squeeze else want)))
    _same_device(v, lo, hi)
    return v, lo.reshape(want), hi.reshape(want), squeeze


def band_sgm_aggregate(vol_b, lo, hi, n_disps, p1, p2, paths=8, maximise=False, return_volume=False):
    """Semi-global path aggregation of a band volume -> (idx int64, best f32[, S_b f32]).
    vol_b [N,slots,H,W] | [slots,H,W] f32 (never written) with the lo, hi int32 [N,H,W] | [H,W] it was made with; idx and
    best shaped as lo; S_b shaped as vol_b."""
    who = "band_sgm_aggregate"
    v, l3, h3, squeeze = _band_volume_inputs(vol_b, lo, hi, who)
    p1, p2 = float(p1), float(p2)
    if not (0.0 <= p1 <= p2 < float("inf")):
        raise RuntimeError("%s: need 0 <= p1 <= p2, both finite" % who)
    if paths not in (4, 8):
        raise RuntimeError("%s: paths must be 4 or 8" % who)
    dev = v.device
    N, s, H, W = v.shape
    D = int(n_disps)
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    L = lib()
    S = torch.empty_like(v) if return_volume else None
    ws = None if return_volume else _workspace(L.ctd_band_sgm_workspace_bytes(N, s, H, W, D, paths, 0), dev)
    _call(L.ctd_band_sgm_aggregate_f32, who, _ptr(v), _ptr(l3), _ptr(h3), 1 if maximise else 0, p1, p2, paths, _ptr(S),
          _ptr(idx), _ptr(best), N, s, H, W, D, _ptr(ws), ws.numel() if ws is not None else 0, dev.index, _stream(dev))
    out = (idx, best) + ((S,) if return_volume else ())
    return tuple(t[0] for t in out) if squeeze else out


def xcorrvol_band_sgm(in0, in1, lo, hi, n_disps, block_size, p1, p2, paths=8, slots=None, prepared=None,
                      return_volume=False):
    """`xcorrvol_band_volume` aggregated by `band_sgm_aggregate` with maximise=True -> (idx int64, best f32[, S_b]),
    idx and best shaped as lo; best is in cost sign (the aggregated -NCC)."""
    vb = xcorrvol_band_volume(in0, in1, lo, hi, n_disps, block_size, slots, prepared)
    return band_sgm_aggregate(vb, lo, hi, n_disps, p1, p2, paths, True, return_volume)


def costvol_band_sgm(im, pattern, lo, hi, n_disps, block_size, type, eps, p1, p2, paths=8, slots=None,
                     return_volume=False):
    """`costvol_band_volume` aggregated by `band_sgm_aggregate` -> (idx int64, best f32[, S_b]), idx and best shaped as
    im."""
    vb = costvol_band_volume(im, pattern, lo, hi, n_disps, block_size, type, eps, slots)
    return band_sgm_aggregate(vb, lo, hi, n_disps, p1, p2, paths, False, return_volume)


def band_volume_expand(vol_b, lo, hi, n_disps, fill):
    """A band volume back as a full one (torch only, any device): [N,D,H,W] | [D,H,W] f32 with vol_b's held slots at
    their disparities and `fill` everywhere else.  With fill=+inf (costs) or -inf (scores) the result composes with
    `torchext.match_validity`."""
    v, l3, h3, squeeze = _band_volume_inputs(vol_b, lo, hi, "band_volume_expand", cuda=False)
    N, s, H, W = v.shape
    D = int(n_disps)
    lc = l3.clamp(0, D).to(torch.int64)
    n = (torch.minimum(h3.clamp(-1, D - 1).to(torch.int64), lc + s - 1) - lc + 1).clamp(min=0)
    k = torch.arange(s, device=v.device).view(1, s, 1, 1)
    held = k < n.unsqueeze(1)
    d = torch.where(held, lc.unsqueeze(1) + k, torch.full_like(k, D))          # unheld slots land in a spare plane
    out = torch.full((N, D + 1, H, W), float(fill), dtype=torch.float32, device=v.device)
    out.scatter_(1, d, v)
    out = out[:, :D].contiguous()
    return out[0] if squeeze else out


band_sgm_aggregate.__doc__ += _BAND_SGM_RULE
xcorrvol_band_sgm.__doc__ += _BAND_SGM_RULE
costvol_band_sgm.__doc__ += _BAND_SGM_RULE
