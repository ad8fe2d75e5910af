# Wraps include/ctd_hip.h: ctd_lcn_*, ctd_lcn_xcorrvol_* (csrc/lcn.hip, csrc/lcn_stream.hip).
import torch

from .. import _lib
from ._common import _call, _check, _ptr, _same_device, _stream, _subpixel_mode, _workspace
from .ncc import _check_prepared, xcorrvol_argmax
from .subpixel import xcorrvol_subpixel


# LCN (reference: networks.LCN.tforward, model/networks.py:523-533 -- not part of the
# reference's torchext; exposed here so the whole pre-normalisation is one kernel)
def lcn(data, radius, epsilon, algo=None):
    """data [N,1,H,W] f32 -> ((data - avg) / std, std), std = sqrt(E[x^2] - avg^2 + 1e-6) + epsilon,
    box statistics over a (2*radius+1)^2 reflect-padded window.  Not differentiable (the reference
    only ever applies it to input images, exp_synph.py:84-91).
    algo (additive): 'exact' (default: f64 box sums, bit-identical to the oracle) | 'fast' (radius 7: f32 sliding sums of
    tile-centred samples, within 1e-6 |b| + 1e-6 + 64 u kappa of the float64 reference and at most 1.25 x the stock-f32
    error plus a floor, the rule of tests/test_lcn_f64_gpu.py; every other radius runs 'exact', see include/ctd_hip.h)."""
    _check(data, "data", (torch.float32,))
    if data.dim() != 4 or data.shape[1] != 1:
        raise RuntimeError("lcn expects [N,1,H,W]")
    N, _, H, W = data.shape
    if not (0 <= int(radius) < min(H, W)):
        raise RuntimeError("lcn: radius must be smaller than the image (ReflectionPad2d rule)")
    dev = data.device
    y = torch.empty_like(data)
    std = torch.empty_like(data)
    algo = algo or "exact"
    if algo not in ("exact", "fast"):
        raise RuntimeError("unknown algo %r" % (algo,))
    fn = _lib.lib().ctd_lcn_fast_f32 if (algo == "fast" and int(radius) == 7) else _lib.lib().ctd_lcn_f32
    _call(fn, "lcn", _ptr(data), _ptr(y), _ptr(std), N, H, W, int(radius), float(epsilon), dev.index, _stream(dev))
    return y, std


def lcn_xcorrvol_argmax(raw, in1, n_disps, block_size, radius=5, epsilon=0.05, return_volume=False, lcn_algo="exact",
                        rerank_eps=1e-5, prepared=None, subpixel=None):
    """Additive: `lcn` of the raw frames, then `xcorrvol_argmax(..., algo='fast')` against the (already LCN'd) pattern,
    as ONE call whose first kernel streams the raw frames once and leaves both the LCN outputs and the matcher's window
    statistics (ctd_lcn_xcorrvol_argmax_f32).  raw [N,1,H,W]; in1 [1,H,W] | [N,1,H,W].
    Returns (lcn, std, idx, best[, volume]).  lcn_algo 'exact': lcn / std carry the bits of `lcn(..., algo='exact')`;
    'fast': f32 box sums, within 1e-6 |b| + 4e-6 + 64 u kappa of the float64 LCN (the rule of
    tests/test_lcn_f64_gpu.py) on frames without long runs of a dark level next to a bright one -- there use 'exact'
    (see include/ctd_hip.h).
    Shapes the fused kernel does not cover, and rerank_eps < 0 with return_volume=True (a plain argmax of the fast
    scores, as `xcorrvol_argmax` defines it), run the two calls it replaces.
    subpixel: None (default) | "parabola" | "equiangular": also return (disp, refined) of
    `xcorrvol_subpixel(lcn, in1, idx, ...)` -- against the LCN output this call returns -- at the end of the tuple."""
    if subpixel is not None:
        _subpixel_mode(subpixel, "lcn_xcorrvol_argmax")
        out = lcn_xcorrvol_argmax(raw, in1, n_disps, block_size, radius, epsilon, return_volume, lcn_algo, rerank_eps,
                                  prepared)
        return tuple(out) + xcorrvol_subpixel(out[0], in1, out[2], n_disps, block_size, subpixel, prepared)
    _check(raw, "raw", (torch.float32,))
    _check(in1, "in1", (torch.float32,))
    if raw.dim() != 4 or raw.shape[1] != 1 or in1.dim() not in (3, 4):
        raise RuntimeError("lcn_xcorrvol_argmax expects raw [N,1,H,W] and in1 [1,H,W] or [N,1,H,W]")
    if lcn_algo not in ("exact", "fast"):
        raise RuntimeError("unknown lcn_algo %r" % (lcn_algo,))
    L = _lib.lib()
    dev = _same_device(raw, in1)
    N, C, H, W = raw.shape
    if tuple(in1.shape[-3:]) != (C, H, W):
        raise RuntimeError("raw and in1 must have the same [C,H,W] shape")
    D, bs = int(n_disps), int(block_size)
    if not (0 <= int(radius) < min(H, W)):
        raise RuntimeError("lcn: radius must be smaller than the image (ReflectionPad2d rule)")
    # rerank_eps < 0 with a volume means a plain argmax of the fast scores (xcorrvol_argmax); the fused kernel always
    # ranks with eps >= 0, so that call runs as the two calls it replaces, as on the shapes the fused kernel does not cover
    if not L.ctd_lcn_xcorrvol_supported(H, W, D, int(radius), bs) or (float(rerank_eps) < 0 and return_volume):
        y, std = lcn(raw, radius, epsilon, algo=lcn_algo)
        out = xcorrvol_argmax(y, in1, D, bs, return_volume=return_volume, algo="fast", rerank_eps=rerank_eps, prepared=prepared)
        return (y, std) + tuple(out)
    stride1 = 0 if in1.dim() == 3 else C * H * W
    y, std = torch.empty_like(raw), torch.empty_like(raw)
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    vol = torch.empty((N, D, H, W), dtype=torch.float32, device=dev) if return_volume else None
    a = 1
    if prepared is not None:
        _check_prepared(prepared, "lcn_xcorrvol_argmax", a, in1, N, D, bs, dev)
        ws, a = prepared.workspace, a | 0x100                        # CTD_PATTERN_PREPARED
    else:
        ws = _workspace(L.ctd_xcorrvol_argmax_workspace_bytes(N, C, H, W, D, bs, a), dev)
    _call(L.ctd_lcn_xcorrvol_argmax_f32, "lcn_xcorrvol_argmax", _ptr(raw), _ptr(y), _ptr(std), int(radius),
          float(epsilon), 0 if lcn_algo == "exact" else 1, _ptr(in1), stride1, _ptr(vol), _ptr(idx), _ptr(best), N, H,
          W, D, bs, a, float(rerank_eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    return (y, std, idx, best, vol) if return_volume else (y, std, idx, best)


def lcn_normalize(img, kernel_size=4, epsilon=0.01):
    """Additive: the data generator's LCN, `lcn.normalize(img, kernel_size, epsilon)` of data/lcn/lcn.pyx:16-58
    (two-pass mean / std, zero border of width kernel_size, returns (lcn, raw std)); img [H,W] or [N,H,W]."""
    _check(img, "img", (torch.float32,))
    squeeze = img.dim() == 2
    a = img.unsqueeze(0) if squeeze else img
    if a.dim() != 3:
        raise RuntimeError("lcn_normalize expects [H,W] or [N,H,W]")
    N, H, W = a.shape
    dev = a.device
    out, std = torch.empty_like(a), torch.empty_like(a)
    _call(_lib.lib().ctd_lcn_datagen_f32, "lcn_normalize", _ptr(a), _ptr(out), _ptr(std), N, H, W, int(kernel_size),
          float(epsilon), dev.index, _stream(dev))
    return (out[0], std[0]) if squeeze else (out, std)
