# Wraps include/ctd_hip.h: ctd_disp_components_*, ctd_disp_speckle_f32, ctd_disp_median_f32 (csrc/disp_filter.hip).
import torch

from .. import _lib
from ._common import _call, _check, _ptr, _same_device, _stream, _workspace


# Disparity post-filters (additive; include/ctd_hip.h states the rules word for word)
_DISP_FILTER_RULE = """
    The rule (include/ctd_hip.h).  A pixel is live when its `valid` entry is nonzero (valid=None: everywhere) and its
    disparity is finite.  Two neighbours are linked when both are live and fabsf(disp[p] - disp[q]) <= max_diff (one f32
    subtraction); neighbours are the 4 edge neighbours, plus the 4 diagonal ones for connectivity=8, never across
    frames.  Components are the transitive closure of the links."""


def _disp_filter_inputs(disp, valid, who):
    """-> (disp f32 [N,H,W], valid u8 [N,H,W] | None, squeeze); int64 indices convert exactly below 2^24"""
    _check(disp, "disp", (torch.float32, torch.int64))
    squeeze = disp.dim() == 2
    d = disp.unsqueeze(0) if squeeze else disp
    if d.dim() != 3 or d.shape[1] == 0 or d.shape[2] == 0:
        raise RuntimeError("%s expects disp [N,H,W] or [H,W] with H, W >= 1" % who)
    if d.dtype == torch.int64:
        d = d.to(torch.float32)
    v = None
    if valid is not None:
        _check(valid, "valid", (torch.bool, torch.uint8))
        if valid.shape != disp.shape:
            raise RuntimeError("%s: valid must have the shape of disp" % who)
        _same_device(disp, valid)
        v = (valid.unsqueeze(0) if squeeze else valid).view(torch.uint8)
    return d, v, squeeze


def _disp_link_params(max_diff, connectivity, who):
    max_diff = float(max_diff)
    if not max_diff >= 0.0:
        raise RuntimeError("%s: max_diff must be >= 0" % who)
    if connectivity not in (4, 8):
        raise RuntimeError("%s: connectivity must be 4 or 8" % who)
    return max_diff, int(connectivity)


def disp_components(disp, valid=None, max_diff=1.0, connectivity=4):
    """Additive: connected components of a disparity map -> (label int32, size int32), each shaped as disp.
    disp [N,H,W] | [H,W], f32 or the matchers' int64 idx; valid None, bool or uint8 (e.g. flags == 7).  label = the
    smallest in-frame linear index h * W + w of the pixel's component, -1 for a pixel that is not live; size = the
    component's pixel count, 0 for a pixel that is not live.  max_diff = inf gives the components of the live mask."""
    d, v, squeeze = _disp_filter_inputs(disp, valid, "disp_components")
    max_diff, connectivity = _disp_link_params(max_diff, connectivity, "disp_components")
    dev = d.device
    N, H, W = d.shape
    label = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    size = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _workspace(L.ctd_disp_components_workspace_bytes(N, H, W), dev)
    _call(L.ctd_disp_components_f32, "disp_components", _ptr(d), _ptr(v), max_diff, connectivity, _ptr(label),
          _ptr(size), N, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    return (label[0], size[0]) if squeeze else (label, size)


def disp_speckle(disp, valid=None, max_diff=1.0, max_size=20, connectivity=4, return_sizes=False):
    """Additive: speckle removal -> keep uint8 (and size int32 with return_sizes), shaped as disp.  keep = 1 where the
    pixel is live and its component (see `disp_components`) has more than max_size pixels, 0 elsewhere; max_size = 0
    keeps every live pixel."""
    d, v, squeeze = _disp_filter_inputs(disp, valid, "disp_speckle")
    max_diff, connectivity = _disp_link_params(max_diff, connectivity, "disp_speckle")
    if int(max_size) != max_size or max_size < 0 or max_size >= 2 ** 31:
        raise RuntimeError("disp_speckle: max_size must be an integer in [0, 2^31)")
    dev = d.device
    N, H, W = d.shape
    keep = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    size = torch.empty((N, H, W), dtype=torch.int32, device=dev) if return_sizes else None
    L = _lib.lib()
    ws = _workspace(L.ctd_disp_components_workspace_bytes(N, H, W), dev)
    _call(L.ctd_disp_speckle_f32, "disp_speckle", _ptr(d), _ptr(v), max_diff, int(max_size), connectivity, _ptr(keep),
          _ptr(size), N, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    out = (keep, size) if return_sizes else (keep,)
    out = tuple(t[0] for t in out) if squeeze else out
    return out if return_sizes else out[0]


def disp_median(disp, valid=None, window=3, fill_min=0):
    """Additive: validity-aware median -> (disp_out f32, valid_out uint8), shaped as disp.  For pixel p, the m live
    pixels inside the window x window square centred on p (in-image pixels only, no border replication) are put in
    ascending order (ties in window raster order; the two signed zeros compare equal).  If p is live, or if
    fill_min > 0 and m >= fill_min (hole filling), the output is the element of rank (m - 1) // 2, the lower median,
    and valid_out = 1; otherwise NaN and 0.  window is 3, 5 or 7."""
    d, v, squeeze = _disp_filter_inputs(disp, valid, "disp_median")
    if window not in (3, 5, 7):
        raise RuntimeError("disp_median: window must be 3, 5 or 7")
    if int(fill_min) != fill_min or fill_min < 0 or fill_min >= 2 ** 31:
        raise RuntimeError("disp_median: fill_min must be an integer >= 0")
    dev = d.device
    N, H, W = d.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    valid_out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    _call(_lib.lib().ctd_disp_median_f32, "disp_median", _ptr(d), _ptr(v), int(window), int(fill_min), _ptr(out),
          _ptr(valid_out), N, H, W, dev.index, _stream(dev))
    return (out[0], valid_out[0]) if squeeze else (out, valid_out)


def disparity_filter(disp, valid=None, max_diff=1.0, max_size=20, connectivity=4, window=3, fill_min=0):
    """Additive: `disp_speckle`, then `disp_median` on the kept pixels -> (disp_out f32, valid_out uint8), exactly the
    composition of the two (keep already implies valid).  window=0 skips the median: disp with NaN where not kept, and
    keep."""
    keep = disp_speckle(disp, valid, max_diff, max_size, connectivity)
    if window == 0:
        d = disp.to(torch.float32)
        return torch.where(keep != 0, d, torch.full_like(d, float("nan"))), keep
    return disp_median(disp, keep, window, fill_min)


disp_components.__doc__ += _DISP_FILTER_RULE
disp_speckle.__doc__ += _DISP_FILTER_RULE
