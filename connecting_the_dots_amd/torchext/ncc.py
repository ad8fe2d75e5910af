# Wraps include/ctd_hip.h: ctd_xcorrvol_*, ctd_argmax_disp_f32 (csrc/ncc_*.hip, csrc/argmax_rerank.hip).
import torch

from .. import _lib
from ._common import _call, _check, _ncc_fast_covers, _ncc_pair, _ptr, _resolve_ncc_algo, _same_device, _stream, _subpixel_mode, \
    _workspace
from .subpixel import xcorrvol_subpixel
from .validity import _validity_kwargs, xcorrvol_validity


def _check_prepared(prepared, who, a, in1, N, D, bs, dev):
    if (a != 1 or prepared.in1 is not in1 or prepared.n_frames != N or prepared.n_disps != D or prepared.block_size != bs
            or prepared.workspace.device != dev):
        raise RuntimeError("%s: `prepared` belongs to another pattern, frame count, shape or device "
                           "(or the call does not take the fast path)" % who)


# NCC volume (reference: XCorrVolFunction, functions.py:59-74)
def _xcorrvol_impl(in0, in1, n_disps, block_size, algo, prepared=None):
    """in0 [N,C,H,W], in1 [C,H,W] | [N,C,H,W] -> [N,D,H,W]"""
    L = _lib.lib()
    dev = _same_device(in0, in1)
    if in0.dtype != in1.dtype:
        raise RuntimeError("in0 and in1 must have the same dtype")
    N, C, H, W = in0.shape
    if tuple(in1.shape[-3:]) != (C, H, W):
        raise RuntimeError("in0 and in1 must have the same [C,H,W] shape")
    stride1 = 0 if in1.dim() == 3 else C * H * W
    if in1.dim() == 4 and in1.shape[0] != N:
        raise RuntimeError("in1 batch does not match in0")
    D, bs = int(n_disps), int(block_size)
    out = torch.empty((N, D, H, W), dtype=in0.dtype, device=dev)
    a = _resolve_ncc_algo(algo, in0.dtype, D, bs)
    if prepared is not None:
        _check_prepared(prepared, "xcorrvol_batch", a, in1, N, D, bs, dev)
        ws, a = prepared.workspace, a | 0x100                        # CTD_PATTERN_PREPARED
    else:
        ws = _workspace(L.ctd_xcorrvol_workspace_bytes(N, C, H, W, D, bs, a), dev)
    if in0.dtype == torch.float32:
        st = L.ctd_xcorrvol_f32(_ptr(in0), _ptr(in1), stride1, _ptr(out), N, C, H, W, D, bs, a, _ptr(ws),
                                ws.numel(), dev.index, _stream(dev))
    else:
        st = L.ctd_xcorrvol_f64(_ptr(in0), _ptr(in1), stride1, _ptr(out), N, C, H, W, D, bs, _ptr(ws), ws.numel(),
                                dev.index, _stream(dev))
    _lib.check(st, "xcorrvol")
    return out


class XCorrVolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1, n_disps, block_size, algo=None):
        _check(in0, "in0")
        _check(in1, "in1")
        if in0.dim() != 3 or in1.dim() != 3:
            raise RuntimeError("xcorrvol expects [C,H,W] tensors")
        return _xcorrvol_impl(in0.unsqueeze(0), in1, n_disps, block_size, algo)[0]

    @staticmethod
    def backward(ctx, grad_out):
        return None, None, None, None, None


def xcorrvol(in0, in1, n_disps, block_size, algo=None):
    """Zero-mean NCC volume [D,H,W] between in0 [C,H,W] at (h,w) and in1 at (h,w-d).
    algo (additive): 'fast' (default) | 'exact', see the module docstring."""
    return XCorrVolFunction.apply(in0, in1, n_disps, block_size, algo)


def xcorrvol_batch(in0, in1, n_disps, block_size, algo=None, prepared=None):
    """Additive: xcorrvol for a batch of frames in one launch.
    in0 [N,C,H,W]; in1 [C,H,W] (shared pattern) or [N,C,H,W] -> [N,D,H,W].  `prepared`: see `prepare_pattern`."""
    _check(in0, "in0")
    _check(in1, "in1")
    if in0.dim() != 4 or in1.dim() not in (3, 4):
        raise RuntimeError("xcorrvol_batch expects in0 [N,C,H,W] and in1 [C,H,W] or [N,C,H,W]")
    return _xcorrvol_impl(in0, in1, n_disps, block_size, algo, prepared)


def argmax_disp(vol):
    """Additive: (torch.argmax(vol, -3), vol.max(-3)) for vol [D,H,W] or [N,D,H,W]; first index wins ties."""
    _check(vol, "vol", (torch.float32,))
    squeeze = vol.dim() == 3
    v = vol.unsqueeze(0) if squeeze else vol
    if v.dim() != 4:
        raise RuntimeError("argmax_disp expects [D,H,W] or [N,D,H,W]")
    N, D, H, W = v.shape
    dev = v.device
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    _call(_lib.lib().ctd_argmax_disp_f32, "argmax_disp", _ptr(v), _ptr(idx), _ptr(best), N, D, H, W, dev.index,
          _stream(dev))
    return (idx[0], best[0]) if squeeze else (idx, best)


class PreparedPattern:
    """The pattern half of the fast NCC path, done once (`prepare_pattern`): holds the workspace the pattern's window
    statistics and fix-up lists live in -- dedicated to the calls that pass this object -- and the shape it is valid for."""

    def __init__(self, in1, n_frames, n_disps, block_size, workspace):
        self.in1, self.n_frames, self.n_disps, self.block_size, self.workspace = in1, n_frames, n_disps, block_size, workspace
        self.subpixel = {}            # (H, W, D, block_size) -> workspace of xcorrvol_subpixel, pattern planes filled


def prepare_pattern(in1, n_frames, n_disps, block_size):
    """Additive: window statistics / fix-up lists of the pattern `in1` ([1,H,W] shared, or [N,1,H,W] per frame), computed
    ONCE for all later `xcorrvol_argmax(..., prepared=handle)` calls with `n_frames` frames of the same shape -- the
    reference prepares its pattern once per run too (model/exp_synph.py:64-71).  Fast path, C == 1."""
    _check(in1, "in1", (torch.float32,))
    if in1.dim() not in (3, 4) or in1.shape[-3] != 1:
        raise RuntimeError("prepare_pattern expects in1 [1,H,W] or [N,1,H,W]")
    H, W = in1.shape[-2:]
    D, bs, N = int(n_disps), int(block_size), int(n_frames)
    if not _ncc_fast_covers(in1.dtype, D, bs):
        raise RuntimeError("prepare_pattern: the fast NCC path does not cover this block size / disparity range")
    L = _lib.lib()
    dev = in1.device
    ws = _workspace(L.ctd_xcorrvol_argmax_workspace_bytes(N, 1, H, W, D, bs, 1), dev)
    stride1 = 0 if in1.dim() == 3 else H * W
    _call(L.ctd_xcorrvol_pattern_prepare_f32, "prepare_pattern", _ptr(in1), stride1, N, 1, H, W, D, bs, _ptr(ws),
          ws.numel(), dev.index, _stream(dev))
    return PreparedPattern(in1, N, D, bs, ws)


def xcorrvol_argmax(in0, in1, n_disps, block_size, return_volume=False, algo=None, rerank_eps=1e-5, prepared=None,
                    subpixel=None, validity=None):
    """Additive: fused NCC volume + argmax over disparity (C == 1).
    in0 [N,1,H,W] | [1,H,W]; in1 [1,H,W] | [N,1,H,W].
    Returns (idx int64, best f32[, volume]); idx == torch.argmax(xcorrvol(...), 0) of the reference.
    `prepared`: a `prepare_pattern` handle of the same `in1`, frame count and shape (fast path only): the pattern half of
    the pre-pass is skipped and the handle's workspace is used.
    subpixel: None (default) | "parabola" | "equiangular": also return (disp f32, refined u8) of
    `xcorrvol_subpixel(in0, in1, idx, ...)` at the end of the tuple.
    validity: None (default) | dict(lr_tol=..., min_gap=...): also return (flags, idx_r, gap) of
    `xcorrvol_validity(in0, in1, idx, ..., algo=algo)` at the end of the tuple (after the sub-pixel outputs)."""
    if validity is not None:
        kw = _validity_kwargs(validity, "xcorrvol_argmax")
        out = xcorrvol_argmax(in0, in1, n_disps, block_size, return_volume, algo, rerank_eps, prepared, subpixel)
        return tuple(out) + xcorrvol_validity(in0, in1, out[0], n_disps, block_size, algo=algo, **kw)
    if subpixel is not None:
        _subpixel_mode(subpixel, "xcorrvol_argmax")
        out = xcorrvol_argmax(in0, in1, n_disps, block_size, return_volume, algo, rerank_eps, prepared)
        return tuple(out) + xcorrvol_subpixel(in0, in1, out[0], n_disps, block_size, subpixel, prepared)
    _check(in0, "in0", (torch.float32,))
    _check(in1, "in1", (torch.float32,))
    # C != 1 is left to the library, and in1's N is not compared with in0's
    a0, _, stride1, dev = _ncc_pair(in0, in1, "xcorrvol_argmax expects in0 [N,1,H,W] or [1,H,W]",
                                    "in0 and in1 must have the same [C,H,W] shape", c1=False, batch=False)
    squeeze = in0.dim() == 3
    L = _lib.lib()
    N, C, H, W = a0.shape
    D, bs = int(n_disps), int(block_size)
    a = _resolve_ncc_algo(algo, a0.dtype, D, bs)
    idx = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    # the fast path ranks inside the volume kernel where it can (no volume needed); other shapes rank a materialised one
    need_vol = a == 1 and not L.ctd_xcorrvol_rank_supported(C, H, W, D, bs)
    vol = torch.empty((N, D, H, W), dtype=torch.float32, device=dev) if (return_volume or need_vol) else None
    if prepared is not None:
        _check_prepared(prepared, "xcorrvol_argmax", a, in1, N, D, bs, dev)
        ws, a_flag = prepared.workspace, a | 0x100                   # CTD_PATTERN_PREPARED
    else:
        ws, a_flag = _workspace(L.ctd_xcorrvol_argmax_workspace_bytes(N, C, H, W, D, bs, a), dev), a
    _call(L.ctd_xcorrvol_argmax_f32, "xcorrvol_argmax", _ptr(a0), _ptr(in1), stride1, _ptr(vol), _ptr(idx), _ptr(best),
          N, C, H, W, D, bs, a_flag, float(rerank_eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    if squeeze:
        idx, best = idx[0], best[0]
        vol = vol[0] if vol is not None else None
    return (idx, best, vol) if return_volume else (idx, best)
