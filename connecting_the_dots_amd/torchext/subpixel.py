# Wraps include/ctd_hip.h: ctd_xcorrvol_subpixel_* and ctd_costvol_subpixel_f32 (csrc/subpixel.hip).
import torch

from .. import _lib
from ._common import _call, _check, _cost_pair, _loss_type, _ncc_pair, _ptr, _stream, _subpixel_mode, _workspace


_SUBPIXEL_RULE = """
    The rule (include/ctd_hip.h, word for word there), in float32, no FMA, IEEE divide, around d = idx:
      NCC, a maximum (sm, s0, sp = the exact scores at d-1, d, d+1):
        parabola:    den = (sm - s0) + (sp - s0); refined iff den < 0, delta = 0.5 * ((sm - sp) / den)
        equiangular: sp > sm: delta = 0.5 * ((sp - sm) / (s0 - sm)), refined iff s0 - sm > 0;
                     else:    delta = 0.5 * ((sp - sm) / (s0 - sp)), refined iff s0 - sp > 0
      costs, a minimum (cm, c0, cp = the exact costs at d-1, d, d+1):
        parabola:    den = (cm - c0) + (cp - c0); refined iff den > 0, delta = 0.5 * ((cm - cp) / den)
        equiangular: cp < cm: delta = 0.5 * ((cm - cp) / (cm - c0)), refined iff cm - c0 > 0;
                     else:    delta = 0.5 * ((cm - cp) / (cp - c0)), refined iff cp - c0 > 0
      delta is clamped to [-0.5, 0.5]; disp = d + delta where refined, d where not (d == 0, d == D-1, flat windows);
      idx outside [0, D) gives disp = NaN, refined = 0."""


def _subpixel_outputs(idx):
    _check(idx, "idx", (torch.int64,))
    return torch.empty(idx.shape, dtype=torch.float32, device=idx.device), \
        torch.empty(idx.shape, dtype=torch.uint8, device=idx.device)


def _pattern_planes_workspace(prepared, who, in1, N, H, W, D, bs, nws, dev):
    """(workspace, flag) of the ops that keep the pattern's window statistics in the band / sub-pixel workspace
    (xcorrvol_subpixel, xcorrvol_argmax_band, xcorrvol_band_validity): a fresh one, or the one the `prepare_pattern`
    handle keeps per (H, W, D, block) -- with CTD_PATTERN_PREPARED once an earlier call has filled its planes."""
    if prepared is None:
        return _workspace(nws, dev), 0
    if prepared.in1 is not in1 or prepared.n_frames != N or prepared.workspace.device != dev:
        raise RuntimeError("%s: `prepared` belongs to another pattern, frame count or device" % who)
    key = (H, W, D, bs)
    ws = prepared.subpixel.get(key)
    if ws is None:
        ws = prepared.subpixel[key] = _workspace(nws, dev)
        return ws, 0
    return ws, 0x100                                                    # CTD_PATTERN_PREPARED: the pattern planes are in ws


def _pattern_planes_check(st, who, prepared, flag, H, W, D, bs):
    if st != 0 and flag == 0 and prepared is not None:
        prepared.subpixel.pop((H, W, D, bs), None)                      # the planes were not written
    _lib.check(st, who)


def xcorrvol_subpixel(in0, in1, idx, n_disps, block_size, mode="parabola", prepared=None):
    """Additive: sub-pixel refinement of NCC matcher indices -> (disp f32, refined u8), shaped as idx.
    in0 [N,1,H,W] | [1,H,W] and in1 [1,H,W] | [N,1,H,W] as `xcorrvol_argmax` takes them, idx int64 [N,H,W] | [H,W] as it
    returns them (any index: it need not be the argmax).  The fit runs through the scores of
    `xcorrvol(..., algo="exact")` -- the reference's bits -- at idx - 1, idx, idx + 1 (ctd_xcorrvol_subpixel_f32).
    mode: "parabola" (default; measured the better fit for NCC) | "equiangular".
    `prepared`: a `prepare_pattern` handle of the same in1 and shape keeps the pattern's window statistics of this op
    too, computed at its first use, so later calls recompute the frame half only.
    Use: disp_to_depth(disp + disp_offset, baseline_focal)."""
    _check(in0, "in0", (torch.float32,))
    _check(in1, "in1", (torch.float32,))
    m = _subpixel_mode(mode, "xcorrvol_subpixel")
    a0, shape, stride1, dev = _ncc_pair(in0, in1, "xcorrvol_subpixel expects in0 [N,1,H,W] or [1,H,W] and in1 [1,H,W] or "
                                        "[N,1,H,W]", "xcorrvol_subpixel: in1 does not match in0", others=(idx,))
    N, C, H, W = a0.shape
    if tuple(idx.shape) != shape:
        raise RuntimeError("xcorrvol_subpixel: idx must be shaped as xcorrvol_argmax returns it")
    disp, refined = _subpixel_outputs(idx)
    D, bs = int(n_disps), int(block_size)
    L = _lib.lib()
    nws = L.ctd_xcorrvol_subpixel_workspace_bytes(N, H, W, D, bs, 1 if stride1 else 0)
    ws, flag = _pattern_planes_workspace(prepared, "xcorrvol_subpixel", in1, N, H, W, D, bs, nws, dev)
    st = L.ctd_xcorrvol_subpixel_f32(_ptr(a0), _ptr(in1), stride1, _ptr(idx), _ptr(disp), _ptr(refined), N, H, W, D, bs,
                                     m | flag, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _pattern_planes_check(st, "xcorrvol_subpixel", prepared, flag, H, W, D, bs)
    return disp, refined


def costvol_subpixel(im, pattern, idx, n_disps, block_size, type='census_sad', eps=0.1, mode="equiangular"):
    """Additive: sub-pixel refinement of cost-volume indices -> (disp f32, refined u8), shaped as idx.
    im [N,H,W] | [H,W] and pattern [H,W] | [N,H,W] as `costvol_argmin` takes them, idx int64 shaped as it returns it.
    The fit runs through the costs of `costvol(..., algo="exact")` at idx - 1, idx, idx + 1
    (ctd_costvol_subpixel_f32).  mode: "equiangular" (default; measured the better fit for SAD) | "parabola".
    The soft-census types (census_mse, census_sad) are refined by the same rule, bit for bit, but their costs are too
    non-linear in d for either fit to improve accuracy: refine SAD / MSE or NCC instead."""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    m = _subpixel_mode(mode, "costvol_subpixel")
    ty = _loss_type(type, "costvol_subpixel")
    a, stride, dev = _cost_pair(im, pattern, "costvol_subpixel", others=(idx,))
    N, H, W = a.shape
    if tuple(idx.shape) != tuple(im.shape):
        raise RuntimeError("costvol_subpixel: idx must be shaped as costvol_argmin returns it")
    disp, refined = _subpixel_outputs(idx)
    _call(_lib.lib().ctd_costvol_subpixel_f32, "costvol_subpixel", _ptr(a), _ptr(pattern), stride, _ptr(idx),
          _ptr(disp), _ptr(refined), N, H, W, int(n_disps), int(block_size), ty, float(eps), m, dev.index, _stream(dev))
    return disp, refined


xcorrvol_subpixel.__doc__ += _SUBPIXEL_RULE
costvol_subpixel.__doc__ += _SUBPIXEL_RULE
