# Wraps include/ctd_hip.h: ctd_match_validity_f32, ctd_xcorrvol_validity_*, ctd_costvol_validity_*.
import torch

from .. import _lib
from ._common import _call, _check, _cost_pair, _loss_type, _ncc_pair, _photo_fast, _ptr, _resolve_ncc_algo, _same_device, _stream, \
    _workspace


# Match validity: left-right consistency and uniqueness (additive; include/ctd_hip.h states the rule word for word)
VALID_IN_PATTERN, VALID_LR_OK, VALID_UNIQUE = 1, 2, 4

_VALIDITY_RULE = """
    The rule (include/ctd_hip.h), on the reference-order volume V (NCC: xcorrvol(algo="exact"), higher is better; costs:
    costvol(algo="exact"), lower is better), d0 = idx:
      idx_r[f,h,x] = first index of the best V[f,d,h,x+d] over d in [0, min(D, W-x))     (the pattern-side match)
      gap[f,h,w]   = s1 - s2 (NCC) | s2 - s1 (costs), s1 = V[d0], s2 = the best V[d] over |d - d0| >= 2; +inf when no
                     such d exists, NaN when idx is outside [0, D)
      flags bit 0 IN_PATTERN: 0 <= idx < D and w - idx >= 0;  bit 1 LR_OK: bit 0 and |idx_r[f,h,w-idx] - idx| <= lr_tol;
            bit 2 UNIQUE: 0 <= idx < D and gap > min_gap;  valid = (flags == 7).
    flags and idx_r are exact with either algo; gap is exact with algo="exact" and on re-scored pixels, otherwise within
    1e-5 (|s1| + |s2|) + 2e-6."""


def _validity_params(lr_tol, min_gap, who):
    if isinstance(lr_tol, bool) or int(lr_tol) != lr_tol or int(lr_tol) < 0:
        raise RuntimeError("%s: lr_tol must be an int >= 0" % who)
    min_gap = float(min_gap)
    if not min_gap >= 0.0:
        raise RuntimeError("%s: min_gap must be a number >= 0" % who)
    return int(lr_tol), min_gap


def _validity_outputs(idx):
    dev = idx.device
    return (torch.empty(idx.shape, dtype=torch.uint8, device=dev), torch.empty(idx.shape, dtype=torch.int64, device=dev),
            torch.empty(idx.shape, dtype=torch.float32, device=dev))


def _validity_rescored(ws, P, dev):
    """(sorted flat indices of the re-scored pixels, of the re-scored pattern columns) from the workspace (ctd_hip.h)"""
    n = ws[:8].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    n_pix, n_col = int(n[0]), int(n[1])
    off = (256 + 4 * P + 255) // 256 * 256
    pix = (ws[256:256 + 4 * n_pix].view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sort()[0]
    col = (ws[off:off + 4 * n_col].view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sort()[0]
    return pix, col


def match_validity(vol, idx, maximise, lr_tol=1, min_gap=0.0):
    """Additive: (flags u8, idx_r int64, gap f32), each shaped as idx, of a materialised volume taken as exact.
    vol [N,D,H,W] | [D,H,W] f32, idx int64 [N,H,W] | [H,W] (any index); maximise: True for scores (NCC), False for costs."""
    _check(vol, "vol", (torch.float32,))
    _check(idx, "idx", (torch.int64,))
    lr_tol, min_gap = _validity_params(lr_tol, min_gap, "match_validity")
    squeeze = vol.dim() == 3
    v = vol.unsqueeze(0) if squeeze else vol
    if v.dim() != 4:
        raise RuntimeError("match_validity expects vol [N,D,H,W] or [D,H,W]")
    dev = _same_device(v, idx)
    N, D, H, W = v.shape
    if tuple(idx.shape) != ((H, W) if squeeze else (N, H, W)):
        raise RuntimeError("match_validity: idx must be shaped [N,H,W] (or [H,W]) like the volume without its D axis")
    flags, idx_r, gap = _validity_outputs(idx)
    _call(_lib.lib().ctd_match_validity_f32, "match_validity", _ptr(v), 1 if maximise else 0, _ptr(idx), _ptr(flags),
          _ptr(idx_r), _ptr(gap), N, D, H, W, lr_tol, min_gap, dev.index, _stream(dev))
    return flags, idx_r, gap


def xcorrvol_validity(in0, in1, idx, n_disps, block_size, lr_tol=1, min_gap=0.0, algo=None, return_rescored=False):
    """Additive: left-right consistency and uniqueness of NCC matcher indices -> (flags u8, idx_r int64, gap f32), each
    shaped as idx.  in0 [N,C,H,W] | [C,H,W] and in1 [C,H,W] | [N,C,H,W] as `xcorrvol_batch` / `xcorrvol_argmax` take them,
    idx int64 [N,H,W] | [H,W] as `xcorrvol_argmax` returns it (any index).  The volume is computed into a workspace
    (N * D * H * W floats) and read once.
    algo: 'fast' (default) | 'exact'; shapes the fast NCC path does not cover here (C > 1, block sizes other than
    3/5/7/9, D > 512) take 'exact'.
    return_rescored: also return (pixels, columns), the sorted int64 flat indices of the pixels and pattern columns the
    fast path settled by exact re-scoring (both empty with 'exact')."""
    _check(in0, "in0", (torch.float32,))
    _check(in1, "in1", (torch.float32,))
    _check(idx, "idx", (torch.int64,))
    lr_tol, min_gap = _validity_params(lr_tol, min_gap, "xcorrvol_validity")
    a0, shape, stride1, dev = _ncc_pair(in0, in1, "xcorrvol_validity expects in0 [N,C,H,W] or [C,H,W] and in1 [C,H,W] or "
                                        "[N,C,H,W]", "xcorrvol_validity: in1 does not match in0", c1=False, others=(idx,))
    N, C, H, W = a0.shape
    if tuple(idx.shape) != shape:
        raise RuntimeError("xcorrvol_validity: idx must be shaped as xcorrvol_argmax returns it")
    D, bs = int(n_disps), int(block_size)
    a = _resolve_ncc_algo(algo, a0.dtype, D, bs, fast_ok=C == 1)
    flags, idx_r, gap = _validity_outputs(idx)
    L = _lib.lib()
    ws = _workspace(L.ctd_xcorrvol_validity_workspace_bytes(N, C, H, W, D, bs, a), dev)
    _call(L.ctd_xcorrvol_validity_f32, "xcorrvol_validity", _ptr(a0), _ptr(in1), stride1, _ptr(idx), _ptr(flags),
          _ptr(idx_r), _ptr(gap), N, C, H, W, D, bs, a, lr_tol, min_gap, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    if return_rescored:
        return (flags, idx_r, gap) + _validity_rescored(ws, N * H * W, dev)
    return flags, idx_r, gap


def costvol_validity(im, pattern, idx, n_disps, block_size, type='census_sad', eps=0.1, lr_tol=1, min_gap=0.0, algo=None,
                     return_rescored=False):
    """Additive: left-right consistency and uniqueness of cost-volume indices -> (flags u8, idx_r int64, gap f32), each
    shaped as idx.  im [N,H,W] | [H,W] and pattern [H,W] | [N,H,W] as `costvol_argmin` takes them, idx int64 shaped as it
    returns it (any index).  The volume is computed into a workspace (N * D * H * W floats) and read once.
    algo: 'fast' (default, or env CTD_PHOTO_ALGO) | 'exact'; block sizes other than 3/5/7/9 take 'exact'.
    return_rescored: as `xcorrvol_validity`."""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    _check(idx, "idx", (torch.int64,))
    lr_tol, min_gap = _validity_params(lr_tol, min_gap, "costvol_validity")
    ty = _loss_type(type, "costvol_validity")
    a, stride, dev = _cost_pair(im, pattern, "costvol_validity", others=(idx,))
    N, H, W = a.shape
    if tuple(idx.shape) != tuple(im.shape):
        raise RuntimeError("costvol_validity: idx must be shaped as costvol_argmin returns it")
    D, bs = int(n_disps), int(block_size)
    fast = 1 if _photo_fast(a, bs, algo) else 0
    flags, idx_r, gap = _validity_outputs(idx)
    L = _lib.lib()
    ws = _workspace(L.ctd_costvol_validity_workspace_bytes(N, H, W, D, bs, ty, fast, 1 if stride else 0), dev)
    _call(L.ctd_costvol_validity_f32, "costvol_validity", _ptr(a), _ptr(pattern), stride, _ptr(idx), _ptr(flags),
          _ptr(idx_r), _ptr(gap), N, H, W, D, bs, ty, float(eps), fast, lr_tol, min_gap, _ptr(ws), ws.numel(),
          dev.index, _stream(dev))
    if return_rescored:
        return (flags, idx_r, gap) + _validity_rescored(ws, N * H * W, dev)
    return flags, idx_r, gap


def _validity_kwargs(validity, who):
    if not isinstance(validity, dict) or not set(validity) <= {"lr_tol", "min_gap"}:
        raise RuntimeError("%s: validity must be None or a dict with the keys lr_tol and / or min_gap" % who)
    return validity


match_validity.__doc__ += _VALIDITY_RULE
xcorrvol_validity.__doc__ += _VALIDITY_RULE
costvol_validity.__doc__ += _VALIDITY_RULE
