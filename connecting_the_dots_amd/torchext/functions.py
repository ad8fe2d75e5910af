"""Mirror of the reference's `torchext/functions.py` on top of libctd_hip.so.

Same names, argument meaning, autograd contract and error behaviour as the reference
(torchext/functions.py:1-147); every op takes CUDA(=HIP) tensors that are contiguous and
launches on the caller's current stream and the tensor's device.  There is no CPU path in
this package: CPU tensors raise (the reference's CPU path is `ext_cpu`, which lives on as
the test oracle only).

Additive API (no reference counterpart): `xcorrvol_batch`, `argmax_disp`,
`xcorrvol_argmax`, `lcn`, ... and the keyword `algo` of the ops that have two kernel families:
    'fast'  (default) tolerance-level kernels, |a-b| <= 1e-5*|b| + 1e-6 against the reference (LDS-tiled, HBM- or
            issue-bound; f32 and odd block sizes up to 9 -- anything else runs the reference-order kernels); the NCC
            volume of C > 1 channels is within the sum of that bound over its per-channel NCCs, 1e-5 * sum_c |b_c| +
            C * 1e-6 (include/ctd_hip.h);
    'exact' the reference's operation order, bit-identical to its CPU build (the parity anchor).
The default can be changed with the environment variables CTD_NCC_ALGO (xcorrvol family) and CTD_PHOTO_ALGO
(photometric loss, cost volumes, pattern similarity loss).
"""
import numbers
import os

import torch

from .. import _lib

_ALGOS = {"exact": 0, "fast": 1}


def _default_algo():
    return os.environ.get("CTD_NCC_ALGO", "fast")


def _ncc_fast_covers(dtype, n_disps, block_size):
    """the separable-sum kernels: f32, block 3/5/7/9, D <= 512; everything else is the reference-order kernel's"""
    return dtype == torch.float32 and int(block_size) in (3, 5, 7, 9) and int(n_disps) <= 512


def _check(t, name, dtypes=(torch.float32, torch.float64)):
    # CHECK_CUDA / CHECK_CONTIGUOUS of the reference binding (ext.h:6-10) -> RuntimeError
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (connecting_the_dots_amd has no CPU path)" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if t.dtype not in dtypes:
        raise RuntimeError("%s: unsupported dtype %s" % (name, t.dtype))


def _same_device(*ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _workspace(nbytes, dev):
    # torch's caching allocator makes this a stream-ordered sub-allocation, no hipMalloc
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _ptr(t):
    return t.data_ptr() if t is not None else None


_TICKETS = {}


def _ticket(dev):
    """Zeroed device words (128 of them) per (device, stream) for kernels whose last workgroup finishes a reduction: they
    take them at zero and leave them at zero (ctd_hip.h: ctd_geometric_sym_fwd_f32)."""
    key = (dev.index, _stream(dev))
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(128, dtype=torch.int32, device=dev)
    return t


def _call_with_ticket(call, ticket, what):
    """Runs `call(ticket)` (a C-ABI launch that takes its ticket words at zero and leaves them at zero).  When it
    returns an error the words may be anywhere in between -- a later launch on them would then have no "last"
    workgroup and leave its result unwritten -- so they are cleared (stream-ordered, like the launch) before the error
    is raised."""
    st = call(ticket)
    if st != 0:
        ticket.zero_()
    _lib.check(st, what)


# --------------------------------------------------------------------------------------
# Nearest-neighbour consistency ops (reference: NNFunction / CrossCheckFunction / ProjNNFunction,
# functions.py:5-56; bindings ext_cuda.cpp:17-68)
# --------------------------------------------------------------------------------------
class NNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1):
        _check(in0, "in0")
        _check(in1, "in1")
        dev = _same_device(in0, in1)
        # shape asserts of the reference binding (ext_cuda.cpp:25-28)
        if in0.dim() != 2 or in1.dim() != 2:
            raise RuntimeError("in0 has to be N0 x 3, in1 has to be N1 x 3")
        if in0.shape[1] != in1.shape[1]:
            raise RuntimeError("in0 and in1 have to be the same shape")
        if in0.shape[1] != 3:
            raise RuntimeError("dim hast to be 3")
        if in0.dtype != in1.dtype:
            raise RuntimeError("in0 and in1 must have the same dtype")
        out = torch.empty((in0.shape[0],), dtype=torch.int64, device=dev)
        fn = _lib.lib().ctd_nn_f32 if in0.dtype == torch.float32 else _lib.lib().ctd_nn_f64
        _lib.check(fn(_ptr(in0), _ptr(in1), in0.shape[0], in1.shape[0], _ptr(out), dev.index, _stream(dev)), "nn")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return None, None


def nn(in0, in1):
    """Index of the nearest in1 point [N1,3] for every in0 point [N0,3] (int64 [N0], -1 if none within 1e9)."""
    return NNFunction.apply(in0, in1)


class CrossCheckFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0, in1):
        _check(in0, "in0", (torch.int64,))
        _check(in1, "in1", (torch.int64,))
        dev = _same_device(in0, in1)
        if in0.dim() != 1 or in1.dim() != 1:
            raise RuntimeError("crosscheck expects 1-D index tensors")
        out = torch.empty((in0.shape[0],), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().ctd_crosscheck(_ptr(in0), _ptr(in1), in0.shape[0], in1.shape[0], _ptr(out), dev.index,
                                             _stream(dev)), "crosscheck")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return None, None


def crosscheck(in0, in1):
    """uint8 [N0]: 1 where in1[in0[i]] == i (mutual nearest neighbours)."""
    return CrossCheckFunction.apply(in0, in1)


class ProjNNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz0, xyz1, K, patch_size):
        _check(xyz0, "xyz0")
        _check(xyz1, "xyz1")
        _check(K, "K")
        dev = _same_device(xyz0, xyz1, K)
        if xyz0.dim() != 4 or xyz1.dim() != 4 or xyz0.shape[3] != 3 or tuple(xyz0.shape) != tuple(xyz1.shape):
            raise RuntimeError("proj_nn expects xyz0 and xyz1 of the same shape [B,H,W,3]")
        if K.numel() != 9:
            raise RuntimeError("K has to be 3 x 3")
        if not (xyz0.dtype == xyz1.dtype == K.dtype):
            raise RuntimeError("xyz0, xyz1 and K must have the same dtype")
        B, H, W, _ = xyz0.shape
        out = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        fn = _lib.lib().ctd_proj_nn_f32 if xyz0.dtype == torch.float32 else _lib.lib().ctd_proj_nn_f64
        _lib.check(fn(_ptr(xyz0), _ptr(xyz1), _ptr(K), B, H, W, int(patch_size), _ptr(out), dev.index, _stream(dev)),
                   "proj_nn")
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return None, None, None, None


def proj_nn(xyz0, xyz1, K, patch_size):
    """Flat index (int64 [B,H,W]) of the xyz1 point closest to each xyz0 point inside the patch_size^2 patch
    around its projection with K; -1 where the patch falls outside the image."""
    return ProjNNFunction.apply(xyz0, xyz1, K, patch_size)


# --------------------------------------------------------------------------------------
# NCC volume (reference: XCorrVolFunction, functions.py:59-74)
# --------------------------------------------------------------------------------------
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
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    if algo == "fast" and not _ncc_fast_covers(in0.dtype, D, bs):
        algo = "exact"
    a = _ALGOS[algo]
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
        return _xcorrvol_impl(in0.unsqueeze(0), in1, n_disps, block_size, algo or _default_algo())[0]

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
    return _xcorrvol_impl(in0, in1, n_disps, block_size, algo or _default_algo(), prepared)


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
    st = _lib.lib().ctd_argmax_disp_f32(_ptr(v), _ptr(idx), _ptr(best), N, D, H, W, dev.index, _stream(dev))
    _lib.check(st, "argmax_disp")
    return (idx[0], best[0]) if squeeze else (idx, best)


def _check_prepared(prepared, who, a, in1, N, D, bs, dev):
    if (a != 1 or prepared.in1 is not in1 or prepared.n_frames != N or prepared.n_disps != D or prepared.block_size != bs
            or prepared.workspace.device != dev):
        raise RuntimeError("%s: `prepared` belongs to another pattern, frame count, shape or device "
                           "(or the call does not take the fast path)" % who)


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
    st = L.ctd_xcorrvol_pattern_prepare_f32(_ptr(in1), stride1, N, 1, H, W, D, bs, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "prepare_pattern")
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
    squeeze = in0.dim() == 3
    a0 = in0.unsqueeze(0) if squeeze else in0
    if a0.dim() != 4 or in1.dim() not in (3, 4):
        raise RuntimeError("xcorrvol_argmax expects in0 [N,1,H,W] or [1,H,W]")
    L = _lib.lib()
    dev = _same_device(a0, in1)
    N, C, H, W = a0.shape
    if tuple(in1.shape[-3:]) != (C, H, W):
        raise RuntimeError("in0 and in1 must have the same [C,H,W] shape")
    stride1 = 0 if in1.dim() == 3 else C * H * W
    D, bs = int(n_disps), int(block_size)
    algo = algo or _default_algo()
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    if algo == "fast" and not _ncc_fast_covers(a0.dtype, D, bs):
        algo = "exact"
    a = _ALGOS[algo]
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
    st = L.ctd_xcorrvol_argmax_f32(_ptr(a0), _ptr(in1), stride1, _ptr(vol), _ptr(idx), _ptr(best), N, C, H, W, D, bs,
                                   a_flag, float(rerank_eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "xcorrvol_argmax")
    if squeeze:
        idx, best = idx[0], best[0]
        vol = vol[0] if vol is not None else None
    return (idx, best, vol) if return_volume else (idx, best)


# --------------------------------------------------------------------------------------
# LCN (reference: networks.LCN.tforward, model/networks.py:523-533 -- not part of the
# reference's torchext; exposed here so the whole pre-normalisation is one kernel)
# --------------------------------------------------------------------------------------
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
    st = fn(_ptr(data), _ptr(y), _ptr(std), N, H, W, int(radius), float(epsilon), dev.index, _stream(dev))
    _lib.check(st, "lcn")
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
    st = L.ctd_lcn_xcorrvol_argmax_f32(_ptr(raw), _ptr(y), _ptr(std), int(radius), float(epsilon),
                                       0 if lcn_algo == "exact" else 1, _ptr(in1), stride1, _ptr(vol), _ptr(idx), _ptr(best),
                                       N, H, W, D, bs, a, float(rerank_eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "lcn_xcorrvol_argmax")
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
    st = _lib.lib().ctd_lcn_datagen_f32(_ptr(a), _ptr(out), _ptr(std), N, H, W, int(kernel_size), float(epsilon), dev.index,
                                        _stream(dev))
    _lib.check(st, "lcn_normalize")
    return (out[0], std[0]) if squeeze else (out, std)


# --------------------------------------------------------------------------------------
# Photometric block loss (reference: PhotometricLossFunction, functions.py:79-118)
# --------------------------------------------------------------------------------------
def _photo_args(es, ta):
    _check(es, "es")
    _check(ta, "ta")
    if es.dim() != 4 or es.shape != ta.shape or es.dtype != ta.dtype:
        raise RuntimeError("photometric_loss expects es and ta of the same [B,C,H,W] shape and dtype")
    return _same_device(es, ta)


def _photo_fast(es, block_size, algo):
    """algo 'fast' (default) = tolerance-level kernels (f32, odd block sizes up to 9); anything else they do not
    cover runs the reference-order kernels."""
    algo = algo or os.environ.get("CTD_PHOTO_ALGO", "fast")
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    return algo == "fast" and es.dtype == torch.float32 and int(block_size) in (3, 5, 7, 9)


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
        st = fn(_ptr(es), _ptr(ta), _ptr(out), B, C, H, W, int(block_size), int(type), float(eps), dev.index,
                _stream(dev))
        _lib.check(st, "photometric_loss_forward")
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
        st = fn(_ptr(es), _ptr(ta), _ptr(grad_out), _ptr(grad_es), B, C, H, W, int(ctx.block_size), int(ctx.type),
                float(ctx.eps), dev.index, _stream(dev))
        _lib.check(st, "photometric_loss_backward")
        return grad_es, None, None, None, None, None


_PHOTO_TYPES = {"mse": 0, "sad": 1, "census_mse": 2, "census_sad": 3}


def photometric_loss(es, ta, block_size, type='mse', eps=0.1, algo=None):
    """[B,C,H,W] x2 -> [B,1,H,W]: mean over a block_size^2 replicate-clamped block, summed over channels, of
    (es-ta)^2 | |es-ta| | soft-census squared / absolute difference.  Gradient flows to `es` only.
    algo (additive): 'fast' (default, or env CTD_PHOTO_ALGO) = tolerance-level kernels, ~10x faster for the census
    types; 'exact' = reference operation order, bit-identical to the reference CPU build."""
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')                  # functions.py:117
    return PhotometricLossFunction.apply(es, ta, block_size, _PHOTO_TYPES[type], eps, algo)


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
        st = L.ctd_pattern_loss_fwd_f32(_ptr(disp), _ptr(im), _ptr(mask), _ptr(pattern), _ptr(proj), _ptr(terms), B, H, W,
                                        int(type), float(eps), _ptr(ws), ws.numel(), dev.index, _stream(dev))
        _lib.check(st, "pattern_loss_forward")
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
        st = _lib.lib().ctd_pattern_loss_bwd_f32(_ptr(disp), _ptr(im), _ptr(mask), _ptr(pattern), _ptr(terms), _ptr(gv),
                                                 _ptr(gp), _ptr(grad_disp), B, H, W, ctx.type, ctx.eps, dev.index,
                                                 _stream(dev))
        _lib.check(st, "pattern_loss_backward")
        return grad_disp, None, None, None, None, None


def pattern_loss(disp, im, mask, pattern, type='census_sad', eps=0.5):
    """Fused pattern similarity loss: (val, pattern_proj, terms); gradient flows to `disp` only."""
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')
    return PatternLossFunction.apply(disp, im, mask, pattern, _PHOTO_TYPES[type], eps)


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
        st = L.ctd_pattern_loss_multi_fwd_f32(n, levels, _ptr(terms), int(type), float(eps), _ptr(ws), ws.numel(), dev.index,
                                              _stream(dev))
        _lib.check(st, "pattern_loss_multi_forward")
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
        st = _lib.lib().ctd_pattern_loss_multi_bwd_f32(n, levels, _ptr(terms), _ptr(gv), ctx.type, ctx.eps, dev.index,
                                                       _stream(dev))
        _lib.check(st, "pattern_loss_multi_backward")
        return (None, None, None) + tuple(grad_disps) + (None,) * (3 * n)


def pattern_loss_multi(disps, ims, masks, patterns, type='census_sad', eps=0.5):
    """Fused pattern similarity loss of several pyramid levels (lists of per-level tensors; masks may hold None)
    in one launch each way: (vals [n], terms [n,3], [pattern_proj per level])."""
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')
    n = len(disps)
    if not (len(ims) == len(masks) == len(patterns) == n) or n < 1 or n > 8:
        raise RuntimeError("pattern_loss_multi expects 1..8 levels with one disp, im, mask and pattern each")
    out = PatternLossMultiFunction.apply(_PHOTO_TYPES[type], eps, n, *[d.contiguous() for d in disps],
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


def costvol(im, pattern, n_disps, block_size, type='sad', eps=0.1, algo=None):
    """Additive: SAD / MSE / soft-census block cost volume between frames and the pattern shifted by d
    (SURVEY 8a/A6): cost[f,d] = photometric_loss(P_d, im[f]) with P_d[h,x] = P[h, clamp(x-d)].
    im [N,H,W] | [H,W] f32, pattern [H,W] | [N,H,W] -> [N,D,H,W] | [D,H,W]; argmin over d is the best match."""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')
    squeeze = im.dim() == 2
    a = im.unsqueeze(0) if squeeze else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("costvol expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]")
    dev = _same_device(a, pattern)
    N, H, W = a.shape
    stride = 0 if pattern.dim() == 2 else H * W
    D = int(n_disps)
    out = torch.empty((N, D, H, W), dtype=torch.float32, device=dev)
    L = _lib.lib()
    if _photo_fast(a, block_size, algo):
        # SAD / MSE, block 9: the separable path stages padded operand planes in a workspace (0 bytes: other kernels)
        nws = L.ctd_costvol_workspace_bytes(N, H, W, D, int(block_size), _PHOTO_TYPES[type], 1 if stride else 0)
        ws = _workspace(nws, dev) if nws else None
        st = L.ctd_costvol_fast_f32(_ptr(a), _ptr(pattern), stride, _ptr(out), N, H, W, D, int(block_size),
                                    _PHOTO_TYPES[type], float(eps), _ptr(ws), nws, dev.index, _stream(dev))
    else:
        st = L.ctd_costvol_f32(_ptr(a), _ptr(pattern), stride, _ptr(out), N, H, W, D, int(block_size),
                               _PHOTO_TYPES[type], float(eps), dev.index, _stream(dev))
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
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise Exception('invalid loss type')
    rerank_rel = float(rerank_rel)
    if rerank_rel != rerank_rel:
        raise RuntimeError("costvol_argmin: rerank_rel is NaN")
    squeeze = im.dim() == 2
    a = im.unsqueeze(0) if squeeze else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("costvol_argmin expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]")
    dev = _same_device(a, pattern)
    N, H, W = a.shape
    stride = 0 if pattern.dim() == 2 else H * W
    D, bs, ty = int(n_disps), int(block_size), _PHOTO_TYPES[type]
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


_SUBPIXEL_MODES = {"parabola": 0, "equiangular": 1}

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


def _subpixel_mode(mode, who):
    if mode not in _SUBPIXEL_MODES:
        raise RuntimeError("%s: unknown sub-pixel mode %r (parabola | equiangular)" % (who, mode))
    return _SUBPIXEL_MODES[mode]


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
    squeeze = in0.dim() == 3
    a0 = in0.unsqueeze(0) if squeeze else in0
    if a0.dim() != 4 or a0.shape[1] != 1 or in1.dim() not in (3, 4):
        raise RuntimeError("xcorrvol_subpixel expects in0 [N,1,H,W] or [1,H,W] and in1 [1,H,W] or [N,1,H,W]")
    dev = _same_device(a0, in1, idx)
    N, C, H, W = a0.shape
    if tuple(in1.shape[-3:]) != (C, H, W) or (in1.dim() == 4 and in1.shape[0] != N):
        raise RuntimeError("xcorrvol_subpixel: in1 does not match in0")
    if tuple(idx.shape) != ((H, W) if squeeze else (N, H, W)):
        raise RuntimeError("xcorrvol_subpixel: idx must be shaped as xcorrvol_argmax returns it")
    disp, refined = _subpixel_outputs(idx)
    stride1 = 0 if in1.dim() == 3 else H * W
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
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise RuntimeError("costvol_subpixel: invalid loss type %r" % (type,))
    squeeze = im.dim() == 2
    a = im.unsqueeze(0) if squeeze else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("costvol_subpixel expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]")
    dev = _same_device(a, pattern, idx)
    N, H, W = a.shape
    if pattern.dim() == 3 and pattern.shape[0] != N:
        raise RuntimeError("costvol_subpixel: pattern batch does not match im")
    if tuple(idx.shape) != tuple(im.shape):
        raise RuntimeError("costvol_subpixel: idx must be shaped as costvol_argmin returns it")
    disp, refined = _subpixel_outputs(idx)
    stride = 0 if pattern.dim() == 2 else H * W
    st = _lib.lib().ctd_costvol_subpixel_f32(_ptr(a), _ptr(pattern), stride, _ptr(idx), _ptr(disp), _ptr(refined), N, H,
                                             W, int(n_disps), int(block_size), _PHOTO_TYPES[type], float(eps), m,
                                             dev.index, _stream(dev))
    _lib.check(st, "costvol_subpixel")
    return disp, refined


xcorrvol_subpixel.__doc__ += _SUBPIXEL_RULE
costvol_subpixel.__doc__ += _SUBPIXEL_RULE


# --------------------------------------------------------------------------------------
# Band-limited matching: the best score within a per-pixel disparity range (additive; include/ctd_hip_band.h states
# the definition word for word)
# --------------------------------------------------------------------------------------
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
    squeeze = in0.dim() == 3
    a0 = in0.unsqueeze(0) if squeeze else in0
    if a0.dim() != 4 or a0.shape[1] != 1 or in1.dim() not in (3, 4):
        raise RuntimeError("%s expects in0 [N,1,H,W] or [1,H,W] and in1 [1,H,W] or [N,1,H,W]" % who)
    dev = _same_device(a0, in1)
    N, C, H, W = a0.shape
    if tuple(in1.shape[-3:]) != (C, H, W) or (in1.dim() == 4 and in1.shape[0] != N):
        raise RuntimeError("%s: in1 does not match in0" % who)
    shape = (H, W) if squeeze else (N, H, W)
    _band_range(lo, hi, shape, dev, who)
    return a0, shape, (0 if in1.dim() == 3 else H * W), dev


def _cost_band_inputs(im, pattern, lo, hi, type, who):
    """checks of the cost band ops -> (a [N,H,W], type code, pattern frame stride, device)"""
    _check(im, "im", (torch.float32,))
    _check(pattern, "pattern", (torch.float32,))
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise RuntimeError("%s: invalid loss type %r" % (who, type))
    squeeze = im.dim() == 2
    a = im.unsqueeze(0) if squeeze else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("%s expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]" % who)
    dev = _same_device(a, pattern)
    if pattern.dim() == 3 and pattern.shape[0] != a.shape[0]:
        raise RuntimeError("%s: pattern batch does not match im" % who)
    _band_range(lo, hi, im.shape, dev, who)
    return a, _PHOTO_TYPES[type], (0 if pattern.dim() == 2 else a.shape[1] * a.shape[2]), dev


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
    st = _lib.lib().ctd_costvol_argmin_band_f32(_ptr(a), _ptr(pattern), stride, _ptr(lo), _ptr(hi), _ptr(idx), _ptr(best),
                                                N, H, W, int(n_disps), int(block_size), ty, float(eps), dev.index,
                                                _stream(dev))
    _lib.check(st, who)
    return idx, best


xcorrvol_argmax_band.__doc__ += _BAND_RULE
costvol_argmin_band.__doc__ += _BAND_RULE


# --------------------------------------------------------------------------------------
# Match validity: left-right consistency and uniqueness (additive; include/ctd_hip.h states the rule word for word)
# --------------------------------------------------------------------------------------
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
    st = _lib.lib().ctd_costvol_band_validity_f32(_ptr(a), _ptr(pattern), stride, _ptr(lo), _ptr(hi), _ptr(idx),
                                                  _ptr(best), _ptr(flags), _ptr(idx_r), _ptr(gap), N, H, W, int(n_disps),
                                                  int(block_size), ty, float(eps), lr_tol, min_gap, dev.index,
                                                  _stream(dev))
    _lib.check(st, who)
    return idx, best, flags, idx_r, gap


xcorrvol_band_validity.__doc__ += _BAND_VALIDITY_RULE
costvol_band_validity.__doc__ += _BAND_VALIDITY_RULE


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
    st = _lib.lib().ctd_match_validity_f32(_ptr(v), 1 if maximise else 0, _ptr(idx), _ptr(flags), _ptr(idx_r), _ptr(gap),
                                           N, D, H, W, lr_tol, min_gap, dev.index, _stream(dev))
    _lib.check(st, "match_validity")
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
    squeeze = in0.dim() == 3
    a0 = in0.unsqueeze(0) if squeeze else in0
    if a0.dim() != 4 or in1.dim() not in (3, 4):
        raise RuntimeError("xcorrvol_validity expects in0 [N,C,H,W] or [C,H,W] and in1 [C,H,W] or [N,C,H,W]")
    dev = _same_device(a0, in1, idx)
    N, C, H, W = a0.shape
    if tuple(in1.shape[-3:]) != (C, H, W) or (in1.dim() == 4 and in1.shape[0] != N):
        raise RuntimeError("xcorrvol_validity: in1 does not match in0")
    if tuple(idx.shape) != ((H, W) if squeeze else (N, H, W)):
        raise RuntimeError("xcorrvol_validity: idx must be shaped as xcorrvol_argmax returns it")
    D, bs = int(n_disps), int(block_size)
    algo = algo or _default_algo()
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    if algo == "fast" and not (C == 1 and _ncc_fast_covers(a0.dtype, D, bs)):
        algo = "exact"
    a = _ALGOS[algo]
    stride1 = 0 if in1.dim() == 3 else C * H * W
    flags, idx_r, gap = _validity_outputs(idx)
    L = _lib.lib()
    ws = _workspace(L.ctd_xcorrvol_validity_workspace_bytes(N, C, H, W, D, bs, a), dev)
    st = L.ctd_xcorrvol_validity_f32(_ptr(a0), _ptr(in1), stride1, _ptr(idx), _ptr(flags), _ptr(idx_r), _ptr(gap), N, C, H,
                                     W, D, bs, a, lr_tol, min_gap, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "xcorrvol_validity")
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
    type = type.lower()
    if type not in _PHOTO_TYPES:
        raise RuntimeError("costvol_validity: invalid loss type %r" % (type,))
    squeeze = im.dim() == 2
    a = im.unsqueeze(0) if squeeze else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("costvol_validity expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]")
    dev = _same_device(a, pattern, idx)
    N, H, W = a.shape
    if pattern.dim() == 3 and pattern.shape[0] != N:
        raise RuntimeError("costvol_validity: pattern batch does not match im")
    if tuple(idx.shape) != tuple(im.shape):
        raise RuntimeError("costvol_validity: idx must be shaped as costvol_argmin returns it")
    D, bs, ty = int(n_disps), int(block_size), _PHOTO_TYPES[type]
    fast = 1 if _photo_fast(a, bs, algo) else 0
    stride = 0 if pattern.dim() == 2 else H * W
    flags, idx_r, gap = _validity_outputs(idx)
    L = _lib.lib()
    ws = _workspace(L.ctd_costvol_validity_workspace_bytes(N, H, W, D, bs, ty, fast, 1 if stride else 0), dev)
    st = L.ctd_costvol_validity_f32(_ptr(a), _ptr(pattern), stride, _ptr(idx), _ptr(flags), _ptr(idx_r), _ptr(gap), N, H, W,
                                    D, bs, ty, float(eps), fast, lr_tol, min_gap, _ptr(ws), ws.numel(), dev.index,
                                    _stream(dev))
    _lib.check(st, "costvol_validity")
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


# --------------------------------------------------------------------------------------
# Semi-global cost aggregation (additive; include/ctd_hip.h states the rule word for word)
# --------------------------------------------------------------------------------------
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
    st = L.ctd_sgm_aggregate_f32(_ptr(v), 1 if maximise else 0, p1, p2, paths, _ptr(S), _ptr(idx), _ptr(best), N, D, H, W,
                                 _ptr(ws), ws.numel() if ws is not None else 0, dev.index, _stream(dev))
    _lib.check(st, "sgm_aggregate")
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


# --------------------------------------------------------------------------------------
# Disparity post-filters (additive; include/ctd_hip.h states the rules word for word)
# --------------------------------------------------------------------------------------
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
    st = L.ctd_disp_components_f32(_ptr(d), _ptr(v), max_diff, connectivity, _ptr(label), _ptr(size), N, H, W, _ptr(ws),
                                   ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "disp_components")
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
    st = L.ctd_disp_speckle_f32(_ptr(d), _ptr(v), max_diff, int(max_size), connectivity, _ptr(keep), _ptr(size), N, H, W,
                                _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "disp_speckle")
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
    st = _lib.lib().ctd_disp_median_f32(_ptr(d), _ptr(v), int(window), int(fill_min), _ptr(out), _ptr(valid_out), N, H, W,
                                        dev.index, _stream(dev))
    _lib.check(st, "disp_median")
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


# --------------------------------------------------------------------------------------
# Multi-view depth consistency and point-cloud fusion (additive; include/ctd_hip.h states the rules word for word)
# --------------------------------------------------------------------------------------
_DEPTH_FUSION_RULE = """
    The rule (include/ctd_hip.h).  depth [B,V,H,W] f32 holds V views of each of B tracks; ray [H*W,3], K [3,3] as for
    `geometric_loss`; R [B,V,3,3], t [B,V,3] with X_cam = R X_world + t.  A pixel is live when its `valid` entry is
    nonzero (valid=None: everywhere) and its depth is finite and > 0.  A source view s != r is consistent with the live
    pixel p of view r when p, projected into s (the geometric projection u = uvd0 / uvd2, rounded to the nearest pixel),
    lands inside the image on a live pixel q, and q projected back with its own depth lands within max_px pixels of p at a
    depth z' with |z' - depth| <= max_rel * depth.  count = the number of consistent views, keep = live and
    count >= min_views, fused = (depth + the z' of the consistent views, ascending) / (1 + count), NaN where not kept."""


def _track_inputs(depth, ray, K, R, t, valid, who):
    """the tensors of a track of posed views -> (device, valid as uint8 or None)"""
    ts = [_f32(x, n) for x, n in ((depth, "depth"), (ray, "ray"), (K, "K"), (R, "R"), (t, "t"))]
    dev = _same_device(*ts)
    if depth.dim() != 4 or min(depth.shape[1:]) == 0:
        raise RuntimeError("%s expects depth [B,V,H,W] with V, H, W >= 1" % who)
    B, V, H, W = depth.shape
    if V > 64:
        raise RuntimeError("%s: at most 64 views" % who)
    if ray.numel() != H * W * 3 or K.numel() != 9 or R.numel() != B * V * 9 or t.numel() != B * V * 3:
        raise RuntimeError("%s: ray [H*W,3], K [3,3], R [B,V,3,3], t [B,V,3] expected" % who)
    v = None
    if valid is not None:
        _check(valid, "valid", (torch.bool, torch.uint8))
        if valid.shape != depth.shape:
            raise RuntimeError("%s: valid must have the shape of depth" % who)
        _same_device(depth, valid)
        v = valid.view(torch.uint8)
    return dev, v


def _depth_fusion_inputs(depth, ray, K, R, t, valid, max_px, max_rel, min_views, who):
    dev, v = _track_inputs(depth, ray, K, R, t, valid, who)
    if not all(isinstance(x, numbers.Real) and 0.0 <= x < float("inf") for x in (max_px, max_rel)):
        raise RuntimeError("%s: max_px and max_rel must be finite numbers >= 0" % who)
    max_px, max_rel = float(max_px), float(max_rel)
    if not isinstance(min_views, numbers.Real) or not 0 <= min_views <= 255 or int(min_views) != min_views:
        raise RuntimeError("%s: min_views must be an integer in [0, 255]" % who)
    return dev, v, max_px, max_rel, int(min_views)


def depth_consistency(depth, ray, K, R, t, valid=None, max_px=1.0, max_rel=0.01, min_views=1):
    """Additive: which depths of a track's views the other views confirm -> (count uint8, keep uint8, fused f32), each
    [B,V,H,W].  Not differentiable."""
    dev, v, max_px, max_rel, min_views = _depth_fusion_inputs(depth, ray, K, R, t, valid, max_px, max_rel, min_views,
                                                              "depth_consistency")
    B, V, H, W = depth.shape
    count = torch.empty(depth.shape, dtype=torch.uint8, device=dev)
    keep = torch.empty(depth.shape, dtype=torch.uint8, device=dev)
    fused = torch.empty(depth.shape, dtype=torch.float32, device=dev)
    if B == 0:
        return count, keep, fused
    st = _lib.lib().ctd_depth_consistency_f32(_ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t), max_px, max_rel,
                                              min_views, _ptr(count), _ptr(keep), _ptr(fused), B, V, H, W, dev.index,
                                              _stream(dev))
    _lib.check(st, "depth_consistency")
    return count, keep, fused


def depth_fuse_points(depth, ray, K, R, t, valid=None, max_px=1.0, max_rel=0.01, min_views=1, dedupe=True,
                      return_maps=False):
    """Additive: the fused world points of a track's depth maps -> (points [M,3] f32, src [M] int64, n_per_track [B]
    int64), and (count, keep, fused) of `depth_consistency` behind them with return_maps.  A kept pixel is emitted;
    with dedupe, only if no earlier view s < r is consistent with it and keeps the pixel it lands on ("first view
    wins").  point = (fused * ray[p] - t_r) @ R_r, src = the pixel's flat index ((b*V + r)*H + y)*W + x; the points come
    in ascending src order, so track b's are the n_per_track[b] entries after those of the tracks before it.  The counts
    are read back once (one synchronisation) to slice the outputs.  Not differentiable."""
    dev, v, max_px, max_rel, min_views = _depth_fusion_inputs(depth, ray, K, R, t, valid, max_px, max_rel, min_views,
                                                              "depth_fuse_points")
    B, V, H, W = depth.shape
    n = depth.numel()
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    src = torch.empty((n,), dtype=torch.int64, device=dev)
    n_per_track = torch.zeros((B,), dtype=torch.int64, device=dev)
    maps = ()
    if return_maps:
        maps = (torch.empty(depth.shape, dtype=torch.uint8, device=dev),
                torch.empty(depth.shape, dtype=torch.uint8, device=dev),
                torch.empty(depth.shape, dtype=torch.float32, device=dev))
    if B == 0:
        return (points, src, n_per_track) + maps
    mp = [_ptr(m) for m in maps] or [None] * 3
    L = _lib.lib()
    ws = _workspace(L.ctd_depth_fuse_workspace_bytes(B, V, H, W), dev)
    st = L.ctd_depth_fuse_points_f32(_ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t), max_px, max_rel, min_views,
                                     1 if dedupe else 0, _ptr(points), _ptr(src), _ptr(n_per_track), mp[0], mp[1], mp[2],
                                     B, V, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _lib.check(st, "depth_fuse_points")
    m = int(n_per_track.sum().item())
    return (points[:m], src[:m], n_per_track) + maps


depth_consistency.__doc__ += _DEPTH_FUSION_RULE
depth_fuse_points.__doc__ += _DEPTH_FUSION_RULE


# --------------------------------------------------------------------------------------
# Forward depth warping and the windowed band: from the views matched so far to the search range of the next one
# (additive; include/ctd_hip_warp.h states both definitions word for word)
# --------------------------------------------------------------------------------------
_DEPTH_WARP_RULE = """
    The definition (include/ctd_hip_warp.h).  depth, ray, K, R, t, valid and "live" are those of `depth_consistency`.
    For a target view r with targets[b,r] != 0, every live pixel q = (yq, xq) of every view s != r with
    sources[b,s] != 0 is transformed into r, uvd = transform(depth, ray[q], R_s, t_s, R_r, t_r, K) in the association of
    the consistency rule; it is dropped unless 0 < uvd2 < inf; xs = floor(uvd0 / uvd2 + 0.5), ys likewise (f32); it is
    dropped unless -splat <= xs <= W-1+splat and -splat <= ys <= H-1+splat (f32 compares, a NaN fails them); it is a
    candidate for every (ys+dy, xs+dx), |dy|, |dx| <= splat, inside the image.  At a target pixel the candidate with the
    smallest (z = uvd2, s*H*W + q) wins: z is its uvd2 bit for bit, src = ((b*V + s)*H + yq)*W + xq (the flat index of
    `depth_fuse_points`).  No candidate, targets[b,r] == 0 or V == 1: z = NaN, src = -1.  The winner is an unsigned
    minimum of (bits(z) << 32) | (s*H*W + q), so the same bits come out on every run.
    The nearest surface wins, so a gross foreground outlier in a source view wins too: pass valid = keep of
    `depth_consistency` for the views you warp from."""

_BAND_WINDOW_RULE = """
    The definition (include/ctd_hip_warp.h).  Over the window x window pixels around a pixel, clipped to the image, m
    and M are the minimum and the maximum of the finite priors.  With at least one: lo = clamp(ceil(m - radius), 0, D),
    hi = clamp(floor(M + radius), -1, D - 1), each one float32 subtraction / addition before the rounding.  With none:
    holes="empty" gives lo = D, hi = -1, holes="full" gives lo = 0, hi = D - 1.  A radius that is negative or NaN gives
    the empty band everywhere.  window=1, holes="empty" is `disparity_band(prior, radius, n_disps)` bit for bit."""

_BAND_HOLES = {"empty": 0, "full": 1}


def _view_mask(m, name, depth, who):
    """a [B,V] view mask as uint8 (None: all views); its dtype and shape are checked before any device is looked at"""
    if m is None:
        return None
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError("%s: %s must be a bool or uint8 tensor" % (who, name))
    if not isinstance(depth, torch.Tensor) or tuple(m.shape) != tuple(depth.shape[:2]):
        raise RuntimeError("%s: %s must be shaped [B,V] as depth [B,V,H,W]" % (who, name))
    return m.view(torch.uint8)


def depth_warp(depth, ray, K, R, t, valid=None, sources=None, targets=None, splat=0, return_src=False):
    """Additive: what every view of a track should look like given the track's other views -- a z-buffered forward warp
    -> z f32 [B,V,H,W] (NaN where nothing lands), and with return_src (z, src int64 [B,V,H,W]) (-1 there).
    sources, targets: bool / uint8 [B,V] or None (all): the views warped from and the views warped into (warp views
    0..k-1 into view k with sources[:, :k] and targets[:, k] set).  splat 0, 1 or 2: every source pixel covers the
    (2*splat+1)^2 pixels around where it lands, which closes the cracks between splats.  Not differentiable."""
    who = "depth_warp"
    if isinstance(splat, bool) or not isinstance(splat, numbers.Integral) or not 0 <= splat <= 2:
        raise RuntimeError("%s: splat must be 0, 1 or 2" % who)
    ms = _view_mask(sources, "sources", depth, who)
    mt = _view_mask(targets, "targets", depth, who)
    dev, v = _track_inputs(depth, ray, K, R, t, valid, who)
    B, V, H, W = depth.shape
    for m, name in ((ms, "sources"), (mt, "targets")):
        if m is not None:
            _check(m, name, (torch.uint8,))
            _same_device(depth, m)
    z = torch.empty(depth.shape, dtype=torch.float32, device=dev)
    src = torch.empty(depth.shape, dtype=torch.int64, device=dev) if return_src else None
    if B > 0:
        L = _lib.lib()
        ws = _workspace(L.ctd_depth_warp_workspace_bytes(B, V, H, W), dev)
        st = L.ctd_depth_warp_f32(_ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t), _ptr(ms), _ptr(mt), int(splat),
                                  _ptr(z), _ptr(src), B, V, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
        _lib.check(st, who)
    return (z, src) if return_src else z


def disparity_band_window(prior, radius, n_disps, window=3, holes="full"):
    """Additive: the search range [lo, hi] (int32, shaped as `prior`, inclusive) of the band matchers around a disparity
    prior that has holes and occlusion edges, such as `depth_to_disp(depth_warp(...))`: the band of a pixel spans every
    finite prior of its window, so an edge keeps both the foreground and the background disparity and a crack is
    filled from its neighbours.  prior f32 [N,H,W] | [H,W] on the GPU; radius a float; window odd, 1..15; holes "full"
    (a window without any finite prior searches everything) | "empty" (it searches nothing: idx -1)."""
    who = "disparity_band_window"
    if isinstance(window, bool) or not isinstance(window, numbers.Integral) or not 1 <= window <= 15 or window % 2 == 0:
        raise RuntimeError("%s: window must be an odd integer in [1, 15]" % who)
    if holes not in _BAND_HOLES:
        raise RuntimeError("%s: holes must be 'full' or 'empty', not %r" % (who, holes))
    if isinstance(n_disps, bool) or not isinstance(n_disps, numbers.Integral) or n_disps < 1:
        raise RuntimeError("%s: n_disps must be an integer >= 1" % who)
    if not isinstance(radius, numbers.Real):
        raise RuntimeError("%s: radius must be a number" % who)
    if not isinstance(prior, torch.Tensor) or prior.dtype != torch.float32:
        raise RuntimeError("%s: prior must be a float32 tensor" % who)
    if prior.dim() not in (2, 3) or min(prior.shape[-2:]) == 0:
        raise RuntimeError("%s expects prior [N,H,W] or [H,W] with H, W >= 1" % who)
    _check(prior, "prior", (torch.float32,))
    dev = prior.device
    H, W = prior.shape[-2:]
    N = prior.shape[0] if prior.dim() == 3 else 1
    lo = torch.empty(prior.shape, dtype=torch.int32, device=dev)
    hi = torch.empty(prior.shape, dtype=torch.int32, device=dev)
    if N > 0:
        st = _lib.lib().ctd_disparity_band_window_f32(_ptr(prior), float(radius), int(n_disps), int(window),
                                                      _BAND_HOLES[holes], _ptr(lo), _ptr(hi), N, H, W, dev.index,
                                                      _stream(dev))
        _lib.check(st, who)
    return lo, hi


def depth_to_disp(depth, baseline_focal, disp_offset=0.0):
    """Additive: the inverse of `idx_to_depth`, `baseline_focal / depth - disp_offset` in float32 (one division, one
    subtraction), NaN where depth is not finite and > 0 -- so the holes of `depth_warp` stay holes.  Pure torch, any
    device.  Not differentiable."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32:
        raise RuntimeError("depth_to_disp: depth must be a float32 tensor")
    with torch.no_grad():
        live = torch.isfinite(depth) & (depth > 0)
        d = torch.where(live, depth, torch.ones_like(depth))
        disp = torch.full_like(d, float(baseline_focal)) / d - float(disp_offset)
        return torch.where(live, disp, torch.full_like(disp, float("nan")))


depth_warp.__doc__ += _DEPTH_WARP_RULE
disparity_band_window.__doc__ += _BAND_WINDOW_RULE


# --------------------------------------------------------------------------------------
# Depth-map normals and projective point-to-plane ICP: from slightly wrong poses back to ones that the consistency check
# confirms (additive; include/ctd_hip_icp.h states the three rules word for word)
# --------------------------------------------------------------------------------------
_DEPTH_NORMALS_RULE = """
    The rule (include/ctd_hip_icp.h).  depth, ray, valid and "live" are those of `depth_consistency`.  A pixel (y, x)
    with 1 <= x <= W-2, 1 <= y <= H-2 gets a normal when it and its four axis neighbours are live and every neighbour's
    depth satisfies |d_nb - d| <= max_rel * d.  P(q) = d(q) * ray[q]; a = P(y,x+1) - P(y,x-1), b = P(y+1,x) - P(y-1,x);
    c = a x b, each component as a1*b2 - a2*b1; l = sqrt(c0*c0 + c1*c1 + c2*c2); no normal unless 0 < l < inf; n = c / l,
    negated when n . P(y,x) > 0, so that it faces the camera.  Every other pixel gets three NaNs.  All float32,
    uncontracted, no atomics: the same bits on every run."""

_DEPTH_ICP_RULE = """
    The rule (include/ctd_hip_icp.h).  depth, ray, K, R, t, valid and "live" are those of `depth_consistency`; normal is
    `depth_normals(depth, ray, valid)`.  View s of track b is aligned to view a = target[b,s] (int32 [B,V]; None: every
    view s >= 1 to view 0); a value outside 0..V-1 or equal to s skips the view: a system of zeros, residual NaN,
    assoc -1, pose unchanged.  A live pixel q of view s gives S, its point in the frame of camera a, and uvd = K S (the
    products and sums of the consistency rule); it is dropped unless uvd2 > 0, unless xs = floor(uvd0 / uvd2 + 0.5),
    ys likewise, lie inside the image, unless p = ys*W + xs is live in view a and normal[b,a,p] is finite, and unless
    D = S - d_a(p) * ray[p] has |D|^2 <= max_dist^2.  Then n = normal[b,a,p], e = n . D and J = (S x n, n).
    system float64 [B,V,29] = the 21 upper-triangle entries of sum J J^T (row-major), the 6 of sum J e, sum e^2 and the
    count; every product is exact in float64 and the order of every sum is fixed: the same bits on every run.
    residual = e, assoc = ((b*V + a)*H + ys)*W + xs, NaN / -1 where the pixel was dropped.
    The update, one view at a time in float64: A from the triangle with A_ii += damping * A_ii, factored L D L^T; the
    view is left unchanged (R' = R, t' = t bit for bit, ok = 0) when it is skipped, when count < min_count, or when a
    pivot is not finite or <= min_pivot * A_ii (A_ii undamped) -- the sign of a surface that does not constrain all six
    degrees of freedom, a single plane for one.  Otherwise xi = (omega, v) = -A^-1 g, Rr = exp([omega]x) by Rodrigues
    (the series below an angle of 1e-4), tr = v, and the new pose of s is the one for which every S becomes Rr S + tr
    while view a stays: [R_a|t_a] [R_s'|t_s']^-1 = [Rr|tr] [R_a|t_a] [R_s|t_s]^-1, rounded to float32 once; ok = 1.  R is
    not re-orthonormalised."""


def _icp_number(x, name, who):
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not 0.0 <= x < float("inf"):
        raise RuntimeError("%s: %s must be a finite number >= 0" % (who, name))
    return float(x)


def _icp_count(x, name, who, lo=0):
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not lo <= x < 2 ** 31:
        raise RuntimeError("%s: %s must be an integer >= %d" % (who, name, lo))
    return int(x)


def _icp_target(target, B, V, dev, who):
    """target as int32 [B,V] on the device of the track (None stays None: every view s >= 1 to view 0)"""
    if target is None:
        return None
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int32:
        raise RuntimeError("%s: target must be an int32 tensor" % who)
    if tuple(target.shape) != (B, V):
        raise RuntimeError("%s: target must be shaped [B,V]" % who)
    _check(target, "target", (torch.int32,))
    if target.device != dev:
        raise RuntimeError("all tensors must be on the same device (%s vs %s)" % (dev, target.device))
    return target


def _icp_normal(normal, depth, who):
    _f32(normal, "normal")
    if not isinstance(depth, torch.Tensor) or tuple(normal.shape) != tuple(depth.shape) + (3,):
        raise RuntimeError("%s: normal must be shaped [B,V,H,W,3] as depth [B,V,H,W]" % who)
    return normal


def depth_normals(depth, ray, valid=None, max_rel=0.02):
    """Additive: the surface normal at every pixel of a track's depth maps, in the frame of the pixel's own camera and
    facing it -> normal f32 [B,V,H,W,3], three NaNs where a pixel has none (the image border, holes, depth edges).  With
    the points `depth[..., None] * ray` these are the oriented points a mesher takes.  Not differentiable."""
    who = "depth_normals"
    max_rel = _icp_number(max_rel, "max_rel", who)
    ts = [_f32(depth, "depth"), _f32(ray, "ray")]
    dev = _same_device(*ts)
    if depth.dim() != 4 or min(depth.shape[1:]) == 0:
        raise RuntimeError("%s expects depth [B,V,H,W] with V, H, W >= 1" % who)
    B, V, H, W = depth.shape
    if V > 64:
        raise RuntimeError("%s: at most 64 views" % who)
    if ray.numel() != H * W * 3:
        raise RuntimeError("%s: ray [H*W,3] expected" % who)
    v = None
    if valid is not None:
        _check(valid, "valid", (torch.bool, torch.uint8))
        if valid.shape != depth.shape:
            raise RuntimeError("%s: valid must have the shape of depth" % who)
        _same_device(depth, valid)
        v = valid.view(torch.uint8)
    normal = torch.empty(tuple(depth.shape) + (3,), dtype=torch.float32, device=dev)
    if B > 0:
        st = _lib.lib().ctd_depth_normals_f32(_ptr(depth), _ptr(v), _ptr(ray), max_rel, _ptr(normal), B, V, H, W, dev.index,
                                              _stream(dev))
        _lib.check(st, who)
    return normal


def _icp_system_call(depth, v, normal, ray, K, R, t, target, max_dist, return_maps, dev, who):
    """one launch of the system on validated inputs -> (system, residual or None, assoc or None)"""
    B, V, H, W = depth.shape
    system = torch.empty((B, V, 29), dtype=torch.float64, device=dev)
    residual = torch.empty(depth.shape, dtype=torch.float32, device=dev) if return_maps else None
    assoc = torch.empty(depth.shape, dtype=torch.int64, device=dev) if return_maps else None
    if B > 0:
        L = _lib.lib()
        ws = _workspace(L.ctd_depth_icp_workspace_bytes(B, V, H, W), dev)
        st = L.ctd_depth_icp_system_f32(_ptr(depth), _ptr(v), _ptr(normal), _ptr(ray), _ptr(K), _ptr(R), _ptr(t),
                                        _ptr(target), max_dist, _ptr(system), _ptr(residual), _ptr(assoc), B, V, H, W,
                                        _ptr(ws), ws.numel(), dev.index, _stream(dev))
        _lib.check(st, who)
    return system, residual, assoc


def _icp_pose_shapes(R, t, B, V, who):
    """R [B,V,3,3] and t [B,V,3] exactly: the update sizes its launch and its outputs by them"""
    if not isinstance(R, torch.Tensor) or not isinstance(t, torch.Tensor) or tuple(R.shape) != (B, V, 3, 3) or \
            tuple(t.shape) != (B, V, 3):
        raise RuntimeError("%s: R must be shaped [B,V,3,3] and t [B,V,3]" % who)


def _icp_update_call(system, R, t, target, min_count, min_pivot, damping, B, V, dev, who):
    """one launch of the update on validated inputs: system [B,V,29], R [B,V,3,3], t [B,V,3]"""
    R_out, t_out = torch.empty_like(R), torch.empty_like(t)
    ok = torch.empty((B, V), dtype=torch.uint8, device=dev)
    if B > 0:
        st = _lib.lib().ctd_depth_icp_update_f32(_ptr(system), _ptr(R), _ptr(t), _ptr(target), min_count, min_pivot, damping,
                                                 _ptr(R_out), _ptr(t_out), _ptr(ok), B, V, dev.index, _stream(dev))
        _lib.check(st, who)
    return R_out, t_out, ok


def depth_icp_system(depth, normal, ray, K, R, t, valid=None, target=None, max_dist=0.1, return_maps=False):
    """Additive: the normal equations of one round of projective point-to-plane ICP that aligns views of a track to
    other views of it -> system float64 [B,V,29], and with return_maps (system, residual f32 [B,V,H,W], assoc int64
    [B,V,H,W]).  Feed it to `depth_icp_update`; `depth_icp` runs both in a loop.  Not differentiable."""
    who = "depth_icp_system"
    max_dist = _icp_number(max_dist, "max_dist", who)
    dev, v = _track_inputs(depth, ray, K, R, t, valid, who)
    B, V = depth.shape[:2]
    _icp_normal(normal, depth, who)
    _same_device(depth, normal)
    target = _icp_target(target, B, V, dev, who)
    system, residual, assoc = _icp_system_call(depth, v, normal, ray, K, R, t, target, max_dist, return_maps, dev, who)
    return (system, residual, assoc) if return_maps else system


def _icp_update_inputs(system, R, t, target, who):
    _check(system, "system", (torch.float64,))
    dev = _same_device(system, _f32(R, "R"), _f32(t, "t"))
    if R.dim() != 4 or tuple(R.shape[2:]) != (3, 3) or R.shape[1] == 0:
        raise RuntimeError("%s expects R [B,V,3,3] with V >= 1" % who)
    B, V = R.shape[:2]
    if V > 64:
        raise RuntimeError("%s: at most 64 views" % who)
    if tuple(t.shape) != (B, V, 3) or tuple(system.shape) != (B, V, 29):
        raise RuntimeError("%s: system [B,V,29], R [B,V,3,3], t [B,V,3] expected" % who)
    return dev, B, V, _icp_target(target, B, V, dev, who)


def depth_icp_update(system, R, t, target=None, min_count=64, min_pivot=1e-4, damping=0.0):
    """Additive: solves the systems of `depth_icp_system` and moves the poses -> (R' f32 [B,V,3,3], t' f32 [B,V,3],
    ok uint8 [B,V]); R and t are not written.  `target` must be the one the system was built with.  Not
    differentiable."""
    who = "depth_icp_update"
    min_count = _icp_count(min_count, "min_count", who)
    min_pivot = _icp_number(min_pivot, "min_pivot", who)
    damping = _icp_number(damping, "damping", who)
    dev, B, V, target = _icp_update_inputs(system, R, t, target, who)
    return _icp_update_call(system, R, t, target, min_count, min_pivot, damping, B, V, dev, who)


def depth_icp(depth, ray, K, R, t, valid=None, target=None, iters=10, max_rel=0.02, max_dist=0.1, min_count=64,
              min_pivot=1e-4, damping=0.0):
    """Additive: refines the poses of a track's views by projective point-to-plane ICP between its depth maps
    -> (R' f32 [B,V,3,3], t' f32 [B,V,3], info).  `depth_normals(depth, ray, valid, max_rel)` once, then `iters` rounds of
    `depth_icp_system` and `depth_icp_update` on the current stream, without any host synchronisation.  info, all device
    tensors: "count" and "rmse" float64 [iters,B,V], the number of pixels and sqrt(sum e^2 / count) of the system each
    round solved (NaN where the count is 0), and "ok" uint8 [B,V] of the last round.  target=None aligns every view
    s >= 1 to view 0.  It converges from errors of a few degrees and centimetres on surfaces that constrain all six degrees
    of freedom; on a single plane every round leaves the poses as they are (ok = 0).  Not differentiable."""
    who = "depth_icp"
    iters = _icp_count(iters, "iters", who, 1)
    max_rel = _icp_number(max_rel, "max_rel", who)
    max_dist = _icp_number(max_dist, "max_dist", who)
    min_count = _icp_count(min_count, "min_count", who)
    min_pivot = _icp_number(min_pivot, "min_pivot", who)
    damping = _icp_number(damping, "damping", who)
    if isinstance(depth, torch.Tensor) and depth.dim() == 4:              # (anything else: _track_inputs says so)
        _icp_pose_shapes(R, t, depth.shape[0], depth.shape[1], who)
    dev, v = _track_inputs(depth, ray, K, R, t, valid, who)
    B, V = depth.shape[:2]
    target = _icp_target(target, B, V, dev, who)
    normal = depth_normals(depth, ray, valid, max_rel)
    systems = []
    ok = torch.zeros((B, V), dtype=torch.uint8, device=dev)
    for _ in range(iters):
        system = _icp_system_call(depth, v, normal, ray, K, R, t, target, max_dist, False, dev, who)[0]
        R, t, ok = _icp_update_call(system, R, t, target, min_count, min_pivot, damping, B, V, dev, who)
        systems.append(system)
    systems = torch.stack(systems)
    count = systems[..., 28]
    return R, t, {"count": count, "rmse": torch.sqrt(systems[..., 27] / count), "ok": ok}


depth_normals.__doc__ += _DEPTH_NORMALS_RULE
depth_icp_system.__doc__ += _DEPTH_ICP_RULE
depth_icp_update.__doc__ += _DEPTH_ICP_RULE
depth_icp.__doc__ += _DEPTH_ICP_RULE


# --------------------------------------------------------------------------------------
# Truncated signed distance volumes: a track's views fused into one surface per track, its points, and a ray cast of
# it into a depth map at any pose (additive; include/ctd_hip_tsdf.h states the three rules word for word)
# --------------------------------------------------------------------------------------
_TSDF_RULE = """
    The rules (include/ctd_hip_tsdf.h).  tsdf and weight are f32 [B,nz,ny,nx], x fastest, one grid per track; origin
    f32 [B,3] is the centre of voxel (0,0,0) and voxel the edge, so the centre of voxel (i,j,k) is origin + voxel *
    (i,j,k).  A fresh volume has weight == 0 everywhere, and tsdf is never read where weight == 0.
    Integrate: for each voxel and the views v ascending, S = R_v X + t_v, uvd = K S; the view is skipped unless uvd2 > 0,
    unless xs = floor(uvd0 / uvd2 + 0.5), ys likewise, lie inside the image and q = ys*W + xs is live (valid nonzero,
    depth finite and > 0), and if sdf = depth[q] * ray[q][2] - S2 < -trunc.  obs = min(1, sdf / trunc); tsdf = obs where
    weight == 0, else (tsdf * weight + obs) / (weight + 1); weight = min(weight + 1, max_weight).
    Surface points: a voxel is usable when weight >= min_weight and |tsdf| < 1; for a voxel a and its +c neighbour n,
    both usable with (T_a < 0) != (T_n < 0), the point is the centre of a with component c increased by
    voxel * (T_a / (T_a - T_n)) and src = (((b*nz + k)*ny + j)*nx + i)*3 + c, ascending.  The normal is the central
    difference g_c = T(+c) - T(-c) at whichever of a and n has the smaller |T| (a on a tie), g / |g|, towards free
    space; three NaNs when a neighbour is outside the grid or has weight < min_weight or |g| == 0.
    Ray cast: the samples d_n = d_min + step * n, n < n_steps, of pixel p at X = (d_n * ray[p] - t) @ R; a sample is
    defined when its cell lies inside the grid and its eight corners have weight >= min_weight, its value is trilinear
    (x, then y, then z).  At the first defined sample with T_n <= 0 the ray stops: the depth is
    d_{n-1} + step * (T_{n-1} / (T_{n-1} - T_n)) when sample n-1 was defined with T_{n-1} > 0, else NaN; NaN too when
    no such sample exists.  All float32, uncontracted, no atomics: the same bits on every run."""


def _tsdf_number(x, name, who, lo_open=True, lo=0.0):
    """a finite number > lo (lo_open) or >= lo"""
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not (lo < x if lo_open else lo <= x) or \
            not x < float("inf"):
        raise RuntimeError("%s: %s must be a finite number %s %g" % (who, name, ">" if lo_open else ">=", lo))
    return float(x)


def _tsdf_inputs(tsdf, weight, origin, voxel, who):
    """the tensors of a volume -> (device, B, nx, ny, nz, voxel)"""
    voxel = _tsdf_number(voxel, "voxel", who)
    dev = _same_device(_f32(tsdf, "tsdf"), _f32(weight, "weight"), _f32(origin, "origin"))
    if tsdf.dim() != 4 or min(tsdf.shape[1:]) == 0 or weight.shape != tsdf.shape:
        raise RuntimeError("%s expects tsdf and weight [B,nz,ny,nx] with nx, ny, nz >= 1" % who)
    B, nz, ny, nx = tsdf.shape
    if max(nx, ny, nz) > 2048:
        raise RuntimeError("%s: at most 2048 voxels along an axis" % who)
    if tuple(origin.shape) != (B, 3):
        raise RuntimeError("%s: origin must be shaped [B,3]" % who)
    return dev, B, nx, ny, nz, voxel


def tsdf_volume(B, nx, ny, nz, device="cuda"):
    """Additive: a fresh volume for `tsdf_integrate` -> (tsdf f32 [B,nz,ny,nx] filled with 1, weight f32 [B,nz,ny,nx]
    filled with 0)."""
    who = "tsdf_volume"
    B = _icp_count(B, "B", who)
    nx, ny, nz = (_icp_count(n, name, who, 1) for n, name in ((nx, "nx"), (ny, "ny"), (nz, "nz")))
    if max(nx, ny, nz) > 2048:
        raise RuntimeError("%s: at most 2048 voxels along an axis" % who)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("%s: a CUDA device is needed (connecting_the_dots_amd has no CPU path)" % who)
    return (torch.ones((B, nz, ny, nx), dtype=torch.float32, device=device),
            torch.zeros((B, nz, ny, nx), dtype=torch.float32, device=device))


def tsdf_integrate(tsdf, weight, origin, voxel, depth, ray, K, R, t, valid=None, trunc=None, max_weight=64.0):
    """Additive: integrates the V views of each track into the track's volume, in place, in one launch -> (tsdf,
    weight), the tensors passed in.  trunc=None stands for 4 * voxel.  Pass the `keep` of `depth_consistency` as
    `valid`: gross outliers that reach the volume bias it, and the fused surface then is worse than the raw points.
    Integrating views {0,1} and then {2,3} gives the bits of one call over {0,1,2,3}.  Not differentiable."""
    who = "tsdf_integrate"
    max_weight = _tsdf_number(max_weight, "max_weight", who, False, 1.0)
    if trunc is not None:
        trunc = _tsdf_number(trunc, "trunc", who)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    if trunc is None:
        trunc = 4.0 * voxel
    _, v = _track_inputs(depth, ray, K, R, t, valid, who)
    _same_device(tsdf, depth)
    if depth.shape[0] != B:
        raise RuntimeError("%s: depth [B,V,H,W] must have the B of tsdf [B,nz,ny,nx]" % who)
    V, H, W = depth.shape[1:]
    if B > 0:
        st = _lib.lib().ctd_tsdf_integrate_f32(_ptr(tsdf), _ptr(weight), _ptr(origin), voxel, _ptr(depth), _ptr(v), _ptr(ray),
                                               _ptr(K), _ptr(R), _ptr(t), trunc, max_weight, B, nx, ny, nz, V, H, W,
                                               dev.index, _stream(dev))
        _lib.check(st, who)
    return tsdf, weight


def tsdf_surface_points(tsdf, weight, origin, voxel, min_weight=1.0, return_normals=False):
    """Additive: the zero crossings of a volume between neighbouring voxels -> (points [M,3] f32, src [M] int64,
    n_per_track [B] int64), and normals [M,3] f32 behind them with return_normals.  The points come in ascending src
    order, so track b's are the n_per_track[b] entries after those of the tracks before it.  One call counts, the
    counts are read back once (one synchronisation) to size the outputs, a second call fills them.  Not
    differentiable."""
    who = "tsdf_surface_points"
    min_weight = _tsdf_number(min_weight, "min_weight", who)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    n_per_track = torch.zeros((B,), dtype=torch.int64, device=dev)
    m = 0
    L = _lib.lib()
    if B > 0:
        ws = _workspace(L.ctd_tsdf_surface_workspace_bytes(B, nx, ny, nz), dev)

        def call(points, normals, src, capacity):
            st = L.ctd_tsdf_surface_points_f32(_ptr(tsdf), _ptr(weight), _ptr(origin), voxel, min_weight, _ptr(points),
                                               _ptr(normals), _ptr(src), _ptr(n_per_track), capacity, B, nx, ny, nz, _ptr(ws),
                                               ws.numel(), dev.index, _stream(dev))
            _lib.check(st, who)

        call(None, None, None, 0)
        m = int(n_per_track.sum().item())
    points = torch.empty((m, 3), dtype=torch.float32, device=dev)
    src = torch.empty((m,), dtype=torch.int64, device=dev)
    normals = torch.empty((m, 3), dtype=torch.float32, device=dev) if return_normals else None
    if m > 0:
        call(points, normals, src, m)
    return (points, src, n_per_track) + ((normals,) if return_normals else ())


def tsdf_raycast(tsdf, weight, origin, voxel, ray, R, t, H, W, d_min, step, n_steps, min_weight=1.0):
    """Additive: the depth maps of a volume seen from the poses R [B,V,3,3], t [B,V,3] (any poses, not only those
    integrated) -> depth f32 [B,V,H,W], NaN where the ray finds no surface.  A map without the holes of `depth_warp`:
    put it in front of a track's views as view 0 and `depth_icp` aligns them to the model, or send it through
    `depth_to_disp` into `disparity_band_window` as a band prior.  `depth_normals` of the output gives the model's
    normals.  Not differentiable."""
    who = "tsdf_raycast"
    H, W = _icp_count(H, "H", who, 1), _icp_count(W, "W", who, 1)
    n_steps = _icp_count(n_steps, "n_steps", who, 1)
    d_min = _tsdf_number(d_min, "d_min", who, False)
    step = _tsdf_number(step, "step", who)
    min_weight = _tsdf_number(min_weight, "min_weight", who)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    _same_device(tsdf, _f32(ray, "ray"), _f32(R, "R"), _f32(t, "t"))
    if R.dim() != 4 or tuple(R.shape[2:]) != (3, 3) or R.shape[0] != B or R.shape[1] == 0 or \
            tuple(t.shape) != tuple(R.shape[:2]) + (3,):
        raise RuntimeError("%s: R must be shaped [B,V,3,3] and t [B,V,3] with V >= 1 and the B of tsdf" % who)
    V = R.shape[1]
    if V > 64:
        raise RuntimeError("%s: at most 64 views" % who)
    if ray.numel() != H * W * 3:
        raise RuntimeError("%s: ray [H*W,3] expected" % who)
    depth = torch.empty((B, V, H, W), dtype=torch.float32, device=dev)
    if B > 0:
        st = _lib.lib().ctd_tsdf_raycast_f32(_ptr(tsdf), _ptr(weight), _ptr(origin), voxel, _ptr(ray), _ptr(R), _ptr(t), d_min,
                                             step, n_steps, min_weight, _ptr(depth), B, nx, ny, nz, V, H, W, dev.index,
                                             _stream(dev))
        _lib.check(st, who)
    return depth


tsdf_integrate.__doc__ += _TSDF_RULE
tsdf_surface_points.__doc__ += _TSDF_RULE
tsdf_raycast.__doc__ += _TSDF_RULE


# --------------------------------------------------------------------------------------
# Fused loss kernels (reference: stock-PyTorch modules of model/networks.py; additive API)
# --------------------------------------------------------------------------------------
def _f32(t, name):
    _check(t, name, (torch.float32,))
    return t


class DispToDepthFunction(torch.autograd.Function):
    """depth = baseline_focal / (relu(disp) + 1e-12)   (networks.DispToDepth.tforward, networks.py:318-321)"""

    @staticmethod
    def forward(ctx, disp, baseline_focal):
        disp = _f32(disp.contiguous(), "disp")
        ctx.save_for_backward(disp)
        ctx.bf = float(baseline_focal)
        depth = torch.empty_like(disp)
        dev = disp.device
        st = _lib.lib().ctd_disp_to_depth_fwd_f32(_ptr(disp), _ptr(depth), disp.numel(), ctx.bf, dev.index, _stream(dev))
        _lib.check(st, "disp_to_depth")
        return depth

    @staticmethod
    def backward(ctx, grad_depth):
        (disp,) = ctx.saved_tensors
        grad_depth = _f32(grad_depth.contiguous(), "grad_depth")
        grad = torch.empty_like(disp)
        dev = disp.device
        st = _lib.lib().ctd_disp_to_depth_bwd_f32(_ptr(disp), _ptr(grad_depth), _ptr(grad), disp.numel(), ctx.bf,
                                                  dev.index, _stream(dev))
        _lib.check(st, "disp_to_depth backward")
        return grad, None


def disp_to_depth(disp, baseline_focal):
    return DispToDepthFunction.apply(disp, baseline_focal)


def idx_to_depth(idx, baseline_focal, disp_offset=0.0):
    """Additive: depth of the int64 disparity indices `xcorrvol_argmax` returns, `baseline_focal / (relu(idx +
    disp_offset) + 1e-12)`, same shape as `idx` (f32).  Not differentiable."""
    _check(idx, "idx", (torch.int64,))
    depth = torch.empty(idx.shape, dtype=torch.float32, device=idx.device)
    dev = idx.device
    st = _lib.lib().ctd_idx_to_depth_f32(_ptr(idx), _ptr(depth), idx.numel(), float(baseline_focal), float(disp_offset),
                                         dev.index, _stream(dev))
    _lib.check(st, "idx_to_depth")
    return depth


class DisparityLossFunction(torch.autograd.Function):
    """Sobel 5x5 + edge-aware disparity loss (networks.DisparityLoss.tforward, networks.py:395-412) -> scalar."""

    @staticmethod
    def forward(ctx, disp, edge):
        disp = _f32(disp.contiguous(), "disp")
        if disp.dim() != 4 or disp.shape[1] != 1:
            raise RuntimeError("disparity_loss expects disp [B,1,H,W]")
        if edge is not None:
            edge = _f32(edge.contiguous(), "edge")
            if edge.shape != disp.shape:
                raise RuntimeError("edge must have the shape of disp")
            _same_device(disp, edge)
        B, _, H, W = disp.shape
        dev = disp.device
        L = _lib.lib()
        ws = _workspace(L.ctd_disparity_loss_workspace_bytes(B, H, W), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        st = L.ctd_disparity_loss_fwd_f32(_ptr(disp), _ptr(edge), _ptr(loss), B, H, W, _ptr(ws), ws.numel(), dev.index,
                                          _stream(dev))
        _lib.check(st, "disparity_loss")
        ctx.save_for_backward(disp, edge)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        disp, edge = ctx.saved_tensors
        B, _, H, W = disp.shape
        dev = disp.device
        L = _lib.lib()
        ws = _workspace(L.ctd_disparity_loss_workspace_bytes(B, H, W), dev)
        gl = grad_loss.to(torch.float32).contiguous()
        grad_disp = torch.empty_like(disp)
        want_edge = edge is not None and ctx.needs_input_grad[1]
        grad_edge = torch.empty_like(edge) if want_edge else None
        st = L.ctd_disparity_loss_bwd_f32(_ptr(disp), _ptr(edge), _ptr(gl), _ptr(grad_disp), _ptr(grad_edge), B, H, W,
                                          _ptr(ws), ws.numel(), dev.index, _stream(dev))
        _lib.check(st, "disparity_loss backward")
        return grad_disp, grad_edge


def disparity_loss(disp, edge=None):
    return DisparityLossFunction.apply(disp, edge)


class GeometricLossFunction(torch.autograd.Function):
    """Symmetric two-view geometric loss (networks.ProjectionDepthSimilarityLoss.tforward, networks.py:500-503):
    fwd(depth0 -> view 1) + fwd(depth1 -> view 0), each a mean of clamped |projected depth - sampled depth|."""

    @staticmethod
    def forward(ctx, depth0, depth1, ray, K, R0, t0, R1, t1, clamp):
        ts = [_f32(x.contiguous(), n) for x, n in ((depth0, "depth0"), (depth1, "depth1"), (ray, "ray"), (K, "K"),
                                                   (R0, "R0"), (t0, "t0"), (R1, "R1"), (t1, "t1"))]
        depth0, depth1, ray, K, R0, t0, R1, t1 = ts
        dev = _same_device(*ts)
        if depth0.dim() != 4 or depth0.shape[1] != 1 or depth0.shape != depth1.shape:
            raise RuntimeError("geometric_loss expects depth0, depth1 [B,1,H,W]")
        B, _, H, W = depth0.shape
        if ray.numel() != H * W * 3 or K.numel() != 9 or R0.numel() != B * 9 or R1.numel() != B * 9 or \
                t0.numel() != B * 3 or t1.numel() != B * 3:
            raise RuntimeError("geometric_loss: ray [H*W,3], K [3,3], R [B,3,3], t [B,3] expected")
        L = _lib.lib()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        c = float(clamp)
        if L.ctd_geometric_workspace_bytes(2 * B, H, W) > 0:
            # both directions in one launch, the means formed by its last workgroup (tickets: zeroed words per stream)
            ws = _workspace(L.ctd_geometric_workspace_bytes(2 * B, H, W), dev)
            _call_with_ticket(lambda tk: L.ctd_geometric_sym_fwd_f32(
                _ptr(depth0), _ptr(depth1), _ptr(ray), _ptr(K), _ptr(R0), _ptr(t0), _ptr(R1), _ptr(t1), _ptr(loss), B, H, W,
                c, _ptr(ws), ws.numel(), _ptr(tk), dev.index, _stream(dev)), _ticket(dev), "geometric_loss")
        else:
            ws = _workspace(L.ctd_geometric_workspace_bytes(B, H, W), dev)
            st = L.ctd_geometric_fwd_f32(_ptr(depth0), _ptr(depth1), _ptr(ray), _ptr(K), _ptr(R0), _ptr(t0), _ptr(R1), _ptr(t1),
                                         _ptr(loss), 0, B, H, W, c, _ptr(ws), ws.numel(), dev.index, _stream(dev))
            _lib.check(st, "geometric_loss")
            st = L.ctd_geometric_fwd_f32(_ptr(depth1), _ptr(depth0), _ptr(ray), _ptr(K), _ptr(R1), _ptr(t1), _ptr(R0), _ptr(t0),
                                         _ptr(loss), 1, B, H, W, c, _ptr(ws), ws.numel(), dev.index, _stream(dev))
            _lib.check(st, "geometric_loss")
        ctx.save_for_backward(depth0, depth1, ray, K, R0, t0, R1, t1)
        ctx.clamp = c
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        depth0, depth1, ray, K, R0, t0, R1, t1 = ctx.saved_tensors
        B, _, H, W = depth0.shape
        dev = depth0.device
        L = _lib.lib()
        gl = grad_loss.to(torch.float32).contiguous()
        g0 = torch.zeros_like(depth0)          # both receive bilinear scatter (atomics) from the other direction
        g1 = torch.zeros_like(depth1)
        st = L.ctd_geometric_bwd_f32(_ptr(depth0), _ptr(depth1), _ptr(ray), _ptr(K), _ptr(R0), _ptr(t0), _ptr(R1), _ptr(t1),
                                     _ptr(gl), _ptr(g0), 1, _ptr(g1), B, H, W, ctx.clamp, dev.index, _stream(dev))
        _lib.check(st, "geometric_loss backward")
        st = L.ctd_geometric_bwd_f32(_ptr(depth1), _ptr(depth0), _ptr(ray), _ptr(K), _ptr(R1), _ptr(t1), _ptr(R0), _ptr(t0),
                                     _ptr(gl), _ptr(g1), 1, _ptr(g0), B, H, W, ctx.clamp, dev.index, _stream(dev))
        _lib.check(st, "geometric_loss backward")
        return g0, g1, None, None, None, None, None, None, None


def geometric_loss(depth0, depth1, ray, K, R0, t0, R1, t1, clamp=-1):
    return GeometricLossFunction.apply(depth0, depth1, ray, K, R0, t0, R1, t1, clamp)
