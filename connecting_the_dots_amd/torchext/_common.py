# What every family module shares: tensor and scalar checks, the launch plumbing, the tables of include/ctd_hip.h.
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


def _call(fn, who, *args):
    """one C-ABI call; any status but CTD_OK raises RuntimeError in the name of `who`"""
    _lib.check(fn(*args), who)


def _call_with_ticket(call, ticket, what):
    """Runs `call(ticket)` (a C-ABI launch that takes its ticket words at zero and leaves them at zero).  When it
    returns an error the words may be anywhere in between -- a later launch on them would then have no "last"
    workgroup and leave its result unwritten -- so they are cleared (stream-ordered, like the launch) before the error
    is raised."""
    st = call(ticket)
    if st != 0:
        ticket.zero_()
    _lib.check(st, what)


def _f32(t, name):
    _check(t, name, (torch.float32,))
    return t


_PHOTO_TYPES = {"mse": 0, "sad": 1, "census_mse": 2, "census_sad": 3}


def _photo_fast(es, block_size, algo):
    """algo 'fast' (default) = tolerance-level kernels (f32, odd block sizes up to 9); anything else they do not
    cover runs the reference-order kernels."""
    algo = algo or os.environ.get("CTD_PHOTO_ALGO", "fast")
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    return algo == "fast" and es.dtype == torch.float32 and int(block_size) in (3, 5, 7, 9)


_SUBPIXEL_MODES = {"parabola": 0, "equiangular": 1}


def _subpixel_mode(mode, who):
    if mode not in _SUBPIXEL_MODES:
        raise RuntimeError("%s: unknown sub-pixel mode %r (parabola | equiangular)" % (who, mode))
    return _SUBPIXEL_MODES[mode]


def _number(x, name, who, lo=0.0, lo_open=False):
    """a finite number >= lo (> lo with lo_open) as a float; bool is no number.  lo=None: any real number, NaN and the
    infinities included"""
    if lo is None:
        if not isinstance(x, numbers.Real):
            raise RuntimeError("%s: %s must be a number" % (who, name))
    elif isinstance(x, bool) or not isinstance(x, numbers.Real) or not (lo < x if lo_open else lo <= x) or \
            not x < float("inf"):
        raise RuntimeError("%s: %s must be a finite number %s %g" % (who, name, ">" if lo_open else ">=", lo))
    return float(x)


def _integer(x, name, who, lo=0, hi=2 ** 31 - 1, what=None):
    """an integer in [lo, hi] as an int; neither bool nor an integral float is one.  `what` words the range where
    "an integer >= lo" does not"""
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not lo <= x <= hi:
        raise RuntimeError("%s: %s must be %s" % (who, name, what or "an integer >= %d" % lo))
    return int(x)


def _odd_integer(x, name, who, lo, hi):
    what = "an odd integer in [%d, %d]" % (lo, hi)
    if _integer(x, name, who, lo, hi, what) % 2 == 0:
        raise RuntimeError("%s: %s must be %s" % (who, name, what))
    return int(x)


def _resolve_ncc_algo(algo, dtype, n_disps, block_size, fast_ok=True):
    """the CTD_NCC_* code of `algo` (None: the default); 'fast' runs 'exact' where the fast kernels do not cover the call
    (`fast_ok`: what the op asks for on top of `_ncc_fast_covers`)"""
    algo = algo or _default_algo()
    if algo not in _ALGOS:
        raise RuntimeError("unknown algo %r" % (algo,))
    if algo == "fast" and not (fast_ok and _ncc_fast_covers(dtype, n_disps, block_size)):
        algo = "exact"
    return _ALGOS[algo]


def _ncc_pair(in0, in1, expects, mismatch, c1=True, batch=True, others=()):
    """The NCC pair, both already `_check`ed: in0 [N,C,H,W] | [C,H,W] against in1 [C,H,W] | [N,C,H,W] -> (in0 as
    [N,C,H,W], the shape of a per-pixel output: [N,H,W], or [H,W] for a 3-D in0, in1's frame stride, the device, which
    `others` must share).  c1: C must be 1.  batch=False: in1's N is not compared with in0's.  The messages are the
    caller's: `expects` for a wrong rank (or C), `mismatch` for an in1 of another [C,H,W] (or N)."""
    squeeze = in0.dim() == 3
    a0 = in0.unsqueeze(0) if squeeze else in0
    if a0.dim() != 4 or (c1 and a0.shape[1] != 1) or in1.dim() not in (3, 4):
        raise RuntimeError(expects)
    dev = _same_device(a0, in1, *others)
    N, C, H, W = a0.shape
    if tuple(in1.shape[-3:]) != (C, H, W) or (batch and in1.dim() == 4 and in1.shape[0] != N):
        raise RuntimeError(mismatch)
    return a0, ((H, W) if squeeze else (N, H, W)), (0 if in1.dim() == 3 else C * H * W), dev


def _loss_type(type, who=None):
    """the code of a loss type name, any case.  who=None: the reference's bare Exception (functions.py:117)"""
    type = type.lower()
    if type not in _PHOTO_TYPES:
        if who is None:
            raise Exception('invalid loss type')
        raise RuntimeError("%s: invalid loss type %r" % (who, type))
    return _PHOTO_TYPES[type]


def _cost_pair(im, pattern, who, batch=True, others=()):
    """The cost pair, both already `_check`ed: im [N,H,W] | [H,W] against pattern [H,W] | [N,H,W] -> (im as [N,H,W], the
    pattern's frame stride, the device, which `others` must share); an output is shaped as im.  batch=False: the
    pattern's N is not compared with im's."""
    a = im.unsqueeze(0) if im.dim() == 2 else im
    if a.dim() != 3 or pattern.dim() not in (2, 3) or tuple(pattern.shape[-2:]) != tuple(a.shape[-2:]):
        raise RuntimeError("%s expects im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]" % who)
    dev = _same_device(a, pattern, *others)
    if batch and pattern.dim() == 3 and pattern.shape[0] != a.shape[0]:
        raise RuntimeError("%s: pattern batch does not match im" % who)
    return a, (0 if pattern.dim() == 2 else a.shape[1] * a.shape[2]), dev
