"""What the Python wrappers of the two matcher families reject, and with which words: the ops that take the "NCC pair"
(in0 [N,C,H,W] | [C,H,W] against in1 [C,H,W] | [N,C,H,W]) and the ops that take the "cost pair" (im [N,H,W] | [H,W]
against pattern [H,W] | [N,H,W]).  Every row is a bad call, the exact type of the exception and its full message; a
row whose operands trip two checks pins which check comes first.  The wrappers check `is_cuda` before anything else, so
none of this can be reached without a GPU.  Every row is rejected before any kernel is launched; one accepted call per
op shows that the baseline arguments the rows vary are valid ones.

Pinned as they are (not as they should be): `costvol` and `costvol_argmin` raise a bare `Exception('invalid loss
type')` where the ops next to them raise RuntimeError with the op's name; `xcorrvol_argmax`, `lcn_xcorrvol_argmax`,
`costvol` and `costvol_argmin` do not compare the pattern's batch with N where the sub-pixel, validity and band ops do;
`xcorrvol_argmax` leaves C != 1 to the library (status 3) where the ops next to it say what they expect."""
import pytest
import torch

from connecting_the_dots_amd import torchext as te

pytestmark = pytest.mark.gpu

N, H, W, D, BS = 2, 8, 16, 4, 3
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def f(*shape, dtype=F32):
    return torch.rand(shape, device="cuda", dtype=torch.float32).to(dtype)


def nc(*shape):
    """a non-contiguous f32 tensor of this shape"""
    return f(*shape[:-1], 2 * shape[-1])[..., ::2]


def z(*shape, dtype=I64):
    return torch.zeros(shape, device="cuda", dtype=dtype)


def band(*shape, dtype=I32):
    return z(*shape, dtype=dtype), torch.full(shape, D - 1, device="cuda", dtype=dtype)


def handle(in1, n=N, d=D, bs=BS):
    """a `prepare_pattern` handle of `in1` without the launch that fills it (no row gets as far as reading it)"""
    return te.PreparedPattern(in1, n, d, bs, torch.empty(256, dtype=torch.uint8, device="cuda"))


R, E = RuntimeError, Exception
NCC_PAIR = "in0 [N,1,H,W] or [1,H,W] and in1 [1,H,W] or [N,1,H,W]"
COST_PAIR = "im [N,H,W] or [H,W] and pattern [H,W] or [N,H,W]"
CHW = "in0 and in1 must have the same [C,H,W] shape"
MODE = "%s: unknown sub-pixel mode 'cubic' (parabola | equiangular)"
PREPARED_VOL = "%s: `prepared` belongs to another pattern, frame count, shape or device (or the call does not take the " \
               "fast path)"
PREPARED_PLANES = "%s: `prepared` belongs to another pattern, frame count or device"
VALIDITY = "%s: validity must be None or a dict with the keys lr_tol and / or min_gap"
UNSUPPORTED = "%s failed: unsupported parameter combination (status 3)"

# (id, call, exception type, message)
NCC_ROWS = [
    # ---- xcorrvol: in0 [C,H,W], in1 [C,H,W]; f32 or f64
    ("xcorrvol-in0-rank", lambda: te.xcorrvol(f(1, 1, H, W), f(1, H, W), D, BS), R, "xcorrvol expects [C,H,W] tensors"),
    ("xcorrvol-in1-rank", lambda: te.xcorrvol(f(1, H, W), f(H, W), D, BS), R, "xcorrvol expects [C,H,W] tensors"),
    ("xcorrvol-chw", lambda: te.xcorrvol(f(1, H, W), f(2, H, W), D, BS), R, CHW),
    ("xcorrvol-hw", lambda: te.xcorrvol(f(1, H, W), f(1, H, W + 1), D, BS), R, CHW),
    ("xcorrvol-dtype-pair", lambda: te.xcorrvol(f(1, H, W), f(1, H, W, dtype=F64), D, BS), R,
     "in0 and in1 must have the same dtype"),
    ("xcorrvol-int", lambda: te.xcorrvol(z(1, H, W), f(1, H, W), D, BS), R, "in0: unsupported dtype torch.int64"),
    ("xcorrvol-noncontig", lambda: te.xcorrvol(nc(1, H, W), f(1, H, W), D, BS), R, "in0 must be contiguous"),
    ("xcorrvol-algo", lambda: te.xcorrvol(f(1, H, W), f(1, H, W), D, BS, algo="bogus"), R, "unknown algo 'bogus'"),
    ("xcorrvol-order-contig-before-rank", lambda: te.xcorrvol(f(1, 1, H, W), nc(1, H, W), D, BS), R,
     "in1 must be contiguous"),
    ("xcorrvol-order-dtype-before-chw", lambda: te.xcorrvol(f(1, H, W), f(2, H, W, dtype=F64), D, BS), R,
     "in0 and in1 must have the same dtype"),
    ("xcorrvol-order-chw-before-algo", lambda: te.xcorrvol(f(1, H, W), f(2, H, W), D, BS, algo="bogus"), R, CHW),
    # ---- xcorrvol_batch: in0 [N,C,H,W], in1 [C,H,W] | [N,C,H,W]
    ("batch-in0-rank", lambda: te.xcorrvol_batch(f(1, H, W), f(1, H, W), D, BS), R,
     "xcorrvol_batch expects in0 [N,C,H,W] and in1 [C,H,W] or [N,C,H,W]"),
    ("batch-in1-rank", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(H, W), D, BS), R,
     "xcorrvol_batch expects in0 [N,C,H,W] and in1 [C,H,W] or [N,C,H,W]"),
    ("batch-chw", lambda: te.xcorrvol_batch(f(N, 2, H, W), f(1, H, W), D, BS), R, CHW),
    ("batch-n", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(N + 1, 1, H, W), D, BS), R, "in1 batch does not match in0"),
    ("batch-dtype-pair", lambda: te.xcorrvol_batch(f(N, 1, H, W, dtype=F64), f(1, H, W), D, BS), R,
     "in0 and in1 must have the same dtype"),
    ("batch-noncontig", lambda: te.xcorrvol_batch(f(N, 1, H, W), nc(1, H, W), D, BS), R, "in1 must be contiguous"),
    ("batch-algo", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(1, H, W), D, BS, algo="bogus"), R, "unknown algo 'bogus'"),
    ("batch-prepared-other-pattern", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(1, H, W), D, BS,
                                                               prepared=handle(f(1, H, W))), R,
     PREPARED_VOL % "xcorrvol_batch"),
    ("batch-prepared-exact", lambda: (lambda p: te.xcorrvol_batch(f(N, 1, H, W), p, D, BS, algo="exact",
                                                                  prepared=handle(p)))(f(1, H, W)), R,
     PREPARED_VOL % "xcorrvol_batch"),
    ("batch-order-n-before-algo", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(N + 1, 1, H, W), D, BS, algo="bogus"), R,
     "in1 batch does not match in0"),
    ("batch-order-algo-before-prepared", lambda: te.xcorrvol_batch(f(N, 1, H, W), f(1, H, W), D, BS, algo="bogus",
                                                                   prepared=handle(f(1, H, W))), R,
     "unknown algo 'bogus'"),
    # ---- xcorrvol_argmax: in0 [N,1,H,W] | [1,H,W], in1 [1,H,W] | [N,1,H,W]; f32
    ("argmax-f64", lambda: te.xcorrvol_argmax(f(N, 1, H, W, dtype=F64), f(1, H, W), D, BS), R,
     "in0: unsupported dtype torch.float64"),
    ("argmax-in1-f64", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W, dtype=F64), D, BS), R,
     "in1: unsupported dtype torch.float64"),
    ("argmax-in0-rank", lambda: te.xcorrvol_argmax(f(H, W), f(1, H, W), D, BS), R,
     "xcorrvol_argmax expects in0 [N,1,H,W] or [1,H,W]"),
    ("argmax-in1-rank", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(H, W), D, BS), R,
     "xcorrvol_argmax expects in0 [N,1,H,W] or [1,H,W]"),
    ("argmax-c2", lambda: te.xcorrvol_argmax(f(N, 2, H, W), f(2, H, W), D, BS), R, UNSUPPORTED % "xcorrvol_argmax"),
    ("argmax-chw", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H + 1, W), D, BS), R, CHW),
    ("argmax-noncontig", lambda: te.xcorrvol_argmax(nc(N, 1, H, W), f(1, H, W), D, BS), R, "in0 must be contiguous"),
    ("argmax-algo", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, algo="bogus"), R, "unknown algo 'bogus'"),
    ("argmax-mode", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, subpixel="cubic"), R,
     MODE % "xcorrvol_argmax"),
    ("argmax-validity", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, validity={"tol": 1}), R,
     VALIDITY % "xcorrvol_argmax"),
    ("argmax-prepared-other-pattern", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS,
                                                                 prepared=handle(f(1, H, W))), R,
     PREPARED_VOL % "xcorrvol_argmax"),
    ("argmax-prepared-other-count", lambda: (lambda p: te.xcorrvol_argmax(f(N, 1, H, W), p, D, BS,
                                                                          prepared=handle(p, n=N + 1)))(f(1, H, W)), R,
     PREPARED_VOL % "xcorrvol_argmax"),
    ("argmax-order-validity-before-mode", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, subpixel="cubic",
                                                                     validity=3), R, VALIDITY % "xcorrvol_argmax"),
    ("argmax-order-mode-before-rank", lambda: te.xcorrvol_argmax(f(H, W), f(1, H, W), D, BS, subpixel="cubic"), R,
     MODE % "xcorrvol_argmax"),
    ("argmax-order-contig-before-rank", lambda: te.xcorrvol_argmax(f(H, W), nc(1, H, W), D, BS), R,
     "in1 must be contiguous"),
    ("argmax-order-chw-before-algo", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W + 1), D, BS, algo="bogus"), R,
     CHW),
    ("argmax-order-algo-before-prepared", lambda: te.xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, algo="bogus",
                                                                     prepared=handle(f(1, H, W))), R,
     "unknown algo 'bogus'"),
    # ---- lcn_xcorrvol_argmax: raw [N,1,H,W], in1 [1,H,W] | [N,1,H,W]; f32
    ("lcnargmax-f64", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W, dtype=F64), f(1, H, W), D, BS), R,
     "raw: unsupported dtype torch.float64"),
    ("lcnargmax-raw-rank", lambda: te.lcn_xcorrvol_argmax(f(1, H, W), f(1, H, W), D, BS), R,
     "lcn_xcorrvol_argmax expects raw [N,1,H,W] and in1 [1,H,W] or [N,1,H,W]"),
    ("lcnargmax-c2", lambda: te.lcn_xcorrvol_argmax(f(N, 2, H, W), f(2, H, W), D, BS), R,
     "lcn_xcorrvol_argmax expects raw [N,1,H,W] and in1 [1,H,W] or [N,1,H,W]"),
    ("lcnargmax-in1-rank", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(H, W), D, BS), R,
     "lcn_xcorrvol_argmax expects raw [N,1,H,W] and in1 [1,H,W] or [N,1,H,W]"),
    ("lcnargmax-lcn-algo", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, lcn_algo="bogus"), R,
     "unknown lcn_algo 'bogus'"),
    ("lcnargmax-chw", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W + 1), D, BS), R,
     "raw and in1 must have the same [C,H,W] shape"),
    ("lcnargmax-radius", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, radius=H), R,
     "lcn: radius must be smaller than the image (ReflectionPad2d rule)"),
    ("lcnargmax-noncontig", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), nc(1, H, W), D, BS), R,
     "in1 must be contiguous"),
    ("lcnargmax-mode", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W), D, BS, subpixel="cubic"), R,
     MODE % "lcn_xcorrvol_argmax"),
    ("lcnargmax-order-rank-before-lcn-algo", lambda: te.lcn_xcorrvol_argmax(f(1, H, W), f(1, H, W), D, BS,
                                                                            lcn_algo="bogus"), R,
     "lcn_xcorrvol_argmax expects raw [N,1,H,W] and in1 [1,H,W] or [N,1,H,W]"),
    ("lcnargmax-order-lcn-algo-before-chw", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W + 1), D, BS,
                                                                           lcn_algo="bogus"), R,
     "unknown lcn_algo 'bogus'"),
    ("lcnargmax-order-chw-before-radius", lambda: te.lcn_xcorrvol_argmax(f(N, 1, H, W), f(1, H, W + 1), D, BS,
                                                                         radius=H), R,
     "raw and in1 must have the same [C,H,W] shape"),
    # ---- xcorrvol_subpixel: the pair of xcorrvol_argmax, idx int64 [N,H,W] | [H,W]
    ("subpixel-f64", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W, dtype=F64), z(N, H, W), D, BS), R,
     "in1: unsupported dtype torch.float64"),
    ("subpixel-mode", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS, "cubic"), R,
     MODE % "xcorrvol_subpixel"),
    ("subpixel-in0-rank", lambda: te.xcorrvol_subpixel(f(H, W), f(1, H, W), z(H, W), D, BS), R,
     "xcorrvol_subpixel expects " + NCC_PAIR),
    ("subpixel-c2", lambda: te.xcorrvol_subpixel(f(N, 2, H, W), f(2, H, W), z(N, H, W), D, BS), R,
     "xcorrvol_subpixel expects " + NCC_PAIR),
    ("subpixel-in1-rank", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(H, W), z(N, H, W), D, BS), R,
     "xcorrvol_subpixel expects " + NCC_PAIR),
    ("subpixel-chw", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W + 1), z(N, H, W), D, BS), R,
     "xcorrvol_subpixel: in1 does not match in0"),
    ("subpixel-n", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(N + 1, 1, H, W), z(N, H, W), D, BS), R,
     "xcorrvol_subpixel: in1 does not match in0"),
    ("subpixel-idx-shape", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W), z(H, W), D, BS), R,
     "xcorrvol_subpixel: idx must be shaped as xcorrvol_argmax returns it"),
    ("subpixel-idx-shape-squeezed", lambda: te.xcorrvol_subpixel(f(1, H, W), f(1, H, W), z(1, H, W), D, BS), R,
     "xcorrvol_subpixel: idx must be shaped as xcorrvol_argmax returns it"),
    ("subpixel-idx-dtype", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W), z(N, H, W, dtype=I32), D, BS), R,
     "idx: unsupported dtype torch.int32"),
    ("subpixel-idx-noncontig", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W), z(N, H, 2 * W)[..., ::2], D, BS), R,
     "idx must be contiguous"),
    ("subpixel-prepared-other-pattern", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS,
                                                                     prepared=handle(f(1, H, W))), R,
     PREPARED_PLANES % "xcorrvol_subpixel"),
    ("subpixel-order-dtype-before-mode", lambda: te.xcorrvol_subpixel(f(N, 1, H, W, dtype=F64), f(1, H, W), z(N, H, W), D,
                                                                      BS, "cubic"), R,
     "in0: unsupported dtype torch.float64"),
    ("subpixel-order-mode-before-rank", lambda: te.xcorrvol_subpixel(f(H, W), f(1, H, W), z(H, W), D, BS, "cubic"), R,
     MODE % "xcorrvol_subpixel"),
    ("subpixel-order-match-before-idx", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(N + 1, 1, H, W), z(H, W), D, BS), R,
     "xcorrvol_subpixel: in1 does not match in0"),
    ("subpixel-order-idx-shape-before-dtype", lambda: te.xcorrvol_subpixel(f(N, 1, H, W), f(1, H, W),
                                                                           z(H, W, dtype=I32), D, BS), R,
     "xcorrvol_subpixel: idx must be shaped as xcorrvol_argmax returns it"),
    # ---- xcorrvol_validity: in0 [N,C,H,W] | [C,H,W], in1 [C,H,W] | [N,C,H,W], idx int64 [N,H,W] | [H,W]
    ("validity-f64", lambda: te.xcorrvol_validity(f(N, 1, H, W, dtype=F64), f(1, H, W), z(N, H, W), D, BS), R,
     "in0: unsupported dtype torch.float64"),
    ("validity-idx-dtype", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(N, H, W, dtype=I32), D, BS), R,
     "idx: unsupported dtype torch.int32"),
    ("validity-lr-tol", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS, lr_tol=-1), R,
     "xcorrvol_validity: lr_tol must be an int >= 0"),
    ("validity-min-gap", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS,
                                                      min_gap=float("nan")), R,
     "xcorrvol_validity: min_gap must be a number >= 0"),
    ("validity-in0-rank", lambda: te.xcorrvol_validity(f(H, W), f(1, H, W), z(H, W), D, BS), R,
     "xcorrvol_validity expects in0 [N,C,H,W] or [C,H,W] and in1 [C,H,W] or [N,C,H,W]"),
    ("validity-in1-rank", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(H, W), z(N, H, W), D, BS), R,
     "xcorrvol_validity expects in0 [N,C,H,W] or [C,H,W] and in1 [C,H,W] or [N,C,H,W]"),
    ("validity-chw", lambda: te.xcorrvol_validity(f(N, 2, H, W), f(1, H, W), z(N, H, W), D, BS), R,
     "xcorrvol_validity: in1 does not match in0"),
    ("validity-n", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(N + 1, 1, H, W), z(N, H, W), D, BS), R,
     "xcorrvol_validity: in1 does not match in0"),
    ("validity-idx-shape", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(N, 1, H, W), D, BS), R,
     "xcorrvol_validity: idx must be shaped as xcorrvol_argmax returns it"),
    ("validity-noncontig", lambda: te.xcorrvol_validity(nc(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS), R,
     "in0 must be contiguous"),
    ("validity-algo", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(N, H, W), D, BS, algo="bogus"), R,
     "unknown algo 'bogus'"),
    ("validity-order-idx-dtype-before-lr-tol", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W),
                                                                            z(N, H, W, dtype=I32), D, BS, lr_tol=-1), R,
     "idx: unsupported dtype torch.int32"),
    ("validity-order-lr-tol-before-rank", lambda: te.xcorrvol_validity(f(H, W), f(1, H, W), z(H, W), D, BS, lr_tol=1.5), R,
     "xcorrvol_validity: lr_tol must be an int >= 0"),
    ("validity-order-idx-shape-before-algo", lambda: te.xcorrvol_validity(f(N, 1, H, W), f(1, H, W), z(H, W), D, BS,
                                                                          algo="bogus"), R,
     "xcorrvol_validity: idx must be shaped as xcorrvol_argmax returns it"),
    # ---- prepare_pattern: in1 [1,H,W] | [N,1,H,W]; f32
    ("prepare-f64", lambda: te.prepare_pattern(f(1, H, W, dtype=F64), N, D, BS), R,
     "in1: unsupported dtype torch.float64"),
    ("prepare-rank", lambda: te.prepare_pattern(f(H, W), N, D, BS), R, "prepare_pattern expects in1 [1,H,W] or [N,1,H,W]"),
    ("prepare-c2", lambda: te.prepare_pattern(f(N, 2, H, W), N, D, BS), R,
     "prepare_pattern expects in1 [1,H,W] or [N,1,H,W]"),
    ("prepare-noncontig", lambda: te.prepare_pattern(nc(1, H, W), N, D, BS), R, "in1 must be contiguous"),
    ("prepare-block", lambda: te.prepare_pattern(f(1, H, W), N, D, 4), R,
     "prepare_pattern: the fast NCC path does not cover this block size / disparity range"),
    ("prepare-disps", lambda: te.prepare_pattern(f(1, H, W), N, 513, BS), R,
     "prepare_pattern: the fast NCC path does not cover this block size / disparity range"),
    ("prepare-order-rank-before-cover", lambda: te.prepare_pattern(f(H, W), N, D, 4), R,
     "prepare_pattern expects in1 [1,H,W] or [N,1,H,W]"),
]

for _op, _fn in (("xcorrvol_argmax_band", te.xcorrvol_argmax_band), ("xcorrvol_band_validity", te.xcorrvol_band_validity)):
    def _rows(op=_op, fn=_fn):
        shaped = "%s: %%s must be int32 shaped (%d, %d, %d)" % (op, N, H, W)
        return [
            (op + "-f64", lambda: fn(f(N, 1, H, W, dtype=F64), f(1, H, W), *band(N, H, W), D, BS), R,
             "in0: unsupported dtype torch.float64"),
            (op + "-in0-rank", lambda: fn(f(H, W), f(1, H, W), *band(H, W), D, BS), R, op + " expects " + NCC_PAIR),
            (op + "-c2", lambda: fn(f(N, 2, H, W), f(2, H, W), *band(N, H, W), D, BS), R, op + " expects " + NCC_PAIR),
            (op + "-in1-rank", lambda: fn(f(N, 1, H, W), f(H, W), *band(N, H, W), D, BS), R, op + " expects " + NCC_PAIR),
            (op + "-chw", lambda: fn(f(N, 1, H, W), f(1, H + 1, W), *band(N, H, W), D, BS), R,
             op + ": in1 does not match in0"),
            (op + "-n", lambda: fn(f(N, 1, H, W), f(N + 1, 1, H, W), *band(N, H, W), D, BS), R,
             op + ": in1 does not match in0"),
            (op + "-lo-dtype", lambda: fn(f(N, 1, H, W), f(1, H, W), z(N, H, W), band(N, H, W)[1], D, BS), R,
             "lo: unsupported dtype torch.int64"),
            (op + "-lo-shape", lambda: fn(f(N, 1, H, W), f(1, H, W), z(H, W, dtype=I32), band(N, H, W)[1], D, BS), R,
             shaped % "lo"),
            (op + "-hi-shape", lambda: fn(f(N, 1, H, W), f(1, H, W), band(N, H, W)[0], z(N, 1, H, W, dtype=I32), D, BS), R,
             shaped % "hi"),
            (op + "-hi-noncontig", lambda: fn(f(N, 1, H, W), f(1, H, W), band(N, H, W)[0],
                                              z(N, H, 2 * W, dtype=I32)[..., ::2], D, BS), R, "hi must be contiguous"),
            (op + "-mode", lambda: fn(f(N, 1, H, W), f(1, H, W), *band(N, H, W), D, BS, subpixel="cubic"), R, MODE % op),
            (op + "-prepared-other-pattern", lambda: fn(f(N, 1, H, W), f(1, H, W), *band(N, H, W), D, BS,
                                                        prepared=handle(f(1, H, W))), R, PREPARED_PLANES % op),
            (op + "-order-mode-before-dtype", lambda: fn(f(N, 1, H, W, dtype=F64), f(1, H, W), *band(N, H, W), D, BS,
                                                         subpixel="cubic"), R, MODE % op),
            (op + "-order-match-before-lo", lambda: fn(f(N, 1, H, W), f(N + 1, 1, H, W), z(H, W, dtype=I32),
                                                       band(N, H, W)[1], D, BS), R, op + ": in1 does not match in0"),
            (op + "-order-lo-shape-before-hi-dtype", lambda: fn(f(N, 1, H, W), f(1, H, W), z(H, W, dtype=I32), z(N, H, W),
                                                                D, BS), R, shaped % "lo"),
        ]
    NCC_ROWS += _rows()

NCC_ROWS += [
    ("xcorrvol_band_validity-lr-tol", lambda: te.xcorrvol_band_validity(f(N, 1, H, W), f(1, H, W), *band(N, H, W), D, BS,
                                                                        lr_tol=True), R,
     "xcorrvol_band_validity: lr_tol must be an int >= 0"),
    ("xcorrvol_band_validity-order-min-gap-before-dtype", lambda: te.xcorrvol_band_validity(
        f(N, 1, H, W, dtype=F64), f(1, H, W), *band(N, H, W), D, BS, min_gap=-1.0), R,
     "xcorrvol_band_validity: min_gap must be a number >= 0"),
]

COST_ROWS = [
    # ---- costvol: im [N,H,W] | [H,W], pattern [H,W] | [N,H,W]; f32
    ("costvol-f64", lambda: te.costvol(f(N, H, W, dtype=F64), f(H, W), D, BS), R, "im: unsupported dtype torch.float64"),
    ("costvol-noncontig", lambda: te.costvol(f(N, H, W), nc(H, W), D, BS), R, "pattern must be contiguous"),
    ("costvol-type", lambda: te.costvol(f(N, H, W), f(H, W), D, BS, type="Bogus"), E, "invalid loss type"),
    ("costvol-im-rank", lambda: te.costvol(f(N, 1, H, W), f(H, W), D, BS), R, "costvol expects " + COST_PAIR),
    ("costvol-pattern-rank", lambda: te.costvol(f(N, H, W), f(1, 1, H, W), D, BS), R, "costvol expects " + COST_PAIR),
    ("costvol-hw", lambda: te.costvol(f(N, H, W), f(H, W + 1), D, BS), R, "costvol expects " + COST_PAIR),
    ("costvol-algo", lambda: te.costvol(f(N, H, W), f(H, W), D, BS, algo="bogus"), R, "unknown algo 'bogus'"),
    ("costvol-order-dtype-before-type", lambda: te.costvol(f(N, H, W), f(H, W, dtype=F64), D, BS, type="bogus"), R,
     "pattern: unsupported dtype torch.float64"),
    ("costvol-order-type-before-rank", lambda: te.costvol(f(N, 1, H, W), f(H, W), D, BS, type="bogus"), E,
     "invalid loss type"),
    ("costvol-order-rank-before-algo", lambda: te.costvol(f(N, H, W), f(H, W + 1), D, BS, algo="bogus"), R,
     "costvol expects " + COST_PAIR),
    # ---- costvol_argmin
    ("argmin-f64", lambda: te.costvol_argmin(f(N, H, W, dtype=F64), f(H, W), D, BS), R,
     "im: unsupported dtype torch.float64"),
    ("argmin-noncontig", lambda: te.costvol_argmin(nc(N, H, W), f(H, W), D, BS), R, "im must be contiguous"),
    ("argmin-type", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, type="bogus"), E, "invalid loss type"),
    ("argmin-rerank-nan", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, rerank_rel=float("nan")), R,
     "costvol_argmin: rerank_rel is NaN"),
    ("argmin-im-rank", lambda: te.costvol_argmin(f(N, 1, H, W), f(H, W), D, BS), R, "costvol_argmin expects " + COST_PAIR),
    ("argmin-pattern-rank", lambda: te.costvol_argmin(f(N, H, W), f(W), D, BS), R, "costvol_argmin expects " + COST_PAIR),
    ("argmin-hw", lambda: te.costvol_argmin(f(N, H, W), f(H + 1, W), D, BS), R, "costvol_argmin expects " + COST_PAIR),
    ("argmin-mode", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, subpixel="cubic"), R, MODE % "costvol_argmin"),
    ("argmin-validity", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, validity={"gap": 0.0}), R,
     VALIDITY % "costvol_argmin"),
    ("argmin-order-validity-before-mode", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, subpixel="cubic",
                                                                    validity=[]), R, VALIDITY % "costvol_argmin"),
    ("argmin-order-mode-before-dtype", lambda: te.costvol_argmin(f(N, H, W, dtype=F64), f(H, W), D, BS,
                                                                 subpixel="cubic"), R, MODE % "costvol_argmin"),
    ("argmin-order-type-before-rerank", lambda: te.costvol_argmin(f(N, H, W), f(H, W), D, BS, type="bogus",
                                                                  rerank_rel=float("nan")), E, "invalid loss type"),
    ("argmin-order-rerank-before-rank", lambda: te.costvol_argmin(f(N, 1, H, W), f(H, W), D, BS,
                                                                  rerank_rel=float("nan")), R,
     "costvol_argmin: rerank_rel is NaN"),
    # ---- costvol_subpixel: idx int64 shaped as im
    ("csubpixel-f64", lambda: te.costvol_subpixel(f(N, H, W), f(H, W, dtype=F64), z(N, H, W), D, BS), R,
     "pattern: unsupported dtype torch.float64"),
    ("csubpixel-mode", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(N, H, W), D, BS, mode="cubic"), R,
     "costvol_subpixel: unknown sub-pixel mode 'cubic' (parabola | equiangular)"),
    ("csubpixel-type", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(N, H, W), D, BS, type="Bogus"), R,
     "costvol_subpixel: invalid loss type 'bogus'"),
    ("csubpixel-im-rank", lambda: te.costvol_subpixel(f(N, 1, H, W), f(H, W), z(N, 1, H, W), D, BS), R,
     "costvol_subpixel expects " + COST_PAIR),
    ("csubpixel-hw", lambda: te.costvol_subpixel(f(N, H, W), f(H, W + 1), z(N, H, W), D, BS), R,
     "costvol_subpixel expects " + COST_PAIR),
    ("csubpixel-n", lambda: te.costvol_subpixel(f(N, H, W), f(N + 1, H, W), z(N, H, W), D, BS), R,
     "costvol_subpixel: pattern batch does not match im"),
    ("csubpixel-idx-shape", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(H, W), D, BS), R,
     "costvol_subpixel: idx must be shaped as costvol_argmin returns it"),
    ("csubpixel-idx-dtype", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(N, H, W, dtype=I32), D, BS), R,
     "idx: unsupported dtype torch.int32"),
    ("csubpixel-order-mode-before-type", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(N, H, W), D, BS, type="bogus",
                                                                     mode="cubic"), R,
     "costvol_subpixel: unknown sub-pixel mode 'cubic' (parabola | equiangular)"),
    ("csubpixel-order-type-before-rank", lambda: te.costvol_subpixel(f(N, 1, H, W), f(H, W), z(N, H, W), D, BS,
                                                                     type="bogus"), R,
     "costvol_subpixel: invalid loss type 'bogus'"),
    ("csubpixel-order-n-before-idx", lambda: te.costvol_subpixel(f(N, H, W), f(N + 1, H, W), z(H, W), D, BS), R,
     "costvol_subpixel: pattern batch does not match im"),
    ("csubpixel-order-idx-shape-before-dtype", lambda: te.costvol_subpixel(f(N, H, W), f(H, W), z(H, W, dtype=I32), D,
                                                                           BS), R,
     "costvol_subpixel: idx must be shaped as costvol_argmin returns it"),
    # ---- costvol_validity
    ("cvalidity-f64", lambda: te.costvol_validity(f(N, H, W, dtype=F64), f(H, W), z(N, H, W), D, BS), R,
     "im: unsupported dtype torch.float64"),
    ("cvalidity-idx-dtype", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(N, H, W, dtype=I32), D, BS), R,
     "idx: unsupported dtype torch.int32"),
    ("cvalidity-lr-tol", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(N, H, W), D, BS, lr_tol=-1), R,
     "costvol_validity: lr_tol must be an int >= 0"),
    ("cvalidity-type", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(N, H, W), D, BS, type="bogus"), R,
     "costvol_validity: invalid loss type 'bogus'"),
    ("cvalidity-im-rank", lambda: te.costvol_validity(f(N, 1, H, W), f(H, W), z(N, 1, H, W), D, BS), R,
     "costvol_validity expects " + COST_PAIR),
    ("cvalidity-hw", lambda: te.costvol_validity(f(N, H, W), f(H + 1, W), z(N, H, W), D, BS), R,
     "costvol_validity expects " + COST_PAIR),
    ("cvalidity-n", lambda: te.costvol_validity(f(N, H, W), f(N + 1, H, W), z(N, H, W), D, BS), R,
     "costvol_validity: pattern batch does not match im"),
    ("cvalidity-idx-shape", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(H, W), D, BS), R,
     "costvol_validity: idx must be shaped as costvol_argmin returns it"),
    ("cvalidity-algo", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(N, H, W), D, BS, algo="bogus"), R,
     "unknown algo 'bogus'"),
    ("cvalidity-order-lr-tol-before-type", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(N, H, W), D, BS,
                                                                       type="bogus", lr_tol=-1), R,
     "costvol_validity: lr_tol must be an int >= 0"),
    ("cvalidity-order-type-before-rank", lambda: te.costvol_validity(f(N, 1, H, W), f(H, W), z(N, H, W), D, BS,
                                                                     type="bogus"), R,
     "costvol_validity: invalid loss type 'bogus'"),
    ("cvalidity-order-idx-shape-before-algo", lambda: te.costvol_validity(f(N, H, W), f(H, W), z(H, W), D, BS,
                                                                          algo="bogus"), R,
     "costvol_validity: idx must be shaped as costvol_argmin returns it"),
]

for _op, _fn in (("costvol_argmin_band", te.costvol_argmin_band), ("costvol_band_validity", te.costvol_band_validity)):
    def _rows(op=_op, fn=_fn):
        shaped = "%s: %%s must be int32 shaped (%d, %d, %d)" % (op, N, H, W)
        return [
            (op + "-f64", lambda: fn(f(N, H, W), f(H, W, dtype=F64), *band(N, H, W), D, BS), R,
             "pattern: unsupported dtype torch.float64"),
            (op + "-noncontig", lambda: fn(nc(N, H, W), f(H, W), *band(N, H, W), D, BS), R, "im must be contiguous"),
            (op + "-type", lambda: fn(f(N, H, W), f(H, W), *band(N, H, W), D, BS, type="Bogus"), R,
             op + ": invalid loss type 'bogus'"),
            (op + "-im-rank", lambda: fn(f(N, 1, H, W), f(H, W), *band(N, 1, H, W), D, BS), R, op + " expects " + COST_PAIR),
            (op + "-pattern-rank", lambda: fn(f(N, H, W), f(W), *band(N, H, W), D, BS), R, op + " expects " + COST_PAIR),
            (op + "-hw", lambda: fn(f(N, H, W), f(H, W + 1), *band(N, H, W), D, BS), R, op + " expects " + COST_PAIR),
            (op + "-n", lambda: fn(f(N, H, W), f(N + 1, H, W), *band(N, H, W), D, BS), R,
             op + ": pattern batch does not match im"),
            (op + "-lo-dtype", lambda: fn(f(N, H, W), f(H, W), z(N, H, W), band(N, H, W)[1], D, BS), R,
             "lo: unsupported dtype torch.int64"),
            (op + "-lo-shape", lambda: fn(f(N, H, W), f(H, W), z(H, W, dtype=I32), band(N, H, W)[1], D, BS), R,
             shaped % "lo"),
            (op + "-hi-shape", lambda: fn(f(N, H, W), f(H, W), band(N, H, W)[0], z(N, H, W + 1, dtype=I32), D, BS), R,
             shaped % "hi"),
            (op + "-mode", lambda: fn(f(N, H, W), f(H, W), *band(N, H, W), D, BS, subpixel="cubic"), R, MODE % op),
            (op + "-order-mode-before-type", lambda: fn(f(N, H, W), f(H, W), *band(N, H, W), D, BS, type="bogus",
                                                        subpixel="cubic"), R, MODE % op),
            (op + "-order-type-before-rank", lambda: fn(f(N, 1, H, W), f(H, W), *band(N, H, W), D, BS, type="bogus"), R,
             op + ": invalid loss type 'bogus'"),
            (op + "-order-n-before-lo", lambda: fn(f(N, H, W), f(N + 1, H, W), z(N, H, W), band(N, H, W)[1], D, BS), R,
             op + ": pattern batch does not match im"),
            (op + "-order-lo-shape-before-hi-dtype", lambda: fn(f(N, H, W), f(H, W), z(H, W, dtype=I32), z(N, H, W), D,
                                                                BS), R, shaped % "lo"),
        ]
    COST_ROWS += _rows()

COST_ROWS += [
    ("costvol_band_validity-min-gap", lambda: te.costvol_band_validity(f(N, H, W), f(H, W), *band(N, H, W), D, BS,
                                                                       min_gap=-0.5), R,
     "costvol_band_validity: min_gap must be a number >= 0"),
    ("costvol_band_validity-order-lr-tol-before-type", lambda: te.costvol_band_validity(
        f(N, H, W), f(H, W), *band(N, H, W), D, BS, type="bogus", lr_tol=0.5), R,
     "costvol_band_validity: lr_tol must be an int >= 0"),
]


def _reject(call, exc, message):
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value) is exc and str(e.value) == message, (type(e.value), str(e.value))


@pytest.mark.parametrize("call,exc,message", [r[1:] for r in NCC_ROWS], ids=[r[0] for r in NCC_ROWS])
def test_ncc_pair_op_rejects(call, exc, message):
    _reject(call, exc, message)


@pytest.mark.parametrize("call,exc,message", [r[1:] for r in COST_ROWS], ids=[r[0] for r in COST_ROWS])
def test_cost_pair_op_rejects(call, exc, message):
    _reject(call, exc, message)


def test_row_ids_are_unique_and_every_op_has_rows():
    ids = [r[0] for r in NCC_ROWS + COST_ROWS]
    assert len(ids) == len(set(ids))
    for prefix in ("xcorrvol-", "batch-", "argmax-", "lcnargmax-", "subpixel-", "validity-", "prepare-",
                   "xcorrvol_argmax_band-", "xcorrvol_band_validity-", "costvol-", "argmin-", "csubpixel-", "cvalidity-",
                   "costvol_argmin_band-", "costvol_band_validity-"):
        assert sum(i.startswith(prefix) for i in ids) >= 6, prefix


# ---- one accepted call per op: the documented shapes and dtypes come back
AN, AH, AW, AD = 2, 16, 32, 8
U8 = torch.uint8


def _aband(*shape):
    return z(*shape, dtype=I32), torch.full(shape, AD - 1, device="cuda", dtype=I32)


_M, _V = (AN, AH, AW), (AN, AD, AH, AW)                                   # a map, a volume
_MATCH = [(_M, I64), (_M, F32)]
_FLAGS = [(_M, U8), (_M, I64), (_M, F32)]
ACCEPTED = [
    ("xcorrvol", lambda: (te.xcorrvol(f(1, AH, AW), f(1, AH, AW), AD, BS),), [((AD, AH, AW), F32)]),
    ("xcorrvol-f64", lambda: (te.xcorrvol(f(2, AH, AW, dtype=F64), f(2, AH, AW, dtype=F64), AD, BS),),
     [((AD, AH, AW), F64)]),
    ("xcorrvol_batch", lambda: (te.xcorrvol_batch(f(AN, 1, AH, AW), f(AN, 1, AH, AW), AD, BS),), [(_V, F32)]),
    ("xcorrvol_argmax", lambda: te.xcorrvol_argmax(f(AN, 1, AH, AW), f(1, AH, AW), AD, BS, return_volume=True),
     _MATCH + [(_V, F32)]),
    ("xcorrvol_argmax-larger-pattern-batch",       # the pattern's batch is not compared with N: the first N are read
     lambda: te.xcorrvol_argmax(f(AN, 1, AH, AW), f(AN + 1, 1, AH, AW), AD, BS), _MATCH),
    ("lcn_xcorrvol_argmax", lambda: te.lcn_xcorrvol_argmax(f(AN, 1, AH, AW), f(1, AH, AW), AD, BS),
     [((AN, 1, AH, AW), F32)] * 2 + _MATCH),
    ("xcorrvol_subpixel", lambda: te.xcorrvol_subpixel(f(AN, 1, AH, AW), f(1, AH, AW), z(*_M), AD, BS),
     [(_M, F32), (_M, U8)]),
    ("xcorrvol_validity", lambda: te.xcorrvol_validity(f(AN, 1, AH, AW), f(1, AH, AW), z(*_M), AD, BS), _FLAGS),
    ("xcorrvol_argmax_band", lambda: te.xcorrvol_argmax_band(f(AN, 1, AH, AW), f(1, AH, AW), *_aband(*_M), AD, BS), _MATCH),
    ("xcorrvol_band_validity", lambda: te.xcorrvol_band_validity(f(AN, 1, AH, AW), f(1, AH, AW), *_aband(*_M), AD, BS),
     _MATCH + _FLAGS),
    ("prepare_pattern", lambda: (te.prepare_pattern(f(1, AH, AW), AN, AD, BS).workspace,), None),
    ("costvol", lambda: (te.costvol(f(AN, AH, AW), f(AH, AW), AD, BS),), [(_V, F32)]),
    ("costvol_argmin", lambda: te.costvol_argmin(f(AN, AH, AW), f(AH, AW), AD, BS), _MATCH),
    ("costvol_subpixel", lambda: te.costvol_subpixel(f(AN, AH, AW), f(AH, AW), z(*_M), AD, BS), [(_M, F32), (_M, U8)]),
    ("costvol_validity", lambda: te.costvol_validity(f(AN, AH, AW), f(AH, AW), z(*_M), AD, BS), _FLAGS),
    ("costvol_argmin_band", lambda: te.costvol_argmin_band(f(AN, AH, AW), f(AH, AW), *_aband(*_M), AD, BS), _MATCH),
    ("costvol_band_validity", lambda: te.costvol_band_validity(f(AN, AH, AW), f(AH, AW), *_aband(*_M), AD, BS),
     _MATCH + _FLAGS),
]


@pytest.mark.parametrize("call,expected", [r[1:] for r in ACCEPTED], ids=[r[0] for r in ACCEPTED])
def test_accepted_call_returns_the_documented_shapes(call, expected):
    out = call()
    torch.cuda.synchronize()
    if expected is None:                                   # prepare_pattern: a handle with a byte workspace on the device
        assert out[0].dtype == U8 and out[0].is_cuda and out[0].dim() == 1
        return
    assert [(tuple(t.shape), t.dtype) for t in out] == [(tuple(s), d) for s, d in expected]
