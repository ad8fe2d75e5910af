"""CPU-only checks of the band matchers' validity (include/ctd_hip_band_validity.h: ctd_xcorrvol_band_validity_f32,
ctd_costvol_band_validity_f32): the definition's sentences (the header against its ctypes table and the built library:
tests/test_abi_and_host.py), argument validation before any HIP call and its precedence, the Python surface, and the restatement
tests/band_validity_ref.py against its element-by-element twin and, with the full band, against tests/validity_ref.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import band_validity_ref as bvr
from tests import validity_ref as vr
from tests.band_ref import band_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BV_HEADER = os.path.join(ROOT, "include", "ctd_hip_band_validity.h")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
PREPARED = 0x100
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_definition():
    text = " ".join(open(BV_HEADER).read().replace("*", " ").split())
    for phrase in ("Pixel (f,h,w) holds disparity d when lo' <= d <= hi'",
                   "It is -1 when no pixel holds a disparity that lands on column x",
                   "so -0.0 and +0.0 tie",
                   "+inf when no such d is held. NaN when idx == -1",
                   "A band of width <= 3 around idx always passes UNIQUE",
                   "That idx_r is never -1, because the pixel's own candidate landed there",
                   "The same bits come out on every run",
                   "the contents of idx_r (and of the other outputs) are unspecified"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation
# ---------------------------------------------------------------------------------------------------------------------
class _Buf:
    """a host buffer standing in for device pointers: validation must reject before it is ever dereferenced"""

    def __init__(self, n):
        self.raw = ctypes.create_string_buffer(n + 512)
        a = ctypes.addressof(self.raw)
        self.ptr = (a + 255) // 256 * 256


H, W, D = 8, 8, 4
N_PTRS = 9                                                        # in0, in1, lo, hi, idx, best, flags, idx_r, gap
BEST = 5


def _null_each(call, ptr):
    for k in range(N_PTRS):
        ptrs = [ptr] * N_PTRS
        ptrs[k] = None
        if k == BEST:
            continue                                               # best may be NULL: such a call would pass validation
        assert call(ptrs=tuple(ptrs)) == INVALID_ARG, k


def test_ncc_rejections_need_no_gpu(L):
    nws = L.ctd_xcorrvol_argmax_band_workspace_bytes(1, H, W, D, 3, 0)
    assert nws > 0
    ws = _Buf(nws)

    def call(bs=3, flags=0, stride=0, H=H, W=W, D=D, frames=1, ptrs=(ws.ptr,) * N_PTRS, wsp="ws", nbytes=None, lr_tol=1,
             min_gap=0.0):
        return L.ctd_xcorrvol_band_validity_f32(ptrs[0], ptrs[1], stride, *ptrs[2:], frames, H, W, D, bs, lr_tol, min_gap,
                                                flags, ws.ptr if wsp == "ws" else wsp, nws if nbytes is None else nbytes,
                                                -1, None)

    # those of the band call
    for flags in (0, PREPARED):
        assert call(bs=8, flags=flags) == INVALID_ARG
        assert call(bs=0, flags=flags) == INVALID_ARG
        assert call(bs=-3, flags=flags) == INVALID_ARG
    assert call(flags=1) == INVALID_ARG
    assert call(flags=PREPARED | 2) == INVALID_ARG
    assert call(stride=7) == INVALID_ARG
    assert call(stride=-1) == INVALID_ARG
    assert call(D=0) == INVALID_ARG
    assert call(H=0) == INVALID_ARG
    assert call(W=-1) == INVALID_ARG
    assert call(frames=-1) == INVALID_ARG
    assert call(H=1 << 12, W=1 << 12, D=128) == INVALID_ARG        # D * H * W = 2^31
    _null_each(call, ws.ptr)
    # the validity parameters
    assert call(lr_tol=-1) == INVALID_ARG
    assert call(min_gap=-1e-30) == INVALID_ARG
    assert call(min_gap=NAN) == INVALID_ARG
    assert call(min_gap=float("-inf")) == INVALID_ARG
    # workspace
    assert call(wsp=None) == WORKSPACE
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(wsp=ws.ptr + 4) == WORKSPACE
    big = dict(frames=1 << 11, H=1 << 10, W=1 << 10, D=1)           # frames * H * W = 2^31
    assert call(**big) == UNSUPPORTED
    # precedence: INVALID_ARG (the band call's, then the validity parameters), then UNSUPPORTED, then WORKSPACE
    assert call(wsp=None, **big) == UNSUPPORTED
    assert call(wsp=None, bs=4, **big) == INVALID_ARG
    assert call(wsp=None, lr_tol=-2, **big) == INVALID_ARG
    assert call(wsp=None, min_gap=NAN, **big) == INVALID_ARG
    assert call(wsp=None, ptrs=(None,) * N_PTRS, **big) == INVALID_ARG
    assert call(wsp=None, bs=4) == INVALID_ARG
    assert call(wsp=None, stride=3) == INVALID_ARG
    assert call(wsp=None, lr_tol=-1) == INVALID_ARG
    assert call(wsp=None, min_gap=-1.0) == INVALID_ARG
    # no frames: nothing to do, nothing touched; the band call's own arguments are still checked, the validity
    # parameters come after it in the order and are not looked at
    none = dict(frames=0, ptrs=(None,) * N_PTRS, wsp=None, nbytes=0)
    assert call(**none) == OK
    assert call(flags=PREPARED, **none) == OK
    assert call(bs=4, **none) == INVALID_ARG
    assert call(lr_tol=-1, **none) == OK
    assert call(min_gap=NAN, **none) == OK


def test_cost_rejections_need_no_gpu(L):
    p = _Buf(64).ptr

    def call(bs=3, ty=3, stride=0, H=H, W=W, D=D, frames=1, ptrs=(p,) * N_PTRS, lr_tol=1, min_gap=0.0):
        return L.ctd_costvol_band_validity_f32(ptrs[0], ptrs[1], stride, *ptrs[2:], frames, H, W, D, bs, ty, 0.5, lr_tol,
                                               min_gap, -1, None)

    assert call(bs=8) == INVALID_ARG
    assert call(bs=0) == INVALID_ARG
    assert call(bs=-1) == INVALID_ARG
    assert call(ty=4) == INVALID_ARG
    assert call(ty=-1) == INVALID_ARG
    assert call(stride=63) == INVALID_ARG
    assert call(D=0) == INVALID_ARG
    assert call(H=0) == INVALID_ARG
    assert call(W=0) == INVALID_ARG
    assert call(frames=-2) == INVALID_ARG
    assert call(H=1 << 12, W=1 << 12, D=128) == INVALID_ARG
    _null_each(call, p)
    assert call(lr_tol=-1) == INVALID_ARG
    assert call(min_gap=-0.5) == INVALID_ARG
    assert call(min_gap=NAN) == INVALID_ARG
    big = dict(frames=1 << 11, H=1 << 10, W=1 << 10, D=1)
    assert call(**big) == UNSUPPORTED
    assert call(ty=7, **big) == INVALID_ARG
    assert call(lr_tol=-1, **big) == INVALID_ARG
    assert call(min_gap=NAN, **big) == INVALID_ARG
    assert call(ptrs=(None,) * N_PTRS, **big) == INVALID_ARG
    assert call(frames=0, ptrs=(None,) * N_PTRS) == OK
    assert call(frames=0, ty=4, ptrs=(None,) * N_PTRS) == INVALID_ARG
    assert call(frames=0, lr_tol=-1, ptrs=(None,) * N_PTRS) == OK


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    from connecting_the_dots_amd import torchext as te
    sig = inspect.signature(te.xcorrvol_band_validity)
    assert list(sig.parameters) == ["in0", "in1", "lo", "hi", "n_disps", "block_size", "lr_tol", "min_gap", "prepared",
                                    "subpixel"]
    assert [sig.parameters[k].default for k in ("lr_tol", "min_gap", "prepared", "subpixel")] == [1, 0.0, None, None]
    sig = inspect.signature(te.costvol_band_validity)
    assert list(sig.parameters) == ["im", "pattern", "lo", "hi", "n_disps", "block_size", "type", "eps", "lr_tol",
                                    "min_gap", "subpixel"]
    assert [sig.parameters[k].default for k in ("type", "eps", "lr_tol", "min_gap", "subpixel")] == \
        ["census_sad", 0.1, 1, 0.0, None]
    for fn in (te.xcorrvol_band_validity, te.costvol_band_validity):
        assert "A band of width <= 3 around idx always passes UNIQUE" in fn.__doc__
        assert "lo' = max(lo, 0), hi' = min(hi, D-1)" in fn.__doc__
    # the band functions keep their signatures: the validity is a function of its own, not a keyword
    assert "lr_tol" not in inspect.signature(te.xcorrvol_argmax_band).parameters
    assert "lr_tol" not in inspect.signature(te.costvol_argmin_band).parameters
    x = torch.zeros(1, 1, 4, 4)
    r = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError):                              # no CPU path
        te.xcorrvol_band_validity(x, x[0], r, r, 2, 3)
    with pytest.raises(RuntimeError):
        te.costvol_band_validity(x[0], x[0, 0], r, r, 2, 3)
    for bad in (dict(lr_tol=-1), dict(lr_tol=1.5), dict(min_gap=-1.0), dict(min_gap=NAN)):
        with pytest.raises(RuntimeError, match="lr_tol|min_gap"):
            te.xcorrvol_band_validity(x, x[0], r, r, 2, 3, **bad)
        with pytest.raises(RuntimeError, match="lr_tol|min_gap"):
            te.costvol_band_validity(x[0], x[0, 0], r, r, 2, 3, **bad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b, what, zero_sign=True):
    """bit for bit, NaN positions equal; zero_sign=False: -0.0 and +0.0 count as equal"""
    for name, x, y in zip(("idx", "best", "flags", "idx_r", "gap"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        if x.dtype == np.float32:
            assert np.array_equal(np.isnan(x), np.isnan(y)), (what, name)
            x, y = np.nan_to_num(x, nan=7.0, posinf=np.inf, neginf=-np.inf), np.nan_to_num(y, nan=7.0, posinf=np.inf, neginf=-np.inf)
            if not zero_sign:
                x, y = x + np.float32(0), y + np.float32(0)
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (what, name)
        else:
            assert np.array_equal(x, y), (what, name)


def _volumes(rs, N, Dd, Hh, Ww):
    """name, volume, whether the sign of a zero is determined: a real volume holds zeros of one sign only (NCC scores
    and costs are sums that start at +0), and which of two tying zeros is "the best" is not part of the definition"""
    yield "random", rs.randn(N, Dd, Hh, Ww).astype(np.float32), True
    yield "ties", rs.choice(np.array([-1.0, 0.0, 0.5, 2.0], np.float32), size=(N, Dd, Hh, Ww)), True
    yield "constant", np.zeros((N, Dd, Hh, Ww), np.float32), True
    yield "signed zeros", rs.choice(np.array([-0.0, 0.0], np.float32), size=(N, Dd, Hh, Ww)), False


def _bands(rs, N, Dd, Hh, Ww):
    lo = rs.randint(-2, Dd + 2, size=(N, Hh, Ww)).astype(np.int32)
    hi = (lo + rs.randint(-2, Dd + 1, size=(N, Hh, Ww))).astype(np.int32)        # a share of them empty
    yield "random", lo, hi
    d = rs.randint(0, Dd, size=(N, Hh, Ww)).astype(np.int32)
    yield "width1", d, d.copy()
    yield "full", np.zeros((N, Hh, Ww), np.int32), np.full((N, Hh, Ww), Dd - 1, np.int32)
    yield "empty", np.full((N, Hh, Ww), Dd, np.int32), np.full((N, Hh, Ww), -1, np.int32)


@pytest.mark.parametrize("shape", [(2, 4, 3, 7), (1, 6, 2, 4), (1, 1, 2, 5), (2, 3, 2, 9)])
def test_ref_equals_naive(shape):
    N, Dd, Hh, Ww = shape
    rs = np.random.RandomState(sum(shape))
    n_empty = n_minus = 0
    for vname, vol, zero_sign in _volumes(rs, N, Dd, Hh, Ww):
        for bname, lo, hi in _bands(rs, N, Dd, Hh, Ww):
            for maximise in (True, False):
                for lr_tol, min_gap in ((0, 0.0), (1, 0.25)):
                    a = bvr.band_validity_ref(vol, lo, hi, maximise, lr_tol, min_gap)
                    b = bvr.naive(vol, lo, hi, maximise, lr_tol, min_gap)
                    _same(a, b, (vname, bname, maximise, lr_tol, min_gap), zero_sign)
                    idx, best, flags, idx_r, gap = a
                    assert np.array_equal(np.isnan(gap), idx < 0) and np.array_equal(np.isnan(best), idx < 0)
                    assert not (flags[idx < 0]).any()
                    n_empty += int((idx < 0).sum())
                    n_minus += int((idx_r < 0).sum())
                    if bname == "empty":
                        assert (idx < 0).all() and (idx_r < 0).all()
                    if bname == "width1":
                        assert np.isinf(gap).all() and ((flags & bvr.UNIQUE) != 0).all()
                    i2, b2 = band_ref(torch.from_numpy(vol), torch.from_numpy(lo), torch.from_numpy(hi), maximise)
                    assert np.array_equal(idx, i2.numpy())
                    _same((best,), (b2.numpy(),), (vname, bname, "band_ref"))
    assert n_empty > 0 and n_minus > 0


@pytest.mark.parametrize("shape", [(2, 4, 3, 7), (1, 9, 2, 5), (1, 1, 3, 4)])
def test_full_band_is_the_validity_rule_of_the_volume(shape):
    N, Dd, Hh, Ww = shape
    rs = np.random.RandomState(sum(shape) + 1)
    lo = np.zeros((N, Hh, Ww), np.int32)
    hi = np.full((N, Hh, Ww), Dd - 1, np.int32)
    for vname, vol, zero_sign in _volumes(rs, N, Dd, Hh, Ww):
        for maximise in (True, False):
            for lr_tol, min_gap in ((0, 0.0), (1, 0.0), (3, 0.25)):
                idx, best, flags, idx_r, gap = bvr.band_validity_ref(vol, lo, hi, maximise, lr_tol, min_gap)
                ridx, _ = band_ref(torch.from_numpy(vol), torch.from_numpy(lo), torch.from_numpy(hi), maximise)
                assert np.array_equal(idx, ridx.numpy())
                f2, r2, g2 = vr.validity_ref(vol, ridx.numpy(), maximise, lr_tol, min_gap)
                assert np.array_equal(flags, f2), (vname, maximise)
                assert np.array_equal(idx_r, r2), (vname, maximise)
                _same((gap,), (g2,), (vname, maximise), zero_sign)


def test_ref_on_a_hand_written_row():
    # one row, W = 4, D = 3, scores (NCC: higher is better) V[d][w]
    vol = np.array([[[[5, 1, 2, 9]], [[6, 8, 2, 1]], [[7, 3, 2, 9]]]], np.float32).reshape(1, 3, 1, 4)
    lo = np.array([[[0, 1, 0, 2]]], np.int32)
    hi = np.array([[[2, 1, -1, 5]]], np.int32)              # w0 holds 0..2, w1 holds 1, w2 nothing, w3 holds 2
    idx, best, flags, idx_r, gap = bvr.band_validity_ref(vol, lo, hi, True, 0, 0.0)
    assert idx[0, 0].tolist() == [2, 1, -1, 2]
    assert best[0, 0, [0, 1, 3]].tolist() == [7.0, 8.0, 9.0] and np.isnan(best[0, 0, 2])
    # column 0: d = 0 from w0 (5), d = 1 from w1 (8), d = 2 from w2 (not held) -> 1; column 1: d = 2 from w3 (9) -> 2;
    # columns 2, 3: w2 holds nothing, w3 does not hold 0 -> -1
    assert idx_r[0, 0].tolist() == [1, 2, -1, -1]
    assert gap[0, 0, 0] == 2.0 and np.isinf(gap[0, 0, 1]) and np.isnan(gap[0, 0, 2]) and np.isinf(gap[0, 0, 3])
    # w0: idx 2, w - idx < 0 -> UNIQUE only; w1: column 0 says 1 -> 7; w3: column 1 says 2 -> 7
    assert flags[0, 0].tolist() == [4, 7, 0, 7]
