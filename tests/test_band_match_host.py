"""CPU-only checks of band-limited matching (include/ctd_hip_band.h: ctd_xcorrvol_argmax_band_f32,
ctd_costvol_argmin_band_f32): argument validation before any HIP call and its precedence, the workspace query,
`disparity_band` on CPU tensors and the restatement tests/band_ref.py on a hand-written volume.  (The header against its
ctypes table and the built library: tests/test_abi_and_host.py.)"""
import ctypes
import inspect
import math

import pytest
import torch

from tests.band_ref import band_ref

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
PREPARED = 0x100


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. header == table == exports: tests/test_abi_and_host.py, for every header
# 2. validation
# ---------------------------------------------------------------------------------------------------------------------
class _Buf:
    """a host buffer standing in for device pointers: validation must reject before it is ever dereferenced"""

    def __init__(self, n):
        self.raw = ctypes.create_string_buffer(n + 512)
        a = ctypes.addressof(self.raw)
        self.ptr = (a + 255) // 256 * 256


H, W, D = 8, 8, 4


def _ncc(L, ws, nws, bs=3, flags=0, stride=0, H=H, W=W, D=D, frames=1, ptrs=None, best=None, wsp="ws", nbytes=None):
    p = ws.ptr
    ptrs = (p,) * 5 if ptrs is None else ptrs               # in0, in1, lo, hi, idx
    return L.ctd_xcorrvol_argmax_band_f32(ptrs[0], ptrs[1], stride, ptrs[2], ptrs[3], ptrs[4], best, frames, H, W, D, bs,
                                          flags, ws.ptr if wsp == "ws" else wsp, nws if nbytes is None else nbytes, -1,
                                          None)


def test_ncc_rejections_need_no_gpu(L):
    nws = L.ctd_xcorrvol_argmax_band_workspace_bytes(1, H, W, D, 3, 0)
    assert nws > 0
    ws = _Buf(nws)

    def call(**kw):
        return _ncc(L, ws, nws, **kw)

    for flags in (0, PREPARED):
        assert call(bs=8, flags=flags) == INVALID_ARG              # even, zero, negative block size
        assert call(bs=0, flags=flags) == INVALID_ARG
        assert call(bs=-3, flags=flags) == INVALID_ARG
    assert call(flags=1) == INVALID_ARG                            # flags other than 0 / CTD_PATTERN_PREPARED
    assert call(flags=PREPARED | 2) == INVALID_ARG
    assert call(stride=7) == INVALID_ARG                           # stride neither 0 nor H * W
    assert call(stride=-1) == INVALID_ARG
    assert call(D=0) == INVALID_ARG
    assert call(H=0) == INVALID_ARG
    assert call(W=-1) == INVALID_ARG
    assert call(frames=-1) == INVALID_ARG
    assert call(H=1 << 12, W=1 << 12, D=128) == INVALID_ARG        # D * H * W = 2^31
    for k in range(5):                                             # NULL in0 / in1 / lo / hi / idx
        ptrs = [ws.ptr] * 5
        ptrs[k] = None
        assert call(ptrs=tuple(ptrs)) == INVALID_ARG
    assert call(wsp=None) == WORKSPACE                             # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(wsp=ws.ptr + 4) == WORKSPACE
    big = dict(frames=1 << 11, H=1 << 10, W=1 << 10, D=1)           # frames * H * W = 2^31
    assert call(**big) == UNSUPPORTED
    # precedence: INVALID_ARG, then UNSUPPORTED, then WORKSPACE
    assert call(wsp=None, **big) == UNSUPPORTED
    assert call(wsp=None, bs=4, **big) == INVALID_ARG
    assert call(wsp=None, ptrs=(None,) * 5, **big) == INVALID_ARG
    assert call(wsp=None, bs=4) == INVALID_ARG
    assert call(wsp=None, stride=3) == INVALID_ARG
    # no frames: nothing to do, nothing touched
    assert call(frames=0, ptrs=(None,) * 5, wsp=None, nbytes=0) == OK
    assert call(frames=0, ptrs=(None,) * 5, wsp=None, nbytes=0, flags=PREPARED) == OK
    assert call(frames=0, bs=4, ptrs=(None,) * 5, wsp=None, nbytes=0) == INVALID_ARG


def test_cost_rejections_need_no_gpu(L):
    p = _Buf(64).ptr

    def call(bs=3, ty=3, stride=0, H=H, W=W, D=D, frames=1, ptrs=(p,) * 5):
        return L.ctd_costvol_argmin_band_f32(ptrs[0], ptrs[1], stride, ptrs[2], ptrs[3], ptrs[4], None, frames, H, W, D,
                                             bs, ty, 0.5, -1, None)

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
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert call(ptrs=tuple(ptrs)) == INVALID_ARG
    big = dict(frames=1 << 11, H=1 << 10, W=1 << 10, D=1)
    assert call(**big) == UNSUPPORTED
    assert call(ty=7, **big) == INVALID_ARG
    assert call(ptrs=(None,) * 5, **big) == INVALID_ARG
    assert call(frames=0, ptrs=(None,) * 5) == OK
    assert call(frames=0, ty=4, ptrs=(None,) * 5) == INVALID_ARG


def test_workspace_query_is_the_subpixel_ops(L):
    shapes = [(16, 432, 512, 128, 9), (1, 5, 7, 4, 3), (3, 33, 70, 64, 7), (2, 10, 18, 8, 11), (1, 9, 9, 1, 9)]
    for frames, h, w, d, bs in shapes:
        for per_frame in (0, 1):
            n = L.ctd_xcorrvol_argmax_band_workspace_bytes(frames, h, w, d, bs, per_frame)
            assert n == L.ctd_xcorrvol_subpixel_workspace_bytes(frames, h, w, d, bs, per_frame) and n > 0 and n % 256 == 0
    for args in ((0, 432, 512, 128, 9, 0), (1, 0, 512, 128, 9, 0), (1, 432, 0, 128, 9, 0), (1, 432, 512, 0, 9, 0),
                 (1, 432, 512, 128, 8, 0), (1, 432, 512, 128, -1, 0), (-1, 432, 512, 128, 9, 0),
                 (1, 1 << 12, 1 << 12, 128, 9, 0)):
        assert L.ctd_xcorrvol_argmax_band_workspace_bytes(*args) == 0, args


# ---------------------------------------------------------------------------------------------------------------------
# 3. disparity_band, pinned by hand
# ---------------------------------------------------------------------------------------------------------------------
def _band(prior, radius, D=16):
    from connecting_the_dots_amd import torchext as te
    lo, hi = te.disparity_band(torch.tensor(prior, dtype=torch.float32), radius, D)
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32
    return lo.tolist(), hi.tolist()


def test_disparity_band_pinned_values():
    D = 16
    assert _band([2.5], 1) == ([2], [3])
    lo, hi = _band([0.2], 0)
    assert (lo, hi) == ([1], [0]) and lo[0] > hi[0]                # no integer within [0.2, 0.2]: empty
    assert _band([3.0], 0) == ([3], [3])
    lo, hi = _band([-5.0], 2)
    assert (lo, hi) == ([0], [-1])                                 # wholly left of the range: empty
    assert _band([D + 1.0], 3) == ([D - 2], [D - 1])
    assert _band([D + 5.0], 3) == ([D], [D - 1])                   # wholly right of it: empty
    assert _band([7.0], 1000.0) == ([0], [D - 1])
    assert _band([7.0], math.inf) == ([0], [D - 1])
    for prior in (math.nan, math.inf, -math.inf):
        assert _band([prior], 2) == ([D], [-1])
    assert _band([4.0], -0.5) == ([D], [-1])
    assert _band([4.0], math.nan) == ([D], [-1])
    assert _band([4.0], -math.inf) == ([D], [-1])


def test_disparity_band_tensor_radius_and_shapes():
    from connecting_the_dots_amd import torchext as te
    D = 8
    prior = torch.tensor([[1.5, 4.0, 6.25], [0.0, 7.9, math.nan]], dtype=torch.float32)
    radius = torch.tensor([[0.5, 2.0, 3.0], [0.0, 0.5, 1.0]])
    lo, hi = te.disparity_band(prior, radius, D)
    assert lo.shape == prior.shape and hi.shape == prior.shape and lo.is_contiguous() and hi.is_contiguous()
    assert lo.tolist() == [[1, 2, 4], [0, 8, 8]]
    assert hi.tolist() == [[2, 6, 7], [0, 7, -1]]
    lo, hi = te.disparity_band(prior, torch.tensor([1.0, -1.0, 0.25]), D)      # broadcast along the rows
    assert lo.tolist() == [[1, 8, 6], [0, 8, 8]]
    assert hi.tolist() == [[2, -1, 6], [1, -1, -1]]
    with pytest.raises(RuntimeError):
        te.disparity_band(prior.double(), 1.0, D)


def test_python_surface():
    from connecting_the_dots_amd import torchext as te
    assert list(inspect.signature(te.disparity_band).parameters) == ["prior", "radius", "n_disps"]
    sig = inspect.signature(te.xcorrvol_argmax_band)
    assert list(sig.parameters) == ["in0", "in1", "lo", "hi", "n_disps", "block_size", "prepared", "subpixel"]
    assert sig.parameters["prepared"].default is None and sig.parameters["subpixel"].default is None
    sig = inspect.signature(te.costvol_argmin_band)
    assert list(sig.parameters) == ["im", "pattern", "lo", "hi", "n_disps", "block_size", "type", "eps", "subpixel"]
    assert sig.parameters["type"].default == "census_sad" and sig.parameters["eps"].default == 0.1
    for fn in (te.xcorrvol_argmax_band, te.costvol_argmin_band):
        assert "lo' = max(lo, 0), hi' = min(hi, D-1)" in fn.__doc__
    x = torch.zeros(1, 1, 4, 4)
    r = torch.zeros(1, 4, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError):                              # no CPU path
        te.xcorrvol_argmax_band(x, x[0], r, r, 2, 3)
    with pytest.raises(RuntimeError):
        te.costvol_argmin_band(x[0], x[0, 0], r, r, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_band_ref_on_a_hand_written_volume():
    N, D, Hh, Ww = 2, 4, 3, 3
    vol = torch.zeros(N, D, Hh, Ww)
    # frame 0: per pixel the scores over d
    px = {
        (0, 0, 0): [1.0, 3.0, 3.0, 2.0],        # tie of the maximum at d = 1, 2
        (0, 0, 1): [5.0, 5.0, 5.0, 5.0],        # all equal
        (0, 0, 2): [0.0, -1.0, 4.0, 4.0],       # tie at d = 2, 3
        (0, 1, 0): [2.0, 1.0, 0.0, -1.0],
        (0, 1, 1): [-1.0, 0.0, 1.0, 2.0],
        (0, 1, 2): [1.0, 9.0, 1.0, 9.0],        # tie at d = 1, 3; minimum tie at d = 0, 2
        (1, 2, 2): [-0.0, 0.0, -0.0, 0.0],      # signed zeros compare equal
        (1, 0, 0): [7.0, 6.0, 7.0, 8.0],
    }
    for (n, h, w), s in px.items():
        vol[n, :, h, w] = torch.tensor(s)
    lo = torch.zeros(N, Hh, Ww, dtype=torch.int32)
    hi = torch.full((N, Hh, Ww), D - 1, dtype=torch.int32)
    # the full band: torch's own first-index argmax / argmin on these (the hand-written pixels and the all-zero rest)
    for maximise in (True, False):
        idx, best = band_ref(vol, lo, hi, maximise)
        want = {(0, 0, 0): (1, 0), (0, 0, 1): (0, 0), (0, 0, 2): (2, 1), (0, 1, 0): (0, 3), (0, 1, 1): (3, 0),
                (0, 1, 2): (1, 0), (1, 2, 2): (0, 0), (1, 0, 0): (3, 1), (1, 1, 1): (0, 0)}
        for (n, h, w), (imax, imin) in want.items():
            i = imax if maximise else imin
            assert int(idx[n, h, w]) == i, (n, h, w, maximise)
            assert float(best[n, h, w]) == float(vol[n, i, h, w])
    # restricted, clipped and empty bands
    lo[0, 0, 0], hi[0, 0, 0] = 2, 3             # [2, 3] of 1 3 3 2: max 3.0 at d = 2, min 2.0 at d = 3
    lo[0, 0, 1], hi[0, 0, 1] = -3, 1            # clipped to [0, 1]: equal scores, the first index is 0
    lo[0, 0, 2], hi[0, 0, 2] = 3, 9             # clipped to [3, 3]
    lo[0, 1, 0], hi[0, 1, 0] = 2, 1             # empty
    lo[0, 1, 1], hi[0, 1, 1] = 4, 7             # wholly right of the range: empty
    lo[0, 1, 2], hi[0, 1, 2] = 2, 3             # 1 9: max at 3, min at 2
    lo[1, 2, 2], hi[1, 2, 2] = 1, 3             # signed zeros: the first index of the band
    lo[1, 0, 0], hi[1, 0, 0] = -5, -1           # wholly left: empty
    idx, best = band_ref(vol, lo, hi, True)
    assert idx[0].tolist() == [[2, 0, 3], [-1, -1, 3], [0, 0, 0]]
    assert idx[1].tolist() == [[-1, 0, 0], [0, 0, 0], [0, 0, 1]]
    assert best[0, 0].tolist() == [3.0, 5.0, 4.0] and float(best[0, 1, 2]) == 9.0
    assert math.isnan(float(best[0, 1, 0])) and math.isnan(float(best[0, 1, 1])) and math.isnan(float(best[1, 0, 0]))
    assert torch.isnan(best).sum() == 3 and (idx == -1).sum() == 3
    idx, best = band_ref(vol, lo, hi, False)
    assert idx[0].tolist() == [[3, 0, 3], [-1, -1, 2], [0, 0, 0]]
    assert idx[1].tolist() == [[-1, 0, 0], [0, 0, 0], [0, 0, 1]]
    assert float(best[0, 0, 0]) == 2.0 and float(best[0, 1, 2]) == 1.0
    assert idx.dtype == torch.int64 and best.dtype == torch.float32
