"""CPU-only checks of forward depth warping and the windowed band (include/ctd_hip_warp.h: ctd_depth_warp_f32,
ctd_disparity_band_window_f32; torchext.depth_warp, disparity_band_window, depth_to_disp): argument validation before
any HIP call and its precedence, the workspace query, the Python surface's own errors, `depth_to_disp` pinned by hand,
and the restatements of tests/warp_ref.py -- on hand-written inputs, against `disparity_band`, and for the two
properties that make a warped prior worth having.  (The header against its ctypes table and the built library:
tests/test_abi_and_host.py.)"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import warp_ref as wr

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


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


B, V, H, W = 2, 3, 4, 5


def test_warp_rejections_need_no_gpu(L):
    nws = L.ctd_depth_warp_workspace_bytes(B, V, H, W)
    assert 8 * B * V * H * W == 960 and nws == 1024                     # 8 bytes per output pixel, rounded up to 256
    ws = _Buf(nws)
    p = ws.ptr

    def call(splat=0, B=B, V=V, H=H, W=W, ptrs=None, valid=p, sources=p, targets=p, src=p, wsp="ws", nbytes=None):
        d = dict(depth=p, ray=p, K=p, R=p, t=p, z=p)
        d.update(ptrs or {})
        return L.ctd_depth_warp_f32(d["depth"], valid, d["ray"], d["K"], d["R"], d["t"], sources, targets, splat, d["z"], src,
                                    B, V, H, W, p if wsp == "ws" else wsp, nws if nbytes is None else nbytes, -1, None)

    assert call(splat=-1) == INVALID_ARG
    assert call(splat=3) == INVALID_ARG
    assert call(V=0) == INVALID_ARG
    assert call(H=0) == INVALID_ARG
    assert call(W=-2) == INVALID_ARG
    assert call(B=-1) == INVALID_ARG
    assert call(V=65, H=1, W=1) == INVALID_ARG
    every = ("depth", "ray", "K", "R", "t", "z")
    for k in every:
        assert call(ptrs={k: None}) == INVALID_ARG, k
    big_track = dict(B=0, V=64, H=1 << 13, W=1 << 13)                 # V * H * W = 2^32 (and no track at all)
    big_all = dict(B=1 << 11, V=1, H=1 << 10, W=1 << 10)              # B * V * H * W = 2^31
    assert call(**big_track) == UNSUPPORTED
    assert call(**big_all) == UNSUPPORTED
    assert call(B=1, V=2, H=1 << 15, W=1 << 15) == UNSUPPORTED          # 2^31 pixels in one track
    assert call(wsp=None) == WORKSPACE                                  # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(wsp=p + 8) == WORKSPACE
    # precedence: INVALID_ARG, then UNSUPPORTED, then WORKSPACE
    assert call(wsp=None, **big_all) == UNSUPPORTED
    assert call(wsp=None, splat=3, **big_all) == INVALID_ARG
    assert call(wsp=None, ptrs={"z": None}, **big_all) == INVALID_ARG
    assert call(wsp=None, ptrs={k: None for k in every}) == INVALID_ARG
    assert call(wsp=None, splat=5) == INVALID_ARG
    assert call(wsp=None, V=65) == INVALID_ARG
    # what may be NULL: valid, the two masks and src never turn a call down (the workspace does, behind them)
    assert call(valid=None, sources=None, targets=None, src=None, nbytes=0) == WORKSPACE
    # no tracks: nothing to do, nothing touched, no workspace needed
    assert call(B=0, wsp=None, nbytes=0) == OK
    assert call(B=0, wsp=None, nbytes=0, valid=None, sources=None, targets=None, src=None, splat=2) == OK
    assert call(B=0, wsp=None, nbytes=0, splat=3) == INVALID_ARG
    assert call(B=0, wsp=None, nbytes=0, ptrs={"depth": None}) == INVALID_ARG


def test_warp_workspace_query(L):
    for b, v, h, w in [(4, 4, 432, 512), (1, 2, 5, 7), (2, 3, 17, 65), (1, 1, 1, 1), (1, 64, 3, 3), (3, 5, 1, 75)]:
        n = L.ctd_depth_warp_workspace_bytes(b, v, h, w)
        assert n == (8 * b * v * h * w + 255) // 256 * 256 and n > 0
    for args in ((0, 4, 432, 512), (-1, 4, 432, 512), (1, 0, 432, 512), (1, 4, 0, 512), (1, 4, 432, 0), (1, 4, -3, 512),
                 (1, 65, 4, 4), (1, 64, 1 << 13, 1 << 13), (1 << 11, 1, 1 << 10, 1 << 10)):
        assert L.ctd_depth_warp_workspace_bytes(*args) == 0, args


def test_band_window_rejections_need_no_gpu(L):
    p = _Buf(64).ptr

    def call(window=3, holes=1, D=8, N=1, H=H, W=W, ptrs=(p, p, p), radius=1.0):
        return L.ctd_disparity_band_window_f32(ptrs[0], radius, D, window, holes, ptrs[1], ptrs[2], N, H, W, -1, None)

    for window in (0, 2, 4, 14, 16, 17, -1, -3):
        assert call(window=window) == INVALID_ARG, window
    assert call(holes=2) == INVALID_ARG
    assert call(holes=-1) == INVALID_ARG
    assert call(D=0) == INVALID_ARG
    assert call(H=0) == INVALID_ARG
    assert call(W=-1) == INVALID_ARG
    assert call(N=-1) == INVALID_ARG
    for k in range(3):
        ptrs = [p] * 3
        ptrs[k] = None
        assert call(ptrs=tuple(ptrs)) == INVALID_ARG
    big = dict(N=1 << 11, H=1 << 10, W=1 << 10)                       # N * H * W = 2^31
    assert call(**big) == UNSUPPORTED
    assert call(window=15, holes=0, **big) == UNSUPPORTED
    assert call(window=2, **big) == INVALID_ARG                       # precedence
    assert call(holes=3, **big) == INVALID_ARG
    assert call(ptrs=(None,) * 3, **big) == INVALID_ARG
    assert call(N=0) == OK                                            # nothing to do, nothing touched
    assert call(N=0, window=15, holes=0, radius=math.nan) == OK
    assert call(N=0, window=6) == INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_depth_to_disp_pinned_values(te):
    d = torch.tensor([0.0, -0.0, -2.0, math.nan, math.inf, -math.inf, 2.5, 3.0, 1e-30], dtype=torch.float32)
    out = te.depth_to_disp(d, 100.0)
    assert out.dtype == torch.float32 and out.shape == d.shape
    assert torch.isnan(out[:6]).all() and not torch.isnan(out[6:]).any()
    assert float(out[6]) == 40.0
    assert float(out[7]) == float(np.float32(100.0) / np.float32(3.0))
    assert float(out[8]) == float(np.float32(100.0) / np.float32(1e-30))             # large but finite
    out = te.depth_to_disp(d, 100.0, 0.5)
    assert torch.isnan(out[:6]).all()
    assert float(out[6]) == 39.5 and float(out[7]) == float(np.float32(100.0) / np.float32(3.0) - np.float32(0.5))
    # the inverse of idx_to_depth's formula, depth = bf / (idx + offset), where that is exact
    idx = torch.tensor([[1.0, 4.0], [16.0, 64.0]])
    assert torch.equal(te.depth_to_disp(128.0 / (idx + 0.0), 128.0), idx)
    assert te.depth_to_disp(torch.ones(2, 3, 4, 5), 7.0).shape == (2, 3, 4, 5)
    with pytest.raises(RuntimeError):
        te.depth_to_disp(torch.ones(3, dtype=torch.float64), 1.0)
    with pytest.raises(RuntimeError):
        te.depth_to_disp([1.0], 1.0)


def test_python_surface_and_its_errors(te):
    sig = inspect.signature(te.depth_warp)
    assert list(sig.parameters) == ["depth", "ray", "K", "R", "t", "valid", "sources", "targets", "splat", "return_src"]
    assert [sig.parameters[k].default for k in ("valid", "sources", "targets", "splat", "return_src")] == [
        None, None, None, 0, False]
    sig = inspect.signature(te.disparity_band_window)
    assert list(sig.parameters) == ["prior", "radius", "n_disps", "window", "holes"]
    assert sig.parameters["window"].default == 3 and sig.parameters["holes"].default == "full"
    assert list(inspect.signature(te.depth_to_disp).parameters) == ["depth", "baseline_focal", "disp_offset"]
    assert "smallest (z = uvd2, s*H*W + q)" in te.depth_warp.__doc__ and "nearest surface wins" in te.depth_warp.__doc__
    assert "keep of\n    `depth_consistency`" in te.depth_warp.__doc__
    assert "lo = clamp(ceil(m - radius), 0, D)" in te.disparity_band_window.__doc__

    sc = fr.make_scene("clean", 2, 3, 4, 5, 0)
    depth, ray, K, R, t, valid = [torch.from_numpy(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    ones = torch.ones(2, 3, dtype=torch.uint8)
    # splat, before anything else is looked at
    for splat in (-1, 3, 1.0, "1", None, True):
        with pytest.raises(RuntimeError, match="splat must be 0, 1 or 2"):
            te.depth_warp(depth, ray, K, R, t, splat=splat)
    # masks: dtype and shape
    for name in ("sources", "targets"):
        for bad in (torch.ones(2, 3), torch.ones(2, 3, dtype=torch.int32), [[1, 1, 1], [1, 1, 1]]):
            with pytest.raises(RuntimeError, match="%s must be a bool or uint8 tensor" % name):
                te.depth_warp(depth, ray, K, R, t, **{name: bad})
        for bad in (ones[:1], ones.t(), ones.reshape(-1), torch.ones(2, 3, 1, dtype=torch.bool), torch.ones(2, 4, dtype=torch.bool)):
            with pytest.raises(RuntimeError, match=r"%s must be shaped \[B,V\]" % name):
                te.depth_warp(depth, ray, K, R, t, **{name: bad})
    # dtype, shape, device of the rest (no CPU path: well-formed CPU tensors raise too)
    for args in ((depth.double(), ray, K, R, t), (depth, ray.double(), K, R, t), (depth, ray, K, R, t, valid.float()),
                 (depth[0], ray, K, R, t), (depth, ray[:-1], K, R, t), (depth, ray, K[:2], R, t), (depth, ray, K, R[:1], t),
                 (depth, ray, K, R, t[:, :2]), (depth, ray, K, R, t, valid[0]), (depth.numpy(), ray, K, R, t),
                 (depth, ray, K, R, t), (depth, ray, K, R, t, valid, ones, ones, 1, True)):
        with pytest.raises(RuntimeError):
            te.depth_warp(*args)

    prior = torch.zeros(2, 4, 5)
    for window in (0, 2, 4, 16, 17, -3, 3.0, "3", None, True):
        with pytest.raises(RuntimeError, match="window must be an odd integer"):
            te.disparity_band_window(prior, 1.0, 8, window=window)
    for holes in ("", "Full", "none", 0, 1, None, True):
        with pytest.raises(RuntimeError, match="holes must be 'full' or 'empty'"):
            te.disparity_band_window(prior, 1.0, 8, holes=holes)
    for D in (0, -1, 8.0, None):
        with pytest.raises(RuntimeError, match="n_disps must be an integer >= 1"):
            te.disparity_band_window(prior, 1.0, D)
    for radius in (None, "1", torch.ones(2, 4, 5)):
        with pytest.raises(RuntimeError, match="radius must be a number"):
            te.disparity_band_window(prior, radius, 8)
    for bad in (prior.double(), prior.to(torch.int32), prior.numpy()):
        with pytest.raises(RuntimeError, match="prior must be a float32 tensor"):
            te.disparity_band_window(bad, 1.0, 8)
    for bad in (prior[0, 0], prior[None], torch.zeros(2, 0, 5), torch.zeros(4, 0)):
        with pytest.raises(RuntimeError, match=r"expects prior \[N,H,W\] or \[H,W\]"):
            te.disparity_band_window(bad, 1.0, 8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):                # no CPU path
        te.disparity_band_window(prior, 1.0, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatements themselves
# ---------------------------------------------------------------------------------------------------------------------
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def test_band_restatement_on_a_hand_written_prior():
    """5 x 7, D = 16: a hole region on the left, a foreground / background edge between columns 3 and 4, and values
    below 0 and above D on the right"""
    D = 16
    prior = np.array([[NAN, NAN, NAN, 3.0, 9.5, 9.5, 20.0],
                      [NAN, NAN, NAN, 3.0, 9.5, 9.5, 20.0],
                      [NAN, NAN, INF, 3.25, 9.5, -4.0, -INF],
                      [NAN, NAN, NAN, 3.0, 9.5, 9.5, 15.5],
                      [NAN, NAN, NAN, 3.0, 9.5, 9.5, 17.5]], np.float32)[None]
    # window 1: the per-pixel band; every non-finite prior is a hole
    lo, hi = wr.band_window(prior, 1.0, D, 1, "empty")
    assert lo[0].tolist() == [[16, 16, 16, 2, 9, 9, 16], [16, 16, 16, 2, 9, 9, 16], [16, 16, 16, 3, 9, 0, 16],
                              [16, 16, 16, 2, 9, 9, 15], [16, 16, 16, 2, 9, 9, 16]]
    assert hi[0].tolist() == [[-1, -1, -1, 4, 10, 10, 15], [-1, -1, -1, 4, 10, 10, 15], [-1, -1, -1, 4, 10, -1, -1],
                              [-1, -1, -1, 4, 10, 10, 15], [-1, -1, -1, 4, 10, 10, 15]]
    lo_f, hi_f = wr.band_window(prior, 1.0, D, 1, "full")
    hole = ~np.isfinite(prior)
    assert (lo_f[hole] == 0).all() and (hi_f[hole] == D - 1).all()
    assert np.array_equal(lo_f[~hole], lo[~hole]) and np.array_equal(hi_f[~hole], hi[~hole])
    # window 3: columns 0, 1 see no finite prior at all (rows 1..3 of column 1 see the inf: still a hole); column 2 is
    # filled from column 3; columns 3 and 4 span the edge, [3 - 1, 9.5 + 1]; column 5 sees -4 in rows 1..3 and 20 in
    # rows 0, 1; column 6 clips at the image border
    lo, hi = wr.band_window(prior, 1.0, D, 3, "empty")
    assert lo[0].tolist() == [[16, 16, 2, 2, 2, 9, 9], [16, 16, 2, 2, 0, 0, 0], [16, 16, 2, 2, 0, 0, 0],
                              [16, 16, 2, 2, 0, 0, 0], [16, 16, 2, 2, 2, 9, 9]]
    assert hi[0].tolist() == [[-1, -1, 4, 10, 10, 15, 15], [-1, -1, 4, 10, 10, 15, 15], [-1, -1, 4, 10, 10, 15, 15],
                              [-1, -1, 4, 10, 10, 15, 15], [-1, -1, 4, 10, 10, 15, 15]]
    lo, hi = wr.band_window(prior, 1.0, D, 3, "full")
    assert (lo[0, :, :2] == 0).all() and (hi[0, :, :2] == D - 1).all() and lo[0, 0, 2] == 2 and hi[0, 0, 2] == 4
    # radius 0 keeps exact integers only; a negative or NaN radius empties everything, whatever `holes` is
    lo, hi = wr.band_window(prior, 0.0, D, 1, "empty")
    assert (lo[0, 0, 3], hi[0, 0, 3]) == (3, 3) and (lo[0, 2, 3], hi[0, 2, 3]) == (4, 3) and (lo[0, 0, 4], hi[0, 0, 4]) == (10, 9)
    for radius in (-0.5, math.nan, -math.inf):
        for holes in ("full", "empty"):
            lo, hi = wr.band_window(prior, radius, D, 3, holes)
            assert (lo == D).all() and (hi == -1).all()
    lo, hi = wr.band_window(prior, math.inf, D, 3, "empty")
    assert (lo[0, :, 2:] == 0).all() and (hi[0, :, 2:] == D - 1).all() and (lo[0, :, :2] == D).all()
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and lo.shape == prior.shape


def test_band_restatement_at_window_1_is_disparity_band(te):
    rs = np.random.RandomState(5)
    prior = rs.uniform(-6, 40, (3, 9, 31)).astype(np.float32)
    u = rs.rand(*prior.shape)
    prior[u < 0.15] = np.nan
    prior[(u >= 0.15) & (u < 0.2)] = np.inf
    prior[(u >= 0.2) & (u < 0.25)] = -np.inf
    prior[(u >= 0.25) & (u < 0.4)] = np.round(prior[(u >= 0.25) & (u < 0.4)])          # exact integers: ceil == floor
    for D in (1, 32, 64):
        for radius in (0.0, 1.0, 2.5, 0.3, math.inf, -1.0, math.nan):
            lo, hi = te.disparity_band(torch.from_numpy(prior), radius, D)
            rlo, rhi = wr.band_window(prior, radius, D, 1, "empty")
            assert np.array_equal(rlo, lo.numpy()) and np.array_equal(rhi, hi.numpy()), (D, radius)


def test_warp_restatement_on_a_hand_made_track():
    """two views with the same pose and depth 2 everywhere, a third one shifted so that everything moves one pixel to
    the right in it: view 2 sees view 0's pixel (y, x) at (y, x + 1), and ties go to the lower view"""
    Hh, Ww = 3, 4
    K, ray = fr.camera(Hh, Ww)
    f = float(K[0, 0])
    R = np.tile(np.eye(3, dtype=np.float32), (1, 3, 1, 1))
    t = np.zeros((1, 3, 3), np.float32)
    t[0, 2, 0] = np.float32(2.0 / f)                                      # x_cam = x_world + 2 / f: one pixel at depth 2
    depth = np.full((1, 3, Hh, Ww), 2.0, np.float32)
    depth[0, 0, 1, 1] = np.nan                                            # dead in view 0: view 1 fills in
    depth[0, 1, 1, 1] = 1.5                                               # ... from nearer
    z, src = wr.warp(depth, ray, K, R, t, targets=np.array([[0, 0, 1]]))
    assert np.isnan(z[0, :2]).all() and (src[0, :2] == -1).all()          # not targets
    assert np.isnan(z[0, 2, :, 0]).all() and (src[0, 2, :, 0] == -1).all()   # nothing lands in the first column
    plane = Hh * Ww
    for y in range(Hh):
        for x in range(1, Ww):
            if (y, x) == (1, 2):
                assert z[0, 2, y, x] == np.float32(1.5) and src[0, 2, y, x] == plane + y * Ww + x - 1
            else:
                assert z[0, 2, y, x] == np.float32(2.0) and src[0, 2, y, x] == y * Ww + x - 1, (y, x)
    # without view 0 as a source everything comes from view 1; with splat 1 the first column is covered too
    z1, src1 = wr.warp(depth, ray, K, R, t, sources=np.array([[0, 1, 1]]), targets=np.array([[0, 0, 1]]))
    assert (src1[0, 2, :, 1:] == plane + np.arange(plane).reshape(Hh, Ww)[:, :-1]).all()
    z2, src2 = wr.warp(depth, ray, K, R, t, targets=np.array([[0, 0, 1]]), splat=1)
    assert not np.isnan(z2[0, 2]).any() and (z2[0, 2, :, :] <= 2.0).all()
    assert (z2[0, 2, :, 1:] == 1.5).all() and (src2[0, 2, :, 1:] == plane + Ww + 1).all()   # the near pixel covers 3 x 3
    assert (z2[0, 2, :, 0] == 2.0).all() and src2[0, 2, :, 0].tolist() == [0, 0, 4]         # the lowest index wins ties
    # a single view, and a track without sources: all holes
    z, src = wr.warp(depth[:, :1], ray, K, R[:, :1], t[:, :1])
    assert np.isnan(z).all() and (src == -1).all()
    z, src = wr.warp(depth, ray, K, R, t, sources=np.zeros((1, 3), np.uint8))
    assert np.isnan(z).all() and (src == -1).all()


@pytest.mark.parametrize("shape", [(1, 3, 33, 130), (2, 3, 17, 65), (1, 4, 40, 300)])
def test_a_warped_prior_brackets_the_true_disparity(te, shape):
    """On a scene without occlusion the warp of the other views predicts a view's own depth, and the band around the
    warped disparity contains the true one: bf = 100, D = 64, radius 1, splat 0 and 1, windows 1, 3 and 5, seed 7.
    Every non-hole z within 1 % of the view's depth; every non-empty band contains rint(bf / depth)."""
    Bb, Vv, Hh, Ww = shape
    bf, D, radius = 100.0, 64, 1.0
    sc = fr.make_scene("plane", Bb, Vv, Hh, Ww, 7)
    depth = sc["depth"]
    true_disp = np.rint(np.float32(bf) / depth)
    assert true_disp.min() >= 0 and true_disp.max() <= D - 1
    for splat in (0, 1):
        z, src = wr.warp(depth, sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"], splat=splat)
        hit = ~np.isnan(z)
        assert 0.5 < hit.mean() < 1.0
        assert (np.abs(z[hit] - depth[hit]) <= 0.01 * depth[hit]).all()
        assert ((src >= 0) == hit).all()
        disp = te.depth_to_disp(torch.from_numpy(z), bf).numpy()
        assert np.array_equal(np.isnan(disp), ~hit)
        for window in (1, 3, 5):
            lo, hi = wr.band_window(disp.reshape(Bb * Vv, Hh, Ww), radius, D, window, "empty")
            lo, hi = lo.reshape(depth.shape), hi.reshape(depth.shape)
            some = lo <= hi
            assert some[hit].all() and some.mean() >= hit.mean()
            assert ((lo <= true_disp) & (true_disp <= hi))[some].all(), (splat, window)
            assert (hi - lo + 1)[some].mean() < 4.0
