"""Numpy restatements of the two definitions of include/ctd_hip_warp.h: the z-buffered forward warp of a track's views
into each other (ctd_depth_warp_f32) and the windowed disparity band (ctd_disparity_band_window_f32).

The warp stands on tests/fusion_ref.py: `live_mask` is the rule of a live pixel and `transform` the f32 products and sums
of the projection, in the written association.  It forms the 64-bit key (bits(z) << 32) | (s*H*W + q) literally and
reduces the candidates of a target pixel with np.minimum.at, so "smallest z, then smallest source index" is one unsigned
minimum here as it is in the kernel.  The scenes are fusion_ref.make_scene's."""
import numpy as np

from tests import fusion_ref as fr

F = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _view_mask(m, B, V):
    return np.ones((B, V), bool) if m is None else np.asarray(m).reshape(B, V) != 0


def warp(depth, ray, K, R, t, valid=None, sources=None, targets=None, splat=0):
    """-> z f32 [B,V,H,W] (NaN: no candidate), src int64 [B,V,H,W] (-1 there)"""
    B, V, H, W = depth.shape
    assert depth.dtype == F and ray.dtype == F and K.dtype == F and R.dtype == F and t.dtype == F
    assert 0 <= splat <= 2 and V * H * W < 2 ** 32
    live = fr.live_mask(depth, valid)
    src_on, tgt_on = _view_mask(sources, B, V), _view_mask(targets, B, V)
    keys = np.full((B, V, H * W), NO_KEY, np.uint64)
    q = np.arange(H * W, dtype=np.int64)
    for b in range(B):
        for r in range(V):
            if not tgt_on[b, r]:
                continue
            for s in range(V):
                if s == r or not src_on[b, s]:
                    continue
                with np.errstate(all="ignore"):
                    uvd = fr.transform(depth[b, s].reshape(-1), ray, R[b, s], t[b, s], R[b, r], t[b, r], K)
                    z = uvd[2]
                    ok = live[b, s].reshape(-1) & (z > 0) & (z < F(np.inf))
                    xs = np.floor(uvd[0] / z + F(0.5))
                    ys = np.floor(uvd[1] / z + F(0.5))
                    assert z.dtype == F and xs.dtype == F and ys.dtype == F
                    ok &= (xs >= F(-splat)) & (xs <= F(W - 1 + splat)) & (ys >= F(-splat)) & (ys <= F(H - 1 + splat))
                xi = np.where(ok, xs, F(0)).astype(np.int64)
                yi = np.where(ok, ys, F(0)).astype(np.int64)
                key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (s * H * W + q).astype(np.uint64)
                for dy in range(-splat, splat + 1):
                    for dx in range(-splat, splat + 1):
                        y, x = yi + dy, xi + dx
                        c = ok & (y >= 0) & (y < H) & (x >= 0) & (x < W)
                        np.minimum.at(keys[b, r], (y * W + x)[c], key[c])
    hole = keys == NO_KEY
    z = (keys >> np.uint64(32)).astype(np.uint32).view(F)
    z = np.where(hole, F(np.nan), z).reshape(B, V, H, W)
    track = (np.arange(B, dtype=np.int64) * (V * H * W))[:, None, None]
    src = np.where(hole, np.int64(-1), track + (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).reshape(B, V, H, W)
    assert z.dtype == F and src.dtype == np.int64
    return z, src


def band_window(prior, radius, D, window=3, holes="full"):
    """prior f32 [N,H,W] -> lo, hi int32 [N,H,W].  Min and max over the clipped window by shifting: a hole (a non-finite
    prior, a pixel outside the image) is +inf for the minimum and -inf for the maximum."""
    assert prior.dtype == F and prior.ndim == 3 and window % 2 == 1 and 1 <= window <= 15 and holes in ("full", "empty")
    N, H, W = prior.shape
    k = window // 2
    finite = np.isfinite(prior)
    pm = np.full((N, H + 2 * k, W + 2 * k), F(np.inf), F)
    pM = np.full((N, H + 2 * k, W + 2 * k), F(-np.inf), F)
    pm[:, k:k + H, k:k + W] = np.where(finite, prior, F(np.inf))
    pM[:, k:k + H, k:k + W] = np.where(finite, prior, F(-np.inf))
    m = np.full((N, H, W), F(np.inf), F)
    M = np.full((N, H, W), F(-np.inf), F)
    for dy in range(window):
        for dx in range(window):
            m = np.minimum(m, pm[:, dy:dy + H, dx:dx + W])
            M = np.maximum(M, pM[:, dy:dy + H, dx:dx + W])
    some = m < F(np.inf)
    radius = F(radius)
    with np.errstate(all="ignore"):
        lo = np.clip(np.ceil(np.where(some, m, F(0)) - radius), F(0), F(D))
        hi = np.clip(np.floor(np.where(some, M, F(0)) + radius), F(-1), F(D - 1))
    assert lo.dtype == F and hi.dtype == F
    full = holes == "full"
    lo = np.where(some, lo, F(0) if full else F(D))
    hi = np.where(some, hi, F(D - 1) if full else F(-1))
    if not radius >= 0:                                       # negative or NaN: the empty band everywhere
        lo, hi = np.full_like(lo, D), np.full_like(hi, -1)
    return lo.astype(np.int32), hi.astype(np.int32)
