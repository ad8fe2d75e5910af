# Wraps include/ctd_hip.h (ctd_depth_consistency_f32, ctd_depth_fuse_*), include/ctd_hip_warp.h, include/ctd_hip_icp.h.
import torch

from .. import _lib
from ._common import _call, _check, _f32, _integer, _number, _odd_integer, _ptr, _same_device, _stream, _workspace
from ._track import _depth_ray_inputs, _pose_shapes, _track_inputs


# Multi-view depth consistency and point-cloud fusion (additive; include/ctd_hip.h states the rules word for word)
_DEPTH_FUSION_RULE = """
    The rule (include/ctd_hip.h).  depth [B,V,H,W] f32 holds V views of each of B tracks; ray [H*W,3], K [3,3] as for
    `geometric_loss`; R [B,V,3,3], t [B,V,3] with X_cam = R X_world + t.  A pixel is live when its `valid` entry is
    nonzero (valid=None: everywhere) and its depth is finite and > 0.  A source view s != r is consistent with the live
    pixel p of view r when p, projected into s (the geometric projection u = uvd0 / uvd2, rounded to the nearest pixel),
    lands inside the image on a live pixel q, and q projected back with its own depth lands within max_px pixels of p at a
    depth z' with |z' - depth| <= max_rel * depth.  count = the number of consistent views, keep = live and
    count >= min_views, fused = (depth + the z' of the consistent views, ascending) / (1 + count), NaN where not kept."""


def _depth_fusion_inputs(depth, ray, K, R, t, valid, max_px, max_rel, min_views, who):
    dev, v = _track_inputs(depth, ray, K, R, t, valid, who)
    max_px, max_rel = _number(max_px, "max_px", who), _number(max_rel, "max_rel", who)
    return dev, v, max_px, max_rel, _integer(min_views, "min_views", who, 0, 255, "an integer in [0, 255]")


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
    _call(_lib.lib().ctd_depth_consistency_f32, "depth_consistency", _ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R),
          _ptr(t), max_px, max_rel, min_views, _ptr(count), _ptr(keep), _ptr(fused), B, V, H, W, dev.index,
          _stream(dev))
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
    _call(L.ctd_depth_fuse_points_f32, "depth_fuse_points", _ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t),
          max_px, max_rel, min_views, 1 if dedupe else 0, _ptr(points), _ptr(src), _ptr(n_per_track), mp[0], mp[1],
          mp[2], B, V, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    m = int(n_per_track.sum().item())
    return (points[:m], src[:m], n_per_track) + maps


depth_consistency.__doc__ += _DEPTH_FUSION_RULE
depth_fuse_points.__doc__ += _DEPTH_FUSION_RULE


# Forward depth warping and the windowed band: from the views matched so far to the search range of the next one
# (additive; include/ctd_hip_warp.h states both definitions word for word)
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
    splat = _integer(splat, "splat", who, 0, 2, "0, 1 or 2")
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
        _call(L.ctd_depth_warp_f32, who, _ptr(depth), _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t), _ptr(ms), _ptr(mt),
              int(splat), _ptr(z), _ptr(src), B, V, H, W, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    return (z, src) if return_src else z


def disparity_band_window(prior, radius, n_disps, window=3, holes="full"):
    """Additive: the search range [lo, hi] (int32, shaped as `prior`, inclusive) of the band matchers around a disparity
    prior that has holes and occlusion edges, such as `depth_to_disp(depth_warp(...))`: the band of a pixel spans every
    finite prior of its window, so an edge keeps both the foreground and the background disparity and a crack is
    filled from its neighbours.  prior f32 [N,H,W] | [H,W] on the GPU; radius a float; window odd, 1..15; holes "full"
    (a window without any finite prior searches everything) | "empty" (it searches nothing: idx -1)."""
    who = "disparity_band_window"
    window = _odd_integer(window, "window", who, 1, 15)
    if holes not in _BAND_HOLES:
        raise RuntimeError("%s: holes must be 'full' or 'empty', not %r" % (who, holes))
    n_disps = _integer(n_disps, "n_disps", who, 1)
    radius = _number(radius, "radius", who, None)
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
        _call(_lib.lib().ctd_disparity_band_window_f32, who, _ptr(prior), float(radius), int(n_disps), int(window),
              _BAND_HOLES[holes], _ptr(lo), _ptr(hi), N, H, W, dev.index, _stream(dev))
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


# Depth-map normals and projective point-to-plane ICP: from slightly wrong poses back to ones that the consistency check
# confirms (additive; include/ctd_hip_icp.h states the three rules word for word)
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
    max_rel = _number(max_rel, "max_rel", who)
    dev, v = _depth_ray_inputs(depth, ray, valid, who)
    B, V, H, W = depth.shape
    normal = torch.empty(tuple(depth.shape) + (3,), dtype=torch.float32, device=dev)
    if B > 0:
        _call(_lib.lib().ctd_depth_normals_f32, who, _ptr(depth), _ptr(v), _ptr(ray), max_rel, _ptr(normal), B, V, H, W,
              dev.index, _stream(dev))
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
        _call(L.ctd_depth_icp_system_f32, who, _ptr(depth), _ptr(v), _ptr(normal), _ptr(ray), _ptr(K), _ptr(R), _ptr(t),
              _ptr(target), max_dist, _ptr(system), _ptr(residual), _ptr(assoc), B, V, H, W, _ptr(ws), ws.numel(),
              dev.index, _stream(dev))
    return system, residual, assoc


def _icp_update_call(system, R, t, target, min_count, min_pivot, damping, B, V, dev, who):
    """one launch of the update on validated inputs: system [B,V,29], R [B,V,3,3], t [B,V,3]"""
    R_out, t_out = torch.empty_like(R), torch.empty_like(t)
    ok = torch.empty((B, V), dtype=torch.uint8, device=dev)
    if B > 0:
        _call(_lib.lib().ctd_depth_icp_update_f32, who, _ptr(system), _ptr(R), _ptr(t), _ptr(target), min_count,
              min_pivot, damping, _ptr(R_out), _ptr(t_out), _ptr(ok), B, V, dev.index, _stream(dev))
    return R_out, t_out, ok


def depth_icp_system(depth, normal, ray, K, R, t, valid=None, target=None, max_dist=0.1, return_maps=False):
    """Additive: the normal equations of one round of projective point-to-plane ICP that aligns views of a track to
    other views of it -> system float64 [B,V,29], and with return_maps (system, residual f32 [B,V,H,W], assoc int64
    [B,V,H,W]).  Feed it to `depth_icp_update`; `depth_icp` runs both in a loop.  Not differentiable."""
    who = "depth_icp_system"
    max_dist = _number(max_dist, "max_dist", who)
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
    B, V = _pose_shapes(R, t, who, tail=" with V >= 1")
    if tuple(system.shape) != (B, V, 29):
        raise RuntimeError("%s: system [B,V,29], R [B,V,3,3], t [B,V,3] expected" % who)
    return dev, B, V, _icp_target(target, B, V, dev, who)


def depth_icp_update(system, R, t, target=None, min_count=64, min_pivot=1e-4, damping=0.0):
    """Additive: solves the systems of `depth_icp_system` and moves the poses -> (R' f32 [B,V,3,3], t' f32 [B,V,3],
    ok uint8 [B,V]); R and t are not written.  `target` must be the one the system was built with.  Not
    differentiable."""
    who = "depth_icp_update"
    min_count = _integer(min_count, "min_count", who)
    min_pivot = _number(min_pivot, "min_pivot", who)
    damping = _number(damping, "damping", who)
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
    of freedom; on a single plane every round leaves the poses as they are (ok = 0).  "ok" is the last round's alone: a
    view that ends with ok == 0 may have been moved by earlier rounds (on a rendered box scene one such view came back
    0.55 m from its true pose after a 0.3 degree / 5 mm perturbation, its last round's count 0 and rmse NaN), so such a
    pose is not to be used.  Not differentiable."""
    who = "depth_icp"
    iters = _integer(iters, "iters", who, 1)
    max_rel = _number(max_rel, "max_rel", who)
    max_dist = _number(max_dist, "max_dist", who)
    min_count = _integer(min_count, "min_count", who)
    min_pivot = _number(min_pivot, "min_pivot", who)
    damping = _number(damping, "damping", who)
    if isinstance(depth, torch.Tensor) and depth.dim() == 4:              # (anything else: _track_inputs says so)
        _pose_shapes(R, t, who, depth.shape[0], depth.shape[1])
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
