# Wraps include/ctd_hip_tsdf.h (csrc/tsdf.hip).
import torch

from .. import _lib
from ._common import _call, _f32, _integer, _number, _ptr, _same_device, _stream, _workspace
from ._track import _pose_shapes, _track_inputs


# Truncated signed distance volumes: a track's views fused into one surface per track, its points, and a ray cast of
# it into a depth map at any pose (additive; include/ctd_hip_tsdf.h states the three rules word for word)
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


def _tsdf_inputs(tsdf, weight, origin, voxel, who):
    """the tensors of a volume -> (device, B, nx, ny, nz, voxel)"""
    voxel = _number(voxel, "voxel", who, lo_open=True)
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
    B = _integer(B, "B", who)
    nx, ny, nz = (_integer(n, name, who, 1) for n, name in ((nx, "nx"), (ny, "ny"), (nz, "nz")))
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
    max_weight = _number(max_weight, "max_weight", who, 1.0)
    if trunc is not None:
        trunc = _number(trunc, "trunc", who, lo_open=True)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    if trunc is None:
        trunc = 4.0 * voxel
    _, v = _track_inputs(depth, ray, K, R, t, valid, who)
    _same_device(tsdf, depth)
    if depth.shape[0] != B:
        raise RuntimeError("%s: depth [B,V,H,W] must have the B of tsdf [B,nz,ny,nx]" % who)
    V, H, W = depth.shape[1:]
    if B > 0:
        _call(_lib.lib().ctd_tsdf_integrate_f32, who, _ptr(tsdf), _ptr(weight), _ptr(origin), voxel, _ptr(depth),
              _ptr(v), _ptr(ray), _ptr(K), _ptr(R), _ptr(t), trunc, max_weight, B, nx, ny, nz, V, H, W, dev.index,
              _stream(dev))
    return tsdf, weight


def tsdf_surface_points(tsdf, weight, origin, voxel, min_weight=1.0, return_normals=False):
    """Additive: the zero crossings of a volume between neighbouring voxels -> (points [M,3] f32, src [M] int64,
    n_per_track [B] int64), and normals [M,3] f32 behind them with return_normals.  The points come in ascending src
    order, so track b's are the n_per_track[b] entries after those of the tracks before it.  One call counts, the
    counts are read back once (one synchronisation) to size the outputs, a second call fills them.  Not
    differentiable."""
    who = "tsdf_surface_points"
    min_weight = _number(min_weight, "min_weight", who, lo_open=True)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    n_per_track = torch.zeros((B,), dtype=torch.int64, device=dev)
    m = 0
    L = _lib.lib()
    if B > 0:
        ws = _workspace(L.ctd_tsdf_surface_workspace_bytes(B, nx, ny, nz), dev)

        def call(points, normals, src, capacity):
            _call(L.ctd_tsdf_surface_points_f32, who, _ptr(tsdf), _ptr(weight), _ptr(origin), voxel, min_weight,
                  _ptr(points), _ptr(normals), _ptr(src), _ptr(n_per_track), capacity, B, nx, ny, nz, _ptr(ws),
                  ws.numel(), dev.index, _stream(dev))

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
    H, W = _integer(H, "H", who, 1), _integer(W, "W", who, 1)
    n_steps = _integer(n_steps, "n_steps", who, 1)
    d_min = _number(d_min, "d_min", who)
    step = _number(step, "step", who, lo_open=True)
    min_weight = _number(min_weight, "min_weight", who, lo_open=True)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    _same_device(tsdf, _f32(ray, "ray"), _f32(R, "R"), _f32(t, "t"))
    _, V = _pose_shapes(R, t, who, B, tail=" with V >= 1 and the B of tsdf")
    if ray.numel() != H * W * 3:
        raise RuntimeError("%s: ray [H*W,3] expected" % who)
    depth = torch.empty((B, V, H, W), dtype=torch.float32, device=dev)
    if B > 0:
        _call(_lib.lib().ctd_tsdf_raycast_f32, who, _ptr(tsdf), _ptr(weight), _ptr(origin), voxel, _ptr(ray), _ptr(R),
              _ptr(t), d_min, step, n_steps, min_weight, _ptr(depth), B, nx, ny, nz, V, H, W, dev.index, _stream(dev))
    return depth


tsdf_integrate.__doc__ += _TSDF_RULE
tsdf_surface_points.__doc__ += _TSDF_RULE
tsdf_raycast.__doc__ += _TSDF_RULE
