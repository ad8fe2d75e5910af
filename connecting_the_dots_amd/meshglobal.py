"""Global point-to-mesh registration (include/ext/ctd_hip_mesh_global.h, csrc/mesh_global.hip): finds the pose of a point
set, or of a mesh through its surface samples, against a mesh from ANY starting orientation, by scoring a grid of
rotations times a few offsets against a volume of distances to the mesh and refining the best few with `meshreg.mesh_icp`
(or `meshrobust.robust_mesh_icp`).  `meshreg` and `meshrobust` are local methods that want a start within a few tens of
degrees; this module produces their starts.  For a model fused in the frame of its track's first view against a scanned
truth mesh, or two tracks of one object: an arbitrary rigid motion apart.

    R, t, info = meshglobal.global_mesh_icp(points, truth_verts, truth_faces, n_rotations=4096, max_dist=0.25)
    R, t, info = meshglobal.global_register_mesh(verts, faces, truth_verts, truth_faces)
    err = meshglobal.global_aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds=(0.005, 0.01))
    # the parts
    origin, voxel, dims = meshglobal.default_box(truth_verts, resolution=64, pad=6)
    levels = meshglobal.distance_levels(truth_verts, truth_faces, origin, voxel, dims, trunc=6 * voxel)
    score = meshglobal.pose_scores(points[:2048], R_grid, base, offsets, levels, origin, voxel)      # int64 [M,T]
    Rk, tk, sk, mk = meshglobal.best_starts(score, R_grid, base, offsets, K=8)
    # points[:2048] of fused points (in `src` order) is one corner of the first view; an even subset of any point set is
    # pointcloud.voxel_downsample(points, cell).points, one mean point per occupied cell

A pose (R, t) moves a point p to S = R p + t.  What this does not do: no scale and no reflection, and nothing is
differentiable.  The search is exhaustive over a grid, not guided by features: a grid that is too coarse for the object
(the largest gap of `rotation_grid(n)` is near 27 degrees at n = 512, 20 at n = 1024 and 13 at n = 4096) can miss the
basin, and the offsets cover only a mismatch of the two centroids of about t_steps * t_step / 2: where the points cover
a part of the mesh, or sample it unevenly, the gap between the centroids can be far larger, and then t_steps and t_step
have to be raised to reach it (profiles/mesh_global.txt has such a case: 27 offsets fail, 729 find the pose).  A
symmetric object has several equally good answers, and this returns one of them: which one is decided by ties, not by
anything in the data.

The header's prototypes are bound here, onto the library handle of `_lib.lib()` at first use; this table is not one of
`_lib.TABLES`.  No fallback to torch: a missing kernel is an error.
"""
import ctypes
import math

import torch

from . import _lib
from ._meshargs import _nx3, _resolve_bvh
from .mesheval import AUTO_BVH_MIN_FACES, reconstruction_error, sample_surface
from .meshreg import _mesh_inputs, _metric, mesh_icp, mesh_icp_system, transform_points
from .meshsdf import mesh_to_tsdf
from .torchext._common import _call, _check, _integer, _number, _ptr, _same_device, _stream

_c_int, _c_float, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

HEADER = "ext/ctd_hip_mesh_global.h"

# mirrors include/ext/ctd_hip_mesh_global.h one to one, in the header's order (tests/test_mesh_global_host.py)
TABLE = {
    "ctd_pose_score_u8": (_c_int, [_vp, _c_int, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _c_float, _vp,
                                   _c_int, _vp]),
}

MAX_SCORE_POINTS = 65536                                      # 65536 * 255^2 < 2^32: the kernel's partial sums are 32-bit
MAX_OFFSETS = 4096
MAX_DIM = 1024
OUTSIDE = 255                                                 # the level of "trunc or farther", and of a point off the volume
PSI = 1.533751168755204288118041                              # the super-Fibonacci constant: psi^4 = psi + 4

_bound = None


def lib():
    """the handle of `_lib.lib()` with this module's prototypes bound"""
    global _bound
    if _bound is None:
        l = _lib.lib()
        for name, (res, args) in TABLE.items():
            fn = getattr(l, name)           # AttributeError here means header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _bound = l
    return _bound


_RULE = """
    The rule (include/ext/ctd_hip_mesh_global.h).  Per point p, rotation m and offset j, in f32 in this association:
    Q_c = ((R_m[c][0] p0 + R_m[c][1] p1) + R_m[c][2] p2) + base_m[c], S_c = Q_c + offsets[j][c],
    u_c = (S_c - origin[c]) / voxel, g_c = floorf(u_c + 0.5f).  The point is inside when 0 <= g_c < dim_c for x, y and z,
    compared as floats (a NaN or an infinity fails); q = levels[g_z, g_y, g_x] inside and 255 outside;
    score[m, j] = sum of q * q over the points, an exact integer: any order of the points gives the same bits."""


def rotation_grid(n, device=None):
    """n rotations that cover SO(3) evenly -> f32 [n,3,3]: the super-Fibonacci spiral of unit quaternions (Alexa 2022).
    With s = i + 0.5, t = s / n, d = 2 pi s, r = sqrt(t), r' = sqrt(1 - t), a = d / sqrt(2) and b = d / 1.5337511687552043
    the quaternion is (x, y, z, w) = (r sin a, r cos a, r' sin b, r' cos b); float64 throughout, converted to a matrix
    and rounded to f32 once.  Deterministic and without state.  The largest angle from any rotation to the nearest of the
    grid, over 2000 random rotations, is 26.7 degrees for n = 512, 19.6 for 1024 and 13.1 for 4096
    (tests/test_mesh_global_host.py)."""
    n = _integer(n, "n", "rotation_grid", 1)
    s = torch.arange(n, dtype=torch.float64) + 0.5
    t, d = s / n, 2.0 * math.pi * s
    r, rp, a, b = torch.sqrt(t), torch.sqrt(1.0 - t), d / math.sqrt(2.0), d / PSI
    x, y, z, w = r * torch.sin(a), r * torch.cos(a), rp * torch.sin(b), rp * torch.cos(b)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).reshape(n, 3, 3)
    return R.to(torch.float32).to(device=device).contiguous()


def offset_grid(steps, step, device=None):
    """steps^3 translations on a centred cubic lattice of spacing `step` -> f32 [steps^3,3], x slowest:
    row (ix * steps + iy) * steps + iz is ((ix, iy, iz) - (steps - 1) / 2) * step, in float64, rounded to f32 once.  An
    odd `steps` has the zero offset in the middle."""
    who = "offset_grid"
    steps = _integer(steps, "steps", who, 1, 16)
    step = _number(step, "step", who)
    g = (torch.arange(steps, dtype=torch.float64) - (steps - 1) / 2.0) * step
    out = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).reshape(-1, 3)
    return out.to(torch.float32).to(device=device).contiguous()


def default_box(verts, resolution=64, pad=6):
    """A volume around the mesh's vertices verts f32 [m,3] -> (origin f32 [3] on their device, voxel float, dims
    (nx, ny, nz)): the bounding box of the finite vertices, padded by `pad` voxels on every side, with `voxel` chosen so
    that the longest padded side has `resolution` voxels (the other sides as many as they need).  The defaults go with
    trunc = 6 voxels: then a point off the volume really is "trunc or farther" from the mesh.  64^3 is 256 KiB of levels;
    a voxel is 1/51 of the object's longest side.  One synchronisation."""
    who = "default_box"
    _nx3(verts, who, "verts", torch.float32, letter="m")
    resolution = _integer(resolution, "resolution", who, 2, MAX_DIM)
    pad = _integer(pad, "pad", who, 0)
    inner = resolution - 1 - 2 * pad
    if inner < 1:
        raise RuntimeError("%s: resolution must be above 2 * pad + 1" % who)
    ok = torch.isfinite(verts).all(dim=1)
    if not bool(ok.any()):
        raise RuntimeError("%s: the mesh has no finite vertex" % who)
    v = verts[ok].double()
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    extent = (hi - lo).tolist()
    voxel = max(extent) / inner
    if not voxel > 0:
        raise RuntimeError("%s: the mesh's bounding box is a single point" % who)
    dims = tuple(min(resolution, int(math.ceil(e / voxel - 1e-9)) + 1 + 2 * pad) for e in extent)
    origin = (lo - pad * voxel).to(torch.float32).contiguous()
    return origin, float(voxel), dims


def distance_levels(verts, faces, origin, voxel, dims, trunc, bvh="auto"):
    """The unsigned distance from the centre of every voxel to the mesh verts f32 [m,3], faces int32 [k,3] in units of
    trunc / 255 -> uint8 [nz,ny,nx] (x fastest) for dims = (nx, ny, nz); origin f32 [3] (a CUDA tensor) and voxel as in
    `meshsdf.mesh_to_tsdf`, whose (tsdf, weight) of the same arguments this is built from, in f32 torch ops: where
    weight > 0 level = floor(|tsdf| * 255 + 0.5), elsewhere 255.  So 255 means "trunc or farther".  Unsigned, because
    open meshes must work."""
    tsdf, weight = mesh_to_tsdf(verts, faces, origin, voxel, dims, trunc, bvh=bvh)
    level = torch.floor(tsdf[0].abs() * 255.0 + 0.5)
    level = torch.where(weight[0] > 0, level, torch.full_like(level, float(OUTSIDE)))
    return level.to(torch.uint8).contiguous()


def morton_order(points):
    """The permutation that sorts points f32 [n,3] along a Morton curve of their coordinates, quantised to 10 bits an axis
    over the cube around the finite ones -> int64 [n]; points with a NaN or an infinity go last.  A stable sort in torch
    ops on the device of `points`, no synchronisation.  Neighbours in the order are neighbours in space under every rigid
    motion, so one sort serves every pose of `pose_scores`."""
    n = points.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=points.device)
    ok = torch.isfinite(points).all(dim=1)
    inf = torch.full_like(points, float("inf"))
    lo = torch.where(ok[:, None], points, inf).amin(dim=0)
    hi = torch.where(ok[:, None], points, -inf).amax(dim=0)
    side = torch.nan_to_num((hi - lo).amax(), nan=1.0, posinf=1.0, neginf=1.0).clamp_min(1e-30)
    cell = torch.nan_to_num((points - lo) / side * 1023.0, nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, 1023.0).long()

    def spread(v):                                            # 10 bits -> every third bit of 30
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249

    code = spread(cell[:, 0]) | (spread(cell[:, 1]) << 1) | (spread(cell[:, 2]) << 2)
    code = torch.where(ok, code, torch.full_like(code, 1 << 30))
    return torch.sort(code, stable=True).indices


def pose_scores(points, R, base, offsets, levels, origin, voxel, order="morton"):
    """The score of points f32 [n,3] (n <= 65536) under every pose (R_m, base_m + offsets_j), R f32 [M,3,3], base f32
    [M,3], offsets f32 [T,3] (T <= 4096, M * T < 2^31), against levels uint8 [nz,ny,nx] (dims <= 1024) with origin f32
    [3] and voxel as `distance_levels` takes them (CUDA tensors) -> int64 [M,T]; lower is better, 65025 * n is "nothing
    near the surface".  order: 'morton' (the default) sorts the points by `morton_order` first, which makes the lanes of a
    wavefront gather from neighbouring voxels; None keeps the caller's order.  The order changes the time, never a bit.
    One launch on the current stream, no synchronisation, no workspace."""
    who = "pose_scores"
    _nx3(points, who, "points", torch.float32)
    _check(R, "%s: R" % who, (torch.float32,))
    _check(base, "%s: base" % who, (torch.float32,))
    _nx3(offsets, who, "offsets", torch.float32, letter="T")
    _check(levels, "%s: levels" % who, (torch.uint8,))
    _check(origin, "%s: origin" % who, (torch.float32,))
    dev = _same_device(points, R, base, offsets, levels, origin)
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or tuple(base.shape) != (R.shape[0], 3) or R.shape[0] < 1:
        raise RuntimeError("%s: R must be shaped [M,3,3] and base [M,3], M >= 1" % who)
    if levels.dim() != 3 or min(levels.shape) < 1 or max(levels.shape) > MAX_DIM:
        raise RuntimeError("%s: levels must be shaped [nz,ny,nx], each between 1 and %d, got %s" % (who, MAX_DIM,
                                                                                                     tuple(levels.shape)))
    if tuple(origin.shape) != (3,):
        raise RuntimeError("%s: origin must be shaped [3], got %s" % (who, tuple(origin.shape)))
    voxel = _number(voxel, "voxel", who, lo_open=True)
    if order not in (None, "morton"):
        raise RuntimeError("%s: order must be 'morton' or None" % who)
    n, M, T = points.shape[0], R.shape[0], offsets.shape[0]
    if n > MAX_SCORE_POINTS:
        raise RuntimeError("%s: at most %d points, got %d (subsample: the score is a coarse one)" % (who, MAX_SCORE_POINTS, n))
    if not 1 <= T <= MAX_OFFSETS or M * T >= 2 ** 31:
        raise RuntimeError("%s: between 1 and %d offsets and M * T below 2^31, got M = %d, T = %d" % (who, MAX_OFFSETS, M, T))
    if order == "morton" and n > 1:
        points = points[morton_order(points)].contiguous()
    nz, ny, nx = levels.shape
    score = torch.empty((M, T), dtype=torch.int64, device=dev)
    _call(lib().ctd_pose_score_u8, who, _ptr(points) or None, n, _ptr(R), _ptr(base), M, _ptr(offsets), T, _ptr(levels), nx, ny,
          nz, _ptr(origin), voxel, _ptr(score), dev.index, _stream(dev))
    return score


def best_starts(score, R, base, offsets, K):
    """The K best poses of score int64 [M,T] (`pose_scores`), at most one per rotation because neighbouring offsets of
    one rotation are the same basin -> (R f32 [K,3,3], t f32 [K,3], score int64 [K], rot_index int64 [K]).  Per rotation
    the minimum over the offsets, ties to the lowest j; then the K rotations with the lowest minimum, ties to the lowest
    m (a stable sort); t = base_m + offsets_j in f32.  Torch ops on the device of `score`, no synchronisation."""
    who = "best_starts"
    if not isinstance(score, torch.Tensor) or score.dtype != torch.int64 or score.dim() != 2:
        raise RuntimeError("%s: score must be an int64 tensor shaped [M,T]" % who)
    M, T = score.shape
    if tuple(R.shape) != (M, 3, 3) or tuple(base.shape) != (M, 3) or tuple(offsets.shape) != (T, 3):
        raise RuntimeError("%s: R must be shaped [%d,3,3], base [%d,3] and offsets [%d,3]" % (who, M, M, T))
    _same_device(score, R, base, offsets)
    K = _integer(K, "K", who, 1, M, "an integer in [1, %d], the number of rotations" % M)
    if T > MAX_OFFSETS or bool(score.numel() == 0):
        raise RuntimeError("%s: between 1 and %d offsets" % (who, MAX_OFFSETS))
    # (score, j) as one key: a score is below 2^32 and T at most 2^12, so the minimum of the key is the lowest j of the
    # lowest score whatever order the reduction takes
    key = (score * T + torch.arange(T, dtype=torch.int64, device=score.device)).amin(dim=1)
    low, j = torch.div(key, T, rounding_mode="floor"), key % T
    m = torch.sort(low, stable=True).indices[:K]
    return R[m].contiguous(), (base[m] + offsets[j[m]]).contiguous(), low[m], m


def _centroids(points, verts, faces, who):
    """(the mean of the finite points, the area-weighted centroid of the mesh's faces), float64 [3] each"""
    ok = torch.isfinite(points).all(dim=1)
    count = ok.sum()
    c_points = torch.where(ok[:, None], points, torch.zeros_like(points)).double().sum(dim=0) / count
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise RuntimeError("%s: the mesh has no face" % who)
    idx = faces.long()
    valid = ((idx >= 0) & (idx < verts.shape[0])).all(dim=1)
    idx = torch.where(valid[:, None], idx, torch.zeros_like(idx))          # (an invalid face reads vertex 0: weight 0)
    a, b, c = (verts[idx[:, i]].double() for i in range(3))
    area = torch.linalg.norm(torch.cross(b - a, c - a, dim=1), dim=1)
    area = torch.where(valid & torch.isfinite(area), area, torch.zeros_like(area))
    mid = torch.nan_to_num((a + b + c) / 3.0, nan=0.0, posinf=0.0, neginf=0.0)
    total = area.sum()
    if not bool((count > 0) & (total > 0)):
        raise RuntimeError("%s: needs a finite point and a face of positive finite area" % who)
    return c_points, (mid * area[:, None]).sum(dim=0) / total


def global_mesh_icp(points, verts, faces, n_rotations=4096, t_steps=3, t_step=None, levels=None, origin=None, voxel=None,
                    trunc=None, K=8, iters=40, metric="point", max_dist=None, robust=None, n_score=2048, resolution=64, pad=6,
                    order="morton", bvh="auto", **icp):
    """Registers points f32 [n,3] to the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors) from any start ->
    (R f32 [3,3], t f32 [3], info).  The steps:
    1. every ceil(n / n_score)-th point (at most n_score <= 65536 of them; a fixed stride, so deterministic) is kept for
       the scoring alone;
    2. unless `levels` uint8 [nz,ny,nx], `origin` f32 [3] and `voxel` are given (all three, as `distance_levels` took
       them): `default_box(verts, resolution, pad)` and `distance_levels` with `trunc`, 6 voxels when None (one
       synchronisation for the box);
    3. R_m = `rotation_grid(n_rotations)`, base_m = c_mesh - R_m c_points in float64, rounded to f32 once, with c_mesh the
       area-weighted centroid of the mesh's faces and c_points the mean of the finite points: every rotation turns the
       points about their centroid and lays it on the mesh's; offsets = `offset_grid(t_steps, t_step)` with t_step = 2
       voxels when None;
    4. `pose_scores`, `best_starts(..., K)`, then all K starts refined in ONE `meshreg.mesh_icp` call on ALL the points
       with iters, metric, max_dist and the keyword arguments `icp` (min_count, min_pivot, damping, use_hint); with
       robust=dict(kernel=, rim=, normals=, min_cos=, scale=) one `meshrobust.robust_mesh_icp` call instead;
    5. the final ranking: one more `meshreg.mesh_icp_system(metric='point', max_dist, return_maps=True)` round at the
       refined poses; final_k = the sum over the finite points of min(residual, cap)^2 with a NaN residual (no face within
       max_dist) counted as cap, cap = max_dist or +inf when that is None, a float64 sum; poses with ok = 0 are out; the
       lowest final_k wins, ties to the lowest k.  NOT the plane-metric rms, which does not see points that overhang a
       face's rim (two basins 120 degrees apart had the same plane rms on the test scene), and not an rms over the kept
       points alone, which rewards a pose that drops most of its points under max_dist.
    Raises when no start ends with ok = 1 (one synchronisation).
    info, device tensors: "start_R" [K,3,3], "start_t" [K,3], "start_score" int64 [K], "start_rot" int64 [K] (the index
    into the grid); "R" [K,3,3] and "t" [K,3], the refined poses; "final" float64 [K] (+inf where ok = 0); "ok" uint8 [K];
    "icp", the info of the refinement; "best" int64 [], the k that was returned.  The same inputs give the same bits."""
    who = "global_mesh_icp"
    dev = _mesh_inputs(points, verts, faces, who)
    n_rotations = _integer(n_rotations, "n_rotations", who, 1)
    t_steps = _integer(t_steps, "t_steps", who, 1, 16)
    K = _integer(K, "K", who, 1, min(64, n_rotations), "an integer in [1, min(64, n_rotations)]")
    n_score = _integer(n_score, "n_score", who, 1, MAX_SCORE_POINTS, "an integer in [1, %d]" % MAX_SCORE_POINTS)
    _metric(metric, who)
    if robust is not None and not isinstance(robust, dict):
        raise RuntimeError("%s: robust must be None or a dict of meshrobust.robust_mesh_icp's arguments" % who)
    given = [x is not None for x in (levels, origin, voxel)]
    if any(given) and not all(given):
        raise RuntimeError("%s: give levels, origin and voxel together, or none of them" % who)
    n = points.shape[0]
    if n == 0:
        raise RuntimeError("%s: no points" % who)
    c_points, c_mesh = _centroids(points, verts, faces, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)         # once, for the levels and every round
    if levels is None:
        origin, voxel, dims = default_box(verts, resolution, pad)
        trunc = 6.0 * voxel if trunc is None else _number(trunc, "trunc", who, lo_open=True)
        levels = distance_levels(verts, faces, origin, voxel, dims, trunc, bvh=tree)
    voxel = _number(voxel, "voxel", who, lo_open=True)
    t_step = 2.0 * voxel if t_step is None else _number(t_step, "t_step", who)
    Rg = rotation_grid(n_rotations, dev)
    base = (c_mesh[None, :] - Rg.double() @ c_points).to(torch.float32).contiguous()
    offsets = offset_grid(t_steps, t_step, dev)
    stride = -(-n // n_score)
    score = pose_scores(points[::stride].contiguous(), Rg, base, offsets, levels, origin, voxel, order=order)
    R0, t0, s0, m0 = best_starts(score, Rg, base, offsets, K)
    if robust is None:
        Rk, tk, icp_info = mesh_icp(points, verts, faces, R0, t0, iters=iters, metric=metric, max_dist=max_dist, bvh=tree,
                                    **icp)
    else:
        from .meshrobust import robust_mesh_icp
        Rk, tk, icp_info = robust_mesh_icp(points, verts, faces, R0, t0, iters=iters, metric=metric, max_dist=max_dist,
                                           bvh=tree, **robust, **icp)
    ok = icp_info["ok"]
    residual = mesh_icp_system(points, verts, faces, Rk, tk, metric="point", max_dist=max_dist, bvh=tree, return_maps=True)[2]
    cap = float("inf") if max_dist is None else float(max_dist)
    r = torch.where(torch.isnan(residual), torch.full_like(residual, cap), residual.clamp(max=cap)).double()
    finite = torch.isfinite(points).all(dim=1)
    final = torch.where(finite[None, :], r * r, torch.zeros_like(r)).sum(dim=1)
    final = torch.where(ok != 0, final, torch.full_like(final, float("inf")))
    if not bool((ok != 0).any()):
        raise RuntimeError("%s: no start ended with ok = 1" % who)
    # by (ok first, final, k): two stable sorts
    by_final = torch.sort(final, stable=True).indices
    best = by_final[torch.sort((ok[by_final] == 0).to(torch.uint8), stable=True).indices[0]]
    info = {"start_R": R0, "start_t": t0, "start_score": s0, "start_rot": m0, "R": Rk, "t": tk, "final": final, "ok": ok,
            "icp": icp_info, "best": best}
    return Rk[best], tk[best], info


def global_register_mesh(verts, faces, truth_verts, truth_faces, n_samples=20000, generator=None, **kw):
    """`global_mesh_icp` of `n_samples` area-weighted surface samples (`mesheval.sample_surface`) of the mesh verts f32
    [n,3], faces int32 [m,3] against the mesh truth_verts, truth_faces (CUDA tensors) -> (R, t, info), whose keyword
    arguments pass through: `transform_points(verts, R, t)` is the first mesh in the frame of the second, wherever it
    started."""
    who = "global_register_mesh"
    for x, name, dt in ((verts, "verts", torch.float32), (faces, "faces", torch.int32),
                        (truth_verts, "truth_verts", torch.float32), (truth_faces, "truth_faces", torch.int32)):
        _nx3(x, who, name, dt)
    _same_device(verts, faces, truth_verts, truth_faces)
    n_samples = _integer(n_samples, "n_samples", who, 1)
    pts = sample_surface(verts, faces, n_samples, generator)[0]
    return global_mesh_icp(pts, truth_verts, truth_faces, **kw)


def global_aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples=None, generator=None,
                                        bvh="auto", icp_samples=20000, **kw):
    """`meshreg.aligned_reconstruction_error` with `global_register_mesh` in place of `register_mesh` (its keyword
    arguments pass through) -> the dict of `mesheval.reconstruction_error` of the moved vertices against the truth, plus
    "R" f32 [3,3], "t" f32 [3], "icp" (the info of `global_mesh_icp`, the starts among it), "starts" (its start_R,
    start_t, start_score and start_rot as R, t, score and rot_index) and "before".  Raises when no start was accepted."""
    before = reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples, generator, bvh)
    R, t, info = global_register_mesh(verts, faces, truth_verts, truth_faces, icp_samples, generator, **kw)
    moved = transform_points(verts, R, t).contiguous()
    out = reconstruction_error(moved, faces, truth_verts, truth_faces, thresholds, n_samples, generator, bvh)
    out.update(R=R, t=t, icp=info, before=before,
               starts={"R": info["start_R"], "t": info["start_t"], "score": info["start_score"], "rot_index": info["start_rot"]})
    return out


pose_scores.__doc__ += _RULE
