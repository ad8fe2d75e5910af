"""Numpy restatement of the rule of include/ext/ctd_hip_mesh_global.h (ctd_pose_score_u8), operation for operation, of the
torch steps of connecting_the_dots_amd/meshglobal.py around it (the distance levels, the rotation and offset grids, the
choice of the starts, the final ranking), and the scene of their tests.

Everything the header computes in f32 is np.float32 here in exactly the written association, vectorised over rotations,
offsets and points; the bounds are tested on the floats and only a point that passed is converted to an index.  The score
is an integer sum, so any order gives the kernel's bits and the comparison is array_equal.

The distance levels come from the brute-force nearest face (tests/meshsdf_ref.nearest: tests/pointmesh_ref.py's triangle
distance with the cutoff), at the voxel centres origin[c] + voxel * float(index) in f32, as `meshsdf.mesh_to_tsdf` lays
them out.  The refinement is tests/meshreg_ref.mesh_icp (or tests/meshrobust_ref.robust_mesh_icp), so that the whole
pipeline runs on the CPU with numpy alone.

The scene: the corner of tests/meshreg_ref.py with every coordinate scaled by (1, 0.7, 0.45), so that no proper rotation
maps the mesh onto itself; 512 samples of it (every in-plane coordinate < 0.85 before the scaling) with Gaussian noise
0.002, moved by 140 degrees about a random axis through their centroid and by 0.5 in a random direction."""
import numpy as np

from tests import meshreg_ref as mr
from tests import meshsdf_ref as sr

F = np.float32
OUTSIDE = 255
PSI = 1.533751168755204288118041

SCALE = (1.0, 0.7, 0.45)
SCENE_SEEDS = (1, 2, 3)
# the settings of the issue's check: 1024 rotations x 27 offsets of step 0.1, 40^3 voxels of 0.05 from -0.5, trunc 0.3
N_ROT, T_STEPS, T_STEP = 1024, 3, 0.1
DIMS, VOXEL, ORIGIN, TRUNC = (40, 40, 40), 0.05, (-0.5, -0.5, -0.5), 0.3
K_STARTS, ITERS = 8, 40
# a start this near the truth refines to it: every start of the reference runs that began within 30 degrees ended on the
# truth; the rotation grid has to be finer than BASIN_DEG, and a start inside (BASIN_DEG, BASIN_T) has to be among the K
BASIN_DEG, BASIN_T = 20.0, 0.2


# ---------------------------------------------------------------------------------------------------------------------
def rotation_grid(n):
    """the super-Fibonacci spiral, float64, rounded to f32 once -> f32 [n,3,3]"""
    s = np.arange(n, dtype=np.float64) + 0.5
    t, d = s / n, 2.0 * np.pi * s
    r, rp, a, b = np.sqrt(t), np.sqrt(1.0 - t), d / np.sqrt(2.0), d / PSI
    x, y, z, w = r * np.sin(a), r * np.cos(a), rp * np.sin(b), rp * np.cos(b)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    return np.ascontiguousarray(R.astype(F))


def offset_grid(steps, step):
    """f32 [steps^3,3], centred, x slowest"""
    g = (np.arange(steps, dtype=np.float64) - (steps - 1) / 2.0) * step
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F))


def distance_levels(verts, faces, origin, voxel, dims, trunc):
    """-> uint8 [nz,ny,nx]: floor(min(1, sqrt(d2) / trunc) * 255 + 0.5) in f32 where a face lies within trunc
    (d2 <= trunc * trunc, one f32 product), 255 elsewhere"""
    nx, ny, nz = dims
    origin, voxel, trunc = np.asarray(origin, F), F(voxel), F(trunc)
    xs, ys, zs = (origin[c] + voxel * np.arange(n, dtype=F) for c, n in enumerate(dims))
    assert xs.dtype == F
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    centres = np.stack([X, Y, Z], -1).reshape(-1, 3)
    d2, face, _, _ = sr.nearest(centres, verts, faces, trunc * trunc)
    with np.errstate(invalid="ignore"):
        tsdf = np.minimum(F(1), np.sqrt(d2) / trunc)
        level = np.floor(tsdf * F(255) + F(0.5))
    assert level.dtype == F
    return np.where(face >= 0, level, F(OUTSIDE)).astype(np.uint8).reshape(nz, ny, nx)


def pose_scores(points, R, base, offsets, levels, origin, voxel, chunk=64):
    """the rule -> int64 [M,T]"""
    assert points.dtype == F and R.dtype == F and base.dtype == F and offsets.dtype == F and levels.dtype == np.uint8
    origin, voxel = np.asarray(origin, F), F(voxel)
    nz, ny, nx = levels.shape
    dims = (nx, ny, nz)
    M, T, n = R.shape[0], offsets.shape[0], points.shape[0]
    score = np.zeros((M, T), np.int64)
    if n == 0:
        return score
    p = [points[None, :, i] for i in range(3)]                                          # [1,n]
    flat = levels.reshape(-1).astype(np.int64)
    for m0 in range(0, M, chunk):
        Rm, bm = R[m0:m0 + chunk], base[m0:m0 + chunk]
        inside = np.ones((Rm.shape[0], T, n), bool)
        g = []
        with np.errstate(all="ignore"):
            for c in range(3):
                Q = ((Rm[:, c, 0:1] * p[0] + Rm[:, c, 1:2] * p[1]) + Rm[:, c, 2:3] * p[2]) + bm[:, c:c + 1]   # [m,n]
                S = Q[:, None, :] + offsets[None, :, c, None]                            # [m,T,n]
                u = (S - origin[c]) / voxel
                gc = np.floor(u + F(0.5))
                assert gc.dtype == F
                inside &= (gc >= 0) & (gc < F(dims[c]))                                 # (a NaN or an inf fails)
                g.append(np.where(inside, gc, F(0)).astype(np.int64))
        idx = np.where(inside, (g[2] * ny + g[1]) * nx + g[0], 0)
        q = np.where(inside, flat[idx], OUTSIDE)
        score[m0:m0 + chunk] = (q * q).sum(-1)
    return score


def best_starts(score, R, base, offsets, K):
    """per rotation the minimum over the offsets (ties: the lowest j), then the K rotations with the lowest minimum (ties:
    the lowest m) -> (R [K,3,3], t [K,3] = base_m + offsets_j in f32, score [K], rot_index [K])"""
    j = score.argmin(1)                                                                 # (numpy: the first minimum)
    low = score[np.arange(len(score)), j]
    m = np.argsort(low, kind="stable")[:K]
    return R[m].copy(), (base[m] + offsets[j[m]]).astype(F), low[m], m


def mesh_centroid(verts, faces):
    """the area-weighted centroid of the faces, float64"""
    V = np.asarray(verts, np.float64)
    a, b, c = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return ((a + b + c) / 3.0 * area[:, None]).sum(0) / area.sum()


def bases(R, points, verts, faces):
    """base_m = c_mesh - R_m c_points in float64, rounded to f32 once"""
    ok = np.isfinite(points).all(1)
    c_points = points[ok].astype(np.float64).sum(0) / ok.sum()
    return np.ascontiguousarray((mesh_centroid(verts, faces)[None] - R.astype(np.float64) @ c_points).astype(F))


def final_scores(points, R, t, ok, verts, faces, max_dist=None):
    """the final ranking: one point-metric round at the poses; the sum over the finite points of min(residual, cap)^2 with
    NaN as cap, float64; +inf where ok = 0 -> (final [K], best: the lowest among ok = 1, ties to the lowest k)"""
    max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
    residual = mr.system(points, R, t, verts, faces, 1, max_d2)[2]
    cap = np.inf if max_dist is None else float(max_dist)
    r = np.where(np.isnan(residual), cap, np.minimum(residual.astype(np.float64), cap))
    finite = np.isfinite(points).all(1)
    final = np.where(finite[None], r * r, 0.0).sum(1)
    final = np.where(ok != 0, final, np.inf)
    order = np.argsort(final, kind="stable")
    order = order[np.argsort(ok[order] == 0, kind="stable")]
    return final, int(order[0])


def global_mesh_icp(points, verts, faces, levels, n_rot=N_ROT, t_steps=T_STEPS, t_step=T_STEP, origin=ORIGIN, voxel=VOXEL,
                    K=K_STARTS, iters=ITERS, metric=1, max_dist=None, robust=None, n_score=2048):
    """the pipeline of meshglobal.global_mesh_icp -> (R [3,3], t [3], info); robust: None or the keyword arguments of
    tests/meshrobust_ref.robust_mesh_icp (kernel, rim, ...)"""
    R = rotation_grid(n_rot)
    base = bases(R, points, verts, faces)
    offsets = offset_grid(t_steps, t_step)
    stride = -(-len(points) // n_score)
    score = pose_scores(np.ascontiguousarray(points[::stride]), R, base, offsets, levels, origin, voxel)
    R0, t0, s0, m0 = best_starts(score, R, base, offsets, K)
    if robust is None:
        Rk, tk, icp = mr.mesh_icp(points, verts, faces, R0, t0, iters=iters, metric=metric, max_dist=max_dist)
    else:
        from tests import meshrobust_ref as rr
        Rk, tk, icp = rr.robust_mesh_icp(points, verts, faces, R0, t0, iters=iters, metric=metric, max_dist=max_dist, **robust)
    final, best = final_scores(points, Rk, tk, icp["ok"], verts, faces, max_dist)
    if not icp["ok"].any():
        raise RuntimeError("no start ended with ok = 1")
    info = {"start_R": R0, "start_t": t0, "start_score": s0, "start_rot": m0, "R": Rk, "t": tk, "final": final,
            "ok": icp["ok"], "icp": icp, "best": best, "score": score}
    return Rk[best], tk[best], info


# ---------------------------------------------------------------------------------------------------------------------
def scaled_corner(quads=6):
    verts, faces = mr.corner_mesh(quads)
    return np.ascontiguousarray((verts.astype(np.float64) * SCALE).astype(F)), faces


def make_scene(seed, n=512, limit=0.85, noise=0.002, degrees=140.0, shift=0.5, outliers=0.0, quads=6):
    """-> dict as meshreg_ref.make_corner: verts, faces (the scaled corner), points f32 [n + round(outliers * n),3] (n samples of
    it and after them the outliers, uniform in the scaled box [-0.2, 0.85]^3, all displaced by the rotation about their
    centroid and the shift), R_true, t_true (float64): the pose that takes them back"""
    rs = np.random.RandomState(seed)
    verts, faces = scaled_corner(quads)
    P = mr.corner_points(rs, n, limit=limit) * SCALE + rs.normal(size=(n, 3)) * noise
    n_out = int(round(outliers * n))
    if n_out:
        P = np.concatenate([P, rs.uniform(-0.2, 0.85, size=(n_out, 3)) * SCALE])
    Q = mr.rotation(rs.normal(size=3), degrees)
    d = rs.normal(size=3)
    d = d / np.linalg.norm(d) * shift
    c = P.mean(0)
    moved = (P - c) @ Q.T + c + d
    return {"verts": verts, "faces": faces, "points": np.ascontiguousarray(moved.astype(F)), "R_true": Q.T,
            "t_true": c - Q.T @ (c + d)}


_LEVELS = {}


def scene_levels(quads=6):
    """the levels of the scaled corner at the issue's settings, computed once and shared (read-only)"""
    if quads not in _LEVELS:
        verts, faces = scaled_corner(quads)
        lv = distance_levels(verts, faces, ORIGIN, VOXEL, DIMS, TRUNC)
        lv.setflags(write=False)
        _LEVELS[quads] = lv
    return _LEVELS[quads]
