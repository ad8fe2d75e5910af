"""Numpy restatement of the three rules of include/ctd_hip_tsdf.h (ctd_tsdf_integrate_f32, ctd_tsdf_surface_points_f32,
ctd_tsdf_raycast_f32) and the scenes of their tests.

Everything the header computes is np.float32, in exactly the written association (Python evaluates a + b + c from the
left, as C does), vectorised over the voxels of a track (integrate), the crossings (surface points) or the pixels of a
view (ray cast), with Python loops over the tracks, the views and the march steps, as in tests/fusion_ref.py: elements
that a step drops are carried along (their values may be NaN or inf) and masked at the end.

The scenes are those of tests/fusion_ref.py (make_scene) and the corner of tests/icp_ref.py, with one grid per track
placed by `grid_for`: the grids of the parity tests reach outside every frustum and behind the cameras, the grid of the
"away" scene lies above the cameras where no view looks.
"""
import numpy as np

from tests import fusion_ref as fr
from tests import icp_ref as ir

F = np.float32
NAN = F(np.nan)


# ---------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------
def volume(B, nx, ny, nz):
    """a fresh volume -> tsdf (ones), weight (zeros), each f32 [B,nz,ny,nx]"""
    return np.ones((B, nz, ny, nx), F), np.zeros((B, nz, ny, nx), F)


def centres(origin_b, voxel, nx, ny, nz):
    """the voxel centres of one track -> X0, X1, X2, each f32 [nz*ny*nx] (x fastest)"""
    voxel = F(voxel)
    X0 = origin_b[0] + voxel * np.arange(nx, dtype=F)
    X1 = origin_b[1] + voxel * np.arange(ny, dtype=F)
    X2 = origin_b[2] + voxel * np.arange(nz, dtype=F)
    shape = (nz, ny, nx)
    return (np.broadcast_to(X0[None, None, :], shape).reshape(-1), np.broadcast_to(X1[None, :, None], shape).reshape(-1),
            np.broadcast_to(X2[:, None, None], shape).reshape(-1))


def integrate(tsdf, weight, origin, voxel, depth, ray, K, R, t, valid=None, trunc=None, max_weight=64.0):
    """-> the updated (tsdf, weight), new arrays"""
    B, nz, ny, nx = tsdf.shape
    V, H, W = depth.shape[1:]
    assert all(a.dtype == F for a in (tsdf, weight, origin, depth, ray, K, R, t))
    voxel = F(voxel)
    trunc = F(4) * voxel if trunc is None else F(trunc)
    max_weight = F(max_weight)
    live = fr.live_mask(depth, valid)
    T_out, w_out = tsdf.copy(), weight.copy()
    for b in range(B):
        X = centres(origin[b], voxel, nx, ny, nz)
        T, w = tsdf[b].reshape(-1).copy(), weight[b].reshape(-1).copy()
        for v in range(V):                                        # ascending: the order of the average
            Rv, tv = R[b, v], t[b, v]
            with np.errstate(all="ignore"):
                S = [X[0] * Rv[c, 0] + X[1] * Rv[c, 1] + X[2] * Rv[c, 2] + tv[c] for c in range(3)]
                uvd = [S[0] * K[j, 0] + S[1] * K[j, 1] + S[2] * K[j, 2] for j in range(3)]
                ok = uvd[2] > 0
                xs = np.floor(uvd[0] / uvd[2] + F(0.5))
                ys = np.floor(uvd[1] / uvd[2] + F(0.5))
                assert xs.dtype == F and ys.dtype == F
                ok &= (xs >= F(0)) & (xs <= F(W - 1)) & (ys >= F(0)) & (ys <= F(H - 1))
                q = np.where(ok, ys, F(0)).astype(np.int64) * W + np.where(ok, xs, F(0)).astype(np.int64)
                ok &= live[b, v].reshape(-1)[q]
                sdf = depth[b, v].reshape(-1)[q] * ray[q, 2] - S[2]
                ok &= ~(sdf < -trunc)
                obs = np.fmin(F(1), sdf / trunc)
                new_T = np.where(w == 0, obs, (T * w + obs) / (w + F(1)))
                new_w = np.fmin(w + F(1), max_weight)
            assert new_T.dtype == F and new_w.dtype == F
            T, w = np.where(ok, new_T, T), np.where(ok, new_w, w)
        T_out[b], w_out[b] = T.reshape(nz, ny, nx), w.reshape(nz, ny, nx)
    return T_out, w_out


def usable_mask(tsdf, weight, min_weight=1.0):
    with np.errstate(invalid="ignore"):
        return (weight >= F(min_weight)) & (np.abs(tsdf) < F(1))


def surface_points(tsdf, weight, origin, voxel, min_weight=1.0):
    """-> points [M,3] f32, normals [M,3] f32 (NaN rows where there is none), src [M] int64 ascending, n_per_track [B]"""
    B, nz, ny, nx = tsdf.shape
    assert tsdf.dtype == F and weight.dtype == F and origin.dtype == F
    voxel, mw = F(voxel), F(min_weight)
    use = usable_mask(tsdf, weight, mw)
    neg = tsdf < 0
    emit = np.zeros((B, nz, ny, nx, 3), bool)
    emit[:, :, :, :-1, 0] = use[:, :, :, :-1] & use[:, :, :, 1:] & (neg[:, :, :, :-1] != neg[:, :, :, 1:])
    emit[:, :, :-1, :, 1] = use[:, :, :-1] & use[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    emit[:, :-1, :, :, 2] = use[:, :-1] & use[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    src = np.nonzero(emit.reshape(-1))[0].astype(np.int64)
    n_per_track = emit.reshape(B, -1).sum(1).astype(np.int64)
    g, c = np.divmod(src, 3)
    idx = [g % nx, (g // nx) % ny, (g // (nx * ny)) % nz]
    b = g // (nx * ny * nz)
    dim, stride = (nx, ny, nz), np.array([1, nx, nx * ny], np.int64)
    Tf, wf = tsdf.reshape(-1), weight.reshape(-1)
    n_of = g + stride[c]
    Ta, Tn = Tf[g], Tf[n_of]
    with np.errstate(all="ignore"):
        X = [origin[b, e] + voxel * idx[e].astype(F) for e in range(3)]
        moved = voxel * (Ta / (Ta - Tn))
        points = np.stack([np.where(c == e, X[e] + moved, X[e]) for e in range(3)], 1).reshape(-1, 3)
        at_n = np.abs(Tn) < np.abs(Ta)
        m = np.where(at_n, n_of, g)
        ok = np.ones(len(src), bool)
        gd = []
        for e in range(3):
            ie = idx[e] + (at_n & (c == e))
            inside = (ie >= 1) & (ie + 1 < dim[e])
            up, dn = np.where(inside, m + stride[e], 0), np.where(inside, m - stride[e], 0)
            ok &= inside & (wf[up] >= mw) & (wf[dn] >= mw)
            gd.append(Tf[up] - Tf[dn])
        l2 = gd[0] * gd[0] + gd[1] * gd[1] + gd[2] * gd[2]
        length = np.sqrt(l2)
        ok &= l2 != 0
        normals = np.stack([np.where(ok, gd[e] / length, NAN) for e in range(3)], 1).reshape(-1, 3)
    assert points.dtype == F and normals.dtype == F
    return points, normals, src, n_per_track


def raycast(tsdf, weight, origin, voxel, ray, R, t, H, W, d_min, step, n_steps, min_weight=1.0):
    """-> depth f32 [B,V,H,W], NaN where the ray finds no surface"""
    B, nz, ny, nx = tsdf.shape
    V = R.shape[1]
    assert all(a.dtype == F for a in (tsdf, weight, origin, ray, R, t)) and ray.shape == (H * W, 3)
    voxel, d_min, step, mw = F(voxel), F(d_min), F(step), F(min_weight)
    out = np.full((B, V, H * W), NAN, F)
    sy, sz = nx, nx * ny
    corners = [0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1]
    for b in range(B):
        Tf, wf = tsdf[b].reshape(-1), weight[b].reshape(-1)
        for v in range(V):
            Rv, tv = R[b, v], t[b, v]
            active = np.ones(H * W, bool)
            prev_def = np.zeros(H * W, bool)
            prev_T = np.zeros(H * W, F)
            res = np.full(H * W, NAN, F)
            for n in range(n_steps):
                if not active.any():
                    break
                with np.errstate(all="ignore"):
                    d = d_min + step * F(n)
                    P = [d * ray[:, i] - tv[i] for i in range(3)]
                    X = [P[0] * Rv[0, j] + P[1] * Rv[1, j] + P[2] * Rv[2, j] for j in range(3)]
                    gc = [(X[c] - origin[b, c]) / voxel for c in range(3)]
                    i0 = [np.floor(x) for x in gc]
                    f = [gc[c] - i0[c] for c in range(3)]
                    dfn = np.ones(H * W, bool)
                    for c, n_c in enumerate((nx, ny, nz)):
                        dfn &= (i0[c] >= F(0)) & (i0[c] <= F(n_c - 2))
                    ii = [np.where(dfn, i0[c], F(0)).astype(np.int64) for c in range(3)]
                    base = ii[2] * sz + ii[1] * sy + ii[0]
                    base = np.where(dfn, base, 0)
                    if nx < 2 or ny < 2 or nz < 2:
                        dfn[:] = False
                        cs = [base] * 8
                    else:
                        cs = [base + o for o in corners]
                    for ce in cs:
                        dfn &= wf[ce] >= mw
                    a = [Tf[cs[2 * e]] + f[0] * (Tf[cs[2 * e + 1]] - Tf[cs[2 * e]]) for e in range(4)]
                    lo, hi = a[0] + f[1] * (a[1] - a[0]), a[2] + f[1] * (a[3] - a[2])
                    T = lo + f[2] * (hi - lo)
                    assert T.dtype == F
                    stop = active & dfn & (T <= 0)
                    hit = stop & prev_def & (prev_T > 0)
                    val = (d_min + step * F(n - 1)) + step * (prev_T / (prev_T - T))
                res = np.where(hit, val, res)
                active &= ~stop
                prev_def, prev_T = dfn, np.where(dfn, T, F(0))
            out[b, v] = res
    assert out.dtype == F
    return out.reshape(B, V, H, W)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def grid_for(kind, B, dims, voxel=None, first_xy=None):
    """origin f32 [B,3] and voxel for a grid of dims = (nx, ny, nz) per track.
    clean / noisy / plane / corner: centred on the optical axis in x and y, and z from -0.4 to 2.8 (voxel = 3.2 /
      max(nz, 2) unless given): the cameras sit within 0.05 of the origin and look down +z, so the first slices lie
      behind every camera, the surfaces (1.8 .. 2.7 away) lie inside, and a grid wider than a frustum (the half field
      of view is at most 22.6 degrees) has voxels outside every one.
    away: the same grid lifted above the cameras, all of which look horizontally, by more than half its horizontal
      reach: no view sees any voxel.
    first_xy, when given, is the x and y of voxel (0,0,0) instead (a grid of two voxels across straddles the optical axis
    and would see nothing).  Track b is shifted by b * 0.013 so that no two tracks share their voxel centres."""
    nx, ny, nz = dims
    if voxel is None:
        voxel = 3.2 / max(nz, 2)
    lo = np.array([-0.5 * voxel * (nx - 1), -0.5 * voxel * (ny - 1), -0.4])
    if first_xy is not None:
        lo[:2] = first_xy
    if kind == "away":                                             # y / distance >= 0.5 > tan(22.6 degrees) at every voxel
        lo[1] = 3.0 + 0.5 * np.hypot(0.5 * voxel * (nx - 1) + 0.1, 2.9)
    origin = np.stack([lo + 0.013 * b for b in range(B)]) if B else np.zeros((0, 3))
    return origin.astype(F), float(F(voxel))


def centred_grid(B, n, size, centre):
    """an n^3 grid of edge `size` around `centre` -> origin f32 [B,3], voxel (the accuracy tests: 48^3 over 1.6 m)"""
    voxel = float(F(size / n))
    lo = np.asarray(centre, np.float64) - 0.5 * voxel * (n - 1)
    return np.tile(lo, (B, 1)).astype(F), voxel


def plane_distance(points, plane):
    """unsigned distance of world points [M,3] to the plane (n, c): n . X = c"""
    n, c = plane[0], plane[1]
    return np.abs(points.astype(np.float64) @ n - c) / np.linalg.norm(n)


def scene_surface_distance(points):
    """unsigned distance of world points to the nearer of fusion_ref's two surfaces, the bounded PATCH and the PLANE
    (the patch counts only above its rectangle; beside it, the distance to its border)"""
    P = points.astype(np.float64)
    d_plane = plane_distance(P, fr.PLANE)
    n2, c2, xr, yr = fr.PATCH
    dx = np.maximum(np.maximum(xr[0] - P[:, 0], P[:, 0] - xr[1]), 0)
    dy = np.maximum(np.maximum(yr[0] - P[:, 1], P[:, 1] - yr[1]), 0)
    d_patch = np.sqrt((P[:, 2] - c2) ** 2 + dx ** 2 + dy ** 2)
    return np.minimum(d_plane, d_patch)


def view_points(depth, ray, R, t, mask):
    """the world points of the pixels of a track's views where mask is set -> [M,3] float64"""
    B, V, H, W = depth.shape
    out = []
    for b in range(B):
        for v in range(V):
            m = mask[b, v].reshape(-1) != 0
            P = depth[b, v].reshape(-1)[m, None].astype(np.float64) * ray[m].astype(np.float64) - t[b, v].astype(np.float64)
            out.append(P @ R[b, v].astype(np.float64))
    return np.concatenate(out)


def make_corner_model(shape, seed, dims, voxel, centre):
    """the corner scene of tests/icp_ref.py with V = 5 views: views 0..3 at their true poses are what gets integrated
    (`views`: depth, R, t, valid, and keep of the consistency rule at max_rel 0.01), a grid of dims voxels around `centre`,
    and the poses the model is cast at: that of view 0 and that of view 4, which is not integrated"""
    B, V, H, W = shape
    assert V == 5
    sc = dict(ir.make_corner(B, V, H, W, seed))
    voxel = float(F(voxel))
    lo = np.asarray(centre) - 0.5 * voxel * (np.asarray(dims) - 1)
    sc["origin"], sc["voxel"] = np.tile(lo, (B, 1)).astype(F), voxel
    sc["views"] = {k: np.ascontiguousarray(sc[k][:, :4]) for k in ("depth", "R", "t", "valid")}
    sc["views"]["keep"] = fr.consistency(sc["views"]["depth"], sc["ray"], sc["K"], sc["views"]["R"], sc["views"]["t"],
                                         sc["views"]["valid"], max_px=1.0, max_rel=0.01, min_views=1)[1]
    sc["R_cast"], sc["t_cast"] = np.ascontiguousarray(sc["R"][:, [0, 4]]), np.ascontiguousarray(sc["t"][:, [0, 4]])
    sc["truth_cast"] = np.ascontiguousarray(sc["depth"][:, [0, 4]])
    return sc
