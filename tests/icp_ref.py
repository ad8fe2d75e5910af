"""Numpy restatement of the three rules of include/ctd_hip_icp.h (ctd_depth_normals_f32, ctd_depth_icp_system_f32,
ctd_depth_icp_update_f32), an exact reference for the sums of the system, and an analytic corner scene for their tests.

Everything the header computes in f32 is np.float32 here, in exactly the written association (Python evaluates
a + b + c from the left, as C does), vectorised over the pixels of a view with Python loops over the views, as in
tests/fusion_ref.py: pixels that a step drops are carried along (their values may be NaN or inf) and masked at the end.
The sums of the system are math.fsum over the exact f64 products, i.e. the correctly rounded value of the exact sum:
the header fixes an order for the library's own sums, and any order over exact terms lies within
(count - 1) * 2^-53 * sum |term| of it.  The update is Python floats (IEEE f64), statement by statement as the header
writes it.
"""
import math

import numpy as np

from tests import fusion_ref as fr

F = np.float32
NAN = F(np.nan)
INF = F(np.inf)
N_SYS = 29
TRIANGLE = [(i, j) for i in range(6) for j in range(i, 6)]         # the 21 upper-triangle entries, row-major


# ---------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------
def cross(u, w):
    """u x w, each component as u1*w2 - u2*w1"""
    return [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]


def normals(depth, ray, valid=None, max_rel=0.02):
    """-> normal f32 [B,V,H,W,3], three NaNs where a pixel gets none"""
    B, V, H, W = depth.shape
    assert depth.dtype == F and ray.dtype == F
    out = np.full((B, V, H, W, 3), NAN, F)
    if H < 3 or W < 3:
        return out
    live = fr.live_mask(depth, valid)
    r = ray.reshape(H, W, 3)
    mid = (slice(1, -1), slice(1, -1))
    nbs = [(slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2)),       # (y,x+1), (y,x-1)
           (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))]       # (y+1,x), (y-1,x)
    with np.errstate(all="ignore"):
        P = [depth * r[:, :, i] for i in range(3)]                             # [B,V,H,W] each
        d = depth[(Ellipsis,) + mid]
        tol = F(max_rel) * d
        ok = live[(Ellipsis,) + mid].copy()
        for nb in nbs:
            ok &= live[(Ellipsis,) + nb] & (np.abs(depth[(Ellipsis,) + nb] - d) <= tol)
        a = [P[i][(Ellipsis,) + nbs[0]] - P[i][(Ellipsis,) + nbs[1]] for i in range(3)]
        b = [P[i][(Ellipsis,) + nbs[2]] - P[i][(Ellipsis,) + nbs[3]] for i in range(3)]
        c = cross(a, b)
        l = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        assert l.dtype == F
        ok &= (l > 0) & (l < INF)
        n = [c[i] / l for i in range(3)]
        P0 = [P[i][(Ellipsis,) + mid] for i in range(3)]
        flip = n[0] * P0[0] + n[1] * P0[1] + n[2] * P0[2] > 0
        n = np.stack([np.where(flip, -n[i], n[i]) for i in range(3)], -1)
    assert n.dtype == F
    out[:, :, 1:-1, 1:-1] = np.where(ok[..., None], n, NAN)
    return out


def transform_point(d, rays, Ra, ta, Rb, tb, K):
    """fusion_ref.transform that also hands out S, the point in the frame of camera b -> (S, uvd), lists of 3 [n] f32"""
    P = [d * rays[:, i] - ta[i] for i in range(3)]
    Q = [P[0] * Ra[0, j] + P[1] * Ra[1, j] + P[2] * Ra[2, j] for j in range(3)]
    S = [Q[0] * Rb[j, 0] + Q[1] * Rb[j, 1] + Q[2] * Rb[j, 2] + tb[j] for j in range(3)]
    return S, [S[0] * K[j, 0] + S[1] * K[j, 1] + S[2] * K[j, 2] for j in range(3)]


def target_of(target, b, s, V):
    """the view that view s of track b is aligned to, or -1: skipped (target None: zeros)"""
    a = 0 if target is None else int(target[b][s])
    return -1 if a < 0 or a >= V or a == s else a


def view_terms(depth_t, live_t, normal_t, ray, K, R_t, t_t, s, a, max_dist):
    """The pixels of view s of one track against view a -> dict of [H*W] arrays: `ok` (not dropped), `p` (the in-view
    index of the pixel hit, 0 where unknown), `e` f32 and `J` f32 [H*W,6]"""
    V, H, W = depth_t.shape
    assert depth_t.dtype == F and normal_t.dtype == F and ray.dtype == F and K.dtype == F and R_t.dtype == F and t_t.dtype == F
    d = depth_t[s].reshape(-1)
    with np.errstate(all="ignore"):
        S, uvd = transform_point(d, ray, R_t[s], t_t[s], R_t[a], t_t[a], K)
        ok = live_t[s].reshape(-1) & (uvd[2] > 0)
        xs = np.floor(uvd[0] / uvd[2] + F(0.5))
        ys = np.floor(uvd[1] / uvd[2] + F(0.5))
        assert xs.dtype == F and ys.dtype == F
        ok &= (xs >= F(0)) & (xs <= F(W - 1)) & (ys >= F(0)) & (ys <= F(H - 1))
        p = np.where(ok, ys, F(0)).astype(np.int64) * W + np.where(ok, xs, F(0)).astype(np.int64)
        n = normal_t[a].reshape(-1, 3)[p]
        ok &= live_t[a].reshape(-1)[p] & np.isfinite(n).all(1)
        da = depth_t[a].reshape(-1)[p]
        D = [S[i] - da * ray[p, i] for i in range(3)]
        ok &= D[0] * D[0] + D[1] * D[1] + D[2] * D[2] <= F(max_dist) * F(max_dist)
        n = [n[:, i] for i in range(3)]
        e = n[0] * D[0] + n[1] * D[1] + n[2] * D[2]
        J = np.stack(cross(S, n) + n, 1)
    assert e.dtype == F and J.dtype == F
    return {"ok": ok, "p": p, "e": e, "J": J}


def icp_system(depth, normal, ray, K, R, t, valid=None, target=None, max_dist=0.1, with_abs=False):
    """-> system f64 [B,V,29] (each sum math.fsum over the exact products), residual f32 [B,V,H,W], assoc int64
    [B,V,H,W]; with_abs also abs_sum f64 [B,V,29], the sum of |term| of every entry (the count's is the count)"""
    B, V, H, W = depth.shape
    live = fr.live_mask(depth, valid)
    system = np.zeros((B, V, N_SYS))
    abs_sum = np.zeros((B, V, N_SYS))
    residual = np.full((B, V, H * W), NAN, F)
    assoc = np.full((B, V, H * W), -1, np.int64)
    for b in range(B):
        for s in range(V):
            a = target_of(target, b, s, V)
            if a < 0:
                continue
            m = view_terms(depth[b], live[b], normal[b], ray, K, R[b], t[b], s, a, max_dist)
            ok = m["ok"]
            residual[b, s] = np.where(ok, m["e"], NAN)
            assoc[b, s] = np.where(ok, (b * V + a) * H * W + m["p"], -1)
            J = m["J"][ok].astype(np.float64)
            e = m["e"][ok].astype(np.float64)
            terms = [J[:, i] * J[:, j] for i, j in TRIANGLE] + [J[:, i] * e for i in range(6)] + [e * e, np.ones(len(e))]
            with np.errstate(all="ignore"):
                for k, term in enumerate(terms):
                    term = term.tolist()
                    system[b, s, k] = math.fsum(term) if np.isfinite(term).all() else np.sum(term)
                    abs_sum[b, s, k] = math.fsum(np.abs(term).tolist()) if np.isfinite(term).all() else np.inf
    out = (system, residual.reshape(B, V, H, W), assoc.reshape(B, V, H, W))
    return out + (abs_sum,) if with_abs else out


def factor(sys_row, damping=0.0, min_pivot=0.0):
    """LDL^T of the damped matrix of one system, as the header writes it -> (ok, L, D, ratios), ratios = D_j / A_jj of
    the pivots reached (A_jj undamped)"""
    s = [float(x) for x in sys_row]
    A = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(TRIANGLE):
        A[i][j] = A[j][i] = s[k]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    ratios = []
    for j in range(6):
        d = A[j][j] + damping * A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        if A[j][j] != 0 and math.isfinite(A[j][j]):
            ratios.append(d / A[j][j])
        if not math.isfinite(d) or not d > min_pivot * A[j][j]:
            return False, L, D, ratios
        D[j] = d
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v / d
    return True, L, D, ratios


def icp_update(system, R, t, target=None, min_count=64, min_pivot=1e-4, damping=0.0):
    """-> R' f32 [B,V,3,3], t' f32 [B,V,3], ok uint8 [B,V]"""
    B, V = R.shape[:2]
    assert R.dtype == F and t.dtype == F and system.dtype == np.float64
    R_out, t_out, ok_out = R.copy(), t.copy(), np.zeros((B, V), np.uint8)
    for b in range(B):
        for s in range(V):
            a = target_of(target, b, s, V)
            if a < 0 or not float(system[b, s, 28]) >= min_count:
                continue
            good, L, D, _ = factor(system[b, s], float(damping), float(min_pivot))
            if not good:
                continue
            g = [float(x) for x in system[b, s, 21:27]]
            x = [0.0] * 6
            for i in range(6):
                v = -g[i]
                for k in range(i):
                    v = v - L[i][k] * x[k]
                x[i] = v
            for i in range(6):
                x[i] = x[i] / D[i]
            for i in range(5, -1, -1):
                v = x[i]
                for k in range(i + 1, 6):
                    v = v - L[k][i] * x[k]
                x[i] = v
            w = x[:3]
            th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
            th = math.sqrt(th2)
            if th < 1e-4:
                ca, cb = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
            else:
                ca, cb = math.sin(th) / th, (1.0 - math.cos(th)) / th2
            Wx = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
            Rr = [[(1.0 if i == j else 0.0) + ca * Wx[i][j] + cb * (w[i] * w[j] - th2 * (1.0 if i == j else 0.0))
                   for j in range(3)] for i in range(3)]
            Ra = [[float(R[b, a, i, j]) for j in range(3)] for i in range(3)]
            Rs = [[float(R[b, s, i, j]) for j in range(3)] for i in range(3)]
            ta = [float(v) for v in t[b, a]]
            ts = [float(v) for v in t[b, s]]
            M = [[Rr[0][i] * Ra[0][j] + Rr[1][i] * Ra[1][j] + Rr[2][i] * Ra[2][j] for j in range(3)] for i in range(3)]
            N = [[Ra[0][i] * M[0][j] + Ra[1][i] * M[1][j] + Ra[2][i] * M[2][j] for j in range(3)] for i in range(3)]
            u = [ta[i] - x[3 + i] for i in range(3)]
            ww = [Rr[0][i] * u[0] + Rr[1][i] * u[1] + Rr[2][i] * u[2] - ta[i] for i in range(3)]
            tn = [Ra[0][i] * ww[0] + Ra[1][i] * ww[1] + Ra[2][i] * ww[2] for i in range(3)]
            for i in range(3):
                for j in range(3):
                    R_out[b, s, i, j] = F(Rs[i][0] * N[0][j] + Rs[i][1] * N[1][j] + Rs[i][2] * N[2][j])
                t_out[b, s, i] = F(Rs[i][0] * tn[0] + Rs[i][1] * tn[1] + Rs[i][2] * tn[2] + ts[i])
            ok_out[b, s] = 1
    return R_out, t_out, ok_out


def depth_icp(depth, ray, K, R, t, valid=None, target=None, iters=10, max_rel=0.02, max_dist=0.1, min_count=64,
              min_pivot=1e-4, damping=0.0):
    """normals once, then `iters` rounds of system and update -> R', t', info: count and rmse [iters,B,V] of the system
    each round was solved from, ok [B,V] of the last round, and the poses after every round (R_steps, t_steps)"""
    B, V = R.shape[:2]
    normal = normals(depth, ray, valid, max_rel)
    info = {"count": np.zeros((iters, B, V)), "rmse": np.zeros((iters, B, V)), "ok": np.zeros((B, V), np.uint8),
            "R_steps": [], "t_steps": [], "pivot_ratio": np.full((iters, B, V), np.nan)}
    for it in range(iters):
        system = icp_system(depth, normal, ray, K, R, t, valid, target, max_dist)[0]
        info["count"][it] = system[..., 28]
        with np.errstate(all="ignore"):
            info["rmse"][it] = np.sqrt(system[..., 27] / system[..., 28])
        for b in range(B):
            for s in range(V):
                if target_of(target, b, s, V) >= 0 and system[b, s, 28] > 0:
                    ratios = factor(system[b, s], damping)[3]
                    info["pivot_ratio"][it, b, s] = min(ratios) if ratios else np.nan
        R, t, info["ok"] = icp_update(system, R, t, target, min_count, min_pivot, damping)
        info["R_steps"].append(R)
        info["t_steps"].append(t)
    return R, t, info


# ---------------------------------------------------------------------------------------------------------------------
# the corner scene and its truth
# ---------------------------------------------------------------------------------------------------------------------
# three mutually non-parallel world planes n . X = c with the cameras on the side n . X < c of each: a concave corner
# (a back wall, a wall on the right, a floor); the surface a ray sees is the nearest plane it hits.  The walls are tilted
# by about 22 degrees against the back wall: every plane is seen at less than 45 degrees of incidence, so at 48 x 80 the
# depth of neighbouring pixels differs by well under the 2 % of depth_normals' default max_rel, and each plane takes
# about a third of the image.  The creases are continuous in depth: the normals of the pixels on them blend two planes
# (which is why the truth comparison takes only stencils that lie on one plane).
CORNER = ((np.array([0.10, -0.05, 1.0]), 2.5), (np.array([0.4, 0.0, 1.0]), 2.6), (np.array([0.0, 0.4, 1.0]), 2.56))


def render_corner(ray, R, t, H, W):
    """-> depth f32 [B,V,H,W] (rendered in float64 from the f32 poses, cast to f32), truth normals f64 [B,V,H,W,3] in
    each camera's frame, facing it, and the plane id int [B,V,H,W]"""
    B, V = R.shape[:2]
    ray64 = ray.astype(np.float64)
    depth = np.empty((B, V, H * W))
    normal = np.empty((B, V, H * W, 3))
    plane = np.empty((B, V, H * W), np.int64)
    for b in range(B):
        for v in range(V):
            Rm, tv = R[b, v].astype(np.float64), t[b, v].astype(np.float64)
            o, dirs = -Rm.T @ tv, ray64 @ Rm                       # X_world = R^T (d ray - t) = o + d (R^T ray)
            with np.errstate(all="ignore"):
                ds = np.stack([np.where(dirs @ n > 0, (c - n @ o) / (dirs @ n), np.inf) for n, c in CORNER])
            plane[b, v] = ds.argmin(0)
            depth[b, v] = ds.min(0)
            ncam = np.stack([-(Rm @ n) / np.linalg.norm(n) for n, _ in CORNER])
            normal[b, v] = ncam[plane[b, v]]
    return depth.reshape(B, V, H, W).astype(F), normal.reshape(B, V, H, W, 3), plane.reshape(B, V, H, W)


def perturb_poses(R, t, rs, specs):
    """specs: {view: (degrees, metres)}: X_cam' = dR X_cam + dt with dR a rotation by `degrees` about a random axis and
    dt a random direction of length `metres` -> R', t' f32"""
    R2, t2 = R.astype(np.float64), t.astype(np.float64)
    for b in range(R.shape[0]):
        for v, (deg, dist) in specs.items():
            axis, dirn = rs.normal(size=3), rs.normal(size=3)
            dR = fr._rot(axis / np.linalg.norm(axis) * np.deg2rad(deg))
            R2[b, v] = dR @ R2[b, v]
            t2[b, v] = dR @ t2[b, v] + dirn / np.linalg.norm(dirn) * dist
    return R2.astype(F), t2.astype(F)


def make_corner(B, V, H, W, seed, specs=None):
    """-> dict(depth, valid (all ones), ray, K, R, t: the true poses, R0, t0: the perturbed ones (views 1 and 2 by
    1 degree / 1 cm and 2 degrees / 3 cm unless specs says otherwise), normal_true, plane)"""
    rs = np.random.RandomState(seed)
    K, ray = fr.camera(H, W)
    R, t = fr.overlapping_poses(rs, B, V)
    depth, normal_true, plane = render_corner(ray, R, t, H, W)
    if specs is None:
        specs = {v: s for v, s in ((1, (1.0, 0.01)), (2, (2.0, 0.03))) if v < V}
    R0, t0 = perturb_poses(R, t, rs, specs)
    return {"depth": np.ascontiguousarray(depth), "valid": np.ones((B, V, H, W), np.uint8), "ray": ray, "K": K, "R": R,
            "t": t, "R0": R0, "t0": t0, "normal_true": normal_true, "plane": plane}


def pose_errors(R, t, R_true, t_true):
    """-> rotation error in degrees [B,V] (the angle of R R_true^T) and translation error |t - t_true| [B,V], float64"""
    Rd = np.einsum("bvij,bvkj->bvik", R.astype(np.float64), R_true.astype(np.float64))
    cos = np.clip((np.trace(Rd, axis1=-2, axis2=-1) - 1) / 2, -1, 1)
    skew = np.stack([Rd[..., 2, 1] - Rd[..., 1, 2], Rd[..., 0, 2] - Rd[..., 2, 0], Rd[..., 1, 0] - Rd[..., 0, 1]], -1)
    ang = np.arctan2(np.linalg.norm(skew, axis=-1) / 2, cos)       # accurate for small angles, where acos is not
    return np.rad2deg(ang), np.linalg.norm(t.astype(np.float64) - t_true.astype(np.float64), axis=-1)


def keep_share(depth, ray, K, R, t, valid=None, max_px=1.0, max_rel=0.002):
    """the share of pixels that fusion_ref.consistency keeps"""
    return float(fr.consistency(depth, ray, K, R, t, valid, max_px, max_rel)[1].mean())
