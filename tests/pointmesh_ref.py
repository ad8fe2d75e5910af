"""Restatement of the nearest-face rule of include/ctd_hip_mesh_dist.h in numpy f32, operation for operation as
csrc/ctd_point_tri.h and the brute-force kernel of csrc/point_mesh.hip perform it: `point_tri` for a block of points
against all faces, `nearest` for the selection (smallest d2 among those < +inf, the lowest index among equal ones, -1 /
+inf / NaN when none qualifies; faces with an index outside [0, n_verts) take no part).  Every operator below is one
IEEE f32 operation on arrays of that dtype, associated as the parentheses say, so the kernels have to give these bits.

`dtype=np.float64` runs the same formulas in double: the nearest face in exact-enough arithmetic, which
`forward_bound` needs.  `forward_bound` evaluates the two-sided bound (2) / (3) of csrc/point_mesh.hip's header."""
import numpy as np

U = 2.0 ** -24


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def point_tri(p, a, b, c):
    """p [n,1,3], a, b, c [k,3] (or anything that broadcasts), all of one float dtype -> (d2 [n,k], q [n,k,3])"""
    dt = p.dtype
    zero, one = dt.type(0), dt.type(1)
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        inv = one / ((va + vb) + vc)
        t_bc = e43 / (e43 + e56)
        # the regions in the order of the rule; the first that holds decides
        conds = [(d1 <= zero) & (d2 <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),
                 (va <= zero) & (e43 >= zero) & (e56 >= zero)]
        z = np.zeros_like(d1)
        s_of = [z, z, d1 / (d1 - d3), z, z, one - t_bc]
        t_of = [z, z, z, z, d2 / (d2 - d6), t_bc]
        vert_of = [0, 1, -1, 2, -1, -1]
        s, t = vb * inv, vc * inv
        vertex = np.full(d1.shape, -1, np.int8)
        for cond, sv, tv, vv in reversed(list(zip(conds, s_of, t_of, vert_of))):
            s = np.where(cond, sv, s)
            t = np.where(cond, tv, t)
            vertex = np.where(cond, np.int8(vv), vertex)
        s = np.where(s > zero, s, zero)
        s = np.where(s < one, s, one)
        t = np.where(t > zero, t, zero)
        m = one - s
        t = np.where(t < m, t, m)
        q = (a + s[..., None] * ab) + t[..., None] * ac
        v = vertex[..., None]
        q = np.where(v == 0, a, np.where(v == 1, b, np.where(v == 2, c, q)))
        d = p - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert dist2.dtype == dt and q.dtype == dt
    return dist2, q


def nearest(points, verts, faces, dtype=np.float32, chunk=128):
    """points [n,3], verts [m,3], faces [k,3] -> (d2 [n] dtype, face [n] int32, closest [n,3] dtype) by the rule"""
    P = np.ascontiguousarray(points, dtype).reshape(-1, 3)
    V = np.ascontiguousarray(verts, dtype).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    n, k = P.shape[0], F.shape[0]
    d2 = np.full(n, np.inf, dtype)
    face = np.full(n, -1, np.int32)
    closest = np.full((n, 3), np.nan, dtype)
    if n == 0 or k == 0:
        return d2, face, closest
    valid = ((F >= 0) & (F < V.shape[0])).all(1)
    if not valid.any():
        return d2, face, closest
    Fc = np.where(valid[:, None], F, 0)
    a, b, c = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
    for i in range(0, n, chunk):
        dd, q = point_tri(P[i:i + chunk, None, :], a[None], b[None], c[None])
        dd = np.where(valid[None, :] & (dd < np.inf), dd, dtype(np.inf))     # NaN, +inf and skipped faces never win
        f = dd.argmin(1)                                                     # the first (lowest) index of the minimum
        rows = np.arange(dd.shape[0])
        best = dd[rows, f]
        won = best < np.inf
        d2[i:i + chunk] = best
        face[i:i + chunk] = np.where(won, f, -1)
        closest[i:i + chunk] = np.where(won[:, None], q[rows, f], dtype(np.nan))
    return d2, face, closest


def eta(verts, faces):
    """per face the bound (1) of point_mesh.hip: how far the computed closest point can lie from the exact triangle"""
    V = np.asarray(verts, np.float64)
    a, b, c = (V[faces[:, i]] for i in range(3))
    return 5.1 * U * (np.linalg.norm(a, axis=1) + np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - a, axis=1))


def forward_bound(points, verts, faces, face_star, dist):
    """Per point, the allowed |sqrt(d2_f32) - dist| by (2) and (3) of csrc/point_mesh.hip, evaluated for this mesh:
    below max_f eta_f + 2.6u dist; above eta + 47.5u E^3 R^2 / A^2 + 16u E R / e_min of the truly nearest face
    `face_star` (from the float64 run of `nearest`) + 2.6u dist.  The larger of the two sides, doubled once for the
    second-order terms the first-order analysis of (3) drops and for the final correctly rounded square root."""
    P = np.asarray(points, np.float64)
    V = np.asarray(verts, np.float64)
    F = np.asarray(faces)[face_star]
    a, b, c = (V[F[:, i]] for i in range(3))
    ab, ac, bc = b - a, c - a, c - b
    E = np.maximum(np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1))
    e_min = np.minimum(np.minimum(np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1)), np.linalg.norm(bc, axis=1))
    A = 0.5 * np.linalg.norm(np.cross(ab, ac), axis=1)
    R = np.maximum(np.maximum(np.linalg.norm(P - a, axis=1), np.linalg.norm(P - b, axis=1)), np.linalg.norm(P - c, axis=1))
    et = eta(verts, np.asarray(faces))
    below = et.max() + 2.6 * U * dist
    above = et[face_star] + 47.5 * U * E ** 3 * R ** 2 / A ** 2 + 16 * U * E * R / e_min + 2.6 * U * dist
    return 2.0 * np.maximum(below, above)
