"""Restatement of the signed nearest-face rule of include/ctd_hip_mesh_sdf.h in numpy, operation for operation as
csrc/ctd_point_tri.h, csrc/ctd_point_mesh_nearest.h and csrc/mesh_sdf.hip perform it.  tests/pointmesh_ref.py is imported
and left as it is: `point_tri` here is its f32 arithmetic with the branch code beside it (0, 1, 2 vertex a, b, c; 3, 4, 5
edge ab, ac, bc; 6 interior: the first region test that holds, not a reclassification of the clamped parameters),
`nearest` adds the cutoff (a face qualifies when d2 <= max_d2 and d2 < +inf), `incident_rows` builds the rows of valid
faces by vertex in ascending face order, and `signed` adds the f64 pseudonormal and the sign.  Every operator of the
pseudonormal is one IEEE f64 operation on Python floats in the association the header writes: no np.cross, no
np.linalg.norm, no @.  math.atan2 and math.sqrt are the platform's; the kernel's atan2 may differ by a few ulp, which is
why `signed` also returns, per point, `dot` and the scale S = |r| * W (W = |c| for an interior, the number of terms for an
edge, the sum of alpha_g for a vertex): a test compares signs only where |dot| stands clear of rounding against S."""
import math

import numpy as np

from tests import pointmesh_ref as pr

F = np.float32


def point_tri(p, a, b, c):
    """pointmesh_ref.point_tri with the branch: p [n,1,3], a, b, c [k,3] -> (d2 [n,k], q [n,k,3], region int8 [n,k]).
    d2 and q come from pointmesh_ref itself; the region tests are restated on the same f32 quantities."""
    dist2, q = pr.point_tri(p, a, b, c)
    dt = p.dtype
    zero = dt.type(0)
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = pr._dot(ab, ap), pr._dot(ac, ap)
        d3, d4 = pr._dot(ab, bp), pr._dot(ac, bp)
        d5, d6 = pr._dot(ab, cp), pr._dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= zero) & (d2 <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),
                 (va <= zero) & (e43 >= zero) & (e56 >= zero)]
    region = np.full(d1.shape, 6, np.int8)
    for cond, code in reversed(list(zip(conds, (0, 1, 3, 2, 4, 5)))):       # the first that holds decides
        region = np.where(cond, np.int8(code), region)
    return dist2, q, region


def nearest(points, verts, faces, max_d2=np.inf, chunk=128):
    """points [n,3], verts [m,3], faces [k,3], max_d2 (+inf or a float >= 0) -> (d2 [n] f32, face [n] int32, closest [n,3]
    f32, feature [n] int8) by the rule; (+inf, -1, NaN, -1) where no face qualifies"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    V = np.ascontiguousarray(verts, F).reshape(-1, 3)
    Fa = np.asarray(faces, np.int64).reshape(-1, 3)
    max_d2 = F(max_d2)
    n, k = P.shape[0], Fa.shape[0]
    d2 = np.full(n, np.inf, F)
    face = np.full(n, -1, np.int32)
    closest = np.full((n, 3), np.nan, F)
    feature = np.full(n, -1, np.int8)
    valid = ((Fa >= 0) & (Fa < V.shape[0])).all(1) if k else np.zeros(0, bool)
    if n == 0 or not valid.any():
        return d2, face, closest, feature
    Fc = np.where(valid[:, None], Fa, 0)
    a, b, c = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
    for i in range(0, n, chunk):
        dd, q, reg = point_tri(P[i:i + chunk, None, :], a[None], b[None], c[None])
        with np.errstate(invalid="ignore"):
            ok = valid[None, :] & (dd < np.inf) & (dd <= max_d2)            # NaN, +inf, skipped and cut-off faces never win
        dd = np.where(ok, dd, F(np.inf))
        f = dd.argmin(1)                                                    # the first (lowest) index of the minimum
        rows = np.arange(dd.shape[0])
        best = dd[rows, f]
        won = best < np.inf
        d2[i:i + chunk] = best
        face[i:i + chunk] = np.where(won, f, -1)
        closest[i:i + chunk] = np.where(won[:, None], q[rows, f], F(np.nan))
        feature[i:i + chunk] = np.where(won, reg[rows, f], np.int8(-1))
    return d2, face, closest, feature


def face_valid(g, n_verts):
    i0, i1, i2 = g
    return all(0 <= i < n_verts for i in g) and i0 != i1 and i1 != i2 and i0 != i2


def incident_rows(faces, n_verts):
    """(face_offsets int32 [n_verts+1], face_ids int32 [3 * n_valid]): per vertex its valid faces in ascending order, as
    meshsmooth.MeshAdjacency lays them out"""
    Fa = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = [[] for _ in range(n_verts)]
    for g, idx in enumerate(Fa.tolist()):
        if face_valid(idx, n_verts):
            for i in idx:
                rows[i].append(g)
    offsets = np.zeros(n_verts + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([g for r in rows for g in r], np.int32)
    return offsets, ids


def _cross(V, i0, i1, i2):
    a, b, d = V[i0], V[i1], V[i2]
    e1 = [float(b[0]) - float(a[0]), float(b[1]) - float(a[1]), float(b[2]) - float(a[2])]
    e2 = [float(d[0]) - float(a[0]), float(d[1]) - float(a[1]), float(d[2]) - float(a[2])]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def _len(c):
    s = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    return math.sqrt(s) if s >= 0 else float("nan")          # (a NaN s fails the comparison)


def _unit(V, g):
    c = _cross(V, *g)
    l = _len(c)
    if not (l > 0.0) or not math.isfinite(l):
        return None
    return [_div(c[0], l), _div(c[1], l), _div(c[2], l)]


def _div(x, y):
    return float(np.float64(x) / np.float64(y))               # IEEE division: no ZeroDivisionError, inf / inf = NaN


def _row(offsets, ids, i, n_incident):
    b, e = int(offsets[i]), int(offsets[i + 1])
    return ids[b:e].tolist() if 0 <= b <= e <= n_incident else []


def pseudonormal(V, Fa, offsets, ids, f, feat):
    """(N [3], W) of feature `feat` of face f; V f32 [m,3], Fa a list of index triples"""
    n_verts, n_faces, n_inc = len(V), len(Fa), len(ids)
    i0, i1, i2 = Fa[f]
    if feat == 6:
        c = _cross(V, i0, i1, i2)
        return c, _len(c)
    if feat < 3:
        lo, hi = (i0, i1, i2)[feat], -1
    else:
        ea, eb = (i1 if feat == 5 else i0), (i1 if feat == 3 else i2)
        lo, hi = min(ea, eb), max(ea, eb)
        if lo == hi:
            return [0.0, 0.0, 0.0], 0.0
    N, W = [0.0, 0.0, 0.0], 0.0
    for g in _row(offsets, ids, lo, n_inc):
        if g < 0 or g >= n_faces or not face_valid(Fa[g], n_verts) or lo not in Fa[g]:
            continue
        gi = Fa[g]
        if feat >= 3:
            if hi not in gi:
                continue
            term = _unit(V, gi)
            if term is None:
                continue
            W += 1.0
        else:
            unit = _unit(V, gi)
            if unit is None:
                continue
            at = gi.index(lo)
            o, un, wn = V[lo], V[gi[(at + 1) % 3]], V[gi[(at + 2) % 3]]
            u = [float(un[0]) - float(o[0]), float(un[1]) - float(o[1]), float(un[2]) - float(o[2])]
            w = [float(wn[0]) - float(o[0]), float(wn[1]) - float(o[1]), float(wn[2]) - float(o[2])]
            x = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            alpha = math.atan2(_len(x), (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2])
            term = [alpha * unit[0], alpha * unit[1], alpha * unit[2]]
            if not all(math.isfinite(t) for t in term):
                continue
            W += alpha
        N = [N[0] + term[0], N[1] + term[1], N[2] + term[2]]
    return N, W


def signed(points, verts, faces, max_d2=np.inf, rows=None):
    """-> dict of d2, face, closest, feature (as `nearest`), sign int8 [n], dot f64 [n] and S f64 [n] = |r| * W.  rows:
    (face_offsets, face_ids), `incident_rows` of the faces when None"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    V = np.ascontiguousarray(verts, F).reshape(-1, 3)
    Fa = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    offsets, ids = incident_rows(faces, len(V)) if rows is None else rows
    d2, face, closest, feature = nearest(P, V, faces, max_d2)
    n = len(P)
    sign, dot, S = np.zeros(n, np.int8), np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            if face[i] < 0:
                continue
            N, W = pseudonormal(V, Fa, offsets, ids, int(face[i]), int(feature[i]))
            r = [float(P[i, k]) - float(closest[i, k]) for k in range(3)]
            dt = (r[0] * N[0] + r[1] * N[1]) + r[2] * N[2]
            dot[i] = dt
            S[i] = _len(r) * W
            sign[i] = 1 if dt > 0 else (-1 if dt < 0 else 0)
    return dict(d2=d2, face=face, closest=closest, feature=feature, sign=sign, dot=dot, S=S)


def box_sdf(p, half=1.0):
    """the signed distance of points [n,3] (f64) from the axis-aligned cube [-half, half]^3, negative inside"""
    qd = np.abs(np.asarray(p, np.float64)) - half
    return np.linalg.norm(np.maximum(qd, 0), axis=1) + np.minimum(qd.max(1), 0)


def cube():
    """[-1,1]^3, 12 faces, outward"""
    v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], F)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def wedge():
    """the thin convex wedge: a base triangle in z = 0 and an apex 0.08 above it, four faces, outward"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0.4, 0.08]], F)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, f


def wedge_points(n=4000, seed=1):
    return (np.random.RandomState(seed).uniform(-0.3, 1.3, size=(n, 3)) * [1, 1, 0.3] - [0, 0, 0.1]).astype(F)


def plane_distances(points, verts, faces):
    """[n,k] f64: the signed distance of every point from every face's plane, along its outward unit normal"""
    V = np.asarray(verts, np.float64)
    a, b, c = (V[np.asarray(faces)[:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return ((np.asarray(points, np.float64)[:, None, :] - a[None]) * nrm[None]).sum(-1)


def cone(n=40, h=1.0):
    """a closed cone: a rim of n vertices at radius 1 in z = 0, the apex (vertex n, n incident faces) at height h, the
    base's centre (vertex n + 1); outward"""
    ang = np.arange(n) * 2 * np.pi / n
    v = np.concatenate([np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1), [[0, 0, h], [0, 0, 0]]]).astype(F)
    i = np.arange(n)
    j = (i + 1) % n
    f = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)]).astype(np.int32)
    return v, f


def fan3():
    """three faces on the edge {0, 1}"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.5, 1], [0.5, -0.5, -1]], F)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    return v, f
