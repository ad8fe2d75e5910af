"""Numpy restatement of the rules of include/ext/ctd_hip_mesh_register.h (ctd_mesh_register_system_f32,
ctd_mesh_register_update_f32), operation for operation, and the corner scene of their tests.

The nearest face is tests/meshsdf_ref.nearest (tests/pointmesh_ref.nearest with the cutoff).  Everything the header
computes in f32 is np.float32 here in exactly the written association, vectorised over the points of a pose; points that
a step drops are carried along (their values may be NaN or inf) and masked at the end.  The sums of the system are NOT
math.fsum as in tests/icp_ref.py but the header's own order, step by step in f64 (chunks of 1024 points, slot i takes the
points i, i + 256, i + 512, i + 768, a butterfly over the distances 32 .. 1 inside each group of 64 slots, the four groups
ascending, the chunks ascending): every product of two f32 factors is exact in f64, so each step is one IEEE addition and
the kernel has to give these bits.  A dropped point adds +0.0, which changes no sum (a sum that starts at +0.0 never
becomes -0.0).  The solve is tests/icp_ref.factor and the solves as tests/icp_ref.icp_update writes them, in Python
floats."""
import math

import numpy as np

from tests import icp_ref as ir
from tests import meshsdf_ref as sr

F = np.float32
NAN = F(np.nan)
N_SYS = ir.N_SYS
CHUNK, THREADS = 1024, 256
AXES = [[F(1), F(0), F(0)], [F(0), F(1), F(0)], [F(0), F(0), F(1)]]


def transform(points, R, t):
    """S_j = ((R[j,0] p0 + R[j,1] p1) + R[j,2] p2) + t[j] -> list of 3 [n] f32"""
    assert points.dtype == F and R.dtype == F and t.dtype == F
    p = [points[:, i] for i in range(3)]
    with np.errstate(all="ignore"):
        return [((R[j, 0] * p[0] + R[j, 1] * p[1]) + R[j, 2] * p[2]) + t[j] for j in range(3)]


def ordered_sum(terms):
    """terms f64 [n] or [n,rows] (the rows of a point are added one after the other) -> the sum in the header's order"""
    terms = np.asarray(terms, np.float64)
    if terms.ndim == 1:
        terms = terms[:, None]
    n, rows = terms.shape
    if n == 0:
        return 0.0
    chunks = -(-n // CHUNK)
    padded = np.zeros((chunks * CHUNK, rows))
    padded[:n] = terms
    padded = padded.reshape(chunks, CHUNK // THREADS, THREADS, rows)
    with np.errstate(all="ignore"):
        acc = np.zeros((chunks, THREADS))
        for c in range(CHUNK // THREADS):
            for r in range(rows):
                acc = acc + padded[:, c, :, r]
        v = acc.reshape(chunks, THREADS // 64, 64)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ off]
        w = v[:, 0, 0]
        for g in range(1, THREADS // 64):
            w = w + v[:, g, 0]
        s = w[0]
        for c in range(1, chunks):
            s = s + w[c]
    return float(s)


def pose_terms(points, R, t, verts, faces, metric, max_d2=np.inf):
    """one pose -> dict: ok [n] (not dropped), face int32 [n], residual f32 [n], closest f32 [n,3], e f32 [n,rows],
    J f32 [n,rows,6]"""
    V = np.ascontiguousarray(verts, F).reshape(-1, 3)
    Fa = np.asarray(faces, np.int64).reshape(-1, 3)
    S = transform(points, R, t)
    d2, face, q, _ = sr.nearest(np.stack(S, 1), V, Fa, max_d2)
    ok = face >= 0
    with np.errstate(all="ignore"):
        D = [S[i] - q[:, i] for i in range(3)]
        if metric == 0:
            idx = Fa[np.where(ok, face, 0)] if len(Fa) else np.zeros((len(face), 3), np.int64)
            idx = np.where(ok[:, None], idx, 0)
            if len(V) == 0:
                V = np.zeros((1, 3), F)
            v0, v1, v2 = V[idx[:, 0]], V[idx[:, 1]], V[idx[:, 2]]
            e1 = [v1[:, i] - v0[:, i] for i in range(3)]
            e2 = [v2[:, i] - v0[:, i] for i in range(3)]
            c = ir.cross(e1, e2)
            l = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
            assert l.dtype == F
            ok = ok & (l > 0) & np.isfinite(l)
            n = [c[i] / l for i in range(3)]
            e = n[0] * D[0] + n[1] * D[1] + n[2] * D[2]
            J = np.stack(ir.cross(S, n) + n, 1)[:, None, :]
            e = e[:, None]
            residual = e[:, 0]
        else:
            ones = np.ones_like(S[0])
            J = np.stack([np.stack(ir.cross(S, [u * ones for u in ax]) + [u * ones for u in ax], 1) for ax in AXES], 1)
            e = np.stack(D, 1)
            residual = np.sqrt(d2)
    assert e.dtype == F and J.dtype == F and residual.dtype == F
    return {"ok": ok, "face": np.where(ok, face, -1).astype(np.int32), "residual": np.where(ok, residual, NAN),
            "closest": q, "e": e, "J": J}


def system(points, R, t, verts, faces, metric=0, max_d2=np.inf):
    """R [K,3,3], t [K,3] -> system f64 [K,29] in the header's order, face int32 [K,n], residual f32 [K,n], closest f32
    [K,n,3]"""
    K, n = R.shape[0], points.shape[0]
    out = np.zeros((K, N_SYS))
    face = np.full((K, n), -1, np.int32)
    residual = np.full((K, n), NAN, F)
    closest = np.full((K, n, 3), NAN, F)
    for k in range(K):
        if n == 0:
            continue
        m = pose_terms(points, R[k], t[k], verts, faces, metric, max_d2)
        ok = m["ok"]
        face[k], residual[k], closest[k] = m["face"], m["residual"], m["closest"]
        J, e = m["J"].astype(np.float64), m["e"].astype(np.float64)
        with np.errstate(all="ignore"):
            terms = [J[:, :, i] * J[:, :, j] for i, j in ir.TRIANGLE] + [J[:, :, i] * e for i in range(6)] + [e * e]
            for a, term in enumerate(terms):
                out[k, a] = ordered_sum(np.where(ok[:, None], term, 0.0))
        out[k, 28] = ordered_sum(ok.astype(np.float64))
    return out, face, residual, closest


def solve_step(sys_row, min_count=64, min_pivot=1e-4, damping=0.0):
    """-> (ok, x [6], Rr 3 x 3): the refusals, the three solves and the Rodrigues step of include/ctd_hip_icp.h"""
    if not float(sys_row[28]) >= min_count:
        return False, None, None
    good, L, D, _ = ir.factor(sys_row, float(damping), float(min_pivot))
    if not good:
        return False, None, None
    g = [float(v) for v in sys_row[21:27]]
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
    return True, x, Rr


def update(systems, R, t, min_count=64, min_pivot=1e-4, damping=0.0):
    """-> R' f32 [K,3,3], t' f32 [K,3], ok uint8 [K]"""
    assert R.dtype == F and t.dtype == F and systems.dtype == np.float64
    K = R.shape[0]
    R_out, t_out, ok_out = R.copy(), t.copy(), np.zeros(K, np.uint8)
    for k in range(K):
        good, x, Rr = solve_step(systems[k], min_count, min_pivot, damping)
        if not good:
            continue
        Rd = [[float(R[k, i, j]) for j in range(3)] for i in range(3)]
        td = [float(v) for v in t[k]]
        for i in range(3):
            for j in range(3):
                R_out[k, i, j] = F(Rr[i][0] * Rd[0][j] + Rr[i][1] * Rd[1][j] + Rr[i][2] * Rd[2][j])
            t_out[k, i] = F(Rr[i][0] * td[0] + Rr[i][1] * td[1] + Rr[i][2] * td[2] + x[3 + i])
        ok_out[k] = 1
    return R_out, t_out, ok_out


def mesh_icp(points, verts, faces, R, t, iters=10, metric=0, max_dist=None, min_count=64, min_pivot=1e-4, damping=0.0):
    """`iters` rounds of system and update -> R', t', info: count and rms [iters,K] of the system each round solved, ok
    [K] of the last round, and the poses after every round (R_steps, t_steps)"""
    max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
    K = R.shape[0]
    info = {"count": np.zeros((iters, K)), "rms": np.zeros((iters, K)), "ok": np.zeros(K, np.uint8), "R_steps": [],
            "t_steps": []}
    for it in range(iters):
        s = system(points, R, t, verts, faces, metric, max_d2)[0]
        info["count"][it] = s[:, 28]
        with np.errstate(all="ignore"):
            info["rms"][it] = np.sqrt(s[:, 27] / s[:, 28])
        R, t, info["ok"] = update(s, R, t, min_count, min_pivot, damping)
        info["R_steps"].append(R)
        info["t_steps"].append(t)
    return R, t, info


# ---------------------------------------------------------------------------------------------------------------------
# the corner scene
# ---------------------------------------------------------------------------------------------------------------------
def corner_mesh(quads=6):
    """three orthogonal unit squares that meet at the origin (in the planes x = 0, y = 0 and z = 0, over [0,1]^2), each
    `quads` x `quads` quads of two triangles: 6 x 6 gives 216 faces -> verts f32 [3 (quads+1)^2, 3], faces int32.  The
    squares do not share vertices; square a holds the faces [a * 2 quads^2, (a + 1) * 2 quads^2)."""
    g = np.arange(quads + 1, dtype=np.float64) / quads
    u, v = np.meshgrid(g, g, indexing="ij")
    verts, faces = [], []
    for axis in range(3):
        P = np.zeros((quads + 1, quads + 1, 3))
        P[..., (axis + 1) % 3] = u
        P[..., (axis + 2) % 3] = v
        base = len(verts) * (quads + 1) ** 2
        verts.append(P.reshape(-1, 3))
        for i in range(quads):
            for j in range(quads):
                a = base + i * (quads + 1) + j
                b, c, d = a + quads + 1, a + quads + 2, a + 1
                faces += [[a, b, c], [a, c, d]]                     # (e1 x e2 points along +axis, into the corner)
    return np.concatenate(verts).astype(F), np.array(faces, np.int32)


def corner_points(rs, n=2000, limit=0.85, noise=0.0):
    """n points drawn uniformly from the part of the three squares where every coordinate is < limit, plus Gaussian
    noise of that standard deviation -> f64 [n,3]"""
    axis = rs.randint(0, 3, size=n)
    uv = rs.rand(n, 2) * limit
    P = np.zeros((n, 3))
    P[np.arange(n), (axis + 1) % 3] = uv[:, 0]
    P[np.arange(n), (axis + 2) % 3] = uv[:, 1]
    if noise:
        P = P + rs.normal(size=(n, 3)) * noise
    return P


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a) * np.deg2rad(degrees)
    th = np.linalg.norm(a)
    Wx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def make_corner(seed, n=2000, degrees=20.0, shift=0.1, noise=0.0, quads=6):
    """-> dict(verts, faces, points: the samples displaced by a rotation of `degrees` about a random axis through their
    centroid and a translation of length `shift` in a random direction, R_true, t_true: the pose that takes them back,
    f64).  The rotation is about the centroid, which keeps the samples' displacement near 0.25 (20 degrees on an arm of
    0.6, plus the shift): about the origin the far samples would move by 0.4."""
    rs = np.random.RandomState(seed)
    verts, faces = corner_mesh(quads)
    P = corner_points(rs, n, noise=noise)
    Q = rotation(rs.normal(size=3), degrees)
    d = rs.normal(size=3)
    d = d / np.linalg.norm(d) * shift
    c = P.mean(0)
    moved = (P - c) @ Q.T + c + d                                   # p' = Q (p - c) + c + d
    # p = Q^T (p' - c - d) + c
    return {"verts": verts, "faces": faces, "points": np.ascontiguousarray(moved.astype(F)), "R_true": Q.T,
            "t_true": c - Q.T @ (c + d)}


def pose_error(R, t, R_true, t_true):
    """-> (the angle of R R_true^T in degrees, |t - t_true|), float64"""
    rot, tr = ir.pose_errors(np.asarray(R)[None, None], np.asarray(t)[None, None], np.asarray(R_true)[None, None],
                             np.asarray(t_true)[None, None])
    return float(rot[0, 0]), float(tr[0, 0])
