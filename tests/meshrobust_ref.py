"""Numpy restatement of the rules of include/ext/ctd_hip_mesh_robust.h (ctd_mesh_face_rim_u8, ctd_mesh_robust_system_f32),
operation for operation, on tests/meshreg_ref.py and tests/meshsdf_ref.py, and the scenes of their tests.

`face_rim` walks the incident-face rows as the header says (tests/meshsdf_ref.incident_rows lays them out as a
meshsmooth.MeshAdjacency does) and takes the vertex flags from the edge multiplicities.  `pose_query` is the part of a
pose's work that does not depend on the gates: S, the nearest face with its feature (meshsdf_ref.nearest), D, the face
normal, e, J and the residual, everything f32 in the written association, vectorised over the points; `gate` then gives
every point its status and weight, and `system` sums w * (x * y) in f64 (the inner product exact, one rounding for the
weight) in the header's order, meshreg_ref.ordered_sum.  A gated point adds +0.0.

`robust_scale` is meshrobust.robust_scale: float32(tune * 1.4826) times the lower median of the |residuals| that are not
NaN, one f32 product.  `robust_mesh_icp` is the loop, with scale 'mad': round 0 at c = +inf."""
import numpy as np

from tests import icp_ref as ir
from tests import meshreg_ref as mr
from tests import meshsdf_ref as sr

F = np.float32
NAN = F(np.nan)
BOUNDARY = 2
KERNELS = {"none": 0, "huber": 1, "tukey": 2}
TUNE = {1: 1.345, 2: 4.685}


# ---------------------------------------------------------------------------------------------------------------------
def vertex_flags(faces, n_verts):
    """uint8 [n_verts]: BOUNDARY for the ends of the edges that exactly one valid face uses (the bit the rim reads)"""
    Fa = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    mult = {}
    for g in Fa:
        if sr.face_valid(g, n_verts):
            for i, j in ((g[0], g[1]), (g[0], g[2]), (g[1], g[2])):
                key = (min(i, j), max(i, j))
                mult[key] = mult.get(key, 0) + 1
    flags = np.zeros(n_verts, np.uint8)
    for (i, j), m in mult.items():
        if m == 1:
            flags[i] |= BOUNDARY
            flags[j] |= BOUNDARY
    return flags


def edge_multiplicity(Fa, n_verts, offsets, ids, i, j):
    lo, hi = min(i, j), max(i, j)
    count = 0
    for g in sr._row(offsets, ids, lo, len(ids)):
        if g < 0 or g >= len(Fa) or not sr.face_valid(Fa[g], n_verts):
            continue
        if lo in Fa[g] and hi in Fa[g]:
            count += 1
    return count


def face_rim(faces, n_verts, rows=None, vflags=None):
    """-> uint8 [n_faces]: bits 0..2 the corners with BOUNDARY, bits 3..5 the edges ab, ac, bc of multiplicity 1"""
    Fa = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    offsets, ids = sr.incident_rows(faces, n_verts) if rows is None else rows
    vflags = vertex_flags(faces, n_verts) if vflags is None else vflags
    rim = np.zeros(len(Fa), np.uint8)
    for f, (a, b, c) in enumerate(Fa):
        if not sr.face_valid((a, b, c), n_verts):
            continue
        out = 0
        for bit, v in enumerate((a, b, c)):
            if vflags[v] & BOUNDARY:
                out |= 1 << bit
        for bit, (i, j) in zip((3, 4, 5), ((a, b), (a, c), (b, c))):
            if edge_multiplicity(Fa, n_verts, offsets, ids, i, j) == 1:
                out |= 1 << bit
        rim[f] = out
    return rim


# ---------------------------------------------------------------------------------------------------------------------
def pose_query(points, R, t, verts, faces, metric, max_d2=np.inf):
    """one pose, before the gates -> dict: face int32 [n] (the query's), feature int8 [n], closest f32 [n,3], d2 f32 [n],
    has_normal bool [n] (l > 0 and finite; `gate` asks only when the rule needs the normal), n: list of 3 f32 [n], e f32
    [n,rows], J f32 [n,rows,6], r f32 [n] (|e| or sqrt(d2)), residual f32 [n]"""
    V = np.ascontiguousarray(verts, F).reshape(-1, 3)
    Fa = np.asarray(faces, np.int64).reshape(-1, 3)
    S = mr.transform(points, R, t)
    d2, face, q, feature = sr.nearest(np.stack(S, 1), V, Fa, max_d2)
    hit = face >= 0
    with np.errstate(all="ignore"):
        D = [S[i] - q[:, i] for i in range(3)]
        idx = Fa[np.where(hit, face, 0)] if len(Fa) else np.zeros((len(face), 3), np.int64)
        idx = np.where(hit[:, None], idx, 0)
        if len(V) == 0:
            V = np.zeros((1, 3), F)
        v0, v1, v2 = V[idx[:, 0]], V[idx[:, 1]], V[idx[:, 2]]
        e1 = [v1[:, i] - v0[:, i] for i in range(3)]
        e2 = [v2[:, i] - v0[:, i] for i in range(3)]
        c = ir.cross(e1, e2)
        l = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        assert l.dtype == F
        has_normal = (l > 0) & np.isfinite(l)
        n = [c[i] / l for i in range(3)]
        if metric == 0:
            e = n[0] * D[0] + n[1] * D[1] + n[2] * D[2]
            J = np.stack(ir.cross(S, n) + n, 1)[:, None, :]
            r = np.abs(e)
            residual = e
            e = e[:, None]
        else:
            ones = np.ones_like(S[0])
            J = np.stack([np.stack(ir.cross(S, [u * ones for u in ax]) + [u * ones for u in ax], 1) for ax in mr.AXES], 1)
            e = np.stack(D, 1)
            r = np.sqrt(d2)
            residual = r
    assert e.dtype == F and J.dtype == F and r.dtype == F
    return {"face": face, "feature": feature, "closest": q, "d2": d2, "has_normal": has_normal, "n": n, "e": e, "J": J, "r": r,
            "residual": residual, "R": R, "metric": metric}


def gate(qr, kernel=0, c=None, rim=None, normals=None, min_cos=0.0):
    """the statuses and weights of one pose from its `pose_query` -> (status int8 [n], weight f32 [n])"""
    face, r = qr["face"], qr["r"]
    n_pts = len(face)
    status = np.zeros(n_pts, np.int8)

    def settle(cond, code):
        status[(status == 0) & cond] = code

    settle(face < 0, 1)
    if qr["metric"] == 0 or normals is not None:
        settle(~qr["has_normal"], 2)
    if rim is not None:
        feat = qr["feature"].astype(np.int64)
        bits = np.asarray(rim)[np.where(face >= 0, face, 0)].astype(np.int64) if len(rim) else np.zeros(n_pts, np.int64)
        settle((feat >= 0) & (feat <= 5) & (((bits >> np.clip(feat, 0, 7)) & 1) != 0), 3)
    with np.errstate(all="ignore"):
        if normals is not None:
            assert normals.dtype == F and qr["n"] is not None
            R, a, n = qr["R"], [normals[:, i] for i in range(3)], qr["n"]
            m = [(R[j, 0] * a[0] + R[j, 1] * a[1]) + R[j, 2] * a[2] for j in range(3)]
            cosang = (m[0] * n[0] + m[1] * n[1]) + m[2] * n[2]
            assert cosang.dtype == F
            settle(~(cosang >= F(min_cos)), 4)
        w = np.ones(n_pts, F)
        if kernel != 0:
            c = F(c)
            if not c > 0:
                settle(np.ones(n_pts, bool), 5)
            elif kernel == 1:
                w = np.where(r <= c, F(1), c / r)
            else:
                u = r / c
                v = F(1) - u * u
                w = v * v
                settle(~(r < c), 5)
            assert w.dtype == F
        settle(w == 0, 5)
    return status, np.where(status == 0, w, F(0)).astype(F)


def system(points, R, t, verts, faces, metric=0, max_d2=np.inf, kernel=0, scale=None, rim=None, normals=None, min_cos=0.0,
           queries=None):
    """R [K,3,3], t [K,3], scale [K] -> dict: system f64 [K,29] in the header's order, face int32 [K,n], residual f32
    [K,n], weight f32 [K,n], status int8 [K,n], closest f32 [K,n,3].  queries: the poses' `pose_query` results when the
    caller has them already (they do not depend on the gates)."""
    K, n = R.shape[0], points.shape[0]
    out = {"system": np.zeros((K, mr.N_SYS)), "face": np.full((K, n), -1, np.int32), "residual": np.full((K, n), NAN, F),
           "weight": np.zeros((K, n), F), "status": np.ones((K, n), np.int8), "closest": np.full((K, n, 3), NAN, F)}
    for k in range(K):
        if n == 0:
            continue
        qr = queries[k] if queries is not None else pose_query(points, R[k], t[k], verts, faces, metric, max_d2)
        status, w = gate(qr, kernel, None if scale is None else scale[k], rim, normals, min_cos)
        ok = status == 0
        out["face"][k], out["closest"][k], out["status"][k], out["weight"][k] = qr["face"], qr["closest"], status, w
        out["residual"][k] = np.where(ok, qr["residual"], NAN)
        J, e, wd = qr["J"].astype(np.float64), qr["e"].astype(np.float64), w.astype(np.float64)[:, None]
        with np.errstate(all="ignore"):
            terms = [J[:, :, i] * J[:, :, j] for i, j in ir.TRIANGLE] + [J[:, :, i] * e for i in range(6)] + [e * e]
            for a, term in enumerate(terms):
                out["system"][k, a] = mr.ordered_sum(np.where(ok[:, None], wd * term, 0.0))
        out["system"][k, 28] = mr.ordered_sum(ok.astype(np.float64))
    return out


def robust_scale(residual, kernel):
    """residual f32 [K,n] -> f32 [K]: float32(tune * 1.4826) * the lower median of the |residuals| that are not NaN"""
    factor = F(TUNE[kernel] * 1.4826)
    out = np.full(residual.shape[0], NAN, F)
    for k, row in enumerate(residual):
        v = np.sort(np.abs(row[~np.isnan(row)]))
        if len(v):
            out[k] = v[(len(v) - 1) // 2] * factor
    return out


def robust_mesh_icp(points, verts, faces, R, t, iters=10, metric=0, kernel=2, rim=None, normals=None, min_cos=0.0,
                    max_dist=None, min_count=64, min_pivot=1e-4, damping=0.0):
    """scale 'mad' -> R', t', info: used, rms and scale [iters,K], ok [K] of the last round"""
    max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
    K = R.shape[0]
    info = {"used": np.zeros((iters, K)), "rms": np.zeros((iters, K)), "scale": np.zeros((iters, K), F), "ok": np.zeros(K, np.uint8)}
    c = np.full(K, np.inf, F)
    for it in range(iters):
        out = system(points, R, t, verts, faces, metric, max_d2, kernel, c, rim, normals, min_cos)
        s = out["system"]
        info["used"][it], info["scale"][it] = s[:, 28], c if kernel else NAN
        with np.errstate(all="ignore"):
            info["rms"][it] = np.sqrt(s[:, 27] / s[:, 28])
        R, t, info["ok"] = mr.update(s, R, t, min_count, min_pivot, damping)
        if kernel:
            c = robust_scale(out["residual"], kernel)
    return R, t, info


# ---------------------------------------------------------------------------------------------------------------------
# the scenes of the issue's table: the corner of meshreg_ref, 2000 samples moved by 5 degrees and 0.03, Gaussian noise 0.002
# ---------------------------------------------------------------------------------------------------------------------
def make_scene(seed, n=2000, limit=0.85, outliers=0.0, degrees=5.0, shift=0.03, noise=0.002, quads=6):
    """-> dict as meshreg_ref.make_corner: samples of the corner with every in-plane coordinate < limit (1.2: overhanging
    the unit squares by 0.2), the share `outliers` of them replaced by points uniform in [-0.2, 0.85]^3, all displaced by
    a rotation of `degrees` about their centroid and a shift; R_true, t_true take them back"""
    rs = np.random.RandomState(seed)
    verts, faces = mr.corner_mesh(quads)
    P = mr.corner_points(rs, n, limit=limit, noise=noise)
    n_out = int(round(outliers * n))
    if n_out:
        where = rs.choice(n, n_out, replace=False)
        P[where] = rs.uniform(-0.2, 0.85, size=(n_out, 3))
    Q = mr.rotation(rs.normal(size=3), degrees)
    d = rs.normal(size=3)
    d = d / np.linalg.norm(d) * shift
    c = P.mean(0)
    moved = (P - c) @ Q.T + c + d
    return {"verts": verts, "faces": faces, "points": np.ascontiguousarray(moved.astype(F)), "R_true": Q.T,
            "t_true": c - Q.T @ (c + d)}


# name -> (make_scene arguments, metric, rounds, the robust path's arguments)
SCENES = {
    "outliers, plane": (dict(outliers=0.1), 0, 15, dict(kernel=2, rim=False)),
    "overhang, point": (dict(limit=1.2), 1, 30, dict(kernel=0, rim=True)),
    "overhang and outliers, point": (dict(limit=1.2, outliers=0.1), 1, 30, dict(kernel=2, rim=True)),
}
SCENE_SEEDS = (1, 2, 3)
SCENE_MAX_DIST = 0.25
