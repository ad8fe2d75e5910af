"""Restatement of the view-colour rule of include/ctd_hip_mesh_color.h in numpy f32, operation for operation as
csrc/mesh_color.hip, csrc/ctd_view.h and csrc/ctd_render.h perform it: `ray_tri` (the ray casters' ray/triangle test), the
four steps per (point, view) and the blend in ascending view order.  Every operator below is one IEEE f32 operation on
arrays of that dtype, associated as the parentheses say, so the kernels have to give these bits.  The faces stream in
index order in chunks; the occlusion answer is a boolean, so the chunking cannot show."""
import numpy as np

F = np.float32
IN_IMAGE, FACING, UNOCCLUDED, USED = 1, 2, 4, 7


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def ray_tri(orig, dirs, v0, v1, v2):
    """ray_tri of csrc/ctd_render.h.  orig, dirs [n,1,3] (or [1,1,3]), v0, v1, v2 [1,k,3], f32 -> (accepted bool [n,k],
    ft f32 [n,k]); every rejection is a comparison that a NaN fails, as in the C code"""
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        pvec = _cross(dirs, e2)
        det = _dot(e1, pvec)
        reject = np.abs(det) < F(1e-6)
        inv_det = F(1) / det
        tvec = orig - v0
        u = _dot(tvec, pvec) * inv_det
        reject |= (u < 0) | (u > 1)
        qvec = _cross(tvec, e1)
        v = _dot(dirs, qvec) * inv_det
        reject |= (v < 0) | ((u + v) > 1)
        ft = _dot(e2, qvec) * inv_det
    assert ft.dtype == F
    return ~reject, ft


def camera_centre(R, t):
    """Cv_c = -((R[0][c] t0 + R[1][c] t1) + R[2][c] t2), f32 [3]"""
    R, t = np.asarray(R, F), np.asarray(t, F)
    return np.stack([-((R[0, c] * t[0] + R[1, c] * t[1]) + R[2, c] * t[2]) for c in range(3)]).astype(F)


def occluded(C, dirs, t_max, verts, faces, chunk=256, rows=512):
    """step 3 for the rays C [3] + s dirs [n,3] with limits t_max [n] -> bool [n]"""
    verts = np.ascontiguousarray(verts, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n = dirs.shape[0]
    out = np.zeros(n, bool)
    ok = ((faces >= 0) & (faces < verts.shape[0])).all(1)          # the others are skipped, never dereferenced
    o = np.asarray(C, F).reshape(1, 1, 3)
    for base in range(0, faces.shape[0], chunk):
        f = faces[base:base + chunk][ok[base:base + chunk]]
        if not len(f):
            continue
        v0, v1, v2 = (verts[f[:, k]][None] for k in range(3))
        for a in range(0, n, rows):
            acc, ft = ray_tri(o, dirs[a:a + rows, None, :], v0, v1, v2)
            with np.errstate(invalid="ignore"):
                out[a:a + rows] |= (acc & (ft > 0) & (ft < t_max[a:a + rows, None])).any(1)
    return out


def view_colors(points, images, K, R, t, margin, verts=None, faces=None, normals=None, valid=None, min_cos=0.0, mode=0):
    """points [n,3], images [V,C,H,W], K [3,3], R [V,3,3], t [V,3], verts [m,3], faces [k,3] (None: no mesh), normals [n,3]
    or None, valid [V,H,W] or None, mode 0 | 1 -> (color f32 [n,C], weight f32 [n], n_views int32 [n], flags uint8 [n,V])"""
    X = np.ascontiguousarray(points, F).reshape(-1, 3)
    I = np.ascontiguousarray(images, F)
    K, R, t = np.asarray(K, F), np.asarray(R, F), np.asarray(t, F)
    V, C, H, W = I.shape
    n = X.shape[0]
    margin, min_cos = F(margin), F(min_cos)
    N = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
    if verts is None:
        verts, faces = np.zeros((0, 3), F), np.zeros((0, 3), np.int64)
    flags = np.zeros((n, V), np.uint8)
    acc = np.zeros((n, C), F)
    wsum = np.zeros(n, F)
    count = np.zeros(n, np.int32)
    for v in range(V):
        with np.errstate(all="ignore"):
            # 1. IN_IMAGE
            S = [((X[:, 0] * R[v, j, 0] + X[:, 1] * R[v, j, 1]) + X[:, 2] * R[v, j, 2]) + t[v, j] for j in range(3)]
            uvd = [(S[0] * K[j, 0] + S[1] * K[j, 1]) + S[2] * K[j, 2] for j in range(3)]
            x, y = uvd[0] / uvd[2], uvd[1] / uvd[2]
            ok = (uvd[2] > 0) & (x >= 0) & (x <= F(W - 1)) & (y >= 0) & (y <= F(H - 1))
            x0, y0 = np.minimum(np.floor(x), F(W - 2)), np.minimum(np.floor(y), F(H - 2))
            fx, fy = x - x0, y - y0
            ix, iy = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
            if valid is not None:
                m = np.asarray(valid)[v] != 0
                ok &= m[iy, ix] & m[iy, ix + 1] & m[iy + 1, ix] & m[iy + 1, ix + 1]
            flags[ok, v] |= IN_IMAGE
            # 2. FACING
            Cv = camera_centre(R[v], t[v])
            w = np.ones(n, F)
            if N is not None:
                d = Cv[None] - X
                cosv = _dot(N, d) / np.sqrt(_dot(d, d))
                ok &= (cosv > 0) & (cosv >= min_cos)
                w = cosv
            flags[ok, v] |= FACING
            # 3. UNOCCLUDED
            e = X - Cv[None]
            length = np.sqrt(_dot(e, e))
            dirs = e / length[:, None]
            t_max = length - margin
        idx = np.nonzero(ok)[0]
        occ = occluded(Cv, dirs[idx], t_max[idx], verts, faces)
        used = idx[~occ]
        flags[used, v] |= UNOCCLUDED
        # 4. the sample and the blend
        px, py, gx, gy, wu = ix[used], iy[used], fx[used], fy[used], w[used]
        for c in range(C):
            P = I[v, c]
            i00, i01, i10, i11 = P[py, px], P[py, px + 1], P[py + 1, px], P[py + 1, px + 1]
            top = i00 + gx * (i01 - i00)
            bot = i10 + gx * (i11 - i10)
            s = top + gy * (bot - top)
            if mode == 0:
                acc[used, c] = acc[used, c] + wu * s
            else:
                better = (count[used] == 0) | (wu > wsum[used])
                acc[used[better], c] = s[better]
        if mode == 0:
            wsum[used] = wsum[used] + wu
        else:
            better = (count[used] == 0) | (wu > wsum[used])
            wsum[used[better]] = wu[better]
        count[used] += 1
    none = count == 0
    with np.errstate(all="ignore"):
        color = acc / wsum[:, None] if mode == 0 else acc.copy()
    color[none] = np.nan
    weight = np.where(none, F(0), wsum).astype(F)
    assert color.dtype == F and weight.dtype == F
    return color, weight, count, flags
