"""Numpy restatement of the rule of include/ctd_hip_mesh_simplify.h (ctd_mesh_simplify_f32): f32 for the cells, f64
elementwise for everything else, the sums in the rule's order (the k-th entry of every row at once, k ascending, so every
row is summed from 0 in its own order).  Written from the rule alone; it shares no code with csrc/mesh_simplify.hip.  Also
the small meshes that the tests of both sides use."""
import numpy as np

from tests import meshsmooth_ref as msr

F = np.float32
D = np.float64
MAX_CELLS_PER_AXIS = 1 << 20


def cells(verts, origin, cell):
    """-> (t f32 [n,3], the cell coordinates as floats; ok bool [n], all three finite and in [0, 2^20))"""
    x, o, c = np.asarray(verts, F).reshape(-1, 3), np.asarray(origin, F), F(cell)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = np.floor((x - o) / c)
    assert t.dtype == F
    with np.errstate(invalid="ignore"):
        ok = ((t >= 0) & (t < F(MAX_CELLS_PER_AXIS))).all(1)
    return t, ok


def _usable_rows(starts, total):
    k0, k1 = starts[:-1].astype(np.int64), starts[1:].astype(np.int64)
    ok = (k0 >= 0) & (k0 <= k1) & (k1 <= total)
    return k0, np.where(ok, k1 - k0, 0)


def vertex_quadrics(verts, faces, face_offsets, face_ids, clusterable, origin, n_incident=None):
    """f64 [n,9]: A00 A01 A02 A11 A12 A22 b0 b1 b2 of every vertex (zeros for an unclusterable one)"""
    x = np.asarray(verts, F).reshape(-1, 3)
    n = len(x)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    valid = msr.valid_faces(f, n)
    o = np.asarray(origin, F).astype(D)
    n_incident = len(face_ids) if n_incident is None else n_incident
    k0, length = _usable_rows(np.asarray(face_offsets), n_incident)
    length = np.where(clusterable, length, 0)
    Q = np.zeros((n, 9), D)
    rows = np.nonzero(length > 0)[0] if len(f) else np.zeros(0, np.int64)
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(rows):
            fid = face_ids[k0[rows] + k].astype(np.int64)
            ok = (fid >= 0) & (fid < len(f))
            safe = np.where(ok, fid, 0)
            ok &= valid[safe]
            tri = f[safe[ok]]
            all_in = clusterable[tri].all(1)
            r, tri = rows[ok][all_in], tri[all_in]
            q0, q1, q2 = (x[tri[:, c]].astype(D) - o for c in range(3))
            e1, e2 = q1 - q0, q2 - q0
            cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            d = -((cx * q0[:, 0] + cy * q0[:, 1]) + cz * q0[:, 2])
            add = np.stack([cx * cx, cx * cy, cx * cz, cy * cy, cy * cz, cz * cz, d * cx, d * cy, d * cz], 1)
            Q[r] = Q[r] + add
            k += 1
            rows = rows[length[rows] > k]
    return Q


def place(A, mean, idx, cell, reg):
    """the placement of clusters with quadrics A f64 [c,9], means f64 [c,3] (relative to the origin) and cells idx int
    [c,3] -> (x f64 [c,3] relative to the origin, fall bool [c])"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (A[:, k] for k in range(9))
    m0, m1, m2 = mean[:, 0], mean[:, 1], mean[:, 2]
    reg, dc = D(reg), D(F(cell))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lam = reg * ((a00 + a11) + a22)
        r0 = -(((a00 * m0 + a01 * m1) + a02 * m2) + b0)
        r1 = -(((a01 * m0 + a11 * m1) + a12 * m2) + b1)
        r2 = -(((a02 * m0 + a12 * m1) + a22 * m2) + b2)
        m00, m11, m22, m01, m02, m12 = a00 + lam, a11 + lam, a22 + lam, a01, a02, a12
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        x = np.stack([m0 + ((c00 * r0 + c01 * r1) + c02 * r2) / det, m1 + ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                      m2 + ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
        lo = idx.astype(D) * dc
        inside = (x >= lo - dc * 0.5) & (x <= lo + dc * 1.5)
        fall = ~(np.isfinite(lam) & (lam > 0)) | ~(np.isfinite(det) & (det > 0)) | ~np.isfinite(x).all(1) | ~inside.all(1)
    return np.where(fall[:, None], mean, x), fall


def simplify(verts, faces, face_offsets, face_ids, origin, cell, reg=1e-3, drop_duplicates=True, n_incident=None):
    """-> dict: verts f32 [n',3], leader int32 [n'], vert_cluster int32 [n], faces int32 [k,3], face_index int32 [k], counts
    int64 [8] (n', k, clusters, dropped, collapsed, duplicates, mean fallbacks among the emitted, the largest cluster), and
    for the tests mean f64 [n',3] (the emitted clusters' means, in world coordinates) and fall bool [n']"""
    x = np.ascontiguousarray(verts, F).reshape(-1, 3)
    n = len(x)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    m = len(f)
    o64 = np.asarray(origin, F).astype(D)
    valid = msr.valid_faces(f, n)
    used = np.zeros(n, bool)
    used[f[valid].reshape(-1)] = True
    t, in_range = cells(x, origin, cell)
    clusterable = used & in_range
    idx = np.where(clusterable[:, None], t, 0).astype(np.int64)
    key = (idx[:, 0] << 40) | (idx[:, 1] << 20) | idx[:, 2]
    cv = np.nonzero(clusterable)[0]                                 # ascending: the first vertex of a key is its leader
    _, first, inv = np.unique(key[cv], return_index=True, return_inverse=True)
    vleader = np.full(n, -1, np.int64)
    vleader[cv] = cv[first][inv.reshape(-1)]
    # members by cluster, ascending
    order = np.lexsort((cv, vleader[cv]))
    members = cv[order]
    leaders, start, count = np.unique(vleader[members], return_index=True, return_counts=True)
    Qv = vertex_quadrics(x, f, face_offsets, face_ids, clusterable, origin, n_incident)
    q = x.astype(D) - o64
    A, s = np.zeros((len(leaders), 9), D), np.zeros((len(leaders), 3), D)
    rows = np.arange(len(leaders))
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(rows):
            j = members[start[rows] + k]
            A[rows] = A[rows] + Qv[j]
            s[rows] = s[rows] + q[j]
            k += 1
            rows = rows[count[rows] > k]
        mean = s / count.astype(D)[:, None]
    placed, fall = place(A, mean, idx[leaders], cell, reg)
    # faces
    cand = valid.copy()
    cand[valid] = clusterable[f[valid]].all(1)
    L = np.full((m, 3), -1, np.int64)
    L[cand] = vleader[f[cand]]
    collapsed = cand & ((L[:, 0] == L[:, 1]) | (L[:, 0] == L[:, 2]) | (L[:, 1] == L[:, 2]))
    keep = cand & ~collapsed
    n_dup = 0
    if drop_duplicates:
        ids = np.nonzero(keep)[0]
        _, first = np.unique(np.sort(L[ids], 1), axis=0, return_index=True) if len(ids) else (None, np.zeros(0, np.int64))
        keep = np.zeros(m, bool)
        keep[ids[first]] = True                                     # ids ascends: the first of a triple is its smallest index
        n_dup = len(ids) - len(first)
    kept = np.nonzero(keep)[0]
    emitted = np.unique(L[kept].reshape(-1))                        # leaders, ascending
    out_of = np.full(n, -1, np.int64)
    out_of[emitted] = np.arange(len(emitted))
    at = np.searchsorted(leaders, emitted)                          # the emitted clusters among all of them
    with np.errstate(over="ignore"):
        verts_out = (placed[at] + o64).astype(F)
    vert_cluster = np.full(n, -1, np.int32)
    vert_cluster[vleader >= 0] = out_of[vleader[vleader >= 0]]
    counts = np.array([len(emitted), len(kept), len(leaders), m - cand.sum(), collapsed.sum(), n_dup, fall[at].sum(),
                       count.max() if len(count) else 0], np.int64)
    return dict(verts=verts_out, leader=emitted.astype(np.int32), vert_cluster=vert_cluster,
                faces=out_of[L[kept]].astype(np.int32).reshape(-1, 3), face_index=kept.astype(np.int32), counts=counts,
                mean=mean[at] + o64, fall=fall[at])


def simplify_mesh(verts, faces, origin, cell, reg=1e-3, drop_duplicates=True):
    """`simplify` over the incident-face rows of `meshsmooth_ref.adjacency`"""
    adj = msr.adjacency(faces, len(verts))
    return simplify(verts, faces, adj["face_offsets"], adj["face_ids"], origin, cell, reg, drop_duplicates)


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
def two_sheets(w=9, h=7, gap=0.25):
    """a w x h grid patch at z = 0 and the same patch at z = gap with the opposite winding, the lower sheet's faces first"""
    verts, faces = msr.grid_patch(w, h)
    upper = verts.copy()
    upper[:, 2] = gap
    return np.concatenate([verts, upper]).astype(F), np.concatenate([faces, faces[:, ::-1] + len(verts)]).astype(np.int32)


def cube_corner(k=8, step=0.125, corner=(1.0, 1.0, 1.0)):
    """three tessellated faces of a cube that meet at `corner`: each a (k+1) x (k+1) grid with dyadic spacing that
    reaches back from the corner along two axes; the vertices of the shared edges are stored once per face"""
    c = np.array(corner, D)
    verts, faces = [], []
    g, gf = msr.grid_patch(k + 1, k + 1)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        p = np.tile(c, (len(g), 1))
        p[:, u] -= g[:, 0].astype(D) * step
        p[:, v] -= g[:, 1].astype(D) * step
        faces.append(gf + len(verts) * len(g))
        verts.append(p)
    return np.concatenate(verts).astype(F), np.concatenate(faces).astype(np.int32)
