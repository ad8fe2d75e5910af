"""Numpy restatement of the rule of include/ctd_hip_mesh_smooth.h (ctd_mesh_adjacency_i32, ctd_mesh_smooth_f32,
ctd_mesh_vertex_normals_f32): valid faces, incident faces and one-rings in compressed rows, edge multiplicities, vertex
flags and counts; the smoothing pass and the vertex normals in f32, the sums in the rule's order (the k-th entry of every
row at once, k ascending).  Written from the rule alone; it shares no code with csrc/mesh_smooth.hip.  Also the small
meshes that the tests of both sides use."""
import numpy as np

F = np.float32
REFERENCED, BOUNDARY, NONMANIFOLD = 1, 2, 4
MAX_INCIDENT = 1024


def valid_faces(faces, n_verts):
    """bool [m]: the three indices in [0, n_verts) and pairwise different"""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = ((f >= 0) & (f < n_verts)).all(1)
    return ok & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])


def _rows(owner, n_verts):
    """row starts int32 [n_verts+1] of entries sorted by owner"""
    return np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n_verts))]).astype(np.int32)


def adjacency(faces, n_verts):
    """-> dict: offsets, neighbors, face_offsets, face_ids (int32), vflags (uint8), counts (int64 [6]: nnz, edges,
    boundary edges, non-manifold edges, max_incident, valid faces) and mult (int64 [nnz], the multiplicity of each entry)"""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = valid_faces(f, n_verts)
    ids = np.nonzero(ok)[0]
    v = f[ok]
    # incidence: (vertex, face) pairs by vertex, then face
    owner, face = v.reshape(-1), np.repeat(ids, 3)
    order = np.lexsort((face, owner))
    face_ids, face_offsets = face[order].astype(np.int32), _rows(owner, n_verts)
    incident = np.bincount(owner, minlength=n_verts) if n_verts else np.zeros(0, np.int64)
    # rows: a receives b and c, b receives a and c, c receives a and b
    src = v[:, [0, 0, 1, 1, 2, 2]].reshape(-1)
    dst = v[:, [1, 2, 0, 2, 0, 1]].reshape(-1)
    key, mult = np.unique(src * max(n_verts, 1) + dst, return_counts=True)
    i, j = key // max(n_verts, 1), key % max(n_verts, 1)
    offsets = _rows(i, n_verts)
    vflags = np.zeros(n_verts, np.uint8)
    vflags[i] |= REFERENCED
    vflags[i[mult == 1]] |= BOUNDARY
    vflags[i[mult > 2]] |= NONMANIFOLD
    edge = i < j
    counts = np.array([len(key), edge.sum(), (edge & (mult == 1)).sum(), (edge & (mult > 2)).sum(),
                       incident.max() if len(incident) else 0, ok.sum()], np.int64)
    assert counts[0] == 2 * counts[1]
    return dict(offsets=offsets, neighbors=j.astype(np.int32), face_offsets=face_offsets, face_ids=face_ids, vflags=vflags,
                counts=counts, mult=mult)


def topology(adj):
    """-> (n_referenced, euler, closed) of what `adjacency` returned"""
    n_ref = int((adj["vflags"] & REFERENCED != 0).sum())
    c = adj["counts"]
    return n_ref, n_ref - int(c[1]) + int(c[5]), c[2] == 0 and c[3] == 0


def _usable_rows(starts, total):
    """rows [n] of starts int32 [n+1]: (first, length), the length 0 unless 0 <= first <= end <= total"""
    k0, k1 = starts[:-1].astype(np.int64), starts[1:].astype(np.int64)
    ok = (k0 >= 0) & (k0 <= k1) & (k1 <= total)
    return k0, np.where(ok, k1 - k0, 0)


def smooth_pass(x, offsets, neighbors, nnz, vflags, f, fix_boundary):
    """one pass with factor f over x f32 [n,3] -> f32 [n,3]; any offsets and neighbors (what the rule does not accept is
    skipped)"""
    assert x.dtype == F
    n = len(x)
    k0, length = _usable_rows(np.asarray(offsets), nnz)
    if fix_boundary:
        length = np.where(vflags & BOUNDARY != 0, 0, length)
    s, d = np.zeros((n, 3), F), np.zeros(n, np.int64)
    rows = np.nonzero(length > 0)[0]
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(rows):
            j = neighbors[k0[rows] + k].astype(np.int64)
            ok = (j >= 0) & (j < n)
            r = rows[ok]
            s[r] = s[r] + x[j[ok]]
            d[r] += 1
            k += 1
            rows = rows[length[rows] > k]
        out = x.copy()
        move = d > 0
        m = s[move] / d[move].astype(F)[:, None]
        out[move] = x[move] + F(f) * (m - x[move])
    assert out.dtype == F
    return out


def smooth(x, offsets, neighbors, vflags, iters=10, lam=0.5, mu=-0.53, fix_boundary=True, nnz=None):
    nnz = len(neighbors) if nnz is None else nnz
    x = x.copy()
    for _ in range(iters):
        x = smooth_pass(x, offsets, neighbors, nnz, vflags, lam, fix_boundary)
        if mu != 0:
            x = smooth_pass(x, offsets, neighbors, nnz, vflags, mu, fix_boundary)
    return x


def vertex_normals(x, faces, face_offsets, face_ids, n_incident=None):
    """f32 [n,3]: the sum of (v1 - v0) x (v2 - v0) over the incident faces in the order of the row, over its length; NaN
    where that length is 0 or not finite"""
    assert x.dtype == F
    n = len(x)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    n_incident = len(face_ids) if n_incident is None else n_incident
    k0, length = _usable_rows(np.asarray(face_offsets), n_incident)
    acc = np.zeros((n, 3), F)
    rows = np.nonzero(length > 0)[0]
    k = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while len(rows):
            fid = face_ids[k0[rows] + k].astype(np.int64)
            ok = (fid >= 0) & (fid < len(f))
            tri = f[np.where(ok, fid, 0)] if len(f) else np.zeros((len(rows), 3), np.int64)
            ok &= ((tri >= 0) & (tri < n)).all(1)
            r, tri = rows[ok], tri[ok]
            v0, v1, v2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
            e1, e2 = v1 - v0, v2 - v0
            c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            assert c.dtype == F
            acc[r] = acc[r] + c
            k += 1
            rows = rows[length[rows] > k]
        ln = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
        good = (ln > 0) & np.isfinite(ln)
        out = np.full((n, 3), np.nan, F)
        out[good] = acc[good] / ln[good, None]
    assert out.dtype == F and ln.dtype == F
    return out


# ---------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)


def grid_patch(w, h):
    """w x h vertices in the plane z = 0 (vertex y * w + x at (x, y, 0)), two triangles per cell, normals +z"""
    y, x = np.divmod(np.arange(w * h), w)
    verts = np.stack([x, y, np.zeros_like(x)], 1).astype(F)
    cy, cx = [a.reshape(-1) for a in np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")]
    a = cy * w + cx
    faces = np.stack([np.stack([a, a + 1, a + w + 1], 1), np.stack([a, a + w + 1, a + w], 1)], 1).reshape(-1, 3)
    return verts, faces.astype(np.int32)


def open_fan(k):
    """k faces around the hub, vertex 0; the rim is vertices 1 .. k+1 on a unit circle, not closed"""
    ang = 2 * np.pi * np.arange(k + 1) / (k + 2)
    verts = np.concatenate([[[0, 0, 0.25]], np.stack([np.cos(ang), np.sin(ang), np.zeros(k + 1)], 1)]).astype(F)
    i = np.arange(k)
    return verts, np.stack([np.zeros(k, int), i + 1, i + 2], 1).astype(np.int32)


def icosphere(subdivisions=3):
    """unit sphere: 12, 42, 162, 642 ... vertices; faces counter-clockwise as seen from outside"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts).astype(F), np.array(faces, np.int32)


def noisy_icosphere(sigma=0.01, seed=0, subdivisions=3):
    verts, faces = icosphere(subdivisions)
    noise = np.random.default_rng(seed).normal(0.0, sigma, verts.shape)
    return (verts.astype(np.float64) + noise).astype(F), faces


def mesh_volume(verts, faces):
    p = verts.astype(np.float64)[faces]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def random_faces(n_verts=300, m=2000, seed=3):
    """faces over n_verts vertices with duplicates, repeated indices, out-of-range indices (negative and INT32_MAX among
    them) and edges of multiplicity up to 9"""
    rs = np.random.RandomState(seed)
    faces = rs.randint(0, n_verts, (m, 3)).astype(np.int64)
    rep = rs.rand(m) < 0.05
    faces[rep, 2] = faces[rep, 0]                                   # a repeated index
    bad = rs.rand(m) < 0.05
    faces[bad, rs.randint(0, 3, bad.sum())] = rs.choice([-1, -2147483648, 2147483647, n_verts, n_verts + 7], bad.sum())
    nine = np.array([[5, 9, k] for k in range(20, 26)] + [[k, 9, 5] for k in range(26, 29)])   # the edge {5, 9} nine times
    dup = faces[rs.randint(0, m, 40)]                               # whole faces again
    return np.concatenate([faces, nine, dup]).astype(np.int32)
