"""Meshes and cameras for the BVH ray-caster tests and tools/time_render_bvh.py: a data-generator-like scene (the
1000-unit two-triangle board of data/create_syn_data.py:get_mesh plus four procedural objects, randomly scaled,
rotated and placed like its ShapeNet models) and small adversarial meshes."""
import numpy as np


def icosphere(subdiv):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = np.array(v, np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array(f, np.int64)
    for _ in range(subdiv):
        edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        mid = v[uniq].mean(axis=1)
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = inv.reshape(3, -1).T + len(v)
        v = np.concatenate([v, mid])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[:, 0], m[:, 2]], 1), np.stack([b, m[:, 1], m[:, 0]], 1),
                            np.stack([c, m[:, 2], m[:, 1]], 1), m])
    return v, f


def torus(nu, nv, R=0.7, r=0.3):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v, f


def blob(subdiv, rs):
    v, f = icosphere(subdiv)
    k = rs.normal(size=(6, 3))
    rad = 1 + 0.15 * np.sin(v @ k.T * 3).sum(1) / 3 + 0.02 * rs.uniform(-1, 1, size=len(v))
    return v * rad[:, None], f


def rand_rot(rs):
    q = rs.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def objects_for(n_faces_target, rs):
    """four procedural objects of about n_faces_target / 4 faces each (icosphere, torus, two blobs)"""
    per = max(80, n_faces_target // 4)
    sub = max(1, int(round(np.log(per / 20) / np.log(4))))
    nt = max(4, int((per / 2) ** 0.5))
    return [icosphere(sub), torus(nt, nt), blob(sub, rs), blob(max(1, sub - 1), rs)]


def get_mesh_like(n_faces_target, seed):
    """data/create_syn_data.py:get_mesh with procedural objects: the board (two triangles, x/y scaled by 500, at
    z in [2, 7]) and four objects scaled by U(0.25, 1), randomly rotated, lifted to z >= U(0.5, 3), shifted in x/y."""
    rs = np.random.RandomState(seed)
    verts, faces, n = [], [], 0
    z = rs.uniform(2, 7)
    board = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, -1, z], [1, 1, z], [-1, 1, z]], np.float64)
    board[:, :2] *= 5e2
    verts.append(board)
    faces.append(np.array([[0, 1, 2], [3, 4, 5]]))
    n = 6
    for v, f in objects_for(n_faces_target, rs):
        v = v * rs.uniform(0.25, 1) @ rand_rot(rs).T
        v[:, 2] += -v[:, 2].min() + rs.uniform(0.5, 3)
        v[:, :2] += rs.uniform(-1, 1, size=(1, 2))
        verts.append(v)
        faces.append(f + n)
        n += len(v)
    verts = np.concatenate(verts).astype(np.float32)
    faces = np.concatenate(faces).astype(np.int32)
    colors = rs.uniform(0, 1, size=verts.shape).astype(np.float32)
    return verts, colors, faces


def camera(H, W, t=(0, 0, 0), R=None, f=None):
    f = 0.9 * W if f is None else f
    K = np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], np.float32)
    return K, np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32), np.asarray(t, np.float32), W, H


def pattern(H, W, seed=0):
    return np.random.RandomState(seed).uniform(0, 1, size=(H, W, 3)).astype(np.float32)
