"""Numpy restatement of the rule of include/ctd_hip_mesh_clean.h (ctd_mesh_components_i32, ctd_mesh_clean_i32): which
faces are valid, a plain sequential union-find over the vertex indices, labels and sizes, which faces and vertices are
kept, and the compaction.  Written from the rule alone; it shares no code with csrc/mesh_clean.hip."""
import numpy as np


def valid_faces(faces, n_verts, verts=None, drop_degenerate=False):
    """bool [m]: indices in [0, n_verts), pairwise different and, with drop_degenerate, no two vertices at equal
    positions (x, y, z each == as f32: -0.0 equals 0, a NaN equals nothing).  Out-of-range indices are never looked up."""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = ((faces >= 0) & (faces < n_verts)).all(1)
    ok &= (faces[:, 0] != faces[:, 1]) & (faces[:, 0] != faces[:, 2]) & (faces[:, 1] != faces[:, 2])
    if drop_degenerate:
        assert verts is not None and verts.dtype == np.float32
        safe = np.where(ok[:, None], faces, 0)
        if len(verts):
            p = verts[safe]                                         # [m,3,3]
            for a, b in ((0, 1), (0, 2), (1, 2)):
                with np.errstate(invalid="ignore"):
                    ok &= ~(p[:, a] == p[:, b]).all(1)
    return ok


def components(faces, n_verts, verts=None, drop_degenerate=False):
    """-> label int32 [m] (the smallest vertex index of the face's component, -1 for an invalid face), size int32 [m] (the
    number of valid faces of the component, 0 for an invalid face), n_components"""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = valid_faces(faces, n_verts, verts, drop_degenerate)
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in faces[ok].tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)                   # the root of a set is its smallest index
    label = np.full(len(faces), -1, np.int32)
    label[ok] = [find(a) for a in faces[ok, 0].tolist()]
    size = np.zeros(len(faces), np.int32)
    roots, n = np.unique(label[ok], return_counts=True)
    size[ok] = n[np.searchsorted(roots, label[ok])]
    # the label is the smallest vertex any face of the component uses
    for r in roots.tolist():
        assert faces[label == r].min() == r
    return label, size, len(roots)


def clean(faces, n_verts, verts=None, min_faces=1, keep_largest=False, drop_degenerate=False, comps=None):
    """comps: what `components` returned for the same faces, n_verts, verts and drop_degenerate (computed here when None)
    -> dict: faces int32 [k,3] (kept, remapped), face_index int32 [k], vert_index int32 [n'], counts int64 [4] (kept
    vertices, kept faces, components, components kept), label, size"""
    assert min_faces >= 1
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    label, size, n_comp = components(faces, n_verts, verts, drop_degenerate) if comps is None else comps
    keep = (label >= 0) & (size >= min_faces)
    if keep_largest:
        if (label >= 0).any():
            big = size.max()
            best = label[(label >= 0) & (size == big)].min()        # a tie: the smallest label
            keep &= label == best
        n_kept_comp = 1 if keep.any() else 0
    else:
        n_kept_comp = len(np.unique(label[keep]))
    face_index = np.nonzero(keep)[0].astype(np.int32)
    used = np.zeros(n_verts, bool)
    used[faces[keep].reshape(-1)] = True
    vert_index = np.nonzero(used)[0].astype(np.int32)
    new = np.cumsum(used) - used                                    # the number of kept vertices with a smaller index
    out = new[faces[keep]].astype(np.int32).reshape(-1, 3)
    counts = np.array([len(vert_index), len(face_index), n_comp, n_kept_comp], np.int64)
    return dict(faces=out, face_index=face_index, vert_index=vert_index, counts=counts, label=label, size=size)
