"""Mesh clean-up (include/ctd_hip_mesh_clean.h, csrc/mesh_clean.hip): the connected components of an indexed triangle
mesh, and the removal of small components, of faces with coincident vertices and of unreferenced vertices.

    m = mesh.tsdf_mesh(tsdf, weight, origin, voxel, return_normals=True)
    m = meshops.clean_tsdf_mesh(m, min_faces=32)              # floaters and occlusion-edge fragments go, indices compacted
    verts, faces, normals = m.track(0)                        # ... renderer.MeshBVH(verts, faces), mesh.save_ply
    label, size, n = meshops.mesh_components(faces, verts.shape[0])
    c = meshops.mesh_clean(verts, faces, keep_largest=True)   # any verts f32 [n,3], faces int32 [m,3] on the device

All of it is integer work: the outputs are exact and the same on every run.  No fallback: a missing kernel is an error.
"""
import torch

from . import _lib
from ._meshargs import _cat_or_empty, _flag, _nx3, _ptr_or, _tsdf_mesh_arg
from .mesh import TsdfMesh
from .torchext._common import _call, _integer, _ptr, _same_device, _stream, _workspace

_RULE = """
    The rule (include/ctd_hip_mesh_clean.h).  A face is valid when its three indices lie in [0, n_verts), are pairwise
    different and, with drop_degenerate, no two of its vertices have equal positions (x, y and z each compare == as f32:
    -0.0 equals 0, a NaN coordinate equals nothing).  Two valid faces belong to one component when a chain of valid faces
    links them, each sharing a vertex index with the next (by index, not by position).  A component's label is the
    smallest vertex index any of its faces uses, its size the number of its valid faces; an invalid face has label -1 and
    size 0.  A face is kept when it is valid, its size is at least min_faces and, with keep_largest, its component is
    the one of largest size (on a tie the one with the smallest label; min_faces still applies to it).  A vertex is kept
    when a kept face uses it.  Kept vertices and kept faces keep their order and the faces their winding, with the indices
    remapped; coincident vertices are not welded, so dropping zero-area faces can open a combinatorial hole of zero size
    in an otherwise closed mesh.  The same bits on every run."""


def _sizes_ok(n_verts, n_faces, who):
    if 3 * n_faces >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of faces must stay below 2^31" % who)
    return _lib.lib().ctd_mesh_clean_workspace_bytes(n_verts, n_faces)


def mesh_components(faces, n_verts, verts=None, drop_degenerate=False):
    """The connected components of faces int32 [m,3] over n_verts vertices -> (label int32 [m], size int32 [m],
    n_components int).  verts f32 [n_verts,3] is needed with drop_degenerate only.  One call, one synchronisation (to
    read n_components)."""
    who = "mesh_components"
    faces = _nx3(faces, who, "faces", torch.int32, letter="m")
    n_verts = _integer(n_verts, "n_verts", who)
    drop = _flag(drop_degenerate, "drop_degenerate", who)
    if drop and verts is None:
        raise RuntimeError("%s: drop_degenerate needs verts" % who)
    if verts is not None:
        _nx3(verts, who, "verts", torch.float32, n_verts)
        _same_device(faces, verts)
    dev, m = faces.device, faces.shape[0]
    L = _lib.lib()
    ws = _workspace(_sizes_ok(n_verts, m, who), dev)
    label = torch.empty((m,), dtype=torch.int32, device=dev)
    size = torch.empty((m,), dtype=torch.int32, device=dev)
    n_comp = torch.empty((1,), dtype=torch.int64, device=dev)
    _call(L.ctd_mesh_components_i32, who, _ptr_or(faces, ws), _ptr_or(verts, ws) if drop else None, n_verts, m, drop,
          _ptr_or(label, ws), _ptr_or(size, ws), _ptr(n_comp), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    return label, size, int(n_comp.item())


mesh_components.__doc__ += _RULE


class CleanMesh:
    """What `mesh_clean` returns: verts f32 [n',3], faces int32 [k,3] (indices into verts), normals f32 [n',3] or None,
    vert_index int32 [n'] and face_index int32 [k] (the old index of each kept vertex and face), n_components and
    n_components_kept.  verts and normals are the old rows at vert_index, bit for bit."""

    def __init__(self, verts, faces, normals, vert_index, face_index, n_components, n_components_kept):
        self.verts, self.faces, self.normals = verts, faces, normals
        self.vert_index, self.face_index = vert_index, face_index
        self.n_components, self.n_components_kept = n_components, n_components_kept


def mesh_clean(verts, faces, min_faces=1, keep_largest=False, drop_degenerate=True, normals=None):
    """Removes the components of fewer than min_faces faces (with keep_largest: every component but the largest), with
    drop_degenerate the faces that have two vertices at one position, and every vertex that no kept face uses ->
    `CleanMesh`.  One call, one synchronisation to read the counts; the returned tensors own exactly their size.  Not
    differentiable."""
    who = "mesh_clean"
    verts, faces = _nx3(verts, who, "verts", torch.float32), _nx3(faces, who, "faces", torch.int32, letter="m")
    n, m = verts.shape[0], faces.shape[0]
    if normals is not None:
        _nx3(normals, who, "normals", torch.float32, n)
    dev = _same_device(verts, faces, *(() if normals is None else (normals,)))
    min_faces = _integer(min_faces, "min_faces", who, 1)
    largest, drop = _flag(keep_largest, "keep_largest", who), _flag(drop_degenerate, "drop_degenerate", who)
    L = _lib.lib()
    ws = _workspace(_sizes_ok(n, m, who), dev)
    faces_out = torch.empty((m, 3), dtype=torch.int32, device=dev)
    face_index = torch.empty((m,), dtype=torch.int32, device=dev)
    vert_index = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((4,), dtype=torch.int64, device=dev)
    _call(L.ctd_mesh_clean_i32, who, _ptr_or(faces, ws), _ptr_or(verts, ws), n, m, drop, min_faces, largest, _ptr(faces_out),
          _ptr(face_index), m, _ptr(vert_index), n, _ptr(counts), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    n_kept, m_kept, n_comp, n_comp_kept = counts.cpu().tolist()
    vert_index = vert_index[:n_kept].clone()
    rows = vert_index.long()
    return CleanMesh(verts.index_select(0, rows), faces_out[:m_kept].clone(),
                     None if normals is None else normals.index_select(0, rows), vert_index, face_index[:m_kept].clone(),
                     n_comp, n_comp_kept)


mesh_clean.__doc__ += _RULE


def clean_tsdf_mesh(m, min_faces=1, keep_largest=False, drop_degenerate=True):
    """`mesh_clean` on every track of a `mesh.TsdfMesh` -> a new `TsdfMesh`: verts, src and normals gathered at the kept
    vertices, faces remapped and track-local, the counts rebuilt, so that `.track(b)`, `renderer.MeshBVH` and
    `mesh.save_ply` work on the result.  Track by track: one call and one synchronisation per track."""
    who = "clean_tsdf_mesh"
    _tsdf_mesh_arg(m, who)
    min_faces = _integer(min_faces, "min_faces", who, 1)
    _flag(keep_largest, "keep_largest", who)
    _flag(drop_degenerate, "drop_degenerate", who)
    dev = m.verts.device
    parts, counts = [], []
    for _, verts, faces, normals, v0 in m.tracks():
        c = mesh_clean(verts, faces, min_faces, keep_largest, drop_degenerate, normals)
        src = m.src[v0:v0 + verts.shape[0]].index_select(0, c.vert_index.long())
        parts.append((c.verts, src, c.normals, c.faces))
        counts.append((c.verts.shape[0], c.faces.shape[0]))

    def cat(k, like):
        return _cat_or_empty([p[k] for p in parts], like)

    n_verts = torch.tensor([c[0] for c in counts], dtype=torch.int64, device=dev)
    n_faces = torch.tensor([c[1] for c in counts], dtype=torch.int64, device=dev)
    return TsdfMesh(cat(0, m.verts), cat(1, m.src), None if m.normals is None else cat(2, m.normals), cat(3, m.faces),
                    n_verts, n_faces, counts)
