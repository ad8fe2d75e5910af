"""Mesh connectivity by vertex, Taubin smoothing and vertex normals (include/ctd_hip_mesh_smooth.h, csrc/mesh_smooth.hip).

    m = meshops.clean_tsdf_mesh(mesh.tsdf_mesh(tsdf, weight, origin, voxel, return_normals=True), min_faces=32)
    m = meshsmooth.smooth_tsdf_mesh(m)                         # 10 x (lambda 0.5 | mu -0.53), the rim held, normals recomputed
    verts, faces, normals = m.track(0)                        # ... renderer.MeshBVH, meshcolor.color_tsdf_mesh, mesh.save_ply
    adj = meshsmooth.MeshAdjacency(faces, verts.shape[0])     # one-rings, incident faces, flags, edge counts
    adj.closed, adj.euler, adj.n_boundary_edges               # what the mesh's topology is
    smooth = meshsmooth.mesh_smooth(verts, faces, adjacency=adj)
    normals = meshsmooth.vertex_normals(smooth, faces, adjacency=adj)

The adjacency is integer work and the sums run in one fixed order: every output is the same on every run.  No fallback:
a missing kernel is an error.  Nothing is differentiable.
"""
import torch

from . import _lib
from ._meshargs import _cat_or_empty, _flag, _nx3, _ptr_or, _tsdf_mesh_arg
from .mesh import TsdfMesh
from .torchext._common import _call, _integer, _number, _ptr, _same_device, _stream, _workspace

REFERENCED, BOUNDARY, NONMANIFOLD = 1, 2, 4                     # the bits of MeshAdjacency.vflags
MAX_INCIDENT = 1024                                             # CTD_MESH_ADJ_MAX_INCIDENT

_RULE = """
    The rule (include/ctd_hip_mesh_smooth.h).  A face is valid when its three indices lie in [0, n_verts) and are pairwise
    different.  The incident faces of a vertex are the valid faces that use it, in ascending face index; its one-ring is
    the set of the other corners of these faces, ascending, each once.  The multiplicity of an edge {i,j} is the number of
    valid faces that use it: 1 is a boundary edge, more than 2 a non-manifold edge.  A smoothing pass with factor f leaves
    a vertex without a ring (and, with fix_boundary, one at the end of a boundary edge) as it is, bit for bit, and moves
    every other one to x + f * (m - x), m = the sum of the ring in ascending order (f32, from 0) / the ring's size; one
    iteration is a pass with lam, then a pass with mu over the result (none with mu == 0).  A vertex normal is the sum of
    (v1 - v0) x (v2 - v0) over the incident faces in ascending order, divided by its length: three NaNs where that length
    is 0 or not finite, so for every unreferenced vertex.  The same bits on every run."""


def _sizes_ok(n_verts, n_faces, who):
    if 6 * n_faces >= 2 ** 31:
        raise RuntimeError("%s: 6 * the number of faces must stay below 2^31" % who)
    return _lib.lib().ctd_mesh_adjacency_workspace_bytes(n_verts, n_faces)


class MeshAdjacency:
    """The connectivity by vertex of faces int32 [m,3] over n_verts vertices.  One call, one synchronisation (to read the
    counts); the tensors own exactly their size.

    offsets int32 [n_verts+1], neighbors int32 [nnz]: the one-ring of i is neighbors[offsets[i]:offsets[i+1]], ascending;
    face_offsets int32 [n_verts+1], face_ids int32 [3 * n_valid_faces]: its incident faces, likewise; vflags uint8
    [n_verts]: REFERENCED | BOUNDARY | NONMANIFOLD.  n_edges, n_boundary_edges, n_nonmanifold_edges, n_valid_faces,
    max_incident, n_referenced are ints; euler = n_referenced - n_edges + n_valid_faces; closed = no boundary and no
    non-manifold edge.  Raises when a vertex has more than MAX_INCIDENT incident faces."""

    def __init__(self, faces, n_verts):
        who = "MeshAdjacency"
        faces = _nx3(faces, who, "faces", torch.int32, letter="m")
        n = _integer(n_verts, "n_verts", who)
        dev, m = faces.device, faces.shape[0]
        L = _lib.lib()
        ws = _workspace(_sizes_ok(n, m, who), dev)
        offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        neighbors = torch.empty((6 * m,), dtype=torch.int32, device=dev)
        face_offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        face_ids = torch.empty((3 * m,), dtype=torch.int32, device=dev)
        vflags = torch.empty((n,), dtype=torch.uint8, device=dev)
        counts = torch.empty((6,), dtype=torch.int64, device=dev)
        _call(L.ctd_mesh_adjacency_i32, who, _ptr_or(faces, ws), n, m, _ptr(offsets), _ptr(neighbors), 6 * m, _ptr(face_offsets),
              _ptr(face_ids), 3 * m, _ptr_or(vflags, ws), _ptr(counts), _ptr(ws), ws.numel(), dev.index, _stream(dev))
        n_ref = (vflags & REFERENCED).ne(0).sum()
        nnz, n_edges, n_boundary, n_nonmanifold, max_incident, n_valid, n_ref = torch.cat([counts, n_ref.reshape(1)]).cpu().tolist()
        if max_incident > MAX_INCIDENT:
            raise RuntimeError("%s: a vertex has %d incident faces, more than MAX_INCIDENT = %d" % (who, max_incident, MAX_INCIDENT))
        self.faces, self.n_verts = faces, n
        self.offsets, self.face_offsets, self.vflags = offsets, face_offsets, vflags
        self.neighbors, self.face_ids = neighbors[:nnz].clone(), face_ids[:3 * n_valid].clone()
        self.n_edges, self.n_boundary_edges, self.n_nonmanifold_edges = n_edges, n_boundary, n_nonmanifold
        self.n_valid_faces, self.max_incident, self.n_referenced = n_valid, max_incident, n_ref
        self.euler = n_ref - n_edges + n_valid
        self.closed = n_boundary == 0 and n_nonmanifold == 0

    def matches(self, faces, n_verts):
        return faces.data_ptr() == self.faces.data_ptr() and tuple(faces.shape) == tuple(self.faces.shape) and \
            n_verts == self.n_verts


MeshAdjacency.__doc__ += _RULE


def _adjacency(adjacency, faces, n_verts, who):
    if adjacency is None:
        return MeshAdjacency(faces, n_verts)
    if not isinstance(adjacency, MeshAdjacency):
        raise RuntimeError("%s: adjacency must be a MeshAdjacency" % who)
    if not adjacency.matches(faces, n_verts):
        raise RuntimeError("%s: adjacency was built for other faces or another number of vertices" % who)
    return adjacency


def _smooth_args(iters, lam, mu, fix_boundary, who):
    iters = _integer(iters, "iters", who, 0, 1024, "an integer in [0, 1024]")
    lam = _number(lam, "lam", who, lo_open=True)
    if lam > 1.0:
        raise RuntimeError("%s: lam must be a finite number in (0, 1]" % who)
    mu = _number(mu, "mu", who, lo=-2.0)
    if mu > 0.0:
        raise RuntimeError("%s: mu must be a finite number in [-2, 0]" % who)
    return iters, lam, mu, _flag(fix_boundary, "fix_boundary", who)


def mesh_smooth(verts, faces, iters=10, lam=0.5, mu=-0.53, fix_boundary=True, adjacency=None):
    """Taubin lambda|mu smoothing of verts f32 [n,3] over the one-rings of faces int32 [m,3] -> verts f32 [n,3].  With
    fix_boundary the vertices at the ends of boundary edges stay where they are.  adjacency: a `MeshAdjacency` of these
    faces (built here when None: one synchronisation; none otherwise).  Not differentiable."""
    who = "mesh_smooth"
    verts, faces = _nx3(verts, who, "verts", torch.float32), _nx3(faces, who, "faces", torch.int32, letter="m")
    dev = _same_device(verts, faces)
    iters, lam, mu, fix = _smooth_args(iters, lam, mu, fix_boundary, who)
    n = verts.shape[0]
    adj = _adjacency(adjacency, faces, n, who)
    L = _lib.lib()
    ws = _workspace(L.ctd_mesh_smooth_workspace_bytes(n), dev)
    out = torch.empty_like(verts)
    _call(L.ctd_mesh_smooth_f32, who, _ptr_or(verts, ws), n, _ptr(adj.offsets), _ptr_or(adj.neighbors, ws), adj.neighbors.shape[0],
          _ptr_or(adj.vflags, ws), iters, lam, mu, fix, _ptr_or(out, ws), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    return out


mesh_smooth.__doc__ += _RULE


def vertex_normals(verts, faces, adjacency=None):
    """Area-weighted normals of verts f32 [n,3] from faces int32 [m,3] -> f32 [n,3]; three NaNs for a vertex that no valid
    face uses or whose faces have no area.  adjacency: a `MeshAdjacency` of these faces (built here when None: one
    synchronisation; none otherwise).  Not differentiable."""
    who = "vertex_normals"
    verts, faces = _nx3(verts, who, "verts", torch.float32), _nx3(faces, who, "faces", torch.int32, letter="m")
    dev = _same_device(verts, faces)
    n = verts.shape[0]
    adj = _adjacency(adjacency, faces, n, who)
    out = torch.empty_like(verts)
    spare = adj.face_offsets
    _call(_lib.lib().ctd_mesh_vertex_normals_f32, who, _ptr_or(verts, spare), n, _ptr_or(faces, spare), faces.shape[0],
          _ptr(adj.face_offsets), _ptr_or(adj.face_ids, spare), adj.face_ids.shape[0], _ptr_or(out, spare), dev.index,
          _stream(dev))
    return out


vertex_normals.__doc__ += _RULE


def smooth_tsdf_mesh(m, iters=10, lam=0.5, mu=-0.53, fix_boundary=True, recompute_normals=True):
    """`mesh_smooth` on every track of a `mesh.TsdfMesh` -> a new `TsdfMesh`: verts smoothed, src, faces and the counts
    unchanged; normals are the `vertex_normals` of the smoothed mesh when m.normals is not None and recompute_normals is
    set (else m.normals as they are).  Track by track: one adjacency, so one synchronisation, per track."""
    who = "smooth_tsdf_mesh"
    _tsdf_mesh_arg(m, who)
    _smooth_args(iters, lam, mu, fix_boundary, who)
    renew = _flag(recompute_normals, "recompute_normals", who) and m.normals is not None
    verts_out, normals_out, counts = [], [], []
    for _, verts, faces, _, _ in m.tracks():
        counts.append((verts.shape[0], faces.shape[0]))
        adj = MeshAdjacency(faces, verts.shape[0])
        verts_out.append(mesh_smooth(verts, faces, iters, lam, mu, fix_boundary, adjacency=adj))
        if renew:
            normals_out.append(vertex_normals(verts_out[-1], faces, adjacency=adj))
    normals = _cat_or_empty(normals_out, m.normals) if renew else m.normals
    return TsdfMesh(_cat_or_empty(verts_out, m.verts), m.src, normals, m.faces, m.n_verts_per_track, m.n_faces_per_track,
                    counts)
