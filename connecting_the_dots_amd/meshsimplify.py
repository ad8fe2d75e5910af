"""Mesh simplification: uniform-grid vertex clustering with quadric placement (include/ctd_hip_mesh_simplify.h,
csrc/mesh_simplify.hip).

    m = meshsmooth.smooth_tsdf_mesh(meshops.clean_tsdf_mesh(mesh.tsdf_mesh(tsdf, weight, origin, voxel), min_faces=32))
    light = meshsimplify.simplify_tsdf_mesh(m, cell=2 * voxel)   # one vertex per occupied cell of 2 voxels
    verts, faces, normals = light.track(0)                    # ... renderer.MeshBVH, meshcolor.color_tsdf_mesh, mesh.save_ply
    s = meshsimplify.mesh_simplify(verts, faces, cell=4 * voxel, normals=True)
    s.verts, s.faces, s.normals, s.leader, s.vert_cluster, s.face_index, s.n_collapsed_faces, s.n_mean_fallbacks

Integer atomics only and sums in one fixed order: every output is the same on every run.  No fallback: a missing kernel is
an error.  Nothing is differentiable.
"""
import torch

from . import _lib
from ._meshargs import _cat_or_empty, _flag, _nx3, _ptr_or, _tsdf_mesh_arg
from .mesh import TsdfMesh
from .meshsmooth import _adjacency, vertex_normals
from .torchext._common import _call, _number, _ptr, _same_device, _stream, _workspace

MAX_CELLS_PER_AXIS = 1 << 20                                    # CTD_MESH_SIMPLIFY_MAX_CELLS_PER_AXIS

_RULE = """
    The rule (include/ctd_hip_mesh_simplify.h).  A face is valid when its three indices lie in [0, n_verts) and are
    pairwise different.  The cell of a vertex is floorf((x - origin) / cell) per axis, in f32; a vertex is clusterable when
    a valid face uses it and its three cell indices are finite and in [0, 2^20); a face that uses an unclusterable vertex
    is dropped and counted.  A cluster is the set of clusterable vertices of one cell, its leader the smallest vertex index.
    Every cluster's vertex is the minimum of the cluster's summed plane quadrics, weighted by area squared and summed in
    f64 in ascending face and vertex index, regularised towards the cluster's mean by reg * trace.  The vertex falls back
    to the mean (and is counted) when the solve is not well posed or leaves [lo - cell/2, lo + 3 cell/2] on an axis.  A face
    whose corners fall into fewer than three clusters is collapsed; with drop_duplicates, of the faces with the same set
    of three clusters the one with the smallest face index is kept.  Kept faces keep their order and their winding; a
    cluster is emitted when a kept face uses it, in ascending order of the leaders.  The same bits on every run."""


class SimplifiedMesh:
    """What `mesh_simplify` returns; the tensors own exactly their size.

    verts f32 [n',3]: the placed vertices; faces int32 [k,3]: the kept faces over them; normals f32 [n',3]: the
    `meshsmooth.vertex_normals` of the result, or None; leader int32 [n']: the smallest input vertex of each emitted
    cluster; vert_cluster int32 [n]: the output vertex of each input vertex, or -1; face_index int32 [k]: the input face of
    each kept face.  n_clusters (before the drop), n_dropped_faces (invalid or unclusterable), n_collapsed_faces,
    n_duplicate_faces, n_mean_fallbacks (among the emitted clusters) and max_cluster are ints; origin (three floats) and
    cell are the grid that was used."""

    def __init__(self, verts, faces, normals, leader, vert_cluster, face_index, counts, origin, cell):
        self.verts, self.faces, self.normals = verts, faces, normals
        self.leader, self.vert_cluster, self.face_index = leader, vert_cluster, face_index
        (self.n_clusters, self.n_dropped_faces, self.n_collapsed_faces, self.n_duplicate_faces, self.n_mean_fallbacks,
         self.max_cluster) = counts
        self.origin, self.cell = origin, cell


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _simplify_args(cell, origin, reg, drop_duplicates, who):
    cell = _f32(_number(cell, "cell", who, lo_open=True))
    if not 0.0 < cell < float("inf"):
        raise RuntimeError("%s: cell must be a finite number > 0 in f32" % who)
    if origin is not None:
        if isinstance(origin, torch.Tensor):
            origin = origin.reshape(-1).tolist()
        if not isinstance(origin, (tuple, list)) or len(origin) != 3:
            raise RuntimeError("%s: origin must be None or three finite numbers" % who)
        origin = tuple(_f32(_number(o, "origin", who, lo=None)) for o in origin)
        if not all(abs(o) < float("inf") for o in origin):
            raise RuntimeError("%s: origin must be None or three finite numbers" % who)
    return cell, origin, _number(reg, "reg", who), _flag(drop_duplicates, "drop_duplicates", who)


def _grid_origin(verts, cell, who):
    """the per-axis minimum of the finite coordinates (0 on an axis without one); one synchronisation"""
    if verts.shape[0] == 0:
        return (0.0, 0.0, 0.0)
    finite = torch.isfinite(verts)
    lo = torch.where(finite, verts, torch.full_like(verts, float("inf"))).amin(0)
    hi = torch.where(finite, verts, torch.full_like(verts, float("-inf"))).amax(0)
    lo = torch.where(torch.isfinite(lo), lo, torch.zeros_like(lo))
    hi = torch.where(torch.isfinite(hi), hi, lo)
    cells = torch.floor((hi - lo) / torch.full_like(lo, cell))   # (a tensor: the IEEE division of the rule, no reciprocal)
    lo, cells = lo.cpu().tolist(), cells.cpu().tolist()
    if not all(c < MAX_CELLS_PER_AXIS for c in cells):
        raise RuntimeError("%s: the mesh spans %d cells or more on an axis; cell is too small for its extent"
                           % (who, MAX_CELLS_PER_AXIS))
    return tuple(lo)


def mesh_simplify(verts, faces, cell, origin=None, reg=1e-3, drop_duplicates=True, adjacency=None, normals=False):
    """Vertex clustering of verts f32 [n,3], faces int32 [m,3] on a grid of `cell` from `origin` -> `SimplifiedMesh`.
    origin: three numbers, or None for the per-axis minimum of the finite coordinates (one more synchronisation; raises
    when the extent then needs 2^20 cells or more on an axis).  reg >= 0 pulls every cluster's vertex towards the cluster's
    mean (0: the mean itself; the default 1e-3 keeps flat clusters well posed).  adjacency: a `meshsmooth.MeshAdjacency` of
    these faces (built here when None: one synchronisation).  normals: also the `meshsmooth.vertex_normals` of the result.
    One call and one synchronisation to read the counts.  Not differentiable."""
    who = "mesh_simplify"
    verts, faces = _nx3(verts, who, "verts", torch.float32), _nx3(faces, who, "faces", torch.int32, letter="m")
    dev = _same_device(verts, faces)
    cell, origin, reg, dd = _simplify_args(cell, origin, reg, drop_duplicates, who)
    want_normals = _flag(normals, "normals", who)
    n, m = verts.shape[0], faces.shape[0]
    if 6 * m >= 2 ** 31:
        raise RuntimeError("%s: 6 * the number of faces must stay below 2^31" % who)
    adj = _adjacency(adjacency, faces, n, who)
    if origin is None:
        origin = _grid_origin(verts, cell, who)
    L = _lib.lib()
    ws = _workspace(L.ctd_mesh_simplify_workspace_bytes(n, m), dev)
    verts_out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    leader = torch.empty((n,), dtype=torch.int32, device=dev)
    vert_cluster = torch.empty((n,), dtype=torch.int32, device=dev)
    faces_out = torch.empty((m, 3), dtype=torch.int32, device=dev)
    face_index = torch.empty((m,), dtype=torch.int32, device=dev)
    counts = torch.empty((8,), dtype=torch.int64, device=dev)
    _call(L.ctd_mesh_simplify_f32, who, _ptr_or(verts, ws), n, _ptr_or(faces, ws), m, _ptr(adj.face_offsets),
          _ptr_or(adj.face_ids, ws), adj.face_ids.shape[0], origin[0], origin[1], origin[2], cell, reg, dd, _ptr_or(verts_out, ws),
          _ptr_or(leader, ws), n, _ptr_or(vert_cluster, ws), _ptr_or(faces_out, ws), _ptr_or(face_index, ws), m, _ptr(counts),
          _ptr(ws), ws.numel(), dev.index, _stream(dev))
    c = counts.cpu().tolist()
    nv, k = c[0], c[1]
    verts_out, faces_out = verts_out[:nv].clone(), faces_out[:k].clone()
    return SimplifiedMesh(verts_out, faces_out, vertex_normals(verts_out, faces_out) if want_normals else None,
                          leader[:nv].clone(), vert_cluster, face_index[:k].clone(), c[2:], origin, cell)


mesh_simplify.__doc__ += _RULE


def simplify_tsdf_mesh(m, cell, origin=None, reg=1e-3, drop_duplicates=True):
    """`mesh_simplify` on every track of a `mesh.TsdfMesh` -> a new `TsdfMesh`: the placed vertices, src gathered at the
    clusters' leaders, the kept faces track-local, the counts rebuilt, so that `.track(b)`, `renderer.MeshBVH`,
    `mesh.save_ply`, `meshops.clean_tsdf_mesh` and `meshcolor.color_tsdf_mesh` work on the result.  Normals are the
    `meshsmooth.vertex_normals` of the result when m.normals is not None.  origin=None: every track its own.  Track by
    track."""
    who = "simplify_tsdf_mesh"
    _tsdf_mesh_arg(m, who)
    _simplify_args(cell, origin, reg, drop_duplicates, who)
    dev = m.verts.device
    parts, counts = [], []
    for _, verts, faces, _, v0 in m.tracks():
        s = mesh_simplify(verts, faces, cell, origin, reg, drop_duplicates, normals=m.normals is not None)
        src = m.src[v0:v0 + verts.shape[0]].index_select(0, s.leader.long())
        parts.append((s.verts, src, s.normals, s.faces))
        counts.append((s.verts.shape[0], s.faces.shape[0]))

    def cat(k, like):
        return _cat_or_empty([p[k] for p in parts], like)

    n_verts = torch.tensor([c[0] for c in counts], dtype=torch.int64, device=dev)
    n_faces = torch.tensor([c[1] for c in counts], dtype=torch.int64, device=dev)
    return TsdfMesh(cat(0, m.verts), cat(1, m.src), None if m.normals is None else cat(2, m.normals), cat(3, m.faces),
                    n_verts, n_faces, counts)


simplify_tsdf_mesh.__doc__ += _RULE
