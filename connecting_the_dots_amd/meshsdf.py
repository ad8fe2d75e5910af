"""Which side of a mesh a point is on, and how far (include/ctd_hip_mesh_sdf.h, csrc/mesh_sdf.hip): the signed distance to
the nearest face within an optional cutoff, a mesh turned back into a TSDF volume, and the signed error of a
reconstruction against the truth.

    sdist, face = meshsdf.point_mesh_signed_distance(points, verts, faces, bvh='auto', max_dist=0.05)
    tsdf, weight = meshsdf.mesh_to_tsdf(verts, faces, origin, voxel, (nx, ny, nz), trunc=4 * voxel)
    pts = te.tsdf_surface_points(tsdf, weight, origin.view(1, 3), voxel)      # ... mesh.tsdf_mesh, te.tsdf_raycast
    err = meshsdf.signed_error(verts, faces, truth_verts, truth_faces)        # mean > 0: inflated towards free space

Positive is the side the faces' normals (v1 - v0) x (v2 - v0) point to: free space for a mesh from `mesh.tsdf_mesh`, the
side on which a TSDF is positive.  The distances are `mesheval.point_mesh_distance`'s bit for bit; the tree only makes
them cheaper.  No fallback to torch: a missing kernel is an error.  Nothing is differentiable.
"""
import torch

from . import _lib
from ._meshargs import _call_tree_then_brute, _flag, _nx3, _ptr_or, _resolve_bvh
from .meshsmooth import _adjacency
from .torchext._common import _check, _integer, _number, _ptr, _same_device, _stream

# 'auto' builds a tree from this many faces on: mesheval's value, whose measurement (profiles/point_mesh.txt) is of the
# same nearest-face kernels; the sign pass costs the same with a tree and without (profiles/mesh_sdf.txt)
AUTO_BVH_MIN_FACES = 4096

_RULE = """
    The rule (include/ctd_hip_mesh_sdf.h).  The nearest face is `mesheval.point_mesh_distance`'s, among the faces whose
    squared distance d2 compares <= max_dist * max_dist (one f32 product); without a cutoff the same bits.  The feature is
    the branch the distance function took for that face: 0, 1, 2 a vertex, 3, 4, 5 the edge ab, ac, bc, 6 the interior.
    The sign is that of (p - closest) . N in f64, N the face's normal for the interior, the sum of the unit normals of the
    valid faces on the edge for an edge, and the angle-weighted sum of the unit normals of the valid faces at the vertex
    for a vertex (Baerentzen and Aanaes), each summed in ascending face order: +1, -1, or 0 where the product is 0 or NaN
    (the point lies on the mesh, or no face contributes).  Exact for closed, consistently oriented manifold meshes; on an
    open mesh it is the side of the nearest piece of surface.  Where no face qualifies: face -1, distance +inf, closest
    NaN, feature -1, sign 0."""


def _max_d2(max_dist, who):
    if max_dist is None:
        return float("inf")
    t = torch.tensor(_number(max_dist, "max_dist", who), dtype=torch.float32)
    return float(t * t)


def _signed_query(points, verts, faces, tree, adj, max_d2, want_closest, who):
    """one C call on checked arguments -> (d2, face, closest or None, feature, sign)"""
    dev, n = points.device, points.shape[0]
    d2 = torch.empty((n,), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    closest = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_closest else None
    feature = torch.empty((n,), dtype=torch.int8, device=dev)
    sign = torch.empty((n,), dtype=torch.int8, device=dev)
    if n > 0:
        spare = adj.face_offsets
        head = (_ptr(points), n, _ptr(verts) or None, verts.shape[0], _ptr(faces) or None, faces.shape[0],
                _ptr(adj.face_offsets), _ptr_or(adj.face_ids, spare), adj.face_ids.shape[0])
        tail = (max_d2, _ptr(d2), _ptr(face), _ptr(closest), _ptr(feature), _ptr(sign), dev.index, _stream(dev))
        _call_tree_then_brute(_lib.lib().ctd_point_mesh_signed_f32, head, tree, tail, who)
    return d2, face, closest, feature, sign


def _signed(d2, sign):
    dist = torch.sqrt(d2)
    return torch.where(sign < 0, -dist, dist)


def point_mesh_signed_distance(points, verts, faces, bvh=None, adjacency=None, max_dist=None, return_closest=False,
                               return_feature=False):
    """For every row of points f32 [n,3] the signed distance to the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors)
    -> (sdist f32 [n], face int32 [n]), then closest f32 [n,3] with return_closest, then feature int8 [n] and sign int8
    [n] with return_feature.  sdist is -sqrt(d2) where sign < 0 and +sqrt(d2) elsewhere (torch.sqrt of the kernel's d2),
    +inf where no face qualifies.  max_dist: None, or a finite number >= 0: faces farther than that do not qualify, which
    lets the tree stop early.  bvh: None (brute force over all faces), a `renderer.MeshBVH` built from these very tensors,
    or 'auto' (builds one when the mesh has at least AUTO_BVH_MIN_FACES faces); a tree that is not usable falls back to
    brute force, and all three give the same bits.  adjacency: a `meshsmooth.MeshAdjacency` of these faces (built here
    when None: one synchronisation; none otherwise).  Not differentiable."""
    who = "point_mesh_signed_distance"
    _nx3(points, who, "points", torch.float32)
    _nx3(verts, who, "verts", torch.float32)
    _nx3(faces, who, "faces", torch.int32)
    _same_device(points, verts, faces)
    want_closest = _flag(return_closest, "return_closest", who)
    want_feature = _flag(return_feature, "return_feature", who)
    max_d2 = _max_d2(max_dist, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    adj = _adjacency(adjacency, faces, verts.shape[0], who)
    if 3 * points.shape[0] >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of points must stay below 2^31" % who)
    d2, face, closest, feature, sign = _signed_query(points, verts, faces, tree, adj, max_d2, want_closest, who)
    out = (_signed(d2, sign), face)
    if want_closest:
        out += (closest,)
    if want_feature:
        out += (feature, sign)
    return out


point_mesh_signed_distance.__doc__ += _RULE


def mesh_to_tsdf(verts, faces, origin, voxel, dims, trunc, bvh="auto", adjacency=None, chunk=1 << 22):
    """The mesh verts f32 [m,3], faces int32 [k,3] as a truncated signed distance volume -> (tsdf, weight), both f32
    [1,nz,ny,nx] (x fastest) for dims = (nx, ny, nz), usable with origin.view(1, 3) in `torchext.tsdf_surface_points`,
    `mesh.tsdf_mesh` and `torchext.tsdf_raycast`.  origin f32 [3] (a CUDA tensor) is the centre of voxel (0,0,0) and voxel
    the edge: a voxel's centre is origin[c] + voxel * float(index_c) in f32, one multiplication and one addition, the
    formula of include/ctd_hip_tsdf.h.  The centres are queried with max_dist=trunc, in slabs of whole z-slices of at
    most `chunk` points (at least one slice); where a face qualifies tsdf = minimum(1, s * sqrt(d2) / trunc) with s = -1
    for sign < 0 and +1 otherwise, and weight = 1; where none does tsdf = 0 and weight = 0, as in a voxel that no view
    touched.  `chunk` does not change a bit.  trunc should be at least 3 voxels: the corners of a surface cell lie within
    sqrt(3) voxels of the surface, and `tsdf_surface_points` wants |tsdf| < 1 there.  bvh and adjacency as in
    `point_mesh_signed_distance`; both are resolved once for all slabs.  Plain torch around the point query."""
    who = "mesh_to_tsdf"
    _nx3(verts, who, "verts", torch.float32)
    _nx3(faces, who, "faces", torch.int32)
    _check(origin, "%s: origin" % who, (torch.float32,))
    if tuple(origin.shape) != (3,):
        raise RuntimeError("%s: origin must be shaped [3], got %s" % (who, tuple(origin.shape)))
    dev = _same_device(verts, faces, origin)
    voxel = _number(voxel, "voxel", who, lo_open=True)
    trunc = _number(trunc, "trunc", who, lo_open=True)
    if not isinstance(dims, (tuple, list)) or len(dims) != 3:
        raise RuntimeError("%s: dims must be (nx, ny, nz)" % who)
    nx, ny, nz = (_integer(d, "dims", who, 1) for d in dims)
    chunk = _integer(chunk, "chunk", who, 1)
    if 3 * nx * ny >= 2 ** 31 or nx * ny * nz >= 2 ** 31:
        raise RuntimeError("%s: 3 * nx * ny and nx * ny * nz must stay below 2^31" % who)
    max_d2 = _max_d2(trunc, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    adj = _adjacency(adjacency, faces, verts.shape[0], who)
    f32 = dict(dtype=torch.float32, device=dev)
    vox, tr = torch.tensor(voxel, **f32), torch.tensor(trunc, **f32)
    xs, ys, zs = (origin[c] + vox * torch.arange(n, **f32) for c, n in enumerate((nx, ny, nz)))
    tsdf = torch.empty((1, nz, ny, nx), **f32)
    weight = torch.empty((1, nz, ny, nx), **f32)
    per = max(1, min(chunk, 2 ** 31 // 3 - 1) // (nx * ny))
    one = torch.ones((), **f32)
    for z0 in range(0, nz, per):
        k = min(per, nz - z0)
        pts = torch.stack([xs.view(1, 1, nx).expand(k, ny, nx), ys.view(1, ny, 1).expand(k, ny, nx),
                           zs[z0:z0 + k].view(k, 1, 1).expand(k, ny, nx)], dim=-1).reshape(-1, 3)
        d2, face, _, _, sign = _signed_query(pts, verts, faces, tree, adj, max_d2, False, who)
        hit = (face >= 0).view(k, ny, nx)
        value = torch.minimum(one, _signed(d2, sign) / tr).view(k, ny, nx)
        tsdf[0, z0:z0 + k] = torch.where(hit, value, torch.zeros((), **f32))
        weight[0, z0:z0 + k] = hit.to(torch.float32)
    return tsdf, weight


def signed_error(verts, faces, truth_verts, truth_faces, n_samples=None, generator=None, bvh="auto"):
    """The signed distance of the reconstruction verts f32 [n,3], faces int32 [m,3] from the truth mesh (CUDA tensors): of
    its vertices, or with n_samples of that many surface samples of it (`mesheval.sample_surface`) -> dict of mean and
    median (of the signed distances; positive: the reconstruction lies on the free-space side of the truth),
    share_outside (the share with sign > 0), n (the points that found a face), n_undetermined (those among them with sign
    0 and a distance > 0, which count as positive distances) and n_unmatched (the points with face == -1, which the
    statistics leave out).  bvh: 'auto' or None, as for `point_mesh_signed_distance`.  The distances are the kernels';
    the reductions are torch ops with float64 sums.  `mesheval.reconstruction_error` gives the unsigned summary."""
    from .mesheval import sample_surface
    who = "signed_error"
    for t, name, dt in ((verts, "verts", torch.float32), (faces, "faces", torch.int32),
                        (truth_verts, "truth_verts", torch.float32), (truth_faces, "truth_faces", torch.int32)):
        _nx3(t, who, name, dt)
    _same_device(verts, faces, truth_verts, truth_faces)
    if bvh not in (None, "auto"):
        raise RuntimeError("%s: bvh must be None or 'auto'" % who)
    if n_samples is not None:
        n_samples = _integer(n_samples, "n_samples", who, 1)
    src = verts if n_samples is None else sample_surface(verts, faces, n_samples, generator)[0]
    sdist, face, _, sign = point_mesh_signed_distance(src, truth_verts, truth_faces, bvh=bvh, return_feature=True)
    ok = face >= 0
    d, s = sdist[ok].double(), sign[ok]
    n = d.numel()
    if n == 0:
        nan = float("nan")
        return dict(mean=nan, median=nan, share_outside=nan, n=0, n_undetermined=0, n_unmatched=int(sdist.numel()))
    return dict(mean=float(d.sum() / n), median=float(d.median()), share_outside=float((s > 0).sum()) / n, n=n,
                n_undetermined=int(((s == 0) & (d > 0)).sum()), n_unmatched=int(sdist.numel()) - n)
