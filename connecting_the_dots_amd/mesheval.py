"""How far a reconstruction is from the truth, on the device (include/ctd_hip_mesh_dist.h, csrc/point_mesh.hip): the
nearest face of a mesh for every query point, area-weighted surface samples, and the usual accuracy / completeness /
Chamfer / F-score summary of one mesh against another.

    dist, face = mesheval.point_mesh_distance(points, verts, faces, bvh='auto')
    pts, on_face = mesheval.sample_surface(verts, faces, 100000, generator=g)
    err = mesheval.reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds=(0.005, 0.01))

The distances are the brute-force kernel's bit for bit whether or not a `renderer.MeshBVH` is used; the tree only makes
them cheaper.  No fallback to torch: a missing kernel is an error.
"""
import torch

from . import _lib
from ._meshargs import _call_tree_then_brute, _flag, _nx3, _resolve_bvh
from .torchext._common import _integer, _number, _ptr, _same_device, _stream

# 'auto' builds a tree from this many faces on.  profiles/point_mesh.txt (10^5 near-surface points, brute force against
# build + traversal): the tree loses at 1 172 faces (0.58) and wins at 3 850 (1.24), the crossover is near 2 800; rounded
# up to the power of two at which it already pays
AUTO_BVH_MIN_FACES = 4096

_RULE = """
    The rule (include/ctd_hip_mesh_dist.h).  One function, point_tri, computes the squared distance d2 from a point to a
    face and the closest point on it, in f32 and one fixed operation order: Ericson's seven regions, a vertex region
    returning the vertex itself, every other region clamping its two parameters so that the point is a convex combination
    of the face's corners.  The answer for a point is the face of smallest d2 among those whose d2 compares < +inf, the
    lowest index among equal ones; face -1, distance +inf and closest NaN when no face qualifies.  Faces with an index
    outside [0, n_verts) are skipped, degenerate faces are ordinary faces.  dist is torch.sqrt of the kernel's d2.  The same
    bits on every run, with a tree or without."""


def point_mesh_distance(points, verts, faces, bvh=None, return_closest=False):
    """For every row of points f32 [n,3] the nearest face of the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors) ->
    (dist f32 [n], face int32 [n]) and, with return_closest, closest f32 [n,3].  bvh: None (brute force over all faces),
    a `renderer.MeshBVH` built from these very tensors, or 'auto' (builds one when the mesh has at least
    AUTO_BVH_MIN_FACES faces).  A tree that is not usable (deeper than the traversal stack) falls back to brute force;
    all three give the same bits.  Not differentiable."""
    who = "point_mesh_distance"
    _nx3(points, who, "points", torch.float32)
    _nx3(verts, who, "verts", torch.float32)
    _nx3(faces, who, "faces", torch.int32)
    dev = _same_device(points, verts, faces)
    _flag(return_closest, "return_closest", who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    n = points.shape[0]
    if 3 * n >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of points must stay below 2^31" % who)
    d2 = torch.empty((n,), dtype=torch.float32, device=dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    closest = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_closest else None
    if n > 0:
        args = (_ptr(points), n, _ptr(verts) or None, verts.shape[0], _ptr(faces) or None, faces.shape[0])
        out = (_ptr(d2), _ptr(face), _ptr(closest), dev.index, _stream(dev))
        _call_tree_then_brute(_lib.lib().ctd_point_mesh_distance_f32, args, tree, out, who)
    dist = torch.sqrt(d2)
    return (dist, face, closest) if return_closest else (dist, face)


point_mesh_distance.__doc__ += _RULE


def sample_surface(verts, faces, n, generator=None):
    """n points drawn uniformly from the surface of the mesh -> (points f32 [n,3], face int64 [n]): a face by
    torch.multinomial with its area as weight (faces of zero or non-finite area have weight 0), then the square-root
    barycentric draw on it.  Plain torch ops, on whatever device verts and faces live on (CPU tensors too); `generator`
    must be of that device."""
    who = "sample_surface"
    for t, name, dts in ((verts, "verts", (torch.float32,)), (faces, "faces", (torch.int32, torch.int64))):
        if not isinstance(t, torch.Tensor) or t.dtype not in dts or t.dim() != 2 or t.shape[1] != 3:
            raise RuntimeError("%s: %s must be a tensor shaped [n,3] of dtype %s" % (who, name, dts[0]))
    _same_device(verts, faces)
    n = _integer(n, "n", who)
    idx = faces.long()
    if faces.shape[0] == 0 or bool(((idx < 0) | (idx >= verts.shape[0])).any()):
        raise RuntimeError("%s: needs at least one face, and every index inside [0, %d)" % (who, verts.shape[0]))
    a, b, c = verts[idx[:, 0]], verts[idx[:, 1]], verts[idx[:, 2]]
    area = torch.linalg.norm(torch.cross(b - a, c - a, dim=1).double(), dim=1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    if not bool(area.sum() > 0):
        raise RuntimeError("%s: the mesh has no face of positive finite area" % who)
    if n == 0:
        return verts.new_empty((0, 3)), idx.new_empty((0,))
    f = torch.multinomial(area, n, replacement=True, generator=generator)     # (torch: at most 2^24 faces)
    r = torch.rand((n, 2), dtype=torch.float32, device=verts.device, generator=generator)
    s = torch.sqrt(r[:, :1])
    w = torch.cat([1 - s, s * (1 - r[:, 1:]), s * r[:, 1:]], 1)
    pts = w[:, :1] * a[f] + w[:, 1:2] * b[f] + w[:, 2:] * c[f]
    return pts.contiguous(), f


def _stats(dist, face, thresholds):
    ok = face >= 0
    d = dist[ok].double()
    n = d.numel()
    if n == 0:
        nan = float("nan")
        return dict(mean=nan, rms=nan, median=nan, max=nan, within=[nan] * len(thresholds), n=0,
                    n_unmatched=int(dist.numel()))
    return dict(mean=float(d.sum() / n), rms=float(torch.sqrt((d * d).sum() / n)), median=float(d.median()),
                max=float(d.max()), within=[float((d <= t).sum()) / n for t in thresholds], n=n,
                n_unmatched=int(dist.numel()) - n)


def reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples=None, generator=None, bvh="auto"):
    """The reconstruction verts f32 [n,3], faces int32 [m,3] against the truth mesh (CUDA tensors) -> dict:
    accuracy      the distances from the reconstruction to the truth mesh: from its vertices, or with n_samples from that
                  many surface samples of it;
    completeness  the distances from the truth to the reconstruction: from n_samples surface samples of the truth, or
                  from its vertices when n_samples is None;
    each a dict of mean, rms, median, max, within (the share <= each threshold), n and n_unmatched;
    chamfer       accuracy mean + completeness mean;
    fscore        per threshold the harmonic mean of the two within shares (0 when both are 0);
    thresholds    as given; n_unmatched  the points of both directions with face == -1, which the statistics leave out.
    bvh: 'auto' or None, as for `point_mesh_distance`, for both meshes.  The distances are the kernels'; the reductions
    are torch ops with float64 sums."""
    who = "reconstruction_error"
    for t, name, dt in ((verts, "verts", torch.float32), (faces, "faces", torch.int32),
                        (truth_verts, "truth_verts", torch.float32), (truth_faces, "truth_faces", torch.int32)):
        _nx3(t, who, name, dt)
    _same_device(verts, faces, truth_verts, truth_faces)
    if bvh not in (None, "auto"):
        raise RuntimeError("%s: bvh must be None or 'auto'" % who)
    thresholds = [_number(t, "thresholds", who) for t in thresholds]
    if n_samples is not None:
        n_samples = _integer(n_samples, "n_samples", who, 1)
    src = verts if n_samples is None else sample_surface(verts, faces, n_samples, generator)[0]
    dst = truth_verts if n_samples is None else sample_surface(truth_verts, truth_faces, n_samples, generator)[0]
    acc = _stats(*point_mesh_distance(src, truth_verts, truth_faces, bvh=bvh), thresholds)
    com = _stats(*point_mesh_distance(dst, verts, faces, bvh=bvh), thresholds)
    fscore = [(2 * p * r / (p + r) if p + r > 0 else 0.0) if p == p and r == r else float("nan")
              for p, r in zip(acc["within"], com["within"])]
    return dict(accuracy=acc, completeness=com, chamfer=acc["mean"] + com["mean"], fscore=fscore,
                thresholds=thresholds, n_unmatched=acc["n_unmatched"] + com["n_unmatched"])
