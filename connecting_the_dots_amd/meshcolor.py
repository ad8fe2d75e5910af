"""Colours for mesh points from the views of a track, on the device (include/ctd_hip_mesh_color.h, csrc/mesh_color.hip):
every point is projected into each posed view, a view sees it when the segment from the camera centre to the point
reaches it before any face of an occluding mesh, and the views that see it are sampled bilinearly and blended.

    m = meshops.clean_tsdf_mesh(mesh.tsdf_mesh(tsdf, weight, origin, voxel, return_normals=True), min_faces=32)
    vc = meshcolor.color_tsdf_mesh(m, images, K, R, t, margin=2 * voxel)      # rows align with m.verts
    verts, faces, _ = m.track(0)
    mesh.save_ply("model.ply", verts, faces, colors=meshcolor.to_uint8(vc.color[:verts.shape[0]]))
    vc = meshcolor.view_colors(points, images, K, R, t, margin, verts, faces, bvh='auto', return_flags=True)
    seen = (vc.flags & meshcolor.USED) == meshcolor.USED                     # which views see which point

The colours are the brute-force kernel's bit for bit whether or not a `renderer.MeshBVH` is used; the tree only makes
them cheaper.  No fallback to torch: a missing kernel is an error.
"""
import torch

from . import _lib
from ._meshargs import _call_tree_then_brute, _cat_or_empty, _flag, _nx3, _resolve_bvh, _tsdf_mesh_arg
from .torchext._common import _check, _number, _ptr, _same_device, _stream

IN_IMAGE, FACING, UNOCCLUDED, USED = 1, 2, 4, 7

# 'auto' builds a tree from this many faces on.  profiles/view_colors.txt (10^5 near-surface points, 4 views of 480 x 640,
# brute force against build + traversal): the tree loses at 5 332 faces (0.70) and wins at 18 964 (4.50); the crossover is
# near 6 800 by interpolation in the logarithms, rounded up to the power of two.  Later than the nearest-face query's
# (mesheval.AUTO_BVH_MIN_FACES = 4096): an any-hit ray has no best-so-far to tighten the test with, and the exact pruning
# test widens a node's box by the faces' |e1||e2|, which is large on coarse meshes
AUTO_BVH_MIN_FACES = 8192

_MODES = {"mean": 0, "best": 1}

_RULE = """
    The rule (include/ctd_hip_mesh_color.h), all in f32.  For each point X the views are visited in ascending order; a
    step that fails ends the view.  IN_IMAGE: S = R X + t has K S = (u, v, d) with d > 0, the pixel x = u / d, y = v / d
    lies in [0, W-1] x [0, H-1] and, with valid, the four pixels around it are nonzero.  FACING: with normals, the cosine
    between the normal and the direction to the camera centre is > 0 and >= min_cos, and is the view's weight w; without,
    w = 1.  UNOCCLUDED: no face of the mesh is hit by the ray from the camera centre towards X at a distance in
    (0, |X - C| - margin), by the ray casters' ray/triangle test; faces with an index outside [0, n_verts) are skipped.
    A view that passes all three is sampled bilinearly.  mode 'mean': color = sum(w s) / sum(w) and weight = sum(w) over
    those views; 'best': the sample and w of the view of largest w, the lowest on a tie.  n_views counts them; with none,
    color is NaN and weight 0.  The same bits on every run, with a tree or without."""


class ViewColors:
    """What `view_colors` returns: color f32 [n,C], weight f32 [n], n_views int32 [n] and flags uint8 [n,V] (the bits
    IN_IMAGE, FACING, UNOCCLUDED per point and view; None without return_flags)."""

    def __init__(self, color, weight, n_views, flags):
        self.color, self.weight, self.n_views, self.flags = color, weight, n_views, flags


def _views(images, K, R, t, who, lead=()):
    """images [*lead,V,C,H,W] (or [*lead,V,H,W]: C = 1), K [3,3], R [*lead,V,3,3], t [*lead,V,3], all checked ->
    (images with its channel axis, V, C, H, W)"""
    k = len(lead)
    _check(images, "%s: images" % who, (torch.float32,))
    for x, name in ((K, "K"), (R, "R"), (t, "t")):
        _check(x, "%s: %s" % (who, name), (torch.float32,))
    if images.dim() == k + 3:
        images = images.unsqueeze(k + 1)
    pre = "".join("%s," % c for c in "BT"[:k])
    if images.dim() != k + 4 or tuple(images.shape[:k]) != tuple(lead):
        raise RuntimeError("%s: images must be shaped [%sV,C,H,W] or [%sV,H,W], got %s" % (who, pre, pre, tuple(images.shape)))
    V, C, H, W = images.shape[k:]
    if V < 1 or V > 64:
        raise RuntimeError("%s: between 1 and 64 views, got %d" % (who, V))
    if C < 1 or C > 4:
        raise RuntimeError("%s: between 1 and 4 channels, got %d" % (who, C))
    if H < 2 or W < 2:
        raise RuntimeError("%s: images of at least 2 x 2 pixels, got %d x %d" % (who, H, W))
    if tuple(K.shape) != (3, 3):
        raise RuntimeError("%s: K must be shaped [3,3], got %s" % (who, tuple(K.shape)))
    if tuple(R.shape) != tuple(lead) + (V, 3, 3) or tuple(t.shape) != tuple(lead) + (V, 3):
        raise RuntimeError("%s: R must be shaped [%sV,3,3] and t [%sV,3] with V = %d, got %s and %s"
                           % (who, pre, pre, V, tuple(R.shape), tuple(t.shape)))
    return images, V, C, H, W


def _scalars(margin, min_cos, mode, return_flags, who):
    margin = _number(margin, "margin", who)
    min_cos = _number(min_cos, "min_cos", who)
    if not min_cos < 1.0:
        raise RuntimeError("%s: min_cos must lie in [0, 1)" % who)
    if mode not in _MODES:
        raise RuntimeError("%s: unknown mode %r (mean | best)" % (who, mode))
    _flag(return_flags, "return_flags", who)
    return margin, min_cos, _MODES[mode]


def view_colors(points, images, K, R, t, margin, verts=None, faces=None, normals=None, valid=None, min_cos=0.0,
                mode="mean", bvh=None, return_flags=False):
    """Colours for points f32 [n,3] from the views images f32 [V,C,H,W] (or [V,H,W]: one channel) of one track with
    intrinsics K [3,3] and poses R [V,3,3], t [V,3] (X_cam = R X_world + t), CUDA tensors -> `ViewColors`.
    margin: a length in world units, no default -- faces closer than that to the point along the line of sight do not
    occlude it (the point's own surface), and the right value depends on the mesh (a TSDF mesh: a voxel or two).
    verts f32 [m,3], faces int32 [k,3]: the occluding mesh (None: nothing occludes).  normals f32 [n,3]: views are then
    weighted by the cosine towards the camera and need it > 0 and >= min_cos.  valid uint8 [V,H,W]: pixels that may be
    sampled.  mode: 'mean' or 'best'.  bvh: None (brute force over all faces), a `renderer.MeshBVH` built from these
    very tensors, or 'auto' (builds one when the mesh has at least AUTO_BVH_MIN_FACES faces); a tree that is not usable
    falls back to brute force, and all give the same bits.  Not differentiable."""
    who = "view_colors"
    _nx3(points, who, "points", torch.float32)
    images, V, C, H, W = _views(images, K, R, t, who)
    margin, min_cos, mode = _scalars(margin, min_cos, mode, return_flags, who)
    if (verts is None) != (faces is None):
        raise RuntimeError("%s: verts and faces go together" % who)
    dev = points.device
    if verts is None:
        if bvh is not None and bvh != "auto":
            raise RuntimeError("%s: a bvh needs its verts and faces" % who)
        verts = torch.empty((0, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((0, 3), dtype=torch.int32, device=dev)
    _nx3(verts, who, "verts", torch.float32)
    _nx3(faces, who, "faces", torch.int32)
    n = points.shape[0]
    others = [images, K, R, t, verts, faces]
    if normals is not None:
        _nx3(normals, who, "normals", torch.float32)
        if normals.shape[0] != n:
            raise RuntimeError("%s: normals must have one row per point" % who)
        others.append(normals)
    if valid is not None:
        _check(valid, "%s: valid" % who, (torch.uint8,))
        if tuple(valid.shape) != (V, H, W):
            raise RuntimeError("%s: valid must be shaped [V,H,W] = %s, got %s" % (who, (V, H, W), tuple(valid.shape)))
        others.append(valid)
    _same_device(points, *others)
    if 3 * n >= 2 ** 31 or n * V >= 2 ** 31 or V * C * H * W >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of points, points * views and V * C * H * W must stay below 2^31" % who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    color = torch.empty((n, C), dtype=torch.float32, device=dev)
    weight = torch.empty((n,), dtype=torch.float32, device=dev)
    n_views = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.empty((n, V), dtype=torch.uint8, device=dev) if return_flags else None
    if n == 0:
        return ViewColors(color, weight, n_views, flags)
    args = (_ptr(points), _ptr(normals), n, _ptr(images), _ptr(valid), _ptr(K), _ptr(R), _ptr(t), V, C, H, W,
            _ptr(verts) or None, verts.shape[0], _ptr(faces) or None, faces.shape[0])
    rest = (margin, min_cos, mode, _ptr(color), _ptr(weight), _ptr(n_views), _ptr(flags), dev.index, _stream(dev))
    _call_tree_then_brute(_lib.lib().ctd_mesh_view_colors_f32, args, tree, rest, who)
    return ViewColors(color, weight, n_views, flags)


view_colors.__doc__ += _RULE


def color_tsdf_mesh(m, images, K, R, t, margin, valid=None, min_cos=0.0, mode="mean", return_flags=False):
    """Colours for the vertices of a `mesh.TsdfMesh` from its tracks' views: images f32 [B,V,C,H,W] (or [B,V,H,W]),
    K [3,3], R [B,V,3,3], t [B,V,3], valid uint8 [B,V,H,W] or None -> `ViewColors` whose rows align with m.verts.  Track by
    track on m.track(b): `view_colors` of the track's vertices against the track's own mesh (bvh='auto'), with m.normals
    when the mesh has them.  margin as for `view_colors`: for a TSDF mesh a voxel or two."""
    who = "color_tsdf_mesh"
    B = _tsdf_mesh_arg(m, who).n_tracks
    images, V, C, H, W = _views(images, K, R, t, who, lead=(B,))
    _scalars(margin, min_cos, mode, return_flags, who)
    if valid is not None:
        _check(valid, "%s: valid" % who, (torch.uint8,))
        if tuple(valid.shape) != (B, V, H, W):
            raise RuntimeError("%s: valid must be shaped [B,V,H,W] = %s, got %s" % (who, (B, V, H, W), tuple(valid.shape)))
    _same_device(m.verts, images, K, R, t, *(() if valid is None else (valid,)))
    parts = []
    for b, verts, faces, normals, _ in m.tracks():
        parts.append(view_colors(verts, images[b], K, R[b], t[b], margin, verts, faces, normals=normals,
                                 valid=None if valid is None else valid[b], min_cos=min_cos, mode=mode, bvh="auto",
                                 return_flags=return_flags))

    def cat(name, shape, dtype):
        return _cat_or_empty([getattr(p, name) for p in parts], m.verts.new_empty(shape, dtype=dtype))

    return ViewColors(cat("color", (0, C), torch.float32), cat("weight", (0,), torch.float32),
                      cat("n_views", (0,), torch.int32), cat("flags", (0, V), torch.uint8) if return_flags else None)


def to_uint8(color, fill=(0, 0, 0)):
    """color f32 [n,C] with C = 1 or 3 (a tensor of any device) -> uint8 [n,3] for `mesh.save_ply(colors=)` and for
    viewing: clamped to [0, 1], multiplied by 255 and rounded; a row with a NaN gets `fill`; one channel is repeated to
    three."""
    who = "to_uint8"
    if not isinstance(color, torch.Tensor) or color.dtype != torch.float32 or color.dim() != 2 or color.shape[1] not in (1, 3):
        raise RuntimeError("%s: color must be a float32 tensor shaped [n,1] or [n,3]" % who)
    fill = tuple(fill)
    if len(fill) != 3 or any(isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= 255 for x in fill):
        raise RuntimeError("%s: fill must be three integers in [0, 255]" % who)
    c = color.expand(-1, 3) if color.shape[1] == 1 else color
    bad = torch.isnan(c).any(1, keepdim=True)
    out = torch.round(torch.clamp(torch.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).to(torch.uint8)
    return torch.where(bad, torch.tensor(fill, dtype=torch.uint8, device=c.device).expand_as(out), out).contiguous()
