"""Robust point-to-mesh ICP (include/ext/ctd_hip_mesh_robust.h, csrc/mesh_robust.hip): `meshreg`'s registration with an
M-estimator weight per point (Huber or Tukey), with matches on the rim of an open mesh rejected and with matches whose
normals disagree rejected.  For the inputs the reconstruction chain really produces: a fused mesh with leftover
fragments (outliers), registered against a truth mesh that is open (walls, table tops), which a point set overhangs.

    R, t, info = meshrobust.robust_mesh_icp(points, truth_verts, truth_faces, iters=15, kernel="tukey", rim=True,
                                            max_dist=0.25)
    R, t, info = meshrobust.robust_register_mesh(verts, faces, truth_verts, truth_faces, use_normals=True)
    err = meshrobust.robust_aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds=(0.005, 0.01))
    rim = meshrobust.face_rim(truth_faces, truth_verts.shape[0])              # once per mesh; pass it as rim=

A pose (R, t) moves a point p to S = R p + t, and the update is `meshreg.mesh_icp_update`, unchanged.  What this does
not do: no global registration (`meshglobal.global_mesh_icp(..., robust=dict(...))` finds the starts and runs this
loop on them) and no scale, as `meshreg`.

The header's prototypes are bound here, onto the library handle of `_lib.lib()` at first use; this table is not one of
`_lib.TABLES`.  No fallback to torch: a missing kernel is an error.  Nothing is differentiable.
"""
import ctypes

import torch

from . import _lib
from ._meshargs import _call_tree_then_brute, _flag, _nx3, _ptr_or, _resolve_bvh
from .mesheval import AUTO_BVH_MIN_FACES, reconstruction_error, sample_surface
from .meshreg import _hint, _mesh_inputs, _metric, _poses, _update_call, transform_points
from .meshsdf import _max_d2
from .meshsmooth import _adjacency
from .torchext._common import _call, _check, _integer, _number, _ptr, _same_device, _stream, _workspace

_c_int, _c_float, _c_int64, _c_size_t, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p

HEADER = "ext/ctd_hip_mesh_robust.h"

# mirrors include/ext/ctd_hip_mesh_robust.h one to one, in the header's order (tests/test_mesh_robust_host.py)
TABLE = {
    "ctd_mesh_face_rim_u8": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _c_int64, _vp, _vp, _c_int, _vp]),
    "ctd_mesh_robust_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "ctd_mesh_robust_system_f32": (_c_int, [_vp, _c_int, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_float,
                                            _vp, _c_int, _vp, _vp, _vp, _c_float] + [_vp] * 7 + [_c_size_t, _c_int, _vp]),
}

KERNELS = {"none": 0, "huber": 1, "tukey": 2}
TUNE = {"huber": 1.345, "tukey": 4.685}                      # 95 % efficiency on Gaussian residuals
MAD_TO_SIGMA = 1.4826

_bound = None


def lib():
    """the handle of `_lib.lib()` with this module's prototypes bound"""
    global _bound
    if _bound is None:
        l = _lib.lib()
        for name, (res, args) in TABLE.items():
            fn = getattr(l, name)           # AttributeError here means header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _bound = l
    return _bound


_RULE = """
    The rule (include/ext/ctd_hip_mesh_robust.h).  S, the nearest face within max_dist, D, the face's unit normal n, e and
    J are `meshreg.mesh_icp_system`'s.  Per point and pose the first of these that applies is its status, and any but 0
    gates it away: 1 no face; 2 the face has no normal (asked for by metric 'plane', and by `normals`); 3 `rim` is given
    and the closest point lies on a boundary vertex or edge of the face; 4 `normals` is given and the point's normal
    under the pose, m = R a, has m . n < min_cos (or NaN); 5 the weight is 0: with r = |e| ('plane') or sqrt(d2)
    ('point') and c the pose's scale, Huber is 1 for r <= c and c / r beyond, Tukey (1 - (r / c)^2)^2 for r < c and 0
    from c on; a scale that is not > 0 (NaN too) gates the whole pose, +inf weights every point 1.  Every term of
    `mesh_icp_system`'s sums is multiplied by the weight, once, in f64; system[27] is sum w e^2 and system[28] the number
    of points with status 0.  face is the query's (-1 only with status 1) and stays the next round's hint; residual is
    NaN and weight 0 where the status is not 0.  With kernel 'none', no rim and no normals the system is
    `mesh_icp_system`'s bit for bit."""


def _kernel(kernel, who):
    if kernel not in KERNELS:
        raise RuntimeError("%s: unknown kernel %r (none | huber | tukey)" % (who, kernel))
    return KERNELS[kernel]


def face_rim(faces, n_verts, adjacency=None):
    """Which features of each face of faces int32 [m,3] (a CUDA tensor) over n_verts vertices lie on the boundary of the
    surface -> rim uint8 [m]: bits 0, 1, 2 for the corners a, b, c that are an end of a boundary edge, bits 3, 4, 5 for the
    edges ab, ac, bc that exactly one valid face uses: the feature codes of `meshsdf.point_mesh_signed_distance`.  A
    non-manifold edge is not rim; an invalid face (an index outside [0, n_verts), or two equal) gets 0.  adjacency: a
    `meshsmooth.MeshAdjacency` of these faces (built here when None: one synchronisation; none otherwise).  Integer work:
    the same bits on every run."""
    who = "face_rim"
    _nx3(faces, who, "faces", torch.int32, letter="m")
    n_verts = _integer(n_verts, "n_verts", who)
    adj = _adjacency(adjacency, faces, n_verts, who)
    dev, m = faces.device, faces.shape[0]
    rim = torch.empty((m,), dtype=torch.uint8, device=dev)
    if m > 0:
        spare = adj.face_offsets
        _call(lib().ctd_mesh_face_rim_u8, who, _ptr(faces), m, n_verts, _ptr(adj.face_offsets), _ptr_or(adj.face_ids, spare),
              adj.face_ids.shape[0], _ptr_or(adj.vflags, spare), _ptr(rim), dev.index, _stream(dev))
    return rim


def _rim(rim, faces, n_verts, dev, who):
    """rim: None, True (built here) or a `face_rim` tensor -> uint8 [m] or None"""
    if rim is None:
        return None
    if rim is True:
        return face_rim(faces, n_verts)
    _check(rim, "%s: rim" % who, (torch.uint8,))
    if tuple(rim.shape) != (faces.shape[0],) or rim.device != dev:
        raise RuntimeError("%s: rim must be uint8 shaped [%d] on the device of faces, or True" % (who, faces.shape[0]))
    return rim


def _normals(normals, n, dev, who):
    if normals is None:
        return None
    _nx3(normals, who, "normals", torch.float32, rows=n)
    if normals.device != dev:
        raise RuntimeError("%s: normals must be on the device of points (%s vs %s)" % (who, dev, normals.device))
    return normals


def _min_cos(min_cos, who):
    v = _number(min_cos, "min_cos", who, lo=-1.0)
    if v > 1.0:
        raise RuntimeError("%s: min_cos must lie in [-1, 1], got %r" % (who, min_cos))
    return v


def _scale(scale, kern, K, single, dev, who):
    """scale: None (kernel 'none' only), a number, or an f32 device tensor [K] ([] or [1] for a single pose) -> f32 [K] or
    None.  The values are the kernel's business: a scale that is not > 0 gates its pose away."""
    if scale is None:
        if kern != 0:
            raise RuntimeError("%s: kernel 'huber' and 'tukey' need a scale" % who)
        return None
    if isinstance(scale, torch.Tensor):
        _check(scale, "%s: scale" % who, (torch.float32,))
        if scale.device != dev:
            raise RuntimeError("%s: scale must be on the device of points (%s vs %s)" % (who, dev, scale.device))
        if tuple(scale.shape) != (K,) and not (single and scale.dim() == 0):
            raise RuntimeError("%s: scale must be a number or float32 shaped [%d]" % (who, K))
        return scale.reshape(K)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise RuntimeError("%s: scale must be a number or a float32 tensor shaped [%d]" % (who, K))
    return torch.full((K,), float(scale), dtype=torch.float32, device=dev)


def _system_call(points, verts, faces, Rk, tk, K, metric, max_d2, tree, hint, kern, scale, rim, normals, min_cos, want, who):
    """one C call on checked arguments; want: the maps to allocate, a subset of face, residual, weight, status, closest
    -> dict with "system" [K,29] and those maps"""
    dev, n = points.device, points.shape[0]
    if 3 * K * n >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of poses * the number of points must stay below 2^31" % who)
    shapes = {"face": ((K, n), torch.int32), "residual": ((K, n), torch.float32), "weight": ((K, n), torch.float32),
              "status": ((K, n), torch.int8), "closest": ((K, n, 3), torch.float32)}
    out = {"system": torch.empty((K, 29), dtype=torch.float64, device=dev)}
    for name in want:
        out[name] = torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev)
    opt = lambda x: (_ptr(x) or None) if x is not None else None
    L = lib()
    ws = _workspace(L.ctd_mesh_robust_workspace_bytes(K, n), dev)
    head = (_ptr(points) or None, n, _ptr(Rk), _ptr(tk), K, _ptr(verts) or None, verts.shape[0], _ptr(faces) or None,
            faces.shape[0])
    tail = (metric, max_d2, opt(hint), kern, opt(scale), opt(rim), opt(normals) if n > 0 else None, min_cos, _ptr(out["system"]),
            opt(out.get("face")), opt(out.get("residual")), opt(out.get("weight")), opt(out.get("status")),
            opt(out.get("closest")), _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _call_tree_then_brute(L.ctd_mesh_robust_system_f32, head, tree, tail, who)
    return out


_MAPS = ("face", "residual", "weight", "status", "closest")


def robust_icp_system(points, verts, faces, R, t, metric="plane", kernel="tukey", scale=None, rim=None, normals=None,
                      min_cos=0.0, max_dist=None, bvh="auto", hint=None, return_maps=False):
    """The weighted, gated normal equations of one round of ICP of points f32 [n,3] under the pose(s) R f32 [3,3] |
    [K,3,3], t f32 [3] | [K,3] against the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors) -> system float64 [29] |
    [K,29], and with return_maps (system, face int32, residual f32, weight f32, status int8, all [n] | [K,n], closest f32
    [n,3] | [K,n,3]).  kernel: 'none', 'huber' or 'tukey'; scale: its c, a number or an f32 tensor [K] on the device (one
    per pose; `robust_scale` makes one from a round's residuals), needed unless the kernel is 'none'.  rim: None, a
    `face_rim` tensor of these faces, or True to build one here (one synchronisation).  normals: None, or f32 [n,3], the
    points' normals in the points' frame, with min_cos in [-1, 1].  metric, max_dist, bvh and hint as for
    `meshreg.mesh_icp_system`.  Feed the system to `meshreg.mesh_icp_update`; `robust_mesh_icp` runs both in a loop."""
    who = "robust_icp_system"
    dev = _mesh_inputs(points, verts, faces, who)
    Rk, tk, K, single = _poses(R, t, who)
    _same_device(points, R, t)
    m = _metric(metric, who)
    kern = _kernel(kernel, who)
    want = _flag(return_maps, "return_maps", who)
    max_d2 = _max_d2(max_dist, who)
    min_cos = _min_cos(min_cos, who)
    scale = _scale(scale, kern, K, single, dev, who)
    normals = _normals(normals, points.shape[0], dev, who)
    hint = _hint(hint, K, points.shape[0], single, dev, who)
    rim = _rim(rim, faces, verts.shape[0], dev, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    out = _system_call(points, verts, faces, Rk, tk, K, m, max_d2, tree, hint, kern, scale, rim, normals, min_cos,
                       _MAPS if want else (), who)
    out = tuple(out[name] for name in ("system",) + (_MAPS if want else ()))
    if single:
        out = tuple(x[0] for x in out)
    return out if want else out[0]


def robust_scale(residual, kernel):
    """The scale of a round from the residuals of the round before: tune * 1.4826 * nanmedian(|residual|) over the last
    dimension, residual f32 [n] | [K,n] -> f32 [] | [K]; tune is 1.345 for 'huber' and 4.685 for 'tukey'.  1.4826 times the
    median absolute residual estimates the standard deviation of Gaussian residuals.  The median is torch.nanmedian's
    (the lower of the two middle values), over the points that were not gated away (the others' residuals are NaN); the
    product is one f32 multiplication by float32(tune * 1.4826).  A pose without a residual gets NaN, which gates it away.
    Torch ops on the device of `residual`, no synchronisation."""
    who = "robust_scale"
    if kernel not in TUNE:
        raise RuntimeError("%s: unknown kernel %r (huber | tukey)" % (who, kernel))
    if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float32 or residual.dim() not in (1, 2):
        raise RuntimeError("%s: residual must be a float32 tensor shaped [n] or [K,n]" % who)
    if residual.shape[-1] == 0:
        return torch.full(residual.shape[:-1], float("nan"), dtype=torch.float32, device=residual.device)
    factor = torch.tensor(TUNE[kernel] * MAD_TO_SIGMA, dtype=torch.float32, device=residual.device)
    return residual.abs().nanmedian(dim=-1).values * factor


def robust_mesh_icp(points, verts, faces, R=None, t=None, iters=10, metric="plane", kernel="tukey", scale="mad", rim=None,
                    normals=None, min_cos=0.0, max_dist=None, bvh="auto", min_count=64, min_pivot=1e-4, damping=0.0,
                    rms_tol=None, use_hint=True):
    """`meshreg.mesh_icp` on `robust_icp_system`: registers points f32 [n,3] to the mesh verts f32 [m,3], faces int32 [k,3]
    (CUDA tensors) by `iters` rounds of the weighted system and `meshreg.mesh_icp_update` -> (R' f32, t' f32, info), shaped
    as the start R [3,3] | [K,3,3], t [3] | [K,3] (None: the identity).  The tree and the rim (rim=True) are built once, each
    round's faces are the next round's hint (use_hint=False: no hint, the same bits, more time), and everything runs on the
    current stream without a host synchronisation unless rms_tol is given (as in `mesh_icp`).
    scale: 'mad' (the default), a number, or an f32 tensor [K].  'mad' runs round 0 with c = +inf, which weights every
    point that passes the gates 1, and every later round with `robust_scale` of the residuals of the round before, per
    pose, computed on the device.  With kernel 'none' the scale is not used.  On noise-free data the median goes towards 0
    with the residuals; a pose whose median is exactly 0 gets c = 0, is gated away whole and ends with ok = 0.
    info, device tensors: "rms" float64 [rounds] | [rounds,K] is sqrt(system[27] / system[28]), the root of the WEIGHTED
    sum of squares over the NUMBER of points that took part (not over the sum of the weights), NaN where that number is 0;
    "used" (and "count", the same tensor, `mesh_icp`'s name) float64 is system[28] of each round; "scale" f32 is the c of
    each round (NaN with kernel 'none'); "ok" and "best" as in `mesh_icp`."""
    who = "robust_mesh_icp"
    dev = _mesh_inputs(points, verts, faces, who)
    iters = _integer(iters, "iters", who, 1)
    m = _metric(metric, who)
    kern = _kernel(kernel, who)
    max_d2 = _max_d2(max_dist, who)
    min_cos = _min_cos(min_cos, who)
    min_count = _integer(min_count, "min_count", who)
    min_pivot = _number(min_pivot, "min_pivot", who)
    damping = _number(damping, "damping", who)
    if rms_tol is not None:
        rms_tol = _number(rms_tol, "rms_tol", who)
    _flag(use_hint, "use_hint", who)
    if (R is None) != (t is None):
        raise RuntimeError("%s: give both R and t, or neither" % who)
    if R is None:
        R, t = torch.eye(3, dtype=torch.float32, device=dev), torch.zeros(3, dtype=torch.float32, device=dev)
    Rk, tk, K, single = _poses(R, t, who)
    _same_device(points, R, t)
    mad = isinstance(scale, str)
    if mad and scale != "mad":
        raise RuntimeError("%s: scale must be 'mad', a number or a float32 tensor shaped [%d]" % (who, K))
    if kern == 0:
        c = None
    elif mad:
        c = torch.full((K,), float("inf"), dtype=torch.float32, device=dev)
    else:
        c = _scale(scale, kern, K, single, dev, who)
    normals = _normals(normals, points.shape[0], dev, who)
    rim = _rim(rim, faces, verts.shape[0], dev, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    want = (("face",) if use_hint else ()) + (("residual",) if mad and kern != 0 else ())
    systems, scales, hint, last = [], [], None, None
    ok = torch.zeros((K,), dtype=torch.uint8, device=dev)
    for _ in range(iters):
        out = _system_call(points, verts, faces, Rk, tk, K, m, max_d2, tree, hint, kern, c, rim, normals, min_cos, want, who)
        system, hint = out["system"], out.get("face")
        Rk, tk, ok = _update_call(system, Rk, tk, K, min_count, min_pivot, damping, who)
        systems.append(system)
        scales.append(c if c is not None else torch.full((K,), float("nan"), dtype=torch.float32, device=dev))
        if mad and kern != 0:
            c = robust_scale(out["residual"], kernel)
        if rms_tol is not None:
            rms = torch.sqrt(system[:, 27] / system[:, 28])
            if last is not None and bool(((rms - last).abs() <= rms_tol).all()):
                break
            last = rms
    systems, scales = torch.stack(systems), torch.stack(scales)
    used = systems[..., 28]
    rms = torch.sqrt(systems[..., 27] / used)
    score = torch.where((ok != 0) & ~torch.isnan(rms[-1]), rms[-1], torch.full_like(rms[-1], float("inf")))
    best = torch.where(torch.isinf(score).all(), torch.full((), -1, dtype=torch.int64, device=dev), score.argmin())
    pick = (lambda x: x[:, 0]) if single else (lambda x: x)
    info = {"rms": pick(rms), "used": pick(used), "count": pick(used), "scale": pick(scales), "ok": ok[0] if single else ok,
            "best": best}
    return (Rk[0], tk[0], info) if single else (Rk, tk, info)


def _face_unit_normals(verts, faces, idx):
    """the unit normals of the faces idx int64 [n] in torch ops: (v1 - v0) x (v2 - v0) over its length"""
    tri = faces.long()[idx]
    a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    return (n / torch.linalg.norm(n, dim=1, keepdim=True)).contiguous()


def robust_register_mesh(verts, faces, truth_verts, truth_faces, n_samples=20000, generator=None, use_normals=False, **icp):
    """`robust_mesh_icp` of `n_samples` area-weighted surface samples (`mesheval.sample_surface`) of the mesh verts f32
    [n,3], faces int32 [m,3] against the mesh truth_verts, truth_faces (CUDA tensors) -> (R, t, info), whose keyword
    arguments pass through.  use_normals=True passes the unit normals of the sampled faces as `normals`, so that min_cos
    gates matches between surfaces that face different ways (both meshes must be wound alike)."""
    who = "robust_register_mesh"
    for x, name, dt in ((verts, "verts", torch.float32), (faces, "faces", torch.int32),
                        (truth_verts, "truth_verts", torch.float32), (truth_faces, "truth_faces", torch.int32)):
        _nx3(x, who, name, dt)
    _same_device(verts, faces, truth_verts, truth_faces)
    n_samples = _integer(n_samples, "n_samples", who, 1)
    if _flag(use_normals, "use_normals", who):
        if "normals" in icp:
            raise RuntimeError("%s: give use_normals=True or normals, not both" % who)
        pts, idx = sample_surface(verts, faces, n_samples, generator)
        icp["normals"] = _face_unit_normals(verts, faces, idx)
    else:
        pts = sample_surface(verts, faces, n_samples, generator)[0]
    return robust_mesh_icp(pts, truth_verts, truth_faces, **icp)


def robust_aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples=None, generator=None,
                                        bvh="auto", icp_samples=20000, **icp):
    """`meshreg.aligned_reconstruction_error` with `robust_register_mesh` in place of `register_mesh` (its keyword
    arguments, use_normals among them, pass through) -> the dict of `mesheval.reconstruction_error` of the moved vertices
    against the truth, plus "R", "t", "icp" (the info of `robust_mesh_icp`) and "before".  Raises when the registration
    was refused (ok = 0 in its last round)."""
    who = "robust_aligned_reconstruction_error"
    before = reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples, generator, bvh)
    R, t, info = robust_register_mesh(verts, faces, truth_verts, truth_faces, icp_samples, generator, **icp)
    if R.dim() == 3:
        best = int(info["best"])
        if best < 0:
            raise RuntimeError("%s: no start ended with ok = 1" % who)
        R, t = R[best], t[best]
    elif not bool(info["ok"]):
        raise RuntimeError("%s: the registration was refused in its last round (ok = 0)" % who)
    moved = transform_points(verts, R, t).contiguous()
    out = reconstruction_error(moved, faces, truth_verts, truth_faces, thresholds, n_samples, generator, bvh)
    out.update(R=R, t=t, icp=info, before=before)
    return out


robust_icp_system.__doc__ += _RULE
robust_mesh_icp.__doc__ += _RULE
