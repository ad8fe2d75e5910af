"""Point-to-mesh ICP (include/ext/ctd_hip_mesh_register.h, csrc/mesh_register.hip): brings a point set, or a mesh through
its surface samples, into the frame of a mesh, so that `mesheval.reconstruction_error` and `meshsdf.signed_error` measure
the surface and not a rigid offset between the two.

    R, t, info = meshreg.mesh_icp(points, truth_verts, truth_faces, iters=10, max_dist=0.05)
    moved = meshreg.transform_points(points, R, t)
    R, t, info = meshreg.register_mesh(verts, faces, truth_verts, truth_faces, n_samples=20000)
    err = meshreg.aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds=(0.005, 0.01))

A pose (R, t) moves a point p to S = R p + t.  What this does not do: no global registration (it converges from a few
tens of degrees and a fraction of the object's size at best; pass several starts as R [K,3,3], t [K,3] and take
info["best"]; `meshglobal.global_mesh_icp` finds such starts from any orientation and refines them with this loop) and
no scale.  No robust weights and no rejection of matches on boundary edges here either: a point set
that overhangs an open mesh pulls towards its rim, and outliers pull as hard as their distance.  `max_dist` is the blunt
remedy; `meshrobust` (include/ext/ctd_hip_mesh_robust.h) has Huber and Tukey weights, rim rejection and a normal gate
on the same system.

The header's prototypes are bound here, onto the library handle of `_lib.lib()` at first use; this table is not one of
`_lib.TABLES`.  No fallback to torch: a missing kernel is an error.  Nothing is differentiable.
"""
import ctypes

import torch

from . import _lib
from ._meshargs import _call_tree_then_brute, _flag, _nx3, _resolve_bvh
from .mesheval import AUTO_BVH_MIN_FACES, reconstruction_error, sample_surface
from .meshsdf import _max_d2
from .torchext._common import _call, _check, _integer, _number, _ptr, _same_device, _stream, _workspace

_c_int, _c_float, _c_double, _c_size_t, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p

HEADER = "ext/ctd_hip_mesh_register.h"

# mirrors include/ext/ctd_hip_mesh_register.h one to one, in the header's order (tests/test_mesh_register_host.py)
TABLE = {
    "ctd_mesh_register_workspace_bytes": (_c_size_t, [_c_int, _c_int]),
    "ctd_mesh_register_system_f32": (_c_int, [_vp, _c_int, _vp, _vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _c_int, _c_float] +
                                     [_vp] * 6 + [_c_size_t, _c_int, _vp]),
    "ctd_mesh_register_update_f32": (_c_int, [_vp, _vp, _vp, _c_int, _c_double, _c_double, _vp, _vp, _vp, _c_int, _c_int, _vp]),
}

MAX_POSES = 64
_METRICS = {"plane": 0, "point": 1}

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
    The rule (include/ext/ctd_hip_mesh_register.h).  Per point p and pose: S = ((R0 p0 + R1 p1) + R2 p2) + t in f32 by
    rows; (d2, face, q) is `meshsdf.point_mesh_signed_distance`'s nearest face of S within max_dist, brute force or tree,
    the same bits; a point without a face is dropped; D = S - q.  metric 'plane': n the face's unit normal in f32
    (dropped when its length is 0 or not finite), e = n . D, J = (S x n, n), residual e.  metric 'point': three rows
    e = D_k, J = (S x u_k, u_k) for the unit axes, counted once, residual sqrt(d2).  system [29] is the 21 upper-triangle
    entries of sum J J^T, the 6 of sum J e, sum e e and the count, in f64 from exact products in one fixed order: the same
    bits on every run.  A dropped point has face -1 and residual NaN.  The update is `torchext.depth_icp_update`'s damped
    LDL^T, refusals and Rodrigues step, then R' = Rr R, t' = Rr t + tr in f64, rounded to f32 once; a refused pose comes
    back bit for bit with ok = 0."""


def transform_points(points, R, t):
    """points f32 [n,3] moved by the pose(s) R f32 [3,3] | [K,3,3], t f32 [3] | [K,3] -> f32 [n,3] | [K,n,3]:
    S_j = ((R[j,0] * p0 + R[j,1] * p1) + R[j,2] * p2) + t[j], the association of the kernels, in torch ops on whatever
    device the tensors live on."""
    who = "transform_points"
    for x, name in ((points, "points"), (R, "R"), (t, "t")):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise RuntimeError("%s: %s must be a float32 tensor" % (who, name))
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("%s: points must be shaped [n,3], got %s" % (who, tuple(points.shape)))
    single = R.dim() == 2
    Rk, tk = (R.unsqueeze(0), t.unsqueeze(0)) if single else (R, t)
    if Rk.dim() != 3 or tuple(Rk.shape[1:]) != (3, 3) or tuple(tk.shape) != (Rk.shape[0], 3):
        raise RuntimeError("%s: R must be shaped [3,3] and t [3], or R [K,3,3] and t [K,3]" % who)
    _same_device(points, R, t)
    p = [points[None, :, i] for i in range(3)]                                  # [1,n]
    S = torch.stack([((Rk[:, j, 0:1] * p[0] + Rk[:, j, 1:2] * p[1]) + Rk[:, j, 2:3] * p[2]) + tk[:, j:j + 1]
                     for j in range(3)], dim=-1)                                # [K,n,3]
    return S[0] if single else S


def _poses(R, t, who):
    """R [3,3] | [K,3,3], t [3] | [K,3], f32 CUDA -> (R [K,3,3], t [K,3], K, single)"""
    _check(R, "%s: R" % who, (torch.float32,))
    _check(t, "%s: t" % who, (torch.float32,))
    single = R.dim() == 2
    Rk, tk = (R.unsqueeze(0), t.unsqueeze(0)) if single else (R, t)
    if Rk.dim() != 3 or tuple(Rk.shape[1:]) != (3, 3) or tuple(tk.shape) != (Rk.shape[0], 3):
        raise RuntimeError("%s: R must be shaped [3,3] and t [3], or R [K,3,3] and t [K,3]" % who)
    K = Rk.shape[0]
    if not 1 <= K <= MAX_POSES:
        raise RuntimeError("%s: between 1 and %d poses, got %d" % (who, MAX_POSES, K))
    return Rk, tk, K, single


def _metric(metric, who):
    if metric not in _METRICS:
        raise RuntimeError("%s: unknown metric %r (plane | point)" % (who, metric))
    return _METRICS[metric]


def _system_call(points, verts, faces, Rk, tk, K, metric, max_d2, tree, hint, want_maps, want_face, who):
    """one C call on checked arguments -> (system [K,29], face or None, residual or None, closest or None)"""
    dev, n = points.device, points.shape[0]
    if 3 * K * n >= 2 ** 31:
        raise RuntimeError("%s: 3 * the number of poses * the number of points must stay below 2^31" % who)
    system = torch.empty((K, 29), dtype=torch.float64, device=dev)
    face = torch.empty((K, n), dtype=torch.int32, device=dev) if want_maps or want_face else None
    residual = torch.empty((K, n), dtype=torch.float32, device=dev) if want_maps else None
    closest = torch.empty((K, n, 3), dtype=torch.float32, device=dev) if want_maps else None
    L = lib()
    ws = _workspace(L.ctd_mesh_register_workspace_bytes(K, n), dev)
    head = (_ptr(points) or None, n, _ptr(Rk), _ptr(tk), K, _ptr(verts) or None, verts.shape[0], _ptr(faces) or None,
            faces.shape[0])
    tail = (metric, max_d2, (_ptr(hint) or None) if hint is not None else None, _ptr(system),
            (_ptr(face) or None) if face is not None else None, (_ptr(residual) or None) if residual is not None else None,
            (_ptr(closest) or None) if closest is not None else None, _ptr(ws), ws.numel(), dev.index, _stream(dev))
    _call_tree_then_brute(L.ctd_mesh_register_system_f32, head, tree, tail, who)
    return system, face, residual, closest


def _hint(hint, K, n, single, dev, who):
    if hint is None:
        return None
    _check(hint, "%s: hint" % who, (torch.int32,))
    if tuple(hint.shape) != ((n,) if single else (K, n)):
        raise RuntimeError("%s: hint must be int32 shaped %s" % (who, (n,) if single else (K, n)))
    if hint.device != dev:
        raise RuntimeError("%s: hint must be on the device of points (%s vs %s)" % (who, dev, hint.device))
    return hint


def _mesh_inputs(points, verts, faces, who):
    _nx3(points, who, "points", torch.float32)
    _nx3(verts, who, "verts", torch.float32)
    _nx3(faces, who, "faces", torch.int32)
    return _same_device(points, verts, faces)


def mesh_icp_system(points, verts, faces, R, t, metric="plane", max_dist=None, bvh="auto", hint=None, return_maps=False):
    """The normal equations of one round of ICP of points f32 [n,3] under the pose(s) R f32 [3,3] | [K,3,3], t f32 [3] |
    [K,3] against the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors) -> system float64 [29] | [K,29], and with
    return_maps (system, face int32 [n] | [K,n], residual f32 [n] | [K,n], closest f32 [n,3] | [K,n,3]).  K <= 64 starts cost
    one launch.  max_dist: None, or a finite number >= 0: faces farther than that do not qualify.  bvh: None, 'auto' or a
    `renderer.MeshBVH` of these very tensors, as for `mesheval.point_mesh_distance`; all give the same bits.  hint: int32
    shaped as face, the faces of the round before (any values; it changes the time, never a bit).  Feed the system to
    `mesh_icp_update`; `mesh_icp` runs both in a loop."""
    who = "mesh_icp_system"
    dev = _mesh_inputs(points, verts, faces, who)
    Rk, tk, K, single = _poses(R, t, who)
    _same_device(points, R, t)
    m = _metric(metric, who)
    want = _flag(return_maps, "return_maps", who)
    max_d2 = _max_d2(max_dist, who)
    hint = _hint(hint, K, points.shape[0], single, dev, who)
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    out = _system_call(points, verts, faces, Rk, tk, K, m, max_d2, tree, hint, want, False, who)
    if single:
        out = tuple(None if x is None else x[0] for x in out)
    return out if want else out[0]


def _update_call(system, Rk, tk, K, min_count, min_pivot, damping, who):
    dev = system.device
    R_out, t_out = torch.empty_like(Rk), torch.empty_like(tk)
    ok = torch.empty((K,), dtype=torch.uint8, device=dev)
    _call(lib().ctd_mesh_register_update_f32, who, _ptr(system), _ptr(Rk), _ptr(tk), min_count, min_pivot, damping,
          _ptr(R_out), _ptr(t_out), _ptr(ok), K, dev.index, _stream(dev))
    return R_out, t_out, ok


def mesh_icp_update(system, R, t, min_count=64, min_pivot=1e-4, damping=0.0):
    """Solves the systems of `mesh_icp_system` and moves the poses -> (R' f32, t' f32, ok uint8 [] | [K]), shaped as R
    and t, which are not written.  A pose is refused (copied through, ok = 0) when its count is below min_count or a
    pivot of the damped LDL^T is not finite or not above min_pivot times its diagonal entry: a surface that leaves a
    degree of freedom free (a single plane leaves three) is refused, not guessed at."""
    who = "mesh_icp_update"
    min_count = _integer(min_count, "min_count", who)
    min_pivot = _number(min_pivot, "min_pivot", who)
    damping = _number(damping, "damping", who)
    Rk, tk, K, single = _poses(R, t, who)
    _check(system, "%s: system" % who, (torch.float64,))
    _same_device(system, R, t)
    if tuple(system.shape) != ((29,) if single else (K, 29)):
        raise RuntimeError("%s: system must be float64 shaped %s" % (who, (29,) if single else (K, 29)))
    out = _update_call(system.reshape(K, 29), Rk, tk, K, min_count, min_pivot, damping, who)
    return tuple(x[0] for x in out) if single else out


def mesh_icp(points, verts, faces, R=None, t=None, iters=10, metric="plane", max_dist=None, bvh="auto", min_count=64,
             min_pivot=1e-4, damping=0.0, rms_tol=None, use_hint=True):
    """Registers points f32 [n,3] to the mesh verts f32 [m,3], faces int32 [k,3] (CUDA tensors) by `iters` rounds of
    `mesh_icp_system` and `mesh_icp_update` -> (R' f32, t' f32, info), shaped as the start R [3,3] | [K,3,3], t [3] | [K,3]
    (None: the identity).  The tree is built once; each round's faces are the next round's hint (use_hint=False: no hint,
    the same bits, more time); everything runs on the current stream without a host synchronisation unless rms_tol is
    given.  rms_tol: a number >= 0: after every round but the first the round's rms is read back (one synchronisation
    a round), and the loop ends when every pose's rms differs from the round before by at most rms_tol.
    info, device tensors: "rms" and "count" float64 [rounds] | [rounds,K], sqrt(sum e^2 / count) (NaN where the count is
    0) and the number of points of the system each round solved, i.e. at the pose before that round's update; "ok" uint8
    [] | [K] of the last round; "best" int64 []: the pose with the lowest last-round rms among those with ok = 1, or -1
    when there is none.  "ok" is the last round's alone: a pose that ends with ok == 0 may have been moved by earlier
    rounds and can be far from any surface, so such a pose is not to be used."""
    who = "mesh_icp"
    dev = _mesh_inputs(points, verts, faces, who)
    iters = _integer(iters, "iters", who, 1)
    m = _metric(metric, who)
    max_d2 = _max_d2(max_dist, who)
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
    tree = _resolve_bvh(bvh, verts, faces, who, AUTO_BVH_MIN_FACES)
    systems, hint, last = [], None, None
    ok = torch.zeros((K,), dtype=torch.uint8, device=dev)
    for _ in range(iters):
        system, face, _, _ = _system_call(points, verts, faces, Rk, tk, K, m, max_d2, tree, hint, False, use_hint, who)
        hint = face
        Rk, tk, ok = _update_call(system, Rk, tk, K, min_count, min_pivot, damping, who)
        systems.append(system)
        if rms_tol is not None:
            rms = torch.sqrt(system[:, 27] / system[:, 28])
            if last is not None and bool(((rms - last).abs() <= rms_tol).all()):
                break
            last = rms
    systems = torch.stack(systems)
    count = systems[..., 28]
    rms = torch.sqrt(systems[..., 27] / count)
    score = torch.where((ok != 0) & ~torch.isnan(rms[-1]), rms[-1], torch.full_like(rms[-1], float("inf")))
    best = torch.where(torch.isinf(score).all(), torch.full((), -1, dtype=torch.int64, device=dev), score.argmin())
    info = {"rms": rms[:, 0] if single else rms, "count": count[:, 0] if single else count, "ok": ok[0] if single else ok,
            "best": best}
    return (Rk[0], tk[0], info) if single else (Rk, tk, info)


def register_mesh(verts, faces, truth_verts, truth_faces, n_samples=20000, generator=None, **icp):
    """ICP of `n_samples` area-weighted surface samples (`mesheval.sample_surface`) of the mesh verts f32 [n,3], faces
    int32 [m,3] against the mesh truth_verts, truth_faces (CUDA tensors) -> (R, t, info) of `mesh_icp`, whose keyword
    arguments (R, t, iters, metric, max_dist, ...) pass through: `transform_points(verts, R, t)` is the first mesh in
    the frame of the second."""
    who = "register_mesh"
    for x, name, dt in ((verts, "verts", torch.float32), (faces, "faces", torch.int32),
                        (truth_verts, "truth_verts", torch.float32), (truth_faces, "truth_faces", torch.int32)):
        _nx3(x, who, name, dt)
    _same_device(verts, faces, truth_verts, truth_faces)
    n_samples = _integer(n_samples, "n_samples", who, 1)
    pts = sample_surface(verts, faces, n_samples, generator)[0]
    return mesh_icp(pts, truth_verts, truth_faces, **icp)


def aligned_reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples=None, generator=None,
                                 bvh="auto", icp_samples=20000, **icp):
    """`register_mesh(verts, faces, truth_verts, truth_faces, icp_samples, generator, **icp)`, then
    `mesheval.reconstruction_error` of the moved vertices against the truth -> that dict, plus "R" f32 [3,3] and "t" f32
    [3] (the pose applied; with several starts the one info["best"] names), "icp" (the info of `mesh_icp`) and "before",
    the dict of `reconstruction_error` without the alignment.  thresholds, n_samples and bvh go to both
    `reconstruction_error` calls.  Raises when the registration was refused (ok = 0 in its last round): an error measured
    after a pose that is not to be used would mean nothing."""
    who = "aligned_reconstruction_error"
    before = reconstruction_error(verts, faces, truth_verts, truth_faces, thresholds, n_samples, generator, bvh)
    R, t, info = register_mesh(verts, faces, truth_verts, truth_faces, icp_samples, generator, **icp)
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


mesh_icp_system.__doc__ += _RULE
mesh_icp_update.__doc__ += _RULE
mesh_icp.__doc__ += _RULE
